"""The small calls of the history producers whose outputs tests/golden/history_producers/parent.npz pins bit for bit (recorded
by tests/golden/history_producers/make_golden.py from the commit before the producers got their shared map-row sink, statistics
lanes and branch walk -- DESIGN.md sections 12, 14, 19 and 22 --, compared by tests/test_gpu_history_parent.py).  Shared by the
recorder and the test so that both make the same calls.  TEST INFRASTRUCTURE ONLY.

Unless stated: a 14-tip random tree with one zero-length branch and 70 histories -- two waves, the second with 6 live lanes.
A ``_maps`` case is the two-phase call (the sizing call writes the offsets, the filling call the segments); the statistics it
returns are those after the filling call.  Every input is built from integer-seeded generators and element-wise arithmetic, and
the eigen-system the EXP sampler takes is written in closed form, so that no linear-algebra library enters the recorded bytes."""
import ctypes as C

import numpy as np

import samplecases as sc
import wavegroups as wg
from manymodelscases import pinned
from phylomap_amd import _lib, api, ratemodel, synth

T, R = 14, 70
EXP_KL = 12                                            # phm_exp.hip: jump times of a branch that a lane keeps in LDS
NS = (2, 3, 4, 6)                                      # 2..4: compile-time state counts; 6: the run-time form


def tree(tips=T, seed=0x4157, shuffle=False):
    edge, lens = synth.random_tree(tips, 0.3, seed)
    lens = lens.copy()
    lens[3] = 0.0
    if shuffle:
        perm = np.random.default_rng(seed).permutation(edge.shape[0])
        edge, lens = edge[perm], lens[perm]
    return edge, lens


def as_z(edge, lens, states=None):
    t = edge.shape[0] // 2 + 1
    return {"edge": edge, "edge.length": lens, "Nnode": t - 1, "states": np.ones(t, dtype=np.int32) if states is None else states}


def models(n, k, seed=0):
    """k non-symmetric rate matrices of n states"""
    rs = np.random.default_rng(500 + 10 * n + seed)
    Qs = rs.uniform(0.2, 1.5, (k, n, n))
    for Q in Qs:
        np.fill_diagonal(Q, 0.0)
        np.fill_diagonal(Q, -Q.sum(axis=1))
    return Qs


def pids(n, k):
    return np.random.default_rng(600 + n).uniform(0.2, 1.0, (k, n))


def maps_out(m):
    return {"map_off": m.off, "map_dwell": m.dwell, "map_state": m.state}


# ---- phm_simulate_histories / _maps ----------------------------------------------------------------------------------------------

def _sim(n, maps, Q=None, observe=None, shuffle=False):
    edge, lens = tree(shuffle=shuffle)
    Q = models(n, 1)[0] if Q is None else Q
    r = api.simulate_histories(as_z(edge, lens), Q, pids(n, 1)[0], R, observe=observe, nodes=True, maps=maps, seed=900 + n,
                               replica_offset=17)
    out = {"tips": r[0], "stats": r[1], "nodes": r[2]}
    if maps:
        out.update(maps_out(r[3]))
    return out


def absorbing_Q(n=3):
    Q = models(n, 1, seed=1)[0]
    Q[1] = 0.0                                         # state 2 absorbs
    return Q


# ---- phm_simulate_histories_models -----------------------------------------------------------------------------------------------

KM, RM = 3, 50                                         # the models change at lanes 50 (wave 0) and 36 (wave 1); 22 lanes are dead


def _simm(n, maps, per_model, Qs=None, chunk=0, edge_lens=None, k=KM, reps=RM):
    edge, lens = tree() if edge_lens is None else edge_lens
    Qs = models(n, k) if Qs is None else Qs
    pid = pids(n, k) if per_model else pids(n, 1)[0]
    opt = {"expect_chunk": chunk} if chunk else {}
    r = api.simulate_histories_models(as_z(edge, lens), Qs, pid, reps, nodes=True, maps=maps, seed=1900 + n, replica_offset=5, **opt)
    out = {"tips": r[0], "stats": r[1], "nodes": r[2]}
    if maps:
        out.update(maps_out(r[3]))
    return out


def special_models(n=3):
    """an ordinary model, one with an absorbing state, one with every rate zero"""
    Qs = models(n, 3, seed=2)
    Qs[1, 0] = 0.0
    Qs[2] = 0.0
    return Qs


# ---- phm_sample_histories_models and phm_gibbs_rates -----------------------------------------------------------------------------

def _sample(n, maps, tips=T, k=2, draws=R):
    edge, lens = tree(tips)
    Qs = models(n, k, seed=3)
    states = sc.tips_for(edge, lens, Qs[0], 70 + n, missing=0.1)
    r = api.sample_histories(as_z(edge, lens, states), Qs, pids(n, k), draws, nodes=True, maps=maps, seed=2900 + n)
    out = {"stats": r[0], "loglik": r[1], "nodes": r[2]}
    if maps:
        out.update(maps_out(r[3]))
    return out


def _gibbs():
    """70 chains on two sites, joint: the packed form of sm_branch_kernel (lane = chain)"""
    edge, lens = tree()
    m = ratemodel.sym(3)
    Q0 = models(3, 1, seed=4)[0]
    sites = np.stack([sc.tips_for(edge, lens, Q0, 80 + s) for s in range(2)])
    th0 = np.random.default_rng(700).uniform(0.1, 1.5, (R, m.p))
    r = api.posterior_rates(as_z(edge, lens, sites[0]), m, np.full(3, 1.0 / 3), np.tile([1.5, 2.0], (m.p, 1)), 4, chains=R,
                            sites=sites, theta0=th0, theta_max=20.0, thin=2, seed=78)
    return {k: r[k] for k in ("theta", "loglik", "stats", "rejected", "status")}


# ---- phm_maketreelistEXP / _maps, the (tile, branch) kernels -----------------------------------------------------------------------

def exp_model(n, rate=1.0):
    """Q = rate (1 pi' - I) with pi = (1 .. n) / sum, and its eigen-system in closed form: eigenvalues 0 and -rate; the columns of
    ``lefts`` are 1 and e_k - (pi_k / pi_0) e_0, the rows of ``rights`` pi' and e_k' - pi'.  (lefts, rights, d) as eigen_decompose
    returns them."""
    pi = np.arange(1.0, n + 1.0) / (n * (n + 1) / 2)
    Q = rate * (np.tile(pi, (n, 1)) - np.eye(n))
    lefts = np.eye(n)
    lefts[:, 0] = 1.0
    lefts[0, 1:] = -pi[1:] / pi[0]
    rights = np.eye(n) - np.tile(pi, (n, 1))
    rights[0] = pi
    d = np.diag(np.concatenate([[0.0], np.full(n - 1, -rate)]))
    return Q, pi, (lefts, rights, d)


def _exp(n, maps, tips=12, N=R, long_branch=False):
    Q, pi, eig = exp_model(n)
    rate = float(np.max(-np.diag(Q)))                  # the sampler's Poisson rate
    z = synth.make_tree(tips, Q, rate, 0xE200 + n, pid=pi)
    if long_branch:                                     # Poisson mean 40 on edge row 2: every lane draws far more than EXP_KL jumps
        z["edge.length"] = np.array(z["edge.length"], dtype=np.float64)
        z["edge.length"][2] = 40.0 / rate
        z["maps"][2], z["mapnames"][2] = synth.initial_path(z["edge.length"][2], int(z["mapnames"][2][-1]), 2)
    r =api.sumstatEXP(z, Q, pi, N, eig=eig, maps=maps, seed=3900 + n)
    if not maps:
        return {"out": r}
    out, m = r
    if long_branch:
        # segments <= jumps + 1: a row of more than EXP_KL + 1 segments took the path of more than EXP_KL jump times
        assert int(np.max(m.counts()[:, 2])) > EXP_KL + 1
    return dict({"out": out}, **maps_out(m))


# ---- phm_maketreelistMCMC_maps ------------------------------------------------------------------------------------------------------

def _mcmc_maps(n):
    """70 chains, three sweeps, sweeps 0 and 2 recorded: mcmc_maps_tiles_kernel at n <= 4, mcmc_maps_wtiles_kernel above"""
    if n == 20:
        Q = synth.tridiagonal_Q(20, 0.2)
    else:
        Q = models(n, 1, seed=5)[0] * (0.4 / n)
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    z = synth.make_tree(12, Q, Omega, 0x3A00 + n, init_segments=n if n == 20 else 2)
    pid = np.arange(1.0, n + 1.0) / (n * (n + 1) / 2)
    out, m = api.sumstatMCMC(z, Q, pid, Omega, 3, maps=True, map_iters=[0, 2], seed=4900 + n, n_replicas=R, reduce=False)
    return dict({"out": out}, **maps_out(m))


# ---- the grouped kernels: an item of at least two branches -------------------------------------------------------------------------

GROUP_TIPS, GROUP_HIST = 128, 4130                     # 254 edges x 65 tiles, the last tile with 34 live lanes
GROUP_LEVELS, GROUP_KR = 5, (3, 11000)                 # the complete 32-tip tree, 33 000 histories: 516 tiles, 8 of 64 lanes dead

assert wg.sampler_launch(2 * GROUP_TIPS - 2, (GROUP_HIST + 63) // 64)["group"] >= 2       # sm_branch_kernel, exp_tiles_branch_kernel
assert GROUP_HIST % 64 == 34
_SIMM_GROUPS = [d["group"] for d in wg.simulate_launches(wg.level_counts(wg.complete_tree(GROUP_LEVELS)[0]),
                                                         GROUP_KR[0] * GROUP_KR[1])]
assert max(_SIMM_GROUPS) >= 2                          # simm_level_kernel: the level of 32 edges reaches 16 384 edge-tiles


# ---- refusals of the two simulators ----------------------------------------------------------------------------------------------

def _message(call):
    try:
        call()
    except _lib.PhmError as e:
        return np.frombuffer(f"{e.status}|{e}".encode(), dtype=np.uint8)
    raise AssertionError("the call was not refused")


NO_TARGET = np.array([[-1e-14, 0.0], [100.0, -100.0]])   # row 1 passes the row-sum check, leaves its state and has no target


def _null_sim():
    pt = _lib.PlainTree(as_z(*tree()))
    Q = np.asfortranarray(models(2, 1)[0])
    pid = np.ones(2)
    o = _lib.make_options(n_replicas=4)
    stats = np.zeros((4, 7), order="F")
    _lib.check(_lib.load().phm_simulate_histories(C.byref(pt.c), 2, _lib._p(Q, C.c_double), _lib._p(pid, C.c_double), None, C.byref(o),
                                                  None, None, _lib._p(stats, C.c_double)))


def _null_simm():
    pt = _lib.PlainTree(as_z(*tree()))
    Q = np.ascontiguousarray(models(2, 1))
    pid = np.ones((1, 2))
    o = _lib.make_options()
    stats = np.zeros((7, 1, 4))
    _lib.check(_lib.load().phm_simulate_histories_models(C.byref(pt.c), 2, 1, _lib._p(Q, C.c_double), _lib._p(pid, C.c_double), 1, None,
                                                         4, C.byref(o), None, None, _lib._p(stats, C.c_double), None, 0, None, None))


def _refusals_sim():
    z = as_z(*tree())
    return {"null": _message(_null_sim),
            "n_states": _message(lambda: api.simulate_histories(z, np.zeros((1, 1)), [1.0], 4)),
            "no_target": _message(lambda: api.simulate_histories(z, NO_TARGET, [1.0, 1.0], 4)),
            "pid": _message(lambda: api.simulate_histories(z, models(2, 1)[0], [1.0, -1.0], 4))}


def _refusals_simm():
    z = as_z(*tree())
    Qs = models(2, 3)
    bad = Qs.copy()
    bad[2] = NO_TARGET
    return {"null": _message(_null_simm),
            "n_states": _message(lambda: api.simulate_histories_models(z, np.zeros((2, 1, 1)), [1.0], 4)),
            "no_target": _message(lambda: api.simulate_histories_models(z, bad, [1.0, 1.0], 4)),
            "pid": _message(lambda: api.simulate_histories_models(z, Qs, [[1.0, 1.0], [1.0, -1.0], [1.0, 1.0]], 4))}


def _cases():
    out = []
    for n in NS:
        for maps in (False, True):
            tag = f"n{n}_{'maps' if maps else 'plain'}"
            out.append((f"sim_{tag}", lambda n=n, m=maps: _sim(n, m)))
            out.append((f"simm_{tag}", lambda n=n, m=maps: _simm(n, m, per_model=m)))
            out.append((f"sample_{tag}", lambda n=n, m=maps: _sample(n, m)))
            out.append((f"exp_{tag}", lambda n=n, m=maps: _exp(n, m)))
    out.append(("sim_absorbing", lambda: _sim(3, True, Q=absorbing_Q())))
    out.append(("sim_observe", lambda: _sim(4, True, observe=sc.PARITY)))
    out.append(("sim_shuffled", lambda: _sim(4, True, shuffle=True)))
    out.append(("simm_special", lambda: _simm(3, True, True, Qs=special_models())))
    out.append(("simm_chunks_plain", lambda: _simm(4, False, True, chunk=64)))
    out.append(("simm_chunks_maps", lambda: _simm(4, True, False, chunk=64)))
    out.append(("gibbs_packed", _gibbs))
    out.append(("exp_long_branch", lambda: _exp(4, True, long_branch=True)))
    for n in (2, 4, 6, 20):
        out.append((f"mcmc_maps_n{n}", lambda n=n: _mcmc_maps(n)))
    out.append(("simm_grouped", lambda: _simm(3, True, True, edge_lens=wg.complete_tree(GROUP_LEVELS), k=GROUP_KR[0], reps=GROUP_KR[1])))
    out.append(("sample_grouped", lambda: _sample(3, True, tips=GROUP_TIPS, k=1, draws=GROUP_HIST)))
    out.append(("exp_grouped", lambda: _exp(3, True, tips=GROUP_TIPS, N=GROUP_HIST)))
    out.append(("refusals_sim", _refusals_sim))
    out.append(("refusals_simm", _refusals_simm))
    return out


CASES = dict(_cases())


def run(name):
    """{golden key: pinned array} of one case"""
    return {f"{name}.{k}": pinned(v) for k, v in CASES[name]().items()}
