"""Stochastic maps of the MCMC samplers on the device (phm_maketreelistMCMC_maps) against their Python twin
(tests/mcmcmapsref.py) bit for bit, against the samplers' own statistics and four chains of the CPU oracle on C3's tree, the two-phase contract (tampered offsets,
guard elements), capacity recovery, devices, the exact per-branch expectations, and a drawn history as the start of a chain."""
import ctypes as C

import numpy as np
import pytest

import mcmcmapsclasses
import mcmcmapsref
import oracle_lib as O
from phylomap_amd import _lib, api, synth
from phylomap_amd.maps import Maps, history_tree

pytestmark = pytest.mark.gpu

FN = {"plain": api.sumstatMCMC, "bigtree": api.sumstatMCMC_bigtree, "sparse": api.SPARSEsumstatMCMC,
      "ks": api.sumstatMCMCks_sweep, "bf": api.sumstatMCMCbf_sweep}


def _model(n, kind):
    if kind == "ks":                                                        # hidden rates, k = n/2 - 1 regimes
        k = n // 2 - 1
        return synth.make2sQ(0.3, 0.2, [0.4, 0.3, 0.2][:k], [0.3, 0.2, 0.1][:k], [2.0, 0.5, 1.0][:k])
    if kind == "tri":
        return synth.tridiagonal_Q(n, 0.2)
    if kind == "neighbour":
        return synth.neighbour_Q(n, 6, 0.05)
    if n == 2:
        return np.array([[-0.6, 0.6], [0.9, -0.9]])
    return synth.dense_Q(n, 0.02, 0.2 / n, seed=0x3F00 + n)


def _problem(n, kind, T, seed, shuffled=False, long_branch=False):
    Q = _model(n, kind)
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    z = synth.make_tree(T, Q, Omega, seed, init_segments=n if kind in ("tri", "neighbour") else 2)
    if long_branch:                                                         # more than 64 segments on edge row 0, sweep after sweep
        z["edge.length"] = np.array(z["edge.length"], dtype=np.float64)
        z["edge.length"][0] = 90.0 / Omega
        end = int(z["mapnames"][0][-1])
        z["maps"][0], z["mapnames"][0] = synth.initial_path(z["edge.length"][0], end, 100)
    if shuffled:
        perm = np.random.default_rng(seed).permutation(len(z["edge"]))
        z = dict(z, edge=np.asarray(z["edge"])[perm], **{"edge.length": np.asarray(z["edge.length"])[perm]},
                 maps=[z["maps"][i] for i in perm], mapnames=[z["mapnames"][i] for i in perm])
    pid = np.arange(1.0, n + 1.0) / (n * (n + 1) / 2)
    return z, Q, Omega, pid


def _twin(z, Q, Omega, pid, N, seed, r, variant, its, sites=None):
    zs = z if sites is None else dict(z, states=np.asarray(sites[r], dtype=np.int32))
    nen, nodelist, root = _lib.tree_orders(zs)
    vt = {"plain": "plain", "bigtree": "bigtree", "sparse": "sparse", "ks": "ks", "bf": "bf"}[variant]
    return mcmcmapsref.sumstatMCMC(zs, Q.tolist(), pid.tolist(), Omega, N, [int(v) for v in nen], [int(v) for v in nodelist],
                                   int(root), seed, r, variant=vt, map_iters=its)


def _check_history(m, h, rows, j, E):
    off, dwell, state = mcmcmapsref.history(rows, j, E)
    lo = m.off[h * E]
    assert np.array_equal(m.off[h * E:(h + 1) * E + 1] - lo, off), h
    hi = m.off[(h + 1) * E]
    assert np.array_equal(m.state[lo:hi], state), h
    assert np.array_equal(m.dwell[lo:hi], dwell), h


CASES = [  # n, Q kind, variant, tips, S, map_iters ("all" / list), shuffled, long branch, sites
    (2, "dense", "plain", 12, 1, "all", False, False, False),
    (2, "dense", "bigtree", 12, 63, [0], True, False, False),
    (3, "dense", "sparse", 10, 64, [3], False, False, False),
    (4, "ks", "ks", 10, 130, [0, 2], True, False, False),
    (4, "dense", "bf", 10, 64, "all", False, False, False),
    (4, "dense", "plain", 10, 3, [1, 3], True, False, True),
    (3, "dense", "plain", 8, 2, "all", False, True, False),
    (8, "dense", "plain", 10, 64, [1, 3], True, False, False),
    (8, "ks", "ks", 8, 2, [3], False, False, False),
    (5, "dense", "bf", 8, 130, [0], False, False, False),
    (8, "dense", "plain", 8, 2, "all", False, True, False),
    (20, "tri", "sparse", 8, 1, "all", True, False, False),
    (20, "neighbour", "plain", 8, 2, [1, 3], False, False, True),
    (61, "dense", "plain", 4, 1, [3], False, False, False),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-S{c[4]}" + ("-long" if c[7] else "") + ("-sites" if c[8] else "")
                                             for c in CASES])
def test_mcmc_maps_against_twin(case):
    n, kind, variant, T, S, its, shuffled, long_branch, sites = case
    z, Q, Omega, pid = _problem(n, kind, T, 0x3F1 + n, shuffled, long_branch)
    N, seed = 4, 0x51 + n
    E = len(z["edge"])
    site_m = None
    opt = dict(seed=seed)
    if sites:
        rs = np.random.default_rng(n)
        site_m = np.stack([np.asarray(z["states"])] + [rs.integers(1, n + 1, size=T) for _ in range(S - 1)]).astype(np.int32)
        if kind == "neighbour":                                             # states reachable through the sparse pattern
            site_m[1:] = np.asarray(z["states"])[None, :]
        opt["sites"] = site_m
    elif S > 1:
        opt["n_replicas"] = S
    rec = None if its == "all" else its
    out, m = FN[variant](z, Q, pid, Omega, N, maps=True, map_iters=rec, reduce=False, **opt)
    J = N if its == "all" else len(its)
    assert m.n_hist == S * J and m.n_edge == E
    plain = FN[variant](z, Q, pid, Omega, N, mapping="tiles", reduce=False, **opt)
    assert np.array_equal(out, plain)
    auto = FN[variant](z, Q, pid, Omega, N, reduce=False, **opt)
    nd = n + n * (n - 1) if variant in ("plain", "bigtree", "sparse") else n + n * n
    assert np.array_equal(np.asarray(out)[..., n:nd], np.asarray(auto)[..., n:nd])
    for r in sorted({0, 63, 64, S - 1} & set(range(S))):
        tout, rows = _twin(z, Q, Omega, pid, N, seed, r, variant, rec, site_m)
        for j in range(J):
            _check_history(m, r * J + j, rows, j, E)
        mine = np.asarray(out)[r] if S > 1 else np.asarray(out)
        assert np.array_equal(mine[:, n:nd], np.array(tout)[:, n:nd])


def _args(variant, z, Q, pid, Omega, N, its, **opt):
    Q = np.asfortranarray(Q, dtype=np.float64)
    n = Q.shape[0]
    nen, nodelist, root = _lib.tree_orders(z)
    B = np.asfortranarray(np.eye(n) + Q / Omega)
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    ft = _lib.FlatTree(z)
    o = _lib.make_options(**opt)
    S = max(1, int(o.n_replicas))
    it = np.ascontiguousarray(its, dtype=np.int32)
    out = np.zeros((N, n + n * (n - 1)), order="F") if (o.reduce or S == 1) else np.zeros((S, n + n * (n - 1), N))
    keep = (Q, nen, nodelist, B, pid, ft, o, it)
    args = (int(variant), C.byref(ft.c), n, _lib._p(Q, C.c_double), _lib._p(pid, C.c_double), _lib._p(B, C.c_double), float(Omega),
            _lib._p(nen, C.c_int32), _lib._p(nodelist, C.c_int32), int(root), int(N), _lib._p(it, C.c_int32), int(it.size),
            C.byref(o), _lib._p(out, C.c_double))
    return args, out, keep


def test_c3_mcmc_maps_1024():
    z, Q, pid, Omega = synth.config_problem(3)                               # 10 000 tips, 4 states
    n, S, N, its = 4, 1024, 3, [0, 2]
    E = z["edge"].shape[0]
    T = len(z["states"])
    L = _lib.load()
    args, out, keep = _args(_lib.PHM_MCMC_BIGTREE, z, Q, pid, Omega, N, its, seed=0xC3, n_replicas=S)
    off = np.zeros(S * 2 * E + 1, dtype=np.int64)
    _lib.check(L.phm_maketreelistMCMC_maps(*args, _lib._p(off, C.c_int64), 0, None, None))
    sized = out.copy()
    total = int(off[-1])
    dwell, state = np.empty(total), np.empty(total, dtype=np.int32)
    _lib.check(L.phm_maketreelistMCMC_maps(*args, _lib._p(off, C.c_int64), total, _lib._p(dwell, C.c_double), _lib._p(state, C.c_int32)))
    assert np.array_equal(sized, out)
    assert np.array_equal(out, api.sumstatMCMC_bigtree(z, Q, pid, Omega, N, seed=0xC3, n_replicas=S, reduce=False, mapping="tiles").transpose(0, 2, 1))
    m = Maps(off, dwell, state, E)
    row = np.repeat(np.arange(off.size - 1), np.diff(off))
    same = row[:-1] == row[1:]
    h, a, b = row[:-1][same] // E, state[:-1][same] - 1, state[1:][same] - 1
    assert np.all(a != b)
    col = a * (n - 1) + np.where(b > a, b - 1, b)
    cnt = np.bincount(h * n * (n - 1) + col, minlength=S * 2 * n * (n - 1)).reshape(S, 2, n * (n - 1))
    stats = out.transpose(0, 2, 1)                                            # [S, N, cols]
    assert np.array_equal(cnt.astype(np.float64), stats[:, its, n:])
    length = float(np.sum(z["edge.length"]))
    dw = np.zeros((S * 2, n))
    np.add.at(dw, (row // E, state.astype(np.int64) - 1), dwell)
    assert np.max(np.abs(dw.reshape(S, 2, n) - stats[:, its, :n])) <= 1e-12 * length
    rs = np.zeros(S * 2 * E)
    np.add.at(rs, row, dwell)
    np.testing.assert_allclose(rs.reshape(S * 2, E), np.broadcast_to(z["edge.length"], (S * 2, E)), rtol=1e-10)
    ns = m.node_states()
    edge = np.asarray(z["edge"])
    tip_rows = edge[:, 1] <= T
    assert np.all(ns[:, tip_rows, 1] == np.asarray(z["states"])[edge[tip_rows, 1] - 1][None, :])
    into = np.full(2 * T, -1)
    into[edge[:, 1]] = np.arange(E)
    inner = into[edge[:, 0]] >= 0
    multi = m.counts()[:, inner] > 1                                         # m_b = 1 keeps the child's state throughout
    assert np.array_equal(ns[:, inner, 0][multi], ns[:, into[edge[inner, 0]], 1][multi])
    # Four chains against the oracle (tiles_branch_group = 4 at this size: several branches per wave in mcmc_maps_tiles_kernel): the
    # path sweep ``it`` left is the chain state after it + 1 sweeps; merged, it is the map.  Offsets and states bit for bit, dwell
    # within 4 L 2^-53 relative, L the longest branch of these chains on the oracle after any sweep (both sides add at most L
    # positive numbers left to right).
    nen, nodelist, root = _lib.tree_orders(z)
    B = np.eye(n) + Q / Omega
    chains, want, longest = (0, 63, 64, 1023), {}, 0
    for r in chains:
        for sweeps in range(1, N + 1):
            _, rc, dump = O.maketreelistMCMC(z, Q, pid, B, Omega, nen, nodelist, root, sweeps, variant=O.BIGTREE, seed=0xC3, replica=r, dump=True)
            assert rc == 0
            longest = max(longest, int(dump.seg_count.max()))
            if sweeps - 1 in its:
                want[r, sweeps - 1] = mcmcmapsclasses.merged_dump(dump)
    bar, worst = 4.0 * longest * 2.0 ** -53, 0.0
    for r in chains:
        for j, it in enumerate(its):
            woff, wdwell, wstate = want[r, it]
            k = (r * 2 + j) * E
            lo, hi = off[k], off[k + E]
            assert np.array_equal(off[k:k + E + 1] - lo, woff), (r, it)
            assert np.array_equal(state[lo:hi] - 1, wstate), (r, it)
            worst = max(worst, float(np.max(np.abs(dwell[lo:hi] - wdwell) / wdwell)))
    print(f"C3 maps against the oracle: worst dwell error over the bar {worst / bar:.3g} (L = {longest})")
    assert worst <= bar
    # a tampered offset table names its row and writes nothing past map_cap
    bad = 3 * E + 777
    off2 = off.copy()
    off2[bad + 1:] += 1
    cap = int(off2[-1])
    G = 64
    d2, s2 = np.full(cap + G, -7.25), np.full(cap + G, -7, dtype=np.int32)
    st = L.phm_maketreelistMCMC_maps(*args, _lib._p(off2, C.c_int64), cap, _lib._p(d2, C.c_double), _lib._p(s2, C.c_int32))
    assert st == 1
    msg = L.phm_last_error().decode()
    assert f"row {bad} " in msg and "chain 1 at iteration 2" in msg and "edge row 778" in msg, msg
    assert np.all(d2[cap:] == -7.25) and np.all(s2[cap:] == -7)


def test_recovery_and_devices_give_the_default_maps():
    z, Q, Omega, pid = _problem(4, "dense", 60, 0x6D)
    base = api.sumstatMCMC(z, Q, pid, Omega, 12, maps=True, map_iters=[0, 5, 11], seed=7, n_replicas=200, reduce=False)
    # cap_tail = 0.9 provisions slots too small for the first sweeps: the engine recovers and replays.  The slot sizes order the
    # branches of the dwell reduction, so the statistics keep their counts (and the plain call's dwell bits at that cap_tail).
    for opt in (dict(cap_tail=0.9), dict(devices=[0, 0])):
        got = api.sumstatMCMC(z, Q, pid, Omega, 12, maps=True, map_iters=[0, 5, 11], seed=7, n_replicas=200, reduce=False, **opt)
        if "devices" in opt:
            assert np.array_equal(got[0], base[0])
        else:
            assert np.array_equal(got[0][..., 4:], base[0][..., 4:])
            assert np.array_equal(got[0], api.sumstatMCMC(z, Q, pid, Omega, 12, seed=7, n_replicas=200, reduce=False, mapping="tiles", **opt))
        assert np.array_equal(got[1].off, base[1].off) and np.array_equal(got[1].state, base[1].state), opt
        assert np.array_equal(got[1].dwell, base[1].dwell), opt
    zw, Qw, Ow, pw = _problem(8, "dense", 40, 0x6E)
    b8 = api.sumstatMCMC(zw, Qw, pw, Ow, 6, maps=True, seed=9, n_replicas=100, reduce=False)
    g8 = api.sumstatMCMC(zw, Qw, pw, Ow, 6, maps=True, seed=9, n_replicas=100, reduce=False, cap_tail=0.9)
    assert np.array_equal(b8[0][..., 8:], g8[0][..., 8:])
    assert np.array_equal(b8[1].off, g8[1].off) and np.array_equal(b8[1].state, g8[1].state) and np.array_equal(b8[1].dwell, g8[1].dwell)


def test_mcmc_maps_per_branch_means_match_exact():
    n = 4
    Q = synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0) * 0.5
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    pid = np.full(n, 1.0 / n)
    z = synth.make_tree(40, Q, Omega, 0x40A, pid, init_segments=n)
    S, its = 512, list(range(100, 200, 5))
    J = len(its)
    _, m = api.sumstatMCMC(z, Q, pid, Omega, 200, maps=True, map_iters=its, seed=0x40C, n_replicas=S, reduce=True)
    _, _, exact = api.expected_sumstat(z, Q, pid, per_branch=True)
    exact = exact[0]                                                        # [E, n + n(n-1)]
    E = m.n_edge
    per = np.zeros((S * J, E, n + n * (n - 1)))
    per[:, :, :n] = m.mapped_edge(n)
    row = np.repeat(np.arange(m.off.size - 1), np.diff(m.off))
    same = row[:-1] == row[1:]
    a, b = m.state[:-1][same] - 1, m.state[1:][same] - 1
    col = a * (n - 1) + np.where(b > a, b - 1, b)
    np.add.at(per, (row[:-1][same] // E, row[:-1][same] % E, n + col), 1.0)
    chain = per.reshape(S, J, E, -1).mean(axis=1)                           # chain means: independent units
    mean, sd = chain.mean(axis=0), chain.std(axis=0, ddof=1)
    se = np.sqrt(np.maximum(sd ** 2, np.where(sd == 0, exact, 0.0)) / S)   # a column never seen: a Poisson bound
    z_ = np.abs(mean - exact) / np.maximum(se, 1e-300)
    z_[(se == 0) & (exact == 0)] = 0.0
    assert np.max(z_) < 5, (np.max(z_), np.unravel_index(np.argmax(z_), z_.shape))


def test_mcmc_draw_starts_a_chain():
    n = 4
    Q = synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0)
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    pid = np.full(n, 1.0 / n)
    z = synth.make_tree(60, Q, Omega, 0x51A, pid)
    _, m = api.sumstatMCMC(z, Q, pid, Omega, 20, maps=True, map_iters=[19], seed=0x51E, n_replicas=8, reduce=False)
    zt = history_tree(z, m, 5, n=n)
    assert np.array_equal(zt["states"], z["states"])
    out = api.sumstatMCMC(zt, Q, pid, Omega, 200, seed=0x51F)
    assert out.shape[0] == 200 and np.all(np.isfinite(out))
