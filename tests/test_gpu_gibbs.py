"""The batched posterior sampler of rates on the device (phm_gibbs_rates / api.posterior_rates).

Lock-step equivalence: for every recorded row i the DRIVER'S OWN theta^(i) goes back through the public calls -- the row's counts are
``api.sample_histories(draws=1, replica_offset=i)``'s exactly, its dwell sums agree within 1e-12 of the tree length, its
log-likelihood is ``api.loglik_models``' bit for bit, and the Python twin's Gamma update (tests/gibbsref.py) of those statistics
gives theta^(i+1) within 1e-12 relative.  Then: chunks and devices change no bit; a tight theta_max rejects; an impossible chain
fails alone; and the scheme itself against a posterior computed by quadrature, which no code under test enters."""
import functools
import math

import numpy as np
import pytest

import gibbsref
import samplecases as sc
from phylomap_amd import api, posterior, ratemodel, synth

pytestmark = pytest.mark.gpu

ITERS = 5
HIDDEN_INDEX = [[0, 1, 2, 0], [3, 0, 0, 2], [4, 0, 0, 1], [0, 4, 3, 0]]     # a structural zero in every row, 4 parameters
KEYS = ("theta", "loglik", "stats", "rejected", "status")


def model_of(n):
    return {2: ratemodel.ard(2), 3: ratemodel.sym(3), 4: ratemodel.index_model(HIDDEN_INDEX), 8: ratemodel.er(8),
            5: ratemodel.sym(5), 6: ratemodel.er(6), 7: ratemodel.ard(7)}[n]


@functools.lru_cache(maxsize=None)
def problem(n, S):
    """a 24-tip tree with shuffled edges and one zero-length branch, S sites; n = 4: parity observe and missing tips"""
    edge, lens = sc.tree(shuffle=True)
    assert lens.min() == 0.0
    m = model_of(n)
    obs = sc.PARITY if n == 4 else None
    Q = m.Q(np.linspace(0.2, 0.5, m.p))
    sites = np.stack([sc.tips_for(edge, lens, Q, 70 + s, obs, 0.1 if n == 4 else 0.0) for s in range(S)])
    assert n != 4 or np.any(sites == 0)
    return sc.as_z(edge, lens, sites[0]), m, obs, sites, np.full(n, 1.0 / n)


def flat(res, Cn):
    """the result with one chain axis, whatever the mode"""
    out = {}
    for k in KEYS:
        v = res[k]
        lead = 0 if k in ("rejected", "status") else 1
        out[k] = v.reshape(v.shape[:lead] + (Cn,) + v.shape[lead + (2 if res["per_site"] else 1):])
    return out


@functools.lru_cache(maxsize=None)
def run(n, Cn, joint, per_chain_prior, thin=1, theta_max=20.0, expect_chunk=0, devices=None):
    S = 3 if joint else {1: 1, 63: 3, 64: 2, 130: 2}[Cn]
    z, m, obs, sites, pid = problem(n, S)
    rng = np.random.default_rng(1000 * n + Cn)
    th0 = rng.uniform(0.1, min(1.5, theta_max), (Cn, m.p))
    prior = rng.uniform(0.5, 3.0, (Cn, m.p, 2)) if per_chain_prior else np.tile([1.5, 2.0], (m.p, 1))
    seed = 40 + n + Cn
    opt = {} if devices is None else {"devices": list(devices)}
    if expect_chunk:
        opt["expect_chunk"] = expect_chunk
    res = api.posterior_rates(z, m, pid, prior, ITERS, chains=Cn if joint else Cn // S, sites=sites, observe=obs, per_site=not joint,
                              theta0=th0, theta_max=theta_max, thin=thin, seed=seed, **opt)
    som = res["site_of_chain"]
    assert (som is None) == joint and (joint or (np.bincount(som).min() == Cn // S and Cn // S * S == Cn))
    return dict(flat(res, Cn), z=z, m=m, obs=obs, sites=sites, pid=pid, prior=np.broadcast_to(prior, (Cn, m.p, 2)), seed=seed, som=som,
                theta_max=theta_max, thin=thin, C=Cn)


def check_rows(r, update=True, chains=None):
    """every recorded row of run r against the public calls and the twin's update (``chains``: the chains whose update the twin
    repeats, None: all); returns whether every theta agreed bitwise"""
    m, z, n, Cn = r["m"], r["z"], r["m"].n, r["C"]
    cols = n + n * (n - 1)
    tree_len = float(np.sum(z["edge.length"]))
    rows = r["theta"].shape[0]
    assert rows == -(-ITERS // r["thin"]) and np.all(r["status"] == 0)
    kw = dict(sites=r["sites"], observe=r["obs"], site_of_model=r["som"])
    bitwise, worst_dwell, worst_theta = True, 0.0, 0.0
    for row in range(rows):
        i = row * r["thin"]
        th = r["theta"][row]
        Qs = posterior.rate_matrices(m, th)
        st, ll = api.sample_histories(z, Qs, r["pid"], 1, seed=r["seed"], replica_offset=i, **kw)
        st = st[..., 0, :].reshape(Cn, -1, cols)                            # [C, sites of the chain, cols]
        assert np.array_equal(st[:, :, n:].sum(axis=1), r["stats"][row][:, n:])
        dw = np.zeros((Cn, n))
        for s in range(st.shape[1]):                                         # sites ascending
            dw = dw + st[:, s, :n]
        worst_dwell = max(worst_dwell, float(np.max(np.abs(dw - r["stats"][row][:, :n]))))
        assert np.all(np.abs(r["stats"][row][:, :n].sum(axis=1) - st.shape[1] * tree_len) <= 1e-12 * st.shape[1] * tree_len)
        llm = api.loglik_models(z, Qs, r["pid"], **kw).reshape(Cn, -1)
        tot = np.zeros(Cn)
        for s in range(llm.shape[1]):
            tot = tot + llm[:, s]
        assert np.array_equal(tot, r["loglik"][row]) and np.array_equal(ll.reshape(Cn, -1), llm)
        if update and r["thin"] == 1 and row + 1 < rows:
            for k in (range(Cn) if chains is None else chains):
                want, _ = gibbsref.update(m.index, th[k], st[k], r["prior"][k], r["theta_max"], r["seed"], k, i)
                got = r["theta"][row + 1, k]
                worst_theta = max(worst_theta, float(np.max(np.abs(got - want) / want)))
                bitwise = bitwise and np.array_equal(got, want)
    print(f"n={n} C={Cn}: max |dwell - sample_histories'| = {worst_dwell:.3g} (tree length {tree_len:.3g}), "
          f"max relative theta difference to the twin's update = {worst_theta:.3g}, bitwise = {bitwise}")
    assert worst_dwell <= 1e-12 * tree_len
    assert worst_theta <= 1e-12
    assert np.all(r["theta"] > 0.0) and np.all(r["theta"] <= r["theta_max"])
    return bitwise


@pytest.mark.parametrize("per_chain_prior", [False, True])
@pytest.mark.parametrize("thin", [1, 2])
@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("Cn", [1, 63, 64, 130])
@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_lock_step_equivalence(n, Cn, joint, thin, per_chain_prior):
    r = run(n, Cn, joint, per_chain_prior, thin)
    check_rows(r)
    if thin > 1:                                                             # the rows a thinned run keeps are the full run's
        full = run(n, Cn, joint, per_chain_prior, 1)
        for k in ("theta", "loglik", "stats"):
            assert np.array_equal(r[k], full[k][::thin])
        assert np.array_equal(r["rejected"], full["rejected"])


@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("Cn", [63, 130])
@pytest.mark.parametrize("n", [5, 6, 7])
def test_lock_step_equivalence_run_time_n(n, Cn, joint):
    """5, 6 and 7 states: the run-time-n forms (sm_branch_kernel<0, ...>, sm_draw<0>) between the templated ones and n = 8"""
    check_rows(run(n, Cn, joint, True, 1))


@pytest.mark.parametrize("n,joint", [(4, True), (8, False)])
def test_chunks_and_devices_change_no_bit(n, joint):
    base = run(n, 130, joint, True)
    for kw in (dict(expect_chunk=64), dict(expect_chunk=2), dict(devices=(0, 0))):
        other = run(n, 130, joint, True, **kw)
        for k in KEYS:
            assert np.array_equal(base[k], other[k]), (kw, k)


def test_tight_theta_max_rejects_and_an_impossible_chain_fails_alone():
    r = run(3, 64, False, False, theta_max=0.6)
    assert r["rejected"].sum() > 0 and np.all(r["theta"] <= 0.6)
    check_rows(r)                                                            # the kept values are the twin's too
    # state 3 is never entered and the root is never in it: a tip in state 3 is impossible
    edge, lens = sc.tree(shuffle=True)
    m = ratemodel.index_model([[0, 1, 0], [2, 0, 0], [3, 3, 0]])
    pid = np.array([0.5, 0.5, 0.0])
    good = sc.tips_for(edge, lens, ratemodel.ard(2).Q([0.3, 0.4]), 5)
    bad = good.copy()
    bad[4] = 3
    Cn, dead = 66, 5
    th0 = np.random.default_rng(3).uniform(0.1, 1.0, (Cn, 3))
    # per_site puts chains 0..32 on site 0; the raw order is needed here, so the sites are laid out chain by chain
    sites_of = np.stack([bad if k == dead else good for k in range(Cn)])
    res = api.posterior_rates(sc.as_z(edge, lens, good), m, pid, [1.0, 1.0], ITERS, chains=1, sites=sites_of, per_site=True, theta0=th0,
                              theta_max=20.0, seed=9)
    f = flat(res, Cn)
    assert f["status"][dead] == 1 and f["status"].sum() == 1
    assert np.all(np.isnan(f["theta"][:, dead])) and np.all(np.isnan(f["loglik"][:, dead])) and np.all(np.isnan(f["stats"][:, dead]))
    live = np.arange(Cn) != dead
    assert np.all(np.isfinite(f["theta"][:, live])) and np.all(np.isfinite(f["loglik"][:, live])) and np.all(np.isfinite(f["stats"][:, live]))
    assert np.all(f["rejected"][dead] == 0)


def grid_reference(z, pid, theta_max, G):
    """posterior moments on a G x G midpoint grid over [0, theta_max]^2: loglik_models x the Gamma(1, 1) prior density"""
    m = ratemodel.ard(2)
    g = (np.arange(G) + 0.5) * (theta_max / G)
    a, b = np.meshgrid(g, g, indexing="ij")
    th = np.stack([a.reshape(-1), b.reshape(-1)], axis=1)
    Qs = posterior.rate_matrices(m, th)
    st, ll = api.expected_sumstat_models(z, Qs, pid)
    ll = ll[:, 0]
    assert np.array_equal(ll, api.loglik_models(z, Qs, pid)[:, 0])
    logw = ll - th[:, 0] - th[:, 1]                                          # Gamma(1, 1): density exp(-theta)
    w = np.exp(logw - logw.max())
    w /= w.sum()
    e1, e2 = float(w @ th[:, 0]), float(w @ th[:, 1])
    e11 = float(w @ th[:, 0] ** 2)
    sd = dict(t01=math.sqrt(e11 - e1 ** 2), t10=math.sqrt(float(w @ th[:, 1] ** 2) - e2 ** 2))
    N01, dw0 = st[:, 0, 2], st[:, 0, 0]
    vals = dict(t01=e1, t10=e2, t01sq=e11, N01=float(w @ N01), dwell0=float(w @ dw0))
    # posterior sd of each quantity (of E[. | tips, theta] for the two statistics: a lower bound of the statistic's own sd)
    sd["t01sq"] = math.sqrt(float(w @ th[:, 0] ** 4) - e11 ** 2)
    sd["N01"] = math.sqrt(float(w @ N01 ** 2) - vals["N01"] ** 2)
    sd["dwell0"] = math.sqrt(float(w @ dw0 ** 2) - vals["dwell0"] ** 2)
    return vals, sd


def test_the_scheme_against_quadrature():
    m = ratemodel.ard(2)
    edge, lens = synth.random_tree(40, 0.3, 12)
    pid = np.array([0.5, 0.5])
    tips = sc.tips_for(edge, lens, m.Q([0.3, 0.6]), 31)
    assert len(np.unique(tips)) == 2
    z = sc.as_z(edge, lens, tips)
    theta_max, Cn, iters, burn = 5.0, 256, 400, 100
    fine, sd = grid_reference(z, pid, theta_max, 320)
    coarse, _ = grid_reference(z, pid, theta_max, 160)
    for k in fine:                                                           # the grid is fine enough: halving its step moves nothing
        assert abs(fine[k] - coarse[k]) < 1e-3 * sd[k], (k, fine[k], coarse[k], sd[k])
    th0 = np.exp(np.random.default_rng(8).uniform(math.log(0.05), math.log(4.0), (Cn, 2)))      # dispersed starts
    res = api.posterior_rates(z, m, pid, [[1.0, 1.0], [1.0, 1.0]], iters, chains=Cn, theta0=th0, theta_max=theta_max, seed=77)
    assert np.all(res["status"] == 0)
    th, st = res["theta"][burn:], res["stats"][burn:]
    got = dict(t01=th[:, :, 0], t10=th[:, :, 1], t01sq=th[:, :, 0] ** 2, N01=st[:, :, 2], dwell0=st[:, :, 0])
    for k, x in got.items():
        per_chain = x.mean(axis=0)
        est, se = float(per_chain.mean()), float(per_chain.std(ddof=1)) / math.sqrt(Cn)
        zed = (est - fine[k]) / se
        print(f"{k}: driver {est:.5f} +- {se:.5f}, quadrature {fine[k]:.5f} (posterior sd {sd[k]:.4f}), z = {zed:.2f}")
        assert abs(zed) < 5.0, k
    s = posterior.summary(res, burn=burn)
    assert np.all(s["rhat"] < 1.05) and np.allclose(s["mean"], [fine["t01"], fine["t10"]], atol=0.05)
    d = posterior.dic(res, burn, z, pid)
    assert np.isfinite(d["DIC"]) and abs(d["DIC"] - (d["D"] + 2.0 * d["pD"])) < 1e-9 and d["theta_mean"].shape == (2,)


def test_defaults_and_result_shapes():
    z, m, obs, sites, pid = problem(2, 3)
    T, tree_len = sites.shape[1], float(np.sum(z["edge.length"]))
    r = api.posterior_rates(z, m, pid, [2.0, 1.0], 7, sites=sites, thin=3, seed=4)          # joint, 4 chains, default starts
    assert r["theta"].shape == (3, 4, 2) and r["loglik"].shape == (3, 4) and r["stats"].shape == (3, 4, 4)
    assert r["rejected"].shape == (4, 2) and r["status"].shape == (4,) and r["site_of_chain"] is None
    assert r["theta_max"] == 100.0 * (T / tree_len) and np.all(r["theta"] <= r["theta_max"]) and np.all(r["theta"] > 0.0)
    assert np.allclose(r["theta"][0, 0], T / tree_len) and len(np.unique(r["theta"][0, :, 0])) == 4   # fit.start_points: start 0 at tips / tree length
    assert np.all(np.abs(r["stats"][:, :, :2].sum(axis=2) - 3 * tree_len) <= 1e-12 * 3 * tree_len)   # summed over the three sites
    p = api.posterior_rates(z, m, pid, [2.0, 1.0], 7, chains=2, sites=sites, per_site=True, thin=3, seed=4, stats=False)
    assert p["theta"].shape == (3, 3, 2, 2) and p["loglik"].shape == (3, 3, 2) and p["stats"] is None
    assert p["rejected"].shape == (3, 2, 2) and p["status"].shape == (3, 2) and np.array_equal(p["site_of_chain"], [0, 0, 1, 1, 2, 2])
    assert np.array_equal(p["theta"][0, 0], p["theta"][0, 2]) and not np.array_equal(p["theta"][1, 0], p["theta"][1, 2])
    s = posterior.summary(p)
    assert s["mean"].shape == (3, 2) and s["rhat"].shape == (3, 2) and s["quantiles"].shape == (3, 3, 2)
    d = posterior.dic(p, 1, z, pid, sites=sites)
    assert d["DIC"].shape == (3,) and np.all(np.isfinite(d["DIC"])) and d["theta_mean"].shape == (3, 2)
