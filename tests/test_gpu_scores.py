"""The expected statistics of many rate matrices on the device (phm_expected_stats_models) against the Python
twin (``exactref.expected`` per model), against phm_loglik_models and phm_expected_stats, its long-branch, -inf, mu = 0, chunking
and device rules, and the fits over it: the exact-gradient fit at the rehearsed optima, the per-site study and its standard
errors."""
import os

import numpy as np
import pytest

import exactref
from phylomap_amd import _lib, api, ratemodel, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# the generators of test_gpu_loglik_models.py
def _tree(T, seed, shuffled, mean=1.0):
    edge, lens = synth.random_tree(T, mean, seed)
    lens = lens.copy()
    lens[3] = 0.0                                                             # a zero-length branch
    if shuffled:
        perm = np.random.default_rng(seed).permutation(edge.shape[0])
        edge, lens = edge[perm], lens[perm]
    return {"edge": edge, "edge.length": lens, "Nnode": T - 1, "states": np.ones(T, dtype=np.int32)}


def _models(n, K, seed):
    """K random generators: rates in (0.02, 1.5), a fifth of the entries structurally zero (never a whole row)"""
    rs = np.random.default_rng(seed)
    Qs = rs.uniform(0.02, 1.5, (K, n, n)) * rs.uniform(0.2, 3.0, (K, 1, 1))
    Qs[rs.random((K, n, n)) < 0.2] = 0.0
    idx = np.arange(n)
    Qs[:, idx, (idx + 1) % n] += 0.05
    Qs[:, idx, idx] = 0.0
    Qs[:, idx, idx] = -Qs.sum(axis=2)
    return Qs


def _wide_models(n, K, seed):
    return np.stack([synth.dense_Q(n, 0.01, 0.04, seed=seed + k) * (1.0 + k) for k in range(K)])


def _sites(T, n, S, seed, observe):
    rs = np.random.default_rng(seed)
    top = n if observe is None else int(np.max(observe))
    tips = rs.integers(1, top + 1, (S, T))
    tips[rs.random((S, T)) < 0.1] = 0                                         # missing tips
    return tips.astype(np.int32)


def _positive(Qs):
    """every entry positive: every evaluation possible"""
    n = Qs.shape[1]
    Qs = np.abs(Qs) + 1e-3
    idx = np.arange(n)
    Qs[:, idx, idx] = 0.0
    Qs[:, idx, idx] = -Qs.sum(axis=2)
    return Qs


def _bar(got, want, ll_got, ll_want, length):
    """stats <= 1e-12 relative with section 13's floor of 1e-14 x tree length, loglik <= 1e-12 max(1, |l|); an evaluation the twin
    finds impossible is -inf with a row of NaN.  Returns the largest stats error over its allowance and the largest loglik error."""
    assert got.shape == want.shape and ll_got.shape == ll_want.shape
    ok = np.isfinite(ll_want)
    assert np.array_equal(np.isfinite(ll_got), ok)
    assert np.all(ll_got[~ok] == -np.inf) and np.all(np.isnan(got[~ok]))
    le = np.abs(ll_got[ok] - ll_want[ok]) / np.maximum(1.0, np.abs(ll_want[ok]))
    assert np.all(le <= 1e-12), le.max()
    err = np.abs(got[ok] - want[ok])
    allow = 1e-12 * np.abs(want[ok]) + 1e-14 * length
    assert np.all(err <= allow), (err.max(), np.max(err / allow))
    return (float(np.max(err / allow)) if err.size else 0.0), (float(le.max()) if le.size else 0.0)


def _twin(z, Qs, pid, tips, observe):
    pid = np.atleast_2d(np.asarray(pid, dtype=np.float64))
    st, ll = [], []
    for k in range(len(Qs)):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            s, l = exactref.expected(z["edge"], z["edge.length"], Qs[k], pid[k if pid.shape[0] > 1 else 0], tips, observe)
        st.append(s)
        ll.append(np.where(np.isfinite(l), l, -np.inf))
    return np.array(st), np.array(ll)


@pytest.mark.parametrize("n", [2, 3, 4, 8, 20, 61])
@pytest.mark.parametrize("shuffled,observed", [(False, False), (True, True), (False, True)])
def test_against_the_twin(n, shuffled, observed):
    z = _tree(24, 0xF100 + n, shuffled)
    length = float(np.sum(z["edge.length"]))
    observe = (np.arange(n) % 2 + 1) if observed else None
    tips = _sites(24, n, 5, 7 * n + shuffled, observe)
    worst = [0.0, 0.0]
    for K in ((1, 63, 64, 130) if n <= 8 else (2,)):
        Qs = _models(n, K, 100 * n + K) if n <= 8 else _wide_models(n, K, 0xA0 + n)
        rs = np.random.default_rng(K)
        pid = rs.uniform(0.1, 1.0, (K, n)) if shuffled else np.arange(1.0, n + 1.0)   # per-model / shared
        want, ll_want = _twin(z, Qs, pid, tips, observe)
        got, ll = api.expected_sumstat_models(z, Qs, pid, sites=tips, observe=observe)
        assert got.shape == (K, 5, n * n) and ll.shape == (K, 5)
        w = _bar(got, want, ll, ll_want, length)
        worst = [max(a, b) for a, b in zip(worst, w)]
        ok = np.isfinite(ll)
        np.testing.assert_allclose(got[ok][:, :n].sum(axis=1), length, rtol=1e-12)      # the dwell times fill the tree
        one, ll1 = api.expected_sumstat_models(z, Qs, pid, sites=tips[:1], observe=observe)   # S = 1
        assert np.array_equal(ll1[:, 0], ll[:, 0]) and np.array_equal(one[:, 0], got[:, 0], equal_nan=True)
        som = rs.integers(0, 5, K)
        pst, pll = api.expected_sumstat_models(z, Qs, pid, sites=tips, observe=observe, site_of_model=som)
        assert pst.shape == (K, n * n) and pll.shape == (K,)
        assert np.array_equal(pll, ll[np.arange(K), som])                               # the same arithmetic per evaluation,
        assert np.array_equal(pst, got[np.arange(K), som], equal_nan=True)              # so the twin's bar holds for paired too
    print(f"n={n} shuffled={shuffled} observed={observed}: stats error / allowance {worst[0]:.3g}, "
          f"max |d loglik| / max(1, |loglik|) = {worst[1]:.3g}")


@pytest.mark.parametrize("n", [2, 4, 8, 20])
def test_against_the_existing_entry_points(n):
    z = _tree(40, 0xF200 + n, True)
    length = float(np.sum(z["edge.length"]))
    K = 70 if n <= 8 else 2
    Qs = _positive(_models(n, K, 9 * n) if n <= 8 else _wide_models(n, K, 0xB0))
    pid = np.arange(1.0, n + 1.0)
    tips = _sites(40, n, 3, n, None)
    got, ll = api.expected_sumstat_models(z, Qs, pid, sites=tips)
    assert np.array_equal(ll, api.loglik_models(z, Qs, pid, sites=tips))
    ref = [api.expected_sumstat(z, Qs[k], pid, sites=tips) for k in range(K)]
    assert np.array_equal(ll, np.stack([r[1] for r in ref]))
    w = _bar(got, np.stack([r[0] for r in ref]), ll, ll, length)
    print(f"n={n}: stats against expected_sumstat: error / allowance {w[0]:.3g}")


def test_squamate_long_branches():
    """mu t_b up to 2 280: e^(-mu t) is not representable.  The case the lane's weight rule exists for."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "squamate", "seed101_tips.npz"))
    T = len(d["states"])
    z = {"edge": d["edge"], "edge.length": d["edge_length"], "Nnode": T - 1, "states": d["states"]}
    assert 10.0 * d["edge_length"].max() > 745
    Qs = np.array([[[-10.0, 10.0], [6.0, -6.0]], [[-0.001, 0.001], [0.006, -0.006]], [[-3.0, 3.0], [8.0, -8.0]]])
    tips = np.stack([d["states"], np.where(np.arange(T) % 7 == 0, 0, d["states"])]).astype(np.int32)
    got, ll = api.expected_sumstat_models(z, Qs, [.5, .5], sites=tips)
    ref = [api.expected_sumstat(z, Qs[k], [.5, .5], sites=tips) for k in range(3)]
    assert np.array_equal(ll, np.stack([r[1] for r in ref]))
    w = _bar(got, np.stack([r[0] for r in ref]), ll, ll, float(np.sum(z["edge.length"])))
    print(f"squamate, mu t_b up to {10.0 * d['edge_length'].max():.0f}: error / allowance {w[0]:.3g}")


def test_an_impossible_model_and_a_model_that_leaves_no_state():
    z = _tree(24, 0xF300, False)
    length = float(np.sum(z["edge.length"]))
    tips = _sites(24, 2, 5, 3, None)
    tips[tips == 0] = 1
    tips[:, 0], tips[:, 1] = 1, 2                                             # both states at the tips: a change is needed
    Qs = _models(2, 64, 5)
    Qs[17] = 0.0                                                              # q01 = q10 = 0
    got, ll = api.expected_sumstat_models(z, Qs, [.5, .5], sites=tips)
    assert np.all(ll[17] == -np.inf) and np.all(np.isnan(got[17]))
    rest = np.delete(np.arange(64), 17)
    assert np.all(np.isfinite(ll[rest])) and np.all(np.isfinite(got[rest]))
    assert np.array_equal(ll, api.loglik_models(z, Qs, [.5, .5], sites=tips))
    want, ll_want = _twin(z, Qs[rest], [.5, .5], tips, None)
    _bar(got[rest], want, ll[rest], ll_want, length)
    pst, pll = api.expected_sumstat_models(z, Qs, [.5, .5], sites=tips, site_of_model=np.arange(64) % 5)
    assert pll[17] == -np.inf and np.all(np.isnan(pst[17])) and np.all(np.isfinite(pst[rest]))
    # mu = 0 where it is possible (P = I): the state never changes, so dwell = t_b on the posterior state and no counts.  Tips in
    # state 1 or missing, pid = (0.25, 0.75): the posterior is state 1 with certainty unless every tip is missing
    one = np.ones((2, 24), dtype=np.int32)
    one[0, ::3] = 0
    one[1] = 0
    st, l0 = api.expected_sumstat_models(z, Qs[16:19], [.25, .75], sites=one)
    assert l0[1, 0] == pytest.approx(np.log(.25), rel=1e-15) and abs(l0[1, 1]) < 1e-15
    np.testing.assert_allclose(st[1, 0], [length, 0.0, 0.0, 0.0], rtol=1e-13, atol=0)
    np.testing.assert_allclose(st[1, 1], [.25 * length, .75 * length, 0.0, 0.0], rtol=1e-13, atol=0)
    assert np.all(np.isfinite(st))


@pytest.mark.parametrize("n", [4, 8, 20])
def test_chunks_and_devices_do_not_change_a_bit(n):
    z = _tree(24, 0xF400 + n, True)
    K = 130 if n <= 8 else 3
    Qs = _models(n, K, 77 + n) if n <= 8 else _wide_models(n, K, 0xC0)
    pid = np.random.default_rng(n).uniform(0.1, 1.0, (K, n))
    tips = _sites(24, n, 5, 11, None)
    som = np.arange(K) % 5
    f = api.expected_sumstat_models
    plain = f(z, Qs, pid, sites=tips)
    plain_p = f(z, Qs, pid, sites=tips, site_of_model=som)

    def same(a, b):
        return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])

    try:
        assert same(f(z, Qs, pid, sites=tips, expect_chunk=64), plain)
        assert same(f(z, Qs, pid, sites=tips, expect_chunk=2), plain)
        assert same(f(z, Qs, pid, sites=tips, devices=[0, 0]), plain)
        assert same(f(z, Qs, pid, sites=tips, site_of_model=som, expect_chunk=64), plain_p)
        assert same(f(z, Qs, pid, sites=tips, site_of_model=som, expect_chunk=2), plain_p)
        assert same(f(z, Qs, pid, sites=tips, site_of_model=som, devices=[0, 0]), plain_p)
    finally:
        _lib.set_debug_options()


def _problem(which):
    import test_fit_cpu
    edge, lens, tips, m, pid, ll_want, th_want = test_fit_cpu.problem(which)
    z = {"edge": edge, "edge.length": lens, "Nnode": len(tips) - 1, "states": tips}
    return z, m, pid, ll_want, th_want


@pytest.mark.parametrize("which", [2, 3])
def test_exact_gradient_fit_on_the_device_reaches_the_rehearsed_optimum(which):
    z, m, pid, ll_want, th_want = _problem(which)
    r = api.fit_ml(z, m, pid, gtol=1e-8, gradient="exact", se=True)           # 8 starts
    fd = api.fit_ml(z, m, pid, gtol=1e-5)
    print(f"n={which}: exact: loglik {r['loglik']:.9f} theta {r['theta']} iterations {r['iterations']} calls {r['calls']} "
          f"evaluations {r['evals']} max |score| {np.max(np.abs(r['grad'])):.3g} se_log {r['se_log']}; fd: iterations "
          f"{fd['iterations']} calls {fd['calls']} evaluations {fd['evals']}")
    assert r["converged"] and not np.any(r["at_bound"])
    assert abs(r["loglik"] - ll_want) <= 1e-8
    np.testing.assert_allclose(r["theta"], th_want, rtol=1e-5)
    assert np.max(np.abs(r["grad"])) <= 1e-8 and r["evals"] < fd["evals"]
    stats, _ = api.expected_sumstat(z, r["Q"], pid)                           # `grad` is the score section 13's entry point gives
    np.testing.assert_allclose(r["grad"], m.score(r["theta"], stats[0]), rtol=0, atol=1e-9)
    assert r["se_ok"] and np.all(r["se_log"] > 0) and np.all(r["ci"][:, 0] < r["theta"]) and np.all(r["theta"] < r["ci"][:, 1])
    np.testing.assert_allclose(r["cov_log"], np.linalg.inv(r["information"]), rtol=1e-10)


def test_per_site_fits_with_the_exact_gradient_and_their_intervals():
    """Section 17's study again: 128 datasets simulated under the truth, one fit each in lock-step; "fd" (the parent's behaviour)
    is the reference.  The coverage of the Wald intervals is reported, not gated."""
    z, m, pid, _, _ = _problem(2)
    Q = np.array([[-.3, .3], [.6, -.6]])
    truth = np.array([.3, .6])
    tips, _ = api.simulate_histories(z, Q, pid, 128, seed=5)
    fd = api.fit_ml(z, m, pid, sites=tips, per_site=True, gtol=1e-5)
    r = api.fit_ml(z, m, pid, sites=tips, per_site=True, gtol=1e-5, gradient="exact", se=True)
    rel = np.abs(r["theta"] - fd["theta"]) / fd["theta"]
    print(f"128 sites: max relative theta difference {rel.max():.3g}, min loglik difference {np.min(r['loglik'] - fd['loglik']):.3g}; "
          f"exact: calls {r['calls']} evaluations {r['evals']}; fd: calls {fd['calls']} evaluations {fd['evals']}")
    inside = (r["ci"][:, :, 0] <= truth) & (truth <= r["ci"][:, :, 1])
    ok = r["se_ok"]
    print(f"Wald 95 % intervals: se_ok on {int(ok.sum())} of 128 sites; cover theta_true: q01 {inside[ok, 0].mean():.3f}, "
          f"q10 {inside[ok, 1].mean():.3f}, both {np.all(inside[ok], axis=1).mean():.3f}")
    assert r["theta"].shape == (128, 2) and r["ci"].shape == (128, 2, 2) and r["se_ok"].shape == (128,)
    assert np.all(rel <= 1e-4)
    assert np.all(r["loglik"] >= fd["loglik"] - 1e-8)


def test_c3_tree_1024_models():
    z, Q, pid, _ = synth.config_problem(3)                                    # 10 000 tips, 4 states
    m = ratemodel.hidden_rates(1)
    rs = np.random.default_rng(0xC3)
    thetas = np.array([0.1, 0.1, 0.2, 0.2, 10.0]) * np.exp(rs.normal(0.0, 0.5, (1024, 5)))
    Qs = m.Qs(thetas)
    got, ll = api.expected_sumstat_models(z, Qs, pid)
    length = float(np.sum(z["edge.length"]))
    assert got.shape == (1024, 1, 16) and np.all(np.isfinite(got)) and np.all(np.isfinite(ll))
    np.testing.assert_allclose(got[:, 0, :4].sum(axis=1), length, rtol=1e-12)
    worst = 0.0
    for k in np.linspace(0, 1023, 16).astype(int):
        ws, wl = api.expected_sumstat(z, Qs[k], pid)
        assert ll[k, 0] == wl[0]
        worst = max(worst, _bar(got[k], ws, ll[k], wl, length)[0])
    print(f"C3, 1 024 models, 16 spot checks: error / allowance {worst:.3g}")
