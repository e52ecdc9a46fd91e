"""The batched log-likelihood over many rate matrices on the device (phm_loglik_models) against its Python
twin (tests/fitref.py), against phm_expected_stats and the DIC driver, its -inf, chunking and device rules, and the
maximum-likelihood fit over it: the rehearsed optima, the exact score at the optimum and the calibration of the
likelihood-ratio statistic over 128 simulated datasets."""
import os
import sys

import numpy as np
import pytest

import fitref
from phylomap_amd import api, ratemodel, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GTOL = 1e-5


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


def _bar(got, want):
    assert got.shape == want.shape
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    ok = np.isfinite(want)
    err = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
    assert np.all(err <= 1e-12), err.max()
    return float(err.max()) if err.size else 0.0


@pytest.mark.parametrize("n", [2, 3, 4, 8, 20, 61])
@pytest.mark.parametrize("shuffled,observed", [(False, False), (True, True), (False, True)])
def test_against_the_twin(n, shuffled, observed):
    z = _tree(24, 0xF100 + n, shuffled)
    observe = (np.arange(n) % 2 + 1) if observed else None
    tips = _sites(24, n, 5, 7 * n + shuffled, observe)
    worst = 0.0
    for K in ((1, 63, 64, 130) if n <= 8 else (2,)):
        Qs = _models(n, K, 100 * n + K) if n <= 8 else _wide_models(n, K, 0xA0 + n)
        rs = np.random.default_rng(K)
        pid = rs.uniform(0.1, 1.0, (K, n)) if shuffled else np.arange(1.0, n + 1.0)   # per-model / shared
        want = fitref.loglik_models(z["edge"], z["edge.length"], Qs, pid, tips, observe)
        got = api.loglik_models(z, Qs, pid, sites=tips, observe=observe)
        assert got.shape == (K, 5)
        worst = max(worst, _bar(got, want))
        one = api.loglik_models(z, Qs, pid, sites=tips[:1], observe=observe)        # S = 1
        assert np.array_equal(one[:, 0], got[:, 0])
        som = rs.integers(0, 5, K)
        paired = api.loglik_models(z, Qs, pid, sites=tips, observe=observe, site_of_model=som)
        assert paired.shape == (K,)
        assert np.array_equal(paired, got[np.arange(K), som])                       # the same arithmetic per evaluation
        _bar(paired, fitref.loglik_models(z["edge"], z["edge.length"], Qs, pid, tips, observe, site_of_model=som))
    print(f"n={n} shuffled={shuffled} observed={observed}: max |d loglik| / max(1, |loglik|) = {worst:.3g}")


@pytest.mark.parametrize("n", [2, 4, 8, 20])
def test_against_expected_sumstat_per_model(n):
    z = _tree(40, 0xF200 + n, True)
    K = 70 if n <= 8 else 2
    Qs = _models(n, K, 9 * n) if n <= 8 else _wide_models(n, K, 0xB0)
    pid = np.arange(1.0, n + 1.0)
    Qs = np.abs(Qs) + 1e-3                                                    # every evaluation possible
    idx = np.arange(n)
    Qs[:, idx, idx] = 0.0
    Qs[:, idx, idx] = -Qs.sum(axis=2)
    tips = _sites(40, n, 3, n, None)
    got = api.loglik_models(z, Qs, pid, sites=tips)
    want = np.stack([api.expected_sumstat(z, Qs[k], pid, sites=tips)[1] for k in range(K)])
    worst = _bar(got, want)
    print(f"n={n}: loglik_models vs expected_sumstat: max relative difference {worst:.3g}, "
          f"bit-identical: {bool(np.array_equal(got, want))} ({int(np.sum(got != want))} of {got.size} values differ)")


def test_against_the_dic_driver():
    """Row i of sumstatMCMC2sDICt holds log p(y | Q) for the Q that drove sweep i, and that Q's rates l01, l10."""
    Q = np.array([[-.1, .1], [.1, -.1]])
    Omega, pid = 25.0, np.array([.5, .5])
    z = synth.make_tree(100, Q, Omega / 3, 45, pid)
    mat = api.sumstatMCMC2sDICt(z, Q, pid, Omega, 200, [.55, 1, .56, 1.01], seed=5)
    l01, l10 = mat[:, 6], mat[:, 7]
    Qs = np.zeros((200, 2, 2))
    Qs[:, 0, 1], Qs[:, 0, 0], Qs[:, 1, 0], Qs[:, 1, 1] = l01, -l01, l10, -l10
    got = api.loglik_models(z, Qs, pid)[:, 0]
    rel = np.abs(got - mat[:, -1]) / np.abs(mat[:, -1])
    print(f"DIC driver: max relative difference of log p(y|Q) over 200 rows: {rel.max():.3g}")
    assert np.all(rel <= 7.5e-14)                                             # 10 x the measured maximum, 7.3e-15 (the issue: 1e-10)
    assert len(np.unique(l01)) > 100                                          # the rates did move


def test_an_impossible_model_is_minus_infinity_for_itself_only():
    z = _tree(24, 0xF300, False)
    tips = _sites(24, 2, 5, 3, None)
    tips[tips == 0] = 1
    tips[:, 0], tips[:, 1] = 1, 2                                             # both states at the tips: a change is needed
    Qs = _models(2, 64, 5)
    Qs[17] = 0.0                                                              # q01 = q10 = 0
    got = api.loglik_models(z, Qs, [.5, .5], sites=tips)
    assert np.all(got[17] == -np.inf)
    assert np.all(np.isfinite(np.delete(got, 17, axis=0)))
    want = fitref.loglik_models(z["edge"], z["edge.length"], Qs, [.5, .5], tips)
    _bar(got, want)
    paired = api.loglik_models(z, Qs, [.5, .5], sites=tips, site_of_model=np.arange(64) % 5)
    assert paired[17] == -np.inf and np.all(np.isfinite(np.delete(paired, 17)))
    # all tips in one state: the same model is possible (P = I), and legal
    same = api.loglik_models(z, Qs[17:18], [.5, .5], sites=np.ones((1, 24), dtype=np.int32))
    assert same[0, 0] == pytest.approx(np.log(.5), rel=1e-15)


@pytest.mark.parametrize("n", [4, 8, 20])
def test_chunks_and_devices_do_not_change_a_bit(n):
    z = _tree(24, 0xF400 + n, True)
    K = 130 if n <= 8 else 3
    Qs = _models(n, K, 77 + n) if n <= 8 else _wide_models(n, K, 0xC0)
    pid = np.random.default_rng(n).uniform(0.1, 1.0, (K, n))
    tips = _sites(24, n, 5, 11, None)
    som = np.arange(K) % 5
    plain = api.loglik_models(z, Qs, pid, sites=tips)
    plain_p = api.loglik_models(z, Qs, pid, sites=tips, site_of_model=som)
    assert np.array_equal(api.loglik_models(z, Qs, pid, sites=tips, expect_chunk=64), plain)
    assert np.array_equal(api.loglik_models(z, Qs, pid, sites=tips, expect_chunk=2), plain)
    assert np.array_equal(api.loglik_models(z, Qs, pid, sites=tips, devices=[0, 0]), plain)
    assert np.array_equal(api.loglik_models(z, Qs, pid, sites=tips, site_of_model=som, expect_chunk=64), plain_p)
    assert np.array_equal(api.loglik_models(z, Qs, pid, sites=tips, site_of_model=som, devices=[0, 0]), plain_p)
    from phylomap_amd import _lib
    _lib.set_debug_options()


def _problem(which):
    import test_fit_cpu
    edge, lens, tips, m, pid, ll_want, th_want = test_fit_cpu.problem(which)
    z = {"edge": edge, "edge.length": lens, "Nnode": len(tips) - 1, "states": tips}
    return z, m, pid, ll_want, th_want


@pytest.mark.parametrize("which", [2, 3])
def test_fit_on_the_device_reaches_the_rehearsed_optimum(which):
    z, m, pid, ll_want, th_want = _problem(which)
    r = api.fit_ml(z, m, pid, gtol=GTOL)                                      # 8 starts
    print(f"n={which}: loglik {r['loglik']:.9f} theta {r['theta']} iterations {r['iterations']} calls {r['calls']}")
    assert r["converged"] and not np.any(r["at_bound"])
    assert abs(r["loglik"] - ll_want) <= 1e-8
    np.testing.assert_allclose(r["theta"], th_want, rtol=1e-5)
    stats, _ = api.expected_sumstat(z, r["Q"], pid)
    g = fitref.exact_score(m, r["theta"], stats[0])
    print(f"n={which}: max |exact score| at the optimum {np.max(np.abs(g)):.3g}")
    assert np.max(np.abs(g)) <= 10 * GTOL


def test_per_site_fits_and_the_calibration_of_the_likelihood_ratio():
    """128 datasets simulated under the truth, one fit each in lock-step.  LR_s = 2 (l_s(theta_hat_s) - l_s(theta_true)) is >= 0 and
    asymptotically chi^2_2: its mean lies within 2 +- 4 * 2 / sqrt(128) = [1.29, 2.71].  (CPU rehearsal on this very input with
    scipy's BFGS on the twin: mean 2.100, sd 2.43, no fit on a bound.)"""
    z, m, pid, _, _ = _problem(2)
    Q = np.array([[-.3, .3], [.6, -.6]])
    tips, _ = api.simulate_histories(z, Q, pid, 128, seed=5)
    r = api.fit_ml(z, m, pid, sites=tips, per_site=True, gtol=GTOL)
    assert r["theta"].shape == (128, 2) and r["loglik"].shape == (128,) and r["starts"]["loglik"].shape == (128, 8)
    for s in range(8):                                                        # the exact score at each site's own optimum
        stats, ll = api.expected_sumstat(z, r["Q"][s], pid, sites=tips[s:s + 1])
        g = fitref.exact_score(m, r["theta"][s], stats[0])
        print(f"site {s}: theta {r['theta'][s]} max |exact score| {np.max(np.abs(g)):.3g} converged {r['converged'][s]}")
        if not np.any(r["at_bound"][s]):
            assert np.max(np.abs(g)) <= 10 * GTOL
        assert abs(ll[0] - r["loglik"][s]) <= 1e-10 * abs(ll[0])
    truth = api.loglik_models(z, Q[None], pid, sites=tips)[0]
    LR = 2.0 * (r["loglik"] - truth)
    on_bound = np.any(r["at_bound"], axis=1)
    keep = ~on_bound
    print(f"LR over {int(keep.sum())} sites: mean {LR[keep].mean():.4f} sd {LR[keep].std(ddof=1):.3f} min {LR.min():.3g} "
          f"above 5.99: {int(np.sum(LR[keep] > 5.99))}; median theta {np.median(r['theta'][keep], axis=0)}; on a bound: "
          f"{int(on_bound.sum())}; converged {int(r['converged'].sum())} of 128")
    assert np.all(LR >= -1e-8)
    assert on_bound.sum() <= 2
    assert 1.29 <= LR[keep].mean() <= 2.71


def test_c3_tree_1024_models():
    z, Q, pid, _ = synth.config_problem(3)                                    # 10 000 tips, 4 states
    m = ratemodel.hidden_rates(1)
    rs = np.random.default_rng(0xC3)
    thetas = np.array([0.1, 0.1, 0.2, 0.2, 10.0]) * np.exp(rs.normal(0.0, 0.5, (1024, 5)))
    Qs = m.Qs(thetas)
    got = api.loglik_models(z, Qs, pid)
    assert got.shape == (1024, 1) and np.all(np.isfinite(got))
    for k in np.linspace(0, 1023, 16).astype(int):
        want = api.expected_sumstat(z, Qs[k], pid)[1]
        assert abs(got[k, 0] - want[0]) <= 1e-12 * max(1.0, abs(want[0])), (k, got[k, 0], want[0])


def test_squamate_aic_tool():
    sys.path.insert(0, os.path.join(ROOT, "tools", "squamate_dic"))
    import run_aic
    r = run_aic.run()
    two, four, z = r["ard2"], r["hidden_rates1"], r["tree"]
    print(f"squamate: ard(2) loglik {two['loglik']:.6f} aic {two['aic']:.6f} theta {two['theta']} iterations {two['iterations']} "
          f"calls {two['calls']}; hidden_rates(1) loglik {four['loglik']:.6f} aic {four['aic']:.6f} theta {four['theta']} "
          f"iterations {four['iterations']} calls {four['calls']} max |fd gradient| {np.max(np.abs(four['grad'])):.3g}; "
          f"{r['seconds']:.2f} s")
    assert two["converged"] and four["converged"]
    stats, _ = api.expected_sumstat(z, two["Q"], [.5, .5])
    g = fitref.exact_score(ratemodel.ard(2), two["theta"], stats[0])
    print(f"squamate: ard(2) max |exact score| {np.max(np.abs(g)):.3g}")
    assert np.max(np.abs(g)) <= 10 * GTOL
    assert np.all(np.isfinite(four["grad"]))
