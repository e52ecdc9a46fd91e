"""Rate models, the lock-step BFGS of phylomap_amd/fit.py on the Python twin of the batched likelihood (tests/fitref.py), the
C-ABI surface of phm_loglik_models without a device and the R layer's names.  No GPU needed.

The two optima below were obtained independently of fit.py: scipy's BFGS on the twin likelihood with the same central
differences (h = 1e-4, gtol = 1e-5), four random starts each, every start reaching the same optimum to 1e-7 relative."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import exactref
import fitref
from phylomap_amd import _lib, fit, ratemodel, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THETA3 = (.3, .1, .2, .4, .15, .25)
GTOL = 1e-5


def problem(which):
    """(edge, lens, tips, model, pid, loglik at the optimum, theta at the optimum) of the two rehearsed problems"""
    if which == 2:
        edge, lens = synth.random_tree(200, 0.4, 11)
        Q = np.array([[-.3, .3], [.6, -.6]])
        tips = synth.simulate_tips(edge, lens, Q, [.5, .5], 11)
        return edge, lens, tips, ratemodel.ard(2), [.5, .5], -119.600128570, (0.42786375, 0.61531944)
    edge, lens = synth.random_tree(300, 0.4, 12)
    m = ratemodel.ard(3)
    tips = synth.simulate_tips(edge, lens, m.Q(THETA3), np.full(3, 1 / 3), 12)
    return edge, lens, tips, m, np.full(3, 1 / 3), -240.874447490, (0.27831662, 0.17878944, 0.55368611, 0.25506050, 0.09571630,
                                                                   0.32299572)


def test_rate_models():
    Q = ratemodel.ard(3).Q(THETA3)
    assert np.array_equal(Q, np.array([[-.3 - .1, .3, .1], [.2, -.2 - .4, .4], [.15, .25, -.15 - .25]]))
    hr = ratemodel.hidden_rates(1)
    assert (hr.n, hr.p) == (4, 5)
    assert np.array_equal(hr.Q([.3, .2, .4, .5, 2.0]), synth.make2sQ(.3, .2, .4, .5, 2.0))
    hr2 = ratemodel.hidden_rates(2)
    assert (hr2.n, hr2.p) == (6, 8)
    assert np.array_equal(hr2.Q([.3, .2, .4, .1, .5, .6, 2.0, 3.0]), synth.make2sQ(.3, .2, [.4, .1], [.5, .6], [2.0, 3.0]))
    im = ratemodel.index_model([[0, 1, 0], [2, 0, 1], [0, 2, 0]])
    Qi = im.Q([.7, .2])
    assert im.p == 2 and Qi[0, 2] == 0.0 and Qi[2, 0] == 0.0 and Qi[0, 1] == .7 and Qi[1, 2] == .7 and Qi[1, 0] == .2
    assert ratemodel.er(4).p == 1 and ratemodel.sym(4).p == 6 and ratemodel.ard(4).p == 12
    S = ratemodel.sym(3).Q([.1, .2, .3])
    assert np.array_equal(S - np.diag(np.diag(S)), (S - np.diag(np.diag(S))).T)
    for m, th in ((ratemodel.ard(3), THETA3), (hr, [.3, .2, .4, .5, 2.0]), (im, [.7, .2]), (ratemodel.er(5), [.4])):
        assert np.max(np.abs(m.Q(th).sum(axis=1))) < 1e-15
        many = m.Qs(np.array([th, th]) * np.array([[1.0], [2.0]]))
        assert np.array_equal(many[0], m.Q(th)) and np.array_equal(many[1], m.Q(np.array(th) * 2.0))
    with pytest.raises(ValueError):
        ratemodel.index_model([[0, 1], [3, 0]])                               # parameter 2 is missing
    # d Q / d log theta of a function model (central difference) against the closed form
    d = hr.dQ_dlog([.3, .2, .4, .5, 2.0])
    assert abs(d[0][0, 1] - .3) < 1e-9 and abs(d[0][2, 3] - 2.0 * .3) < 1e-9 and abs(d[4][3, 2] - 2.0 * .2) < 1e-9


@pytest.mark.parametrize("which", [2, 3])
def test_fit_reaches_the_rehearsed_optimum_and_the_exact_score_vanishes(which):
    edge, lens, tips, m, pid, ll_want, th_want = problem(which)
    if which == 2:
        assert list(np.bincount(tips, minlength=3)) == [0, 99, 101]
    r = fit.first_problem(fit.fit(fitref.batch(edge, lens, pid, tips), m, 1, len(tips) / lens.sum(), starts=2, seed=0, gtol=GTOL))
    print(f"n={which}: loglik {r['loglik']:.9f} theta {r['theta']} iterations {r['iterations']} calls {r['calls']}")
    assert r["converged"] and not np.any(r["at_bound"])
    assert abs(r["loglik"] - ll_want) <= 1e-8
    np.testing.assert_allclose(r["theta"], th_want, rtol=1e-5)
    assert r["aic"] == 2 * m.p - 2 * r["loglik"]
    np.testing.assert_allclose(r["starts"]["loglik"], ll_want, atol=1e-7)     # both starts: the surface has one mode
    # the check no fit code produced: the exact score in log theta from the conditional expectations
    stats, _ = exactref.expected(edge, lens, r["Q"], pid, tips)
    g = fitref.exact_score(m, r["theta"], stats[0])
    print(f"n={which}: max |exact score| {np.max(np.abs(g)):.3g}, finite-difference gradient {np.max(np.abs(r['grad'])):.3g}")
    assert np.max(np.abs(g)) <= 10 * GTOL


def test_all_tips_in_one_state_ends_on_the_lower_bound():
    edge, lens = synth.random_tree(40, 0.4, 5)
    tips = np.ones(40, dtype=np.int32)
    rate0 = 40 / lens.sum()
    like = fitref.batch(edge, lens, [.5, .5], tips)
    r = fit.first_problem(fit.fit(like, ratemodel.er(2), 1, rate0, starts=1, max_iter=80))          # the default box
    assert np.isfinite(r["loglik"]) and r["at_bound"][0] and r["converged"]
    assert r["theta"][0] == pytest.approx(fit.DEFAULT_BOUNDS[0] * rate0, rel=1e-12)
    r = fit.first_problem(fit.fit(like, ratemodel.ard(2), 1, rate0, starts=1, max_iter=80, bounds=(1e-3, 10.0)))
    assert np.isfinite(r["loglik"]) and list(r["at_bound"]) == [True, True]    # q01 -> 0: lower; q10 -> infinity: upper
    np.testing.assert_allclose(r["theta"], [1e-3, 10.0], rtol=1e-12)
    # In the default box the two-rate surface goes flat (q10 large makes q01 unobservable) before either bound is reached: the
    # fit stops on its gradient with log l ~ 0, and at_bound says exactly which rates sit on a bound: none
    r = fit.first_problem(fit.fit(like, ratemodel.ard(2), 1, rate0, starts=1, max_iter=80))
    assert r["loglik"] > -1e-4 and np.all(np.isfinite(r["theta"]))
    lo, hi = fit.DEFAULT_BOUNDS[0] * rate0, fit.DEFAULT_BOUNDS[1] * rate0
    assert list(r["at_bound"]) == [bool(t <= lo * (1 + 1e-9) or t >= hi * (1 - 1e-9)) for t in r["theta"]]


def test_an_impossible_start_is_dropped_and_a_seed_reproduces():
    edge, lens = synth.random_tree(30, 0.4, 7)
    Q = np.array([[-.3, .3], [.6, -.6]])
    tips = synth.simulate_tips(edge, lens, Q, [.5, .5], 7)
    assert len(set(tips)) == 2
    m = ratemodel.ard(2)
    ref = fitref.batch(edge, lens, [.5, .5], tips)
    rate0 = 30 / lens.sum()
    x0 = fit.start_points(2, rate0, 3, 4, -np.inf, np.inf)

    def batch(Qs, owner):                                                     # start 1 cannot produce the tips
        v = ref(Qs, owner)
        first = np.all(np.isclose(np.log(np.stack([Qs[:, 0, 1], Qs[:, 1, 0]], axis=1)), x0[1], atol=1e-12), axis=1)
        return np.where(first, -np.inf, v)

    r = fit.first_problem(fit.fit(batch, m, 1, rate0, starts=3, seed=4))
    assert r["starts"]["loglik"][1] == -np.inf and np.all(np.isfinite(r["starts"]["loglik"][[0, 2]]))
    assert np.isfinite(r["loglik"]) and np.all(np.isfinite(r["theta"])) and np.all(np.isfinite(r["grad"])) and r["converged"]
    r2 = fit.first_problem(fit.fit(batch, m, 1, rate0, starts=3, seed=4))
    for k in ("theta", "loglik", "grad", "Q"):
        assert np.array_equal(r[k], r2[k])
    assert np.array_equal(r["starts"]["theta"], r2["starts"]["theta"])
    # a model that can never produce the tips: every start dropped, -inf reported, nothing is NaN
    never = ratemodel.index_model([[0, 0], [1, 0]])                           # state 1 is never left, the root prior is all on it
    r3 = fit.first_problem(fit.fit(fitref.batch(edge, lens, [1.0, 0.0], tips), never, 1, rate0, starts=2))
    assert r3["loglik"] == -np.inf and not r3["converged"] and np.all(np.isfinite(r3["theta"]))
    # per-problem lock-step: two copies of the same problem give the same answer as one
    two = fit.fit(fitref.batch(edge, lens, [.5, .5], np.stack([tips, tips]), per_site=True), m, 2, rate0, starts=1)
    one = fit.fit(ref, m, 1, rate0, starts=1)
    assert np.array_equal(two["theta"][0], one["theta"][0]) and np.array_equal(two["theta"][1], one["theta"][0])


def _raw(z, Qs, pid, n_pid=None, S=2, observe=None, som=None, out=True, tree=True, q=True):
    Qs = np.asarray(Qs, dtype=np.float64)
    K, n = Qs.shape[0], Qs.shape[1]
    Qf = np.ascontiguousarray(Qs.transpose(0, 2, 1))
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    pt = _lib.PlainTree(z, np.tile(z["states"], (S, 1)))
    t = pt.c
    obs = None if observe is None else np.ascontiguousarray(observe, dtype=np.int32)
    so = None if som is None else np.ascontiguousarray(som, dtype=np.int32)
    o = _lib.make_options(n_replicas=S, tips_per_replica=True)
    res = np.zeros(K * S) if out else None
    L = _lib.load()
    status = L.phm_loglik_models(C.byref(t) if tree else None, n, K, _lib._p(Qf, C.c_double) if q else None, _lib._p(pid, C.c_double),
                                 pid.size // n if n_pid is None else n_pid, _lib._p(obs, C.c_int32), _lib._p(so, C.c_int32),
                                 C.byref(o), _lib._p(res, C.c_double))
    return status, L.phm_last_error().decode()


def test_c_abi_checks_need_no_device():
    L = _lib.load()
    assert "phm_loglik_models" in _lib.EXPORTS and hasattr(L, "phm_loglik_models")
    assert L.phm_version() == 300
    assert [L.phm_struct_size(k) for k in range(5)] == [C.sizeof(s) for s in (_lib.Options, _lib.Info, _lib.Tree, _lib.Model,
                                                                            _lib.DebugOptions)]
    assert [L.phm_struct_size(k) for k in range(5)] == [112, 88, 64, 48, 48]
    z, Q, pid, _ = synth.config_problem(2, n_tips=16)
    Qs = np.stack([Q, 2 * Q, 3 * Q])
    assert _raw(z, Qs, pid, out=False)[0] == 1
    assert _raw(z, Qs, pid, tree=False)[0] == 1
    assert _raw(z, Qs, pid, q=False)[0] == 1
    assert _raw(z, Qs, np.tile(pid, 2))[0] == 1                               # n_pid = 2 with K = 3
    assert _raw(z, Qs, pid, n_pid=0)[0] == 1
    assert _raw(z, Qs, pid, som=[0, 1, 2])[0] == 1                            # S = 2
    assert _raw(z, Qs, pid, som=[0, -1, 1])[0] == 1
    assert _raw(z, Qs, pid, observe=[1, 2, 1, 5])[0] == 1
    bad = Qs.copy()
    bad[2, 0, 3], bad[2, 0, 1] = -0.05, bad[2, 0, 1] + 0.05                  # a negative rate in model 2
    st, msg = _raw(z, bad, pid)
    assert st == 1 and "model 2" in msg
    bad = Qs.copy()
    bad[1, 2, 2] = np.nan
    st, msg = _raw(z, bad, pid)
    assert st == 1 and "model 1" in msg
    st, msg = _raw(z, Qs, np.stack([pid, pid, -pid]))
    assert st == 5 and "2" in msg
    if L.phm_device_count() == 0:                                              # a valid call gets as far as the device
        zero = np.stack([Q, np.zeros((4, 4))])                                 # a model that leaves no state is legal here
        assert _raw(z, zero, pid)[0] == 3
        zl = dict(z, **{"edge.length": z["edge.length"] * 1e9})               # and there is no limit on max(-q_ii) t_b
        assert _raw(zl, Qs, pid)[0] == 3


def test_r_layer_names_the_exported_call_symbol():
    src = open(os.path.join(ROOT, "shim", "phylomap_loglik_shim.cpp")).read()
    exported = set(re.findall(r"RcppExport SEXP (phylomap_\w+)\(", src))
    assert exported == {"phylomap_loglik_models"}
    rfile = open(os.path.join(ROOT, "shim", "R", "phylomap_fit.R")).read()
    assert set(re.findall(r"\.Call\('(\w+)'", rfile)) == exported
    assert re.search(r"^sumstatLoglik <- function\(", rfile, re.M)
    assert "phylomap_loglik_models" not in open(os.path.join(ROOT, "shim", "phylomap_shim.cpp")).read()
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "tests", "mock_rcpp"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "shim", "phylomap_loglik_shim.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
