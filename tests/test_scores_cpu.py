"""The exact score, the exact-gradient fit, the observed information and the standard errors of phylomap_amd/fit.py on the Python
twin of the batched statistics (``exactref.expected`` per model, wrapped as a ``batch_stats`` callable), the C-ABI surface of
phm_expected_stats_models without a device and the R layer's names.  No GPU needed."""
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
from test_fit_cpu import THETA3, problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def one_blas_thread():
    """the twin multiplies n x n matrices thousands of times: a BLAS thread pool only gets in its way"""
    try:
        import threadpoolctl
    except ImportError:
        yield
        return
    with threadpoolctl.threadpool_limits(limits=1):
        yield


def twin_stats(edge, lens, pid, tips, observe=None, per_site=False, counter=None):
    """the callable ``fit.fit(gradient="exact")`` takes: (loglik [K], stats [K, cols]), joint over the sites (summed) or one
    problem per site.  ``counter`` (a list) collects the number of models of every call."""
    tips = np.atleast_2d(np.asarray(tips))

    def f(Qs, owner):
        if counter is not None:
            counter.append(len(Qs))
        ll, st = [], []
        for k in range(len(Qs)):
            y = tips[int(owner[k])][None] if per_site else tips
            with np.errstate(divide="ignore", invalid="ignore"):
                s, l = exactref.expected(edge, lens, Qs[k], pid, y, observe)
            ll.append(l.sum())
            st.append(s.sum(axis=0))
        return np.array(ll), np.array(st)
    return f


def counted(batch, counter):
    def f(Qs, owner):
        counter.append(len(Qs))
        return batch(Qs, owner)
    return f


@pytest.mark.parametrize("name", ["er", "sym", "ard", "index_model", "hidden_rates"])
def test_score_is_fitrefs_formula_and_the_derivative_of_the_twins_loglik(name):
    m, th, observe = {
        "er": (ratemodel.er(3), [.3], None),
        "sym": (ratemodel.sym(3), [.2, .5, .3], None),
        "ard": (ratemodel.ard(3), THETA3, None),
        "index_model": (ratemodel.index_model([[0, 1, 0], [2, 0, 1], [0, 2, 0]]), [.7, .2], None),
        "hidden_rates": (ratemodel.hidden_rates(1), [.3, .2, .4, .5, 2.0], (1, 2, 1, 2)),
    }[name]
    th = np.array(th)
    edge, lens = synth.random_tree(30, 0.4, 21)
    top = m.n if observe is None else 2
    tips = np.random.default_rng(3).integers(1, top + 1, (2, 30))
    pid = np.arange(1.0, m.n + 1.0)
    stats, _ = exactref.expected(edge, lens, m.Q(th), pid, tips, observe)
    stats = stats.sum(axis=0)
    g = m.score(th, stats)
    want = fitref.exact_score(m, th, stats)
    np.testing.assert_allclose(g, want, rtol=1e-12, atol=1e-13)
    h = 1e-4                                                                  # central differences of the twin's log l
    like = fitref.batch(edge, lens, pid, tips, observe)
    pts = np.repeat(np.log(th)[None], 2 * m.p, axis=0)
    for c in range(m.p):
        pts[2 * c, c] += h
        pts[2 * c + 1, c] -= h
    v = like(m.Qs(np.exp(pts)), np.zeros(2 * m.p, dtype=np.int32))
    fd = (v[0::2] - v[1::2]) / (2 * h)
    print(f"{name}: score {g}, max |score - central difference| {np.max(np.abs(g - fd)):.3g}")
    assert np.max(np.abs(g - fd)) <= 1e-6


@pytest.fixture(scope="module")
def fits():
    """both modes on the two rehearsed problems, one start each, computed once: which -> (fd result, fd model counts, exact result, exact counts)"""
    out = {}
    for which in (2, 3):
        edge, lens, tips, m, pid, _, _ = problem(which)
        rate0 = len(tips) / lens.sum()
        c_fd, c_ex = [], []
        fd = fit.first_problem(fit.fit(counted(fitref.batch(edge, lens, pid, tips), c_fd), m, 1, rate0, starts=1, seed=0, gtol=1e-5))
        ex = fit.first_problem(fit.fit(None, m, 1, rate0, starts=1, seed=0, gtol=1e-8, gradient="exact",
                                       batch_stats=twin_stats(edge, lens, pid, tips, counter=c_ex)))
        out[which] = (fd, c_fd, ex, c_ex)
    return out


@pytest.mark.parametrize("which", [2, 3])
def test_exact_gradient_reaches_the_rehearsed_optimum_with_fewer_evaluations(which, fits):
    edge, lens, tips, m, pid, ll_want, th_want = problem(which)
    fd, c_fd, ex, c_ex = fits[which]
    print(f"n={which}: exact: loglik {ex['loglik']:.9f} theta {ex['theta']} iterations {ex['iterations']} calls {ex['calls']} "
          f"evaluations {ex['evals']}; fd: iterations {fd['iterations']} calls {fd['calls']} evaluations {fd['evals']}")
    assert ex["converged"] and not np.any(ex["at_bound"])                    # at gtol = 1e-8
    assert abs(ex["loglik"] - ll_want) <= 1e-8
    np.testing.assert_allclose(ex["theta"], th_want, rtol=1e-5)
    assert ex["evals"] == sum(c_ex) and fd["evals"] == sum(c_fd) and ex["calls"] == len(c_ex)
    assert ex["evals"] < fd["evals"]
    # gtol = 1e-8 is honoured: `grad` is the exact score at the optimum, and an independent evaluation of it agrees
    stats, _ = exactref.expected(edge, lens, ex["Q"], pid, tips)
    g = fitref.exact_score(m, ex["theta"], stats[0])
    np.testing.assert_allclose(ex["grad"], g, rtol=0, atol=1e-11)
    assert np.max(np.abs(g)) <= 1e-8
    # which the difference gradient cannot honour: the exact score where "fd" stopped, converged by its own measure
    stats, _ = exactref.expected(edge, lens, fd["Q"], pid, tips)
    g_fd = fitref.exact_score(m, fd["theta"], stats[0])
    print(f"n={which}: max |exact score|: exact mode {np.max(np.abs(g)):.3g}, fd mode {np.max(np.abs(g_fd)):.3g} "
          f"(its own gradient {np.max(np.abs(fd['grad'])):.3g})")
    assert fd["converged"] and np.max(np.abs(g_fd)) > 1e-8


def test_fd_is_unchanged_by_the_new_arguments(fits):
    edge, lens, tips, m, pid, _, _ = problem(2)
    rate0 = len(tips) / lens.sum()
    like = fitref.batch(edge, lens, pid, tips)
    a = fit.fit(like, m, 1, rate0, starts=1, seed=0, gtol=1e-5)
    b = fit.fit(like, m, 1, rate0, starts=1, seed=0, gtol=1e-5, gradient="fd", batch_stats=twin_stats(edge, lens, pid, tips))
    for k in ("theta", "Q", "loglik", "aic", "iterations", "converged", "at_bound", "grad"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k][0], fits[2][0][k])
    assert np.array_equal(a["starts"]["theta"], b["starts"]["theta"]) and np.array_equal(a["starts"]["loglik"], b["starts"]["loglik"])
    assert a["calls"] == b["calls"] and a["evals"] == b["evals"]
    with pytest.raises(ValueError):
        fit.fit(like, m, 1, rate0, gradient="exact")                          # no batch_stats
    with pytest.raises(ValueError):
        fit.fit(like, m, 1, rate0, gradient="newton")


@pytest.mark.parametrize("which", [2, 3])
def test_information_against_second_differences_of_the_twins_loglik(which, fits):
    edge, lens, tips, m, pid, _, _ = problem(which)
    ex = fits[which][2]
    p = m.p
    calls = []
    J = fit.information(twin_stats(edge, lens, pid, tips, counter=calls), m, ex["theta"], [0])
    assert J.shape == (p, p) and np.array_equal(J, J.T) and calls == [2 * p]  # one call of 2p models
    h = 1e-3                                                                  # second differences of log l in log theta
    like = fitref.batch(edge, lens, pid, tips)
    x = np.log(ex["theta"])
    pts, where = [x.copy()], {}
    for a in range(p):
        for b in range(a, p):
            for sa, sb in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                y = x.copy()
                y[a] += sa * h
                y[b] += sb * h
                where[(a, b, sa, sb)] = len(pts)
                pts.append(y)
    v = like(m.Qs(np.exp(np.array(pts))), np.zeros(len(pts), dtype=np.int32))
    H = np.zeros((p, p))
    for a in range(p):
        for b in range(a, p):
            d = v[where[(a, b, 1, 1)]] - v[where[(a, b, 1, -1)]] - v[where[(a, b, -1, 1)]] + v[where[(a, b, -1, -1)]]
            H[a, b] = H[b, a] = -d / (4 * h * h)                              # a == b: steps of 2h
    worst = np.max(np.abs(J - H)) / np.max(np.abs(H))
    print(f"n={which}: information, largest entry {np.max(np.abs(H)):.6g}, max |score route - second differences| / largest "
          f"{worst:.3g}; eigenvalues {np.linalg.eigvalsh(J)}")
    assert worst <= 1e-4
    r = fit.standard_errors(twin_stats(edge, lens, pid, tips), m, ex["theta"][None], [0], ex["at_bound"][None])
    assert r["se_ok"][0] and np.all(np.isfinite(r["se_log"])) and np.all(r["se_log"] > 0)
    np.testing.assert_allclose(r["cov_log"][0], np.linalg.inv(J), rtol=1e-12)
    np.testing.assert_allclose(r["ci"][0, :, 0], ex["theta"] * np.exp(-1.96 * r["se_log"][0]), rtol=1e-15)
    np.testing.assert_allclose(r["ci"][0, :, 1], ex["theta"] * np.exp(1.96 * r["se_log"][0]), rtol=1e-15)


def test_standard_errors_on_a_bound_and_along_a_flat_direction():
    edge, lens = synth.random_tree(30, 0.4, 7)
    Q = np.array([[-.3, .3], [.6, -.6]])
    tips = synth.simulate_tips(edge, lens, Q, [.5, .5], 7)
    m = ratemodel.ard(2)
    rate0 = 30 / lens.sum()
    bs = twin_stats(edge, lens, [.5, .5], tips)
    # q10 held at an upper bound below its optimum: its entries are NaN, q01 gets the se of the one-parameter problem
    r = fit.fit(None, m, 1, rate0, starts=1, gradient="exact", batch_stats=bs, bounds=([1e-4, 1e-4], [10.0, 0.05]))
    assert list(r["at_bound"][0]) == [False, True] and r["converged"][0]
    s = fit.standard_errors(bs, m, r["theta"], [0], r["at_bound"])
    assert s["se_ok"][0] and np.isfinite(s["se_log"][0, 0]) and np.isnan(s["se_log"][0, 1])
    assert np.all(np.isnan(s["cov_log"][0][1])) and np.all(np.isnan(s["cov_log"][0][:, 1])) and np.all(np.isnan(s["ci"][0, 1]))
    assert s["cov_log"][0, 0, 0] == pytest.approx(1.0 / s["information"][0, 0, 0], rel=1e-12)
    assert s["ci"][0, 0, 0] < r["theta"][0, 0] < s["ci"][0, 0, 1]
    # all tips in one state: the two-rate surface is flat where the fit stops (test_fit_cpu.py), no interval is reported
    ones = np.ones(40, dtype=np.int32)
    edge, lens = synth.random_tree(40, 0.4, 5)
    bs = twin_stats(edge, lens, [.5, .5], ones)
    r = fit.fit(fitref.batch(edge, lens, [.5, .5], ones), m, 1, 40 / lens.sum(), starts=1, max_iter=80)
    assert not np.any(r["at_bound"])
    s = fit.standard_errors(bs, m, r["theta"], [0], r["at_bound"])
    print(f"flat: information {s['information'][0].tolist()}")
    assert not s["se_ok"][0] and np.all(np.isnan(s["se_log"])) and np.all(np.isnan(s["cov_log"])) and np.all(np.isnan(s["ci"]))


def _raw(z, Qs, pid, n_pid=None, S=2, observe=None, som=None, stats=True, ll=True, tree=True, q=True):
    Qs = np.asarray(Qs, dtype=np.float64)
    K, n = Qs.shape[0], Qs.shape[1]
    Qf = np.ascontiguousarray(Qs.transpose(0, 2, 1))
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    pt = _lib.PlainTree(z, np.tile(z["states"], (S, 1)))
    t = pt.c
    obs = None if observe is None else np.ascontiguousarray(observe, dtype=np.int32)
    so = None if som is None else np.ascontiguousarray(som, dtype=np.int32)
    o = _lib.make_options(n_replicas=S, tips_per_replica=True)
    res = np.zeros(K * S * n * n) if stats else None
    lik = np.zeros(K * S) if ll else None
    L = _lib.load()
    status = L.phm_expected_stats_models(C.byref(t) if tree else None, n, K, _lib._p(Qf, C.c_double) if q else None,
                                         _lib._p(pid, C.c_double), pid.size // n if n_pid is None else n_pid, _lib._p(obs, C.c_int32),
                                         _lib._p(so, C.c_int32), C.byref(o), _lib._p(res, C.c_double), _lib._p(lik, C.c_double))
    return status, L.phm_last_error().decode()


def test_c_abi_checks_need_no_device():
    L = _lib.load()
    assert "phm_expected_stats_models" in _lib.EXPORTS and hasattr(L, "phm_expected_stats_models")
    assert L.phm_version() == 300
    z, Q, pid, _ = synth.config_problem(2, n_tips=16)
    Qs = np.stack([Q, 2 * Q, 3 * Q])
    assert _raw(z, Qs, pid, stats=False)[0] == 1
    assert _raw(z, Qs, pid, ll=False)[0] == 1
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
    assert st == 1 and "model 2" in msg and msg.startswith("model 2")
    st, msg = _raw(z, Qs, np.stack([pid, pid, -pid]))
    assert st == 5 and "2" in msg
    zl = dict(z, **{"edge.length": z["edge.length"] * 1e9})                   # the branch stage runs ~ mu t_b steps: limited
    st, msg = _raw(zl, Qs, pid)
    assert st == 2 and "model 0" in msg and "1e6" in msg
    if L.phm_device_count() == 0:                                              # a valid call gets as far as the device
        zero = np.stack([Q, np.zeros((4, 4))])                                 # a model that leaves no state is legal here
        assert _raw(z, zero, pid)[0] == 3
        assert _raw(z, Qs, pid, som=[0, 1, 1])[0] == 3


def test_r_layer_names_the_exported_call_symbol():
    src = open(os.path.join(ROOT, "shim", "phylomap_scores_shim.cpp")).read()
    exported = set(re.findall(r"RcppExport SEXP (phylomap_\w+)\(", src))
    assert exported == {"phylomap_expected_stats_models"}
    rfile = open(os.path.join(ROOT, "shim", "R", "phylomap_scores.R")).read()
    assert set(re.findall(r"\.Call\('(\w+)'", rfile)) == exported
    assert re.search(r"^sumstatExpectedModels <- function\(tree, Qs, pid, sites = NULL, observe = NULL, site_of_model = NULL\)", rfile,
                     re.M)
    for other in ("phylomap_shim.cpp", "phylomap_loglik_shim.cpp"):
        assert "phylomap_expected_stats_models" not in open(os.path.join(ROOT, "shim", other)).read()
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "tests", "mock_rcpp"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "shim", "phylomap_scores_shim.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
