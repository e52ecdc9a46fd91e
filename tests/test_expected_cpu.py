"""Exact conditional expectations (phm_expected_stats): the Python twin's two routes against each other and against
independent facts (a derivative of log p, the unconditional closed forms, a plain Felsenstein pass), the C-ABI surface without a
device, and the R layer's names.  No GPU needed."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import exactref
import simref
from phylomap_amd import _lib, api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(n):
    if n == 2:
        return np.array([[-0.6, 0.6], [0.9, -0.9]])
    if n == 3:
        return np.array([[-0.5, 0.3, 0.2], [0.1, -0.4, 0.3], [0.6, 0.0, -0.6]])
    if n == 4:
        return synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0)
    return synth.dense_Q(n, 0.05, 0.2)


def _tips(T, n, S, seed):
    return np.random.default_rng(seed).integers(0, n + 1, (S, T))


def test_poisson_truncation():
    for x in (0.0, 1e-3, 0.7, 13.0, 2280.0):
        p, M = exactref.poisson_weights(x)
        assert p.size == M + 2
        kept = p.sum()
        assert 1.0 - kept <= 2.0 ** -60 + 1e-15
        if x > 0:
            k = np.arange(M + 2)
            want = np.exp(-x + k * math.log(x) - np.array([math.lgamma(i + 1) for i in k]))
            big = want > 1e-25 * want.max()                  # far below the mode the twin keeps 0 (< 1e-30)
            np.testing.assert_allclose(p[big], want[big], rtol=1e-9)
    assert exactref.poisson_weights(2280.0)[1] > 2280


@pytest.mark.parametrize("n,T", [(2, 5), (3, 17), (4, 60), (8, 30)])
def test_van_loan_and_uniformization_routes_agree(n, T):
    Q = _model(n)
    edge, lens = synth.random_tree(T, 1.0, 0xE0 + n)
    pid = np.arange(1.0, n + 1.0)
    tips = _tips(T, n, 6, n)
    a = exactref.expected(edge, lens, Q, pid, tips, per_branch=True)
    b = exactref.expected(edge, lens, Q, pid, tips, route="vanloan", per_branch=True)
    scale = np.max(np.abs(b[0]))
    for x, y in ((a[0], b[0]), (a[2], b[2])):
        assert np.all(np.abs(x - y) <= 1e-10 * np.abs(y) + 1e-14 * scale)
    assert np.array_equal(a[1], b[1])


def test_counts_minus_dwell_are_the_gradient_of_the_loglik():
    """d log p / d q_ij (q_ii = -sum of the row, moving with it) = E[N_ij] / q_ij - E[dwell_i]"""
    n = 3
    Q = _model(3)
    edge, lens = synth.random_tree(25, 1.0, 77)
    tips = _tips(25, n, 2, 5)
    st, _ = exactref.expected(edge, lens, Q, np.ones(n), tips)
    for k, (i, j) in enumerate(exactref.columns(n)):
        if Q[i, j] == 0.0:
            continue
        h = 1e-5 * Q[i, j]
        lp = []
        for d in (h, -h):
            Qd = Q.copy()
            Qd[i, j] += d
            Qd[i, i] -= d
            lp.append(exactref.passes(edge, lens, Qd, np.ones(n), tips)["loglik"])
        grad = (lp[0] - lp[1]) / (2 * h)
        want = st[:, n + k] / Q[i, j] - st[:, i]
        np.testing.assert_allclose(want, grad, rtol=1e-6)


def test_all_tips_missing_gives_the_unconditional_expectations():
    n = 4
    Q = _model(4)
    edge, lens = synth.random_tree(30, 1.0, 3)
    pid = np.array([1.0, 2.0, 3.0, 4.0])
    st, ll = exactref.expected(edge, lens, Q, pid, np.zeros((1, 30), dtype=int))
    dwell, counts, _ = simref.expectations(edge, lens, Q, pid)
    np.testing.assert_allclose(st[0, :n], dwell, rtol=1e-12)
    np.testing.assert_allclose(st[0, n:], [counts[i, j] for i, j in exactref.columns(n)], rtol=1e-12, atol=1e-15)
    assert abs(ll[0]) < 1e-13


@pytest.mark.parametrize("n", [2, 4, 8])
def test_branch_dwell_node_posteriors_and_loglik(n):
    Q = _model(n)
    edge, lens = synth.random_tree(20, 1.0, 11 + n)
    pid = np.ones(n)
    tips = _tips(20, n, 4, 2 * n)
    observe = None if n != 4 else [1, 2, 1, 2]
    if observe is not None:
        tips = np.minimum(tips, 2)
    st, ll, br, post = exactref.expected(edge, lens, Q, pid, tips, observe=observe, per_branch=True, nodes=True)
    np.testing.assert_allclose(br[:, :, :n].sum(axis=2), np.broadcast_to(lens, (4, lens.size)), rtol=1e-12)
    np.testing.assert_allclose(post.sum(axis=2), 1.0, rtol=0, atol=1e-13)
    np.testing.assert_allclose(ll, exactref.felsenstein_loglik(edge, lens, Q, pid, tips, observe=observe), rtol=1e-12)
    np.testing.assert_allclose(br.sum(axis=1), st, rtol=1e-12)
    T = 20                                                     # observed tips: their posterior is the observation
    for s in range(4):
        for t in range(T):
            if tips[s, t] and observe is None:
                assert post[s, t, tips[s, t] - 1] == 1.0


def _raw_call(z, Q, pid, observe=None, S=2, stats=True, loglik=True, tips=None, **opt):
    Qf = np.asfortranarray(np.asarray(Q, dtype=np.float64))
    n = Qf.shape[0]
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    pt = _lib.PlainTree(z, np.tile(z["states"], (S, 1)) if tips is None else tips)
    tree = pt.c
    obs = None if observe is None else np.ascontiguousarray(observe, dtype=np.int32)
    o = _lib.make_options(n_replicas=S, tips_per_replica=True, **opt)
    s = np.zeros((S, n * n)) if stats else None
    ll = np.zeros(S) if loglik else None
    return _lib.load().phm_expected_stats(C.byref(tree), n, _lib._p(Qf, C.c_double), _lib._p(pid, C.c_double),
                                          _lib._p(obs, C.c_int32), C.byref(o), _lib._p(s, C.c_double), _lib._p(ll, C.c_double),
                                          None, None)


def test_symbol_exported_and_no_device_status():
    L = _lib.load()
    assert "phm_expected_stats" in _lib.EXPORTS and hasattr(L, "phm_expected_stats")
    if L.phm_device_count() > 0:
        pytest.skip("GPU present")
    z, Q, pid, _ = synth.config_problem(2, n_tips=16)
    assert _raw_call(z, Q, pid) == 3                                           # PHM_ERR_NO_DEVICE
    with pytest.raises(_lib.PhmError) as e:
        api.expected_sumstat(z, Q, pid, sites=np.ones((3, 16)), per_branch=True, nodes=True)
    assert e.value.status == 3


def test_input_validation_happens_before_the_device():
    z, Q, pid, _ = synth.config_problem(2, n_tips=16)
    assert _raw_call(z, Q, pid, observe=[1, 2, 1, 5]) == 1                    # observe out of range
    assert _raw_call(z, Q, np.zeros(4)) == 5                                   # PHM_ERR_ZERO_PROB
    assert _raw_call(z, Q, [0.5, -0.1, 0.3, 0.3]) == 5
    assert _raw_call(z, Q, pid, reduce=True) == 1
    assert _raw_call(z, Q, pid, stats=False) == 1                              # NULL output
    assert _raw_call(z, Q, pid, loglik=False) == 1
    bad = np.tile(z["states"], (2, 1))
    bad[1, 3] = 5                                                              # tip state out of 0..n
    assert _raw_call(z, Q, pid, tips=bad) == 1
    bad[1, 3] = -1
    assert _raw_call(z, Q, pid, tips=bad) == 1
    Qb = Q.copy()
    Qb[0, 1] -= 0.01                                                           # row does not sum to 0
    assert _raw_call(z, Qb, pid) == 1
    Qb = Q.copy()
    Qb[0, 3], Qb[0, 1] = -0.05, Qb[0, 1] + 0.05                               # negative off-diagonal
    assert _raw_call(z, Qb, pid) == 1
    Qb = Q.copy()
    Qb[2, 2] = np.nan
    assert _raw_call(z, Qb, pid) == 1
    assert _raw_call(z, np.zeros((4, 4)), pid) == 1                            # mu = 0
    zb = dict(z, **{"edge.length": z["edge.length"].copy()})
    zb["edge.length"][3] = -1.0
    assert _raw_call(zb, Q, pid) == 1
    zb["edge.length"][3] = 1e9                                                 # mu t_b above 1e6
    assert _raw_call(zb, Q, pid) == 2
    assert _raw_call(z, np.zeros((1, 1)), [1.0]) == 1                          # n < 2
    Q65 = synth.dense_Q(65, 0.01, 0.02)
    assert _raw_call(z, Q65, np.ones(65)) == 1                                 # n > 64
    ze = dict(z, edge=np.asarray(z["edge"]).copy())
    ze["edge"][0, 0] = ze["edge"][2, 0] if ze["edge"][2, 0] != ze["edge"][0, 0] else ze["edge"][4, 0]
    assert _raw_call(ze, Q, pid) == 1                                          # not strictly bifurcating


def test_r_wrapper_names_the_exported_call_symbol():
    src = open(os.path.join(ROOT, "shim", "phylomap_expected_shim.cpp")).read()
    exported = set(re.findall(r"RcppExport SEXP (phylomap_\w+)\(", src))
    assert exported == {"phylomap_expected_stats"}
    rfile = open(os.path.join(ROOT, "shim", "R", "phylomap_expected.R")).read()
    assert set(re.findall(r"\.Call\('(\w+)'", rfile)) == exported
    assert re.search(r"^sumstatExpected <- function\(", rfile, re.M)
    shim = open(os.path.join(ROOT, "shim", "phylomap_shim.cpp")).read()
    assert "phylomap_expected_stats" not in shim
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "tests", "mock_rcpp"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "shim", "phylomap_expected_shim.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
