"""Forward simulation of character histories (phm_simulate_histories): the Python twin against closed-form expectations, the
C-ABI surface without a device, and the R layer's names.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pyref
import simref
from phylomap_amd import _lib, api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(n):
    if n == 2:
        return np.array([[-0.6, 0.6], [0.9, -0.9]])
    if n == 4:
        return synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0)
    return synth.dense_Q(n, 0.02, 0.08)


def test_twin_building_blocks_match_pyref():
    rs = np.random.default_rng(5)
    k = rs.integers(0, 2 ** 32, 2000, dtype=np.uint64)
    k[:3] = [0, 2 ** 32 - 1, 2 ** 32 - 2]
    got = simref.neglog_v(k)
    want = np.array([pyref.neglog_u32(int(v)) for v in k])
    assert np.array_equal(got, want)
    reps = np.arange(50, dtype=np.uint64) * np.uint64(7919)
    for d in (0, 1, 6, 4099):
        w = simref.word(0x1234_5678_9ABC, d, (1 << 30) | 17, reps)
        want = [pyref.philox((d >> 2, (1 << 30) | 17, simref.SIM_ITER, int(r)), (0x56789ABC, 0x1234))[d & 3] for r in reps]
        assert np.array_equal(w, np.asarray(want, dtype=np.uint64))
    p = np.array([[0.0, 0.2, 0.0, 0.5], [0.3, 0.0, 0.3, 0.4]])
    for u in (1e-9, 0.2, 0.5, 0.75, 0.999999):
        got = simref.categorical_v(p, simref.left_sum(p), np.full(2, u))
        assert list(got) == [pyref.sample(list(p[0]), u), pyref.sample(list(p[1]), u)]


@pytest.mark.parametrize("n", [2, 4, 8])
def test_twin_against_closed_forms(n):
    """E[dwell_i] (Van Loan integral of expm), E[N_ij] = q_ij E[dwell_i] and P(tip = j) = (pid e^{Q depth})_j, |z| < 5."""
    Q = _model(n)
    edge, lens = synth.random_tree(40, 1.0, 0x51A + n)
    pid = np.arange(1.0, n + 1.0)
    tips, stats, nodes = simref.simulate(edge, lens, Q, pid, 4000, seed=123 + n)
    assert tips.shape == (4000, 40) and stats.shape == (4000, n + n * n + 1) and nodes.shape == (4000, 79)
    assert np.array_equal(tips, nodes[:, :40])
    assert np.all(stats[:, [n + i * n + i for i in range(n)]] == 0.0)
    np.testing.assert_allclose(stats[:, :n].sum(axis=1), lens.sum(), rtol=1e-12)      # every branch is dwelt in exactly once
    z = simref.zscores(tips, stats, edge, lens, Q, pid)
    assert z.size > n and z.max() < 5.0, z.max()


def test_twin_observe_and_absorbing_state():
    Q = synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0)
    edge, lens = synth.random_tree(40, 1.0, 9)
    tips, stats, nodes = simref.simulate(edge, lens, Q, [1, 1, 1, 1], 2000, seed=4, observe=[1, 2, 1, 2])
    assert np.array_equal(tips, (nodes[:, :40] - 1) % 2 + 1)
    assert simref.zscores(tips, stats, edge, lens, Q, [1, 1, 1, 1], observe=[1, 2, 1, 2]).max() < 5.0
    Qa = np.array([[-0.5, 0.5, 0.0], [0.0, 0.0, 0.0], [0.2, 0.3, -0.5]])       # state 2 absorbing
    tips, stats, nodes = simref.simulate(edge, lens, Qa, [1, 0, 1], 2000, seed=5)
    assert np.all(stats[:, 3 + 3 * 1:3 + 3 * 2] == 0.0)                        # nothing leaves state 2
    assert simref.zscores(tips, stats, edge, lens, Qa, [1, 0, 1]).max() < 5.0


def _raw_call(z, Q, pid, observe=None, R=4, tips=True, stats=True, **opt):
    Qf = np.asfortranarray(np.asarray(Q, dtype=np.float64))
    n = Qf.shape[0]
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    pt = _lib.PlainTree(z)
    tree, T = pt.c, pt.T
    obs = None if observe is None else np.ascontiguousarray(observe, dtype=np.int32)
    o = _lib.make_options(n_replicas=R, **opt)
    t = np.zeros((R, T), dtype=np.int32) if tips else None
    s = np.zeros((R, n + n * n + 1)) if stats else None
    return _lib.load().phm_simulate_histories(C.byref(tree), n, _lib._p(Qf, C.c_double), _lib._p(pid, C.c_double),
                                              _lib._p(obs, C.c_int32), C.byref(o), _lib._p(t, C.c_int32), None,
                                              _lib._p(s, C.c_double))


def test_symbol_exported_and_no_device_status():
    L = _lib.load()
    assert "phm_simulate_histories" in _lib.EXPORTS and hasattr(L, "phm_simulate_histories")
    if L.phm_device_count() > 0:
        pytest.skip("GPU present")
    z, Q, pid, _ = synth.config_problem(2, n_tips=16)
    assert _raw_call(z, Q, pid) == 3                                           # PHM_ERR_NO_DEVICE
    with pytest.raises(_lib.PhmError) as e:
        api.simulate_histories(z, Q, pid, 8, observe=[1, 2, 1, 2], nodes=True)
    assert e.value.status == 3


def test_input_validation_happens_before_the_device():
    z, Q, pid, _ = synth.config_problem(2, n_tips=16)
    assert _raw_call(z, Q, pid, observe=[1, 2, 1, 5]) == 1                    # observe out of range
    assert _raw_call(z, Q, np.zeros(4)) == 5                                   # PHM_ERR_ZERO_PROB
    assert _raw_call(z, Q, [0.5, -0.1, 0.3, 0.3]) == 5
    assert _raw_call(z, Q, pid, reduce=True) == 1
    assert _raw_call(z, Q, pid, tips=False) == 1                               # NULL output (only nodes may be NULL)
    assert _raw_call(z, Q, pid, stats=False) == 1
    Qb = Q.copy()
    Qb[0, 1] -= 0.01                                                           # row does not sum to 0
    assert _raw_call(z, Qb, pid) == 1
    Qb = Q.copy()
    Qb[0, 3], Qb[0, 1] = -0.05, Qb[0, 1] + 0.05                               # negative off-diagonal
    assert _raw_call(z, Qb, pid) == 1
    Qb = Q.copy()
    Qb[2, 2] = np.nan
    assert _raw_call(z, Qb, pid) == 1
    zb = dict(z, **{"edge.length": z["edge.length"].copy()})
    zb["edge.length"][3] = -1.0
    assert _raw_call(zb, Q, pid) == 1
    assert _raw_call(z, np.zeros((1, 1)), [1.0]) == 1                          # n < 2
    Q65 = synth.dense_Q(65, 0.01, 0.02)
    assert _raw_call(z, Q65, np.ones(65)) == 1                                 # n > 64


def test_with_tip_states_is_the_shape_of_simulate_2_state_tree():
    Q = synth.config_Q(1)
    z = synth.make_tree(12, Q, 0.125, 3, init_segments=3)
    new = np.arange(12) % 2 + 1
    y = synth.with_tip_states(z, new)
    assert np.array_equal(y["states"], new) and np.array_equal(z["states"], synth.make_tree(12, Q, 0.125, 3)["states"])
    for r, (p, c) in enumerate(z["edge"]):
        if c <= 12:
            np.testing.assert_array_equal(y["maps"][r], [z["edge.length"][r] / 2] * 2)
            assert list(y["mapnames"][r]) == [1, new[c - 1]] and y["node.states"][r, 1] == new[c - 1]
        else:
            np.testing.assert_array_equal(y["maps"][r], z["maps"][r])        # internal branches keep their paths
            assert y["node.states"][r, 1] == 1
    # make_tree still builds its paths through the same helper: unchanged output
    zz = synth.make_tree(12, Q, 0.125, 3, init_segments=3)
    for r in range(len(z["maps"])):
        np.testing.assert_array_equal(zz["maps"][r], z["maps"][r])


def test_r_wrappers_name_the_exported_call_symbol():
    src = open(os.path.join(ROOT, "shim", "phylomap_simulate_shim.cpp")).read()
    exported = set(re.findall(r"RcppExport SEXP (phylomap_\w+)\(", src))
    assert exported == {"phylomap_hip_simulate_histories"}
    rfile = open(os.path.join(ROOT, "shim", "R", "phylomap_simulate.R")).read()
    called = set(re.findall(r"\.Call\('(\w+)'", rfile))
    assert called == exported
    for name in ("simulate_histories", "sample2statehistory", "simulate_state_tree"):
        assert re.search(rf"^{name} <- function\(", rfile, re.M), name
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "tests", "mock_rcpp"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "shim", "phylomap_simulate_shim.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
