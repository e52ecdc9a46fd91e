"""Exact expectations through time (phm_expected_through_time) without a device: the twin (tests/timeref.py)
against itself and against section 13's twin, the maps helpers on hand-made maps, the C-ABI checks (all before any device call)
and the R layer's names."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import exactref
import timeref
from phylomap_amd import _lib, api, synth
from phylomap_amd.maps import Maps, node_depths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(n):
    if n == 2:
        return np.array([[-0.6, 0.6], [0.9, -0.9]])
    if n == 3:
        return np.array([[-0.5, 0.3, 0.2], [0.1, -0.4, 0.3], [0.6, 0.0, -0.6]])
    return synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0)


def _case(n, T, seed):
    edge, lens = synth.random_tree(T, 1.0, seed)
    tips = np.random.default_rng(seed).integers(0, n + 1, (5, T))
    d = timeref.depths(edge, lens)
    inner = np.sort(d[T:])
    bounds = np.unique(np.concatenate([[0.0], inner[1:4], [0.5 * (inner[1] + inner[2])], [d.max(), 1.1 * d.max()]]))
    return edge, lens, tips, bounds, d


@pytest.mark.parametrize("n,T", [(2, 9), (3, 14), (4, 12)])
def test_twin_routes_agree_and_bins_sum_to_the_totals(n, T):
    Q = _model(n)
    edge, lens, tips, bounds, _ = _case(n, T, 0x7100 + n)
    pid = np.arange(1.0, n + 1.0)
    a = timeref.through_time(edge, lens, Q, pid, tips, bounds=bounds)
    b = timeref.through_time(edge, lens, Q, pid, tips, bounds=bounds, route="vanloan")
    scale = np.max(np.abs(b["bins"]))
    assert np.all(np.abs(a["bins"] - b["bins"]) <= 1e-10 * np.abs(b["bins"]) + 1e-14 * scale)
    assert np.array_equal(a["occupancy"], b["occupancy"])
    st, ll = exactref.expected(edge, lens, Q, pid, tips)
    np.testing.assert_allclose(a["bins"].sum(axis=1), st, rtol=1e-10, atol=1e-13 * np.sum(lens))
    assert np.array_equal(a["loglik"], ll)


@pytest.mark.parametrize("n", [2, 4])
def test_occupancy_counts_the_lineages(n):
    Q = _model(n)
    edge, lens, tips, _, d = _case(n, 15, 0x7200 + n)
    bounds = np.unique(np.concatenate([[0.0], d, [1.5 * d.max()], np.linspace(0.0, d.max(), 7)[1:]]))
    got = timeref.through_time(edge, lens, Q, np.ones(n), tips, bounds=bounds)
    dp, dc = d[edge[:, 0] - 1], d[edge[:, 1] - 1]
    alive = np.array([np.sum((dp < t) & (t <= dc)) + (t == 0.0) for t in bounds], dtype=float)
    assert alive[0] == 1 and alive[-1] == 0 and alive.max() > 2
    np.testing.assert_allclose(got["occupancy"].sum(axis=2), np.broadcast_to(alive, (5, bounds.size)), rtol=0, atol=1e-12)
    # dwell summed over the states of a bin is the branch length inside it
    inside = np.array([np.sum(np.clip(np.minimum(dc, hi) - np.maximum(dp, lo), 0.0, None)) for lo, hi in zip(bounds[:-1], bounds[1:])])
    np.testing.assert_allclose(got["bins"][:, :, :n].sum(axis=2), np.broadcast_to(inside, (5, inside.size)), rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("n", [2, 3, 4])
def test_posterior_at_the_branch_ends_is_the_node_posterior(n):
    Q = _model(n)
    edge, lens, tips, _, _ = _case(n, 13, 0x7300 + n)
    E = edge.shape[0]
    pe = np.concatenate([np.arange(E), np.arange(E), np.arange(E)])
    pp = np.concatenate([np.zeros(E), lens, 0.3 * lens])
    got = timeref.through_time(edge, lens, Q, np.ones(n), tips, points=(pe, pp))["points"]
    _, _, post = exactref.expected(edge, lens, Q, np.ones(n), tips, nodes=True)
    np.testing.assert_allclose(got[:, :E], post[:, edge[:, 0] - 1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got[:, E:2 * E], post[:, edge[:, 1] - 1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got.sum(axis=2), 1.0, rtol=0, atol=1e-13)


def test_node_depths_are_the_twins():
    edge, lens = synth.random_tree(40, 1.0, 0x74)
    perm = np.random.default_rng(1).permutation(edge.shape[0])
    z = {"edge": edge[perm], "edge.length": lens[perm], "Nnode": 39}
    assert np.array_equal(node_depths(z), timeref.depths(edge, lens))
    assert node_depths(z)[40] == 0.0                                      # the root, node 41


def _hand_maps():
    """root 4 -> 5 (t 1) -> tips 1, 2 (t 1 each); 4 -> tip 3 (t 2).  History 0 has jumps, history 1 stays in state 1."""
    z = {"edge": np.array([[4, 5], [5, 1], [5, 2], [4, 3]]), "edge.length": np.array([1.0, 1.0, 1.0, 2.0]), "Nnode": 2}
    off = np.array([0, 2, 3, 5, 7, 8, 9, 10, 11])
    dwell = np.array([0.5, 0.5, 1.0, 0.25, 0.75, 1.5, 0.5, 1.0, 1.0, 1.0, 2.0])
    state = np.array([1, 2, 2, 2, 1, 1, 3, 1, 1, 1, 1])
    return z, Maps(off, dwell, state, 4)


def test_maps_through_time_on_hand_made_maps():
    z, m = _hand_maps()
    assert np.array_equal(node_depths(z), [2.0, 2.0, 2.0, 0.0, 1.0])
    occ, bins = m.through_time(z, [0.0, 0.5, 1.0, 2.0], 3)
    # tau = 0.5 on edge row 0 is a tie (the first segment ends there): the earlier segment; tau = 1 = d_child: the last one
    assert np.array_equal(occ[0], [[1, 0, 0], [2, 0, 0], [1, 1, 0], [1, 1, 1]])
    assert np.array_equal(occ[1], [[1, 0, 0], [2, 0, 0], [2, 0, 0], [3, 0, 0]])
    want = np.zeros((2, 3, 9))
    want[0, 0, 0] = 1.0
    want[0, 1, :3] = [0.5, 0.5, 0.0]
    want[0, 1, 3] = 1                                                    # 1 -> 2 at depth 0.5: bin [0.5, 1)
    want[0, 2, :3] = [1.25, 1.25, 0.5]
    want[0, 2, 5] = 1                                                    # 2 -> 1 at 1.25
    want[0, 2, 4] = 1                                                    # 1 -> 3 at 1.5
    want[1, :, 0] = [1.0, 1.0, 3.0]
    np.testing.assert_allclose(bins, want, rtol=0, atol=1e-15)
    occ1, bins1 = m.through_time(z, [0.25], 3)
    assert bins1.shape == (2, 0, 9) and np.array_equal(occ1[:, 0], [[2, 0, 0], [2, 0, 0]])
    # parts of branches outside [first, last bound) are left out; a transition at the last bound too
    _, part = m.through_time(z, [0.6, 1.5], 3)
    np.testing.assert_allclose(part[0, 0], [0.9 + 0.25, 0.4 + 0.5 + 0.25, 0.0, 0, 0, 1, 0, 0, 0], rtol=0, atol=1e-14)


def test_maps_states_at_points():
    _, m = _hand_maps()
    got = m.states_at([0, 0, 0, 3, 2, 2, 1], [0.0, 0.5, 0.5000001, 2.0, 0.25, 0.2500001, 0.0])
    assert np.array_equal(got, [[1, 1, 2, 3, 2, 1, 2], [1, 1, 1, 1, 1, 1, 1]])
    assert m.states_at([0], [1.0 + 1e-9]).tolist() == [[2], [1]]      # past the row's end: the last segment


# ---- the C-ABI without a device ----------------------------------------------------------------------------------------------
def _raw_call(z, Q, pid, bounds=(0.0, 0.5), pe=(0,), pp=(0.0,), occ=True, bins=True, pts=True, ll=True, Qnull=False, S=2, **opt):
    Qf = np.asfortranarray(np.asarray(Q, dtype=np.float64))
    n = Qf.shape[0]
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    pt = _lib.PlainTree(z, np.tile(z["states"], (S, 1)))
    tree = pt.c
    o = _lib.make_options(n_replicas=S, tips_per_replica=True, **opt)
    b = np.ascontiguousarray(bounds, dtype=np.float64)
    K = b.size
    pe = np.ascontiguousarray(pe, dtype=np.int32)
    pp = np.ascontiguousarray(pp, dtype=np.float64)
    out = [np.zeros(S * max(K, 1) * n) if occ else None, np.zeros(S * max(K - 1, 1) * n * n) if bins else None,
           np.zeros(S * max(pe.size, 1) * n) if pts else None, np.zeros(S) if ll else None]
    return _lib.load().phm_expected_through_time(C.byref(tree), n, None if Qnull else _lib._p(Qf, C.c_double), _lib._p(pid, C.c_double),
                                                 None, C.byref(o), K, _lib._p(b, C.c_double), _lib._p(out[0], C.c_double),
                                                 _lib._p(out[1], C.c_double), pe.size, _lib._p(pe, C.c_int32), _lib._p(pp, C.c_double),
                                                 _lib._p(out[2], C.c_double), _lib._p(out[3], C.c_double))


def _err():
    return _lib.load().phm_last_error().decode()


def test_input_validation_happens_before_the_device():
    z, Q, pid, _ = synth.config_problem(2, n_tips=16)
    t0 = float(z["edge.length"][0])
    assert _raw_call(z, Q, pid, bounds=(0.0, 0.5, 0.4)) == 1 and "bounds[2]" in _err()          # not increasing
    assert _raw_call(z, Q, pid, bounds=(0.0, 0.5, 0.5)) == 1 and "bounds[2]" in _err()
    assert _raw_call(z, Q, pid, bounds=(-0.1, 0.5)) == 1 and "bounds[0]" in _err()
    assert _raw_call(z, Q, pid, bounds=(0.0, np.nan)) == 1 and "bounds[1]" in _err()
    assert _raw_call(z, Q, pid, bounds=(0.0, np.inf)) == 1
    assert _raw_call(z, Q, pid, bounds=(0.3,)) == 1                                            # bins need two bounds
    assert _raw_call(z, Q, pid, bounds=(), bins=False) == 1                                    # occupancy needs one
    assert _raw_call(z, Q, pid, pe=(0, 1), pp=(0.0, float(z["edge.length"][1]) * 1.0001)) == 1 and "point 1" in _err()
    assert _raw_call(z, Q, pid, pe=(0, 30), pp=(0.0, 0.0)) == 1 and "point 1" in _err()        # edge row out of range
    assert _raw_call(z, Q, pid, pe=(-1,), pp=(0.0,)) == 1 and "point 0" in _err()
    assert _raw_call(z, Q, pid, pe=(0,), pp=(-1e-12,)) == 1 and "point 0" in _err()
    assert _raw_call(z, Q, pid, pe=(0,), pp=(np.nan,)) == 1
    assert _raw_call(z, Q, pid, pe=(), pp=()) == 1                                             # point_post needs a point
    assert _raw_call(z, Q, pid, occ=False, bins=False, pts=False, ll=False) == 1 and "no output" in _err()
    assert _raw_call(z, Q, pid, Qnull=True) == 1                                               # NULL Q
    assert _raw_call(z, Q, pid, reduce=True) == 1
    assert _raw_call(z, Q, np.zeros(4)) == 5                                                   # pid: section 13's checks
    assert _raw_call(z, Q, pid, pe=(0,), pp=(t0,), bounds=(0.0, 1e300)) in (0, 3)              # a point at t_b and huge bounds are fine


def test_symbol_exported_and_no_device_status():
    L = _lib.load()
    assert "phm_expected_through_time" in _lib.EXPORTS and hasattr(L, "phm_expected_through_time")
    if L.phm_device_count() > 0:
        pytest.skip("GPU present")
    z, Q, pid, _ = synth.config_problem(2, n_tips=16)
    assert _raw_call(z, Q, pid) == 3                                                           # PHM_ERR_NO_DEVICE
    assert _raw_call(z, Q, pid, occ=False, bins=False, pts=False) == 3
    with pytest.raises(_lib.PhmError) as e:
        api.expected_through_time(z, Q, pid, bounds=[0.0, 1.0], points=([0], [0.0]), sites=np.ones((3, 16)))
    assert e.value.status == 3


def test_r_wrapper_names_the_exported_call_symbol():
    src = open(os.path.join(ROOT, "shim", "phylomap_time_shim.cpp")).read()
    exported = set(re.findall(r"RcppExport SEXP (phylomap_\w+)\(", src))
    assert exported == {"phylomap_expected_through_time"}
    rfile = open(os.path.join(ROOT, "shim", "R", "phylomap_time.R")).read()
    assert set(re.findall(r"\.Call\('(\w+)'", rfile)) == exported
    assert re.search(r"^sumstatExpectedTime <- function\(tree, Q, pid, bounds, points = NULL, sites = NULL, observe = NULL\)", rfile, re.M)
    shim = open(os.path.join(ROOT, "shim", "phylomap_shim.cpp")).read()
    assert "phylomap_expected_through_time" not in shim
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "tests", "mock_rcpp"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "shim", "phylomap_time_shim.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
