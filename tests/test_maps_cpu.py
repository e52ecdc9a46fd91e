"""Stochastic maps without a device: the twin (tests/mapsref.py) against the twins it restates, the Maps helpers on hand-built
maps, the argument checks of phm_simulate_histories_maps / phm_maketreelistEXP_maps (all before any device call), and the R
layer (shim/phylomap_maps_shim.cpp, shim/R/phylomap_maps.R)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mapsref
import pyref
import simref
from phylomap_amd import _lib, api, synth
from phylomap_amd.maps import Maps, history_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tree(T, seed, shuffled):
    edge, lens = synth.random_tree(T, 1.0, seed)
    if shuffled:
        perm = np.random.default_rng(seed).permutation(edge.shape[0])
        edge, lens = edge[perm], lens[perm]
    return {"edge": edge, "edge.length": lens, "Nnode": T - 1, "states": np.ones(T, dtype=np.int32)}


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("observed", [False, True])
def test_simulator_twin_segments_reproduce_its_statistics(n, shuffled, observed):
    Q = synth.dense_Q(n, 0.05, 0.3) if n == 8 else synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0) if n == 4 else np.array([[-0.6, 0.6], [0.9, -0.9]])
    z = _tree(16, 0x3A0 + n, shuffled)
    pid = np.arange(1.0, n + 1.0)
    observe = (np.arange(n) % 2 + 1) if observed else None
    R, seed = 37, 11 + n
    tips, stats, nodes, (off, dwell, state) = mapsref.simulate(z["edge"], z["edge.length"], Q, pid, R, seed, observe=observe)
    wt, ws, wn = simref.simulate(z["edge"], z["edge.length"], Q, pid, R, seed, observe=observe)
    assert np.array_equal(tips, wt) and np.array_equal(stats, ws) and np.array_equal(nodes, wn)
    E = z["edge"].shape[0]
    order, _ = simref.walk_order(z["edge"], 16)
    dw = np.zeros((R, n))
    cnt = np.zeros((R, n, n))
    for r in range(R):
        for b in order:                                        # the walk order: dwell bit for bit
            k = r * E + b
            s = state[off[k]:off[k + 1]] - 1
            for x, st in zip(dwell[off[k]:off[k + 1]], s):
                dw[r, st] += x
            for a, c in zip(s[:-1], s[1:]):
                assert a != c
                cnt[r, a, c] += 1
            assert s[0] == nodes[r, z["edge"][b, 0] - 1] - 1 and s[-1] == nodes[r, z["edge"][b, 1] - 1] - 1
    assert np.array_equal(dw, stats[:, :n])
    assert np.array_equal(cnt.reshape(R, n * n), stats[:, n:n + n * n])


@pytest.mark.parametrize("n", [2, 4])
def test_exp_twin_segments_reproduce_its_statistics(n):
    Q = {2: synth.config_Q(1), 4: synth.config_Q(2)}[n]
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    pid = np.full(n, 1.0 / n)
    z = synth.make_tree(9, Q, Omega, 0x3B0 + n)
    nen, nodelist, root = _lib.tree_orders(z)
    lefts, rights, d = api.eigen_decompose(Q)
    N, seed = 12, 5
    a = (z, Q.tolist(), pid.tolist(), N, [int(v) for v in nen], [int(v) for v in nodelist], int(root), lefts.tolist(),
         rights.tolist(), np.diag(d).tolist(), seed, 1)
    out, (off, dwell, state) = mapsref.sumstatEXP(*a)
    assert np.array_equal(np.array(out), np.array(pyref.sumstatEXP(*a)))
    E = len(z["edge"])
    got = np.zeros((N, n + n * (n - 1)))
    for it in range(N):
        for b in range(E):                                     # edge-row order: pyref's order
            k = it * E + b
            s = state[off[k]:off[k + 1]] - 1
            for x, y in zip(s[:-1], s[1:]):
                assert x != y
                got[it, n + x * (n - 1) + (y - 1 if x < y else y)] += 1.0
            for x, st in zip(dwell[off[k]:off[k + 1]], s):
                got[it, st] += x
            assert z["edge"][b, 1] > len(z["states"]) or s[-1] == z["states"][z["edge"][b, 1] - 1] - 1
    assert np.array_equal(got, np.array(out))


def _hand_maps():
    # two histories on a 3-tip tree (edges: 4->5, 5->1, 5->2, 4->3), states 1..3
    edge = np.array([[4, 5], [5, 1], [5, 2], [4, 3]])
    z = {"edge": edge, "edge.length": np.array([1.0, 0.5, 0.75, 2.0]), "Nnode": 2, "states": np.array([1, 1, 1]),
         "maps": [np.array([1.0])] * 4, "mapnames": [np.array([1])] * 4}
    segs = [  # history 0
        [(0.25, 1), (0.75, 2)], [(0.5, 2)], [(0.25, 2), (0.5, 3)], [(2.0, 1)],
        # history 1
        [(1.0, 3)], [(0.125, 3), (0.375, 1)], [(0.75, 3)], [(1.5, 1), (0.5, 2)]]
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    dwell = np.array([x for s in segs for x, _ in s])
    state = np.array([y for s in segs for _, y in s], dtype=np.int32)
    return z, Maps(off, dwell, state, 4)


def test_maps_helpers_on_hand_built_maps():
    z, m = _hand_maps()
    assert m.n_hist == 2
    d, s = m.branch(1, 1)
    assert np.array_equal(d, [0.125, 0.375]) and np.array_equal(s, [3, 1])
    me = m.mapped_edge(3)
    assert me.shape == (2, 4, 3)
    assert np.array_equal(me[0], [[0.25, 0.75, 0], [0, 0.5, 0], [0, 0.25, 0.5], [2.0, 0, 0]])
    assert np.array_equal(me[1], [[0, 0, 1.0], [0.375, 0, 0.125], [0, 0, 0.75], [1.5, 0.5, 0]])
    ns = m.node_states()
    assert np.array_equal(ns[0], [[1, 2], [2, 2], [2, 3], [1, 1]])
    assert np.array_equal(ns[1], [[3, 3], [3, 1], [3, 3], [1, 2]])
    assert np.array_equal(m.counts(), [[2, 1, 2, 1], [1, 2, 1, 2]])


def test_history_tree_round_trips_through_flat_tree():
    z, m = _hand_maps()
    zt = history_tree(z, m, 1, n=3)
    assert np.array_equal(zt["states"], [1, 3, 2])
    assert np.array_equal(zt["node.states"], m.node_states()[1])
    assert np.array_equal(zt["mapped.edge"], m.mapped_edge(3)[1])
    ft = _lib.FlatTree(zt)
    off, dwell, state = m.history(1)
    assert np.array_equal(ft.map_off, off) and np.array_equal(ft.maps, dwell) and np.array_equal(ft.mapnames, state)
    assert np.array_equal(ft.states, [1, 3, 2])
    assert np.array_equal(history_tree(z, m, 1, n=3, observe=[1, 2, 1])["states"], [1, 1, 2])
    assert z["maps"][0].tolist() == [1.0]                                  # the input tree is not modified


def _sim_call(off, cap, dwell, state, R=4, mapping="auto"):
    L = _lib.load()
    Q = np.asfortranarray(synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0))
    pid = np.full(4, 0.25)
    edge, lens = synth.random_tree(8, 1.0, 3)
    pt = _lib.PlainTree({"edge": edge, "edge.length": lens, "Nnode": 7})
    o = _lib.make_options(n_replicas=R, mapping=mapping)
    tips, stats = np.zeros((R, 8), dtype=np.int32), np.zeros((R, 21), order="F")
    return L.phm_simulate_histories_maps(C.byref(pt.c), 4, _lib._p(Q, C.c_double), _lib._p(pid, C.c_double), None, C.byref(o),
                                         _lib._p(tips, C.c_int32), None, _lib._p(stats, C.c_double), _lib._p(off, C.c_int64),
                                         int(cap), _lib._p(dwell, C.c_double), _lib._p(state, C.c_int32))


def _exp_call(off, cap, dwell, state, N=4, mapping="auto"):
    L = _lib.load()
    Q = synth.config_Q(2)
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    z = synth.make_tree(8, Q, Omega, 0x3C)
    ft = _lib.FlatTree(z)
    Qf = np.asfortranarray(Q)
    pid = np.full(4, 0.25)
    nen, nodelist, root = _lib.tree_orders(z)
    lefts, rights, d = (np.asfortranarray(a) for a in api.eigen_decompose(Q))
    o = _lib.make_options(mapping=mapping)
    out = np.zeros((N, 16), order="F")
    return L.phm_maketreelistEXP_maps(C.byref(ft.c), 4, _lib._p(Qf, C.c_double), _lib._p(pid, C.c_double), _lib._p(nen, C.c_int32),
                                      _lib._p(nodelist, C.c_int32), int(root), N, _lib._p(lefts, C.c_double),
                                      _lib._p(rights, C.c_double), _lib._p(d, C.c_double), C.byref(o), _lib._p(out, C.c_double),
                                      _lib._p(off, C.c_int64), int(cap), _lib._p(dwell, C.c_double), _lib._p(state, C.c_int32))


@pytest.mark.parametrize("call", [_sim_call, _exp_call])
def test_map_arguments_are_checked_before_the_device(call):
    L = _lib.load()
    rows = 4 * 14
    dwell, state = np.zeros(100), np.zeros(100, dtype=np.int32)
    assert call(None, 0, None, None) == 1                                   # NULL map_off, sizing
    assert "map_off is NULL" in L.phm_last_error().decode()
    assert call(None, 100, dwell, state) == 1
    good = np.arange(rows + 1, dtype=np.int64)
    assert call(good, rows - 1, dwell, state) == 1                          # short map_cap
    assert "map_cap" in L.phm_last_error().decode()
    bad = good.copy()
    bad[10] = 12                                                            # row 10 ends before it starts
    assert call(bad, 100, dwell, state) == 1
    assert "decreases at row 10" in L.phm_last_error().decode()
    nz = good + 1
    assert call(nz, 100, dwell, state) == 1                                 # does not start at 0
    assert call(good, 100, dwell, None) == 1                                # one segment array only


def test_exp_maps_need_the_tile_mapping():
    L = _lib.load()
    off = np.zeros(4 * 14 + 1, dtype=np.int64)
    assert _exp_call(off, 0, None, None, mapping="replicas") == 2
    assert "PHM_MAP_TILES" in L.phm_last_error().decode()


def test_new_symbols_are_exported():
    L = _lib.load()
    for s in ("phm_simulate_histories_maps", "phm_maketreelistEXP_maps"):
        assert hasattr(L, s) and s in _lib.EXPORTS


def test_r_wrappers_name_the_exported_call_symbols():
    src = open(os.path.join(ROOT, "shim", "phylomap_maps_shim.cpp")).read()
    exported = set(re.findall(r"RcppExport SEXP (\w+)\(", src))
    assert exported == {"phylomap_hip_simulate_maps", "phylomap_hip_exp_maps"}
    rfile = open(os.path.join(ROOT, "shim", "R", "phylomap_maps.R")).read()
    assert set(re.findall(r"\.Call\('(\w+)'", rfile)) == exported
    for fn in ("simulate_maps", "sumstatEXPmaps", "history_tree"):
        assert re.search(rf"^{fn} <- function\(", rfile, re.M), fn


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_maps_shim_compiles_against_the_mock():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "tests", "mock_rcpp"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "shim", "phylomap_maps_shim.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
