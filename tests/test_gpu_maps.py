"""Stochastic maps on the device (phm_simulate_histories_maps, phm_maketreelistEXP_maps) against their Python twin
(tests/mapsref.py) bit for bit, against the producers' own statistics on C3's tree, the two-phase contract (tampered offsets,
guard elements), devices, the exact per-branch expectations, and a drawn history as the start of a chain."""
import ctypes as C
import math

import numpy as np
import pytest

import mapsref
import simref
from phylomap_amd import _lib, api, synth
from phylomap_amd.maps import Maps, history_tree

pytestmark = pytest.mark.gpu


def _model(n):
    if n == 2:
        return np.array([[-0.6, 0.6], [0.9, -0.9]])
    if n == 3:
        return np.array([[-0.5, 0.3, 0.2], [0.1, -0.4, 0.3], [0.6, 0.0, -0.6]])
    if n == 4:
        return synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0)
    if n == 20:
        return synth.tridiagonal_Q(20, 0.4)
    return synth.dense_Q(n, 0.01, 0.04)


def _tree(T, seed, shuffled):
    edge, lens = synth.random_tree(T, 1.0, seed)
    if shuffled:
        perm = np.random.default_rng(seed).permutation(edge.shape[0])
        edge, lens = edge[perm], lens[perm]
    return {"edge": edge, "edge.length": lens, "Nnode": T - 1, "states": np.ones(T, dtype=np.int32)}


def _same_maps(m, want):
    off, dwell, state = want
    assert np.array_equal(m.off, off)
    assert np.array_equal(m.state, state)
    assert np.array_equal(m.dwell, dwell)


def _pairs(m):
    """(history, from, to) 0-based of every pair of consecutive segments inside a row"""
    row = np.repeat(np.arange(m.off.size - 1), np.diff(m.off))
    same = row[:-1] == row[1:]
    return row[:-1][same] // m.n_edge, m.state[:-1][same] - 1, m.state[1:][same] - 1


def _walk_dwell(m, order, n):
    """dwell per state summed segment by segment in the walk order of the edges (the simulator's order)"""
    R, E = m.n_hist, m.n_edge
    rows = (np.arange(R)[:, None] * E + np.asarray(order)[None, :]).ravel()
    lens = np.diff(m.off)[rows]
    starts = m.off[rows]
    idx = np.repeat(starts - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(lens.sum())
    hist = np.repeat(rows // E, lens)
    out = np.zeros((R, n))
    np.add.at(out, (hist, m.state[idx].astype(np.int64) - 1), m.dwell[idx])
    return out


def _row_sums(m):
    return np.add.reduceat(m.dwell, m.off[:-1]).reshape(m.n_hist, m.n_edge)


@pytest.mark.parametrize("n", [2, 3, 4, 8, 20, 61])
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("observed", [False, True])
def test_simulator_maps_against_twin(n, shuffled, observed):
    Q = _model(n)
    z = _tree(24, 0x6100 + n, shuffled)
    pid = np.arange(1.0, n + 1.0)
    observe = (np.arange(n) % 2 + 1) if observed else None
    for R in (1, 63, 64, 130):
        seed = 1000 * n + R
        tips, stats, nodes, m = api.simulate_histories(z, Q, pid, R, observe=observe, nodes=True, maps=True, seed=seed)
        wt, ws, wn, wm = mapsref.simulate(z["edge"], z["edge.length"], Q, pid, R, seed, observe=observe)
        _same_maps(m, wm)
        assert np.array_equal(tips, wt) and np.array_equal(nodes, wn)
        assert np.array_equal(stats[:, n:], ws[:, n:])
        p_tips, p_stats, p_nodes = api.simulate_histories(z, Q, pid, R, observe=observe, nodes=True, seed=seed)
        assert np.array_equal(p_tips, tips) and np.array_equal(p_stats, stats) and np.array_equal(p_nodes, nodes)


@pytest.mark.parametrize("n", [2, 4, 8, 20])
def test_exp_maps_against_twin(n):
    Q = {2: synth.config_Q(1), 4: synth.config_Q(2)}.get(n)
    if Q is None:
        Q = synth.tridiagonal_Q(n, 0.3) if n == 20 else synth.dense_Q(n, 0.02, 0.05)
        Q = (Q + Q.T) / 2                                        # symmetric: a real spectrum for matexp
        np.fill_diagonal(Q, 0.0)
        np.fill_diagonal(Q, -Q.sum(axis=1))
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    pid = np.full(n, 1.0 / n)
    z = synth.make_tree(10, Q, Omega, 0xE100 + n)
    nen, nodelist, root = _lib.tree_orders(z)
    eig = api.eigen_decompose(Q)
    lefts, rights, d = eig
    for N in (1, 63, 64, 130):
        out, m = api.sumstatEXP(z, Q, pid, N, eig=eig, maps=True, seed=7 + N)
        want, wm = mapsref.sumstatEXP(z, Q.tolist(), pid.tolist(), N, [int(v) for v in nen], [int(v) for v in nodelist], int(root),
                                      lefts.tolist(), rights.tolist(), np.diag(d).tolist(), 7 + N, 0)
        _same_maps(m, wm)
        assert np.array_equal(out[:, n:], np.array(want)[:, n:])
        assert np.array_equal(out, api.sumstatEXP(z, Q, pid, N, eig=eig, seed=7 + N))


# ---- raw two-phase calls ------------------------------------------------------------------------------------------------------

def _sim_args(z, Q, pid, R, seed, **opt):
    Q = np.asfortranarray(Q, dtype=np.float64)
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    ft = _lib.FlatTree(z)
    o = _lib.make_options(n_replicas=R, seed=seed, **opt)
    T, Nn = ft.T, int(z["Nnode"])
    tips = np.zeros((R, T), dtype=np.int32)
    nodes = np.zeros((R, T + Nn), dtype=np.int32)
    stats = np.zeros((R, Q.shape[0] * (Q.shape[0] + 1) + 1), order="F")
    keep = (Q, pid, ft, o)
    args = (C.byref(ft.c), Q.shape[0], _lib._p(Q, C.c_double), _lib._p(pid, C.c_double), None, C.byref(o),
            _lib._p(tips, C.c_int32), _lib._p(nodes, C.c_int32), _lib._p(stats, C.c_double))
    return args, (tips, stats, nodes), keep


def _exp_args(z, Q, pid, N, seed, **opt):
    Q = np.asfortranarray(Q, dtype=np.float64)
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    n = Q.shape[0]
    nen, nodelist, root = _lib.tree_orders(z)
    lefts, rights, d = (np.asfortranarray(a) for a in api.eigen_decompose(Q))
    ft = _lib.FlatTree(z)
    o = _lib.make_options(seed=seed, **opt)
    out = np.zeros((N, n + n * (n - 1)), order="F")
    keep = (Q, pid, nen, nodelist, lefts, rights, d, ft, o)
    args = (C.byref(ft.c), n, _lib._p(Q, C.c_double), _lib._p(pid, C.c_double), _lib._p(nen, C.c_int32),
            _lib._p(nodelist, C.c_int32), int(root), N, _lib._p(lefts, C.c_double), _lib._p(rights, C.c_double),
            _lib._p(d, C.c_double), C.byref(o), _lib._p(out, C.c_double))
    return args, (out,), keep


def _two_phase(fn, args, outs, R, E):
    """sizing call, copies of its outputs, filling call; returns (outputs after sizing, Maps)"""
    off = np.zeros(R * E + 1, dtype=np.int64)
    _lib.check(fn(*args, _lib._p(off, C.c_int64), 0, None, None))
    sized = [a.copy() for a in outs]
    total = int(off[-1])
    dwell, state = np.empty(total), np.empty(total, dtype=np.int32)
    _lib.check(fn(*args, _lib._p(off, C.c_int64), total, _lib._p(dwell, C.c_double), _lib._p(state, C.c_int32)))
    for a, b in zip(sized, outs):
        assert np.array_equal(a, b), "the filling call changed an output of the sizing call"
    return sized, Maps(off, dwell, state, E)


def _tampered(fn, args, m, row):
    """offsets with row `row` one segment longer (valid shape), guards past map_cap: BAD_INPUT, guards intact"""
    off = m.off.copy()
    off[row + 1:] += 1
    cap = int(off[-1])
    G = 64
    dwell = np.full(cap + G, -7.25)
    state = np.full(cap + G, -7, dtype=np.int32)
    st = fn(*args, _lib._p(off, C.c_int64), cap, _lib._p(dwell, C.c_double), _lib._p(state, C.c_int32))
    assert st == 1, _lib.STATUS.get(st)
    assert f"row {row} " in _lib.load().phm_last_error().decode()
    assert np.all(dwell[cap:] == -7.25) and np.all(state[cap:] == -7)


def test_c3_simulator_maps_1024():
    z, Q, pid, _ = synth.config_problem(3)                                  # 10 000 tips, 4 states
    n, R = 4, 1024
    E = z["edge"].shape[0]
    L = _lib.load()
    args, outs, keep = _sim_args(z, Q, pid, R, 0xC3)
    (tips, stats, nodes), m = _two_phase(L.phm_simulate_histories_maps, args, outs, R, E)
    p_tips, p_stats, p_nodes = api.simulate_histories(z, Q, pid, R, nodes=True, seed=0xC3)
    assert np.array_equal(p_tips, tips) and np.array_equal(p_stats, stats) and np.array_equal(p_nodes, nodes)
    h, a, b = _pairs(m)
    assert np.all(a != b)
    cnt = np.bincount(h * n * n + a * n + b, minlength=R * n * n).reshape(R, n * n)
    assert np.array_equal(cnt.astype(np.float64), stats[:, n:n + n * n])
    order, _ = simref.walk_order(np.asarray(z["edge"]), z["edge"].shape[0] // 2 + 1)
    assert np.array_equal(_walk_dwell(m, order, n), stats[:, :n])
    # the last piece is the reference's gap - ((pos + gap) - t): on a very short edge its rounding is that of the gap, not of t
    np.testing.assert_allclose(_row_sums(m), np.broadcast_to(z["edge.length"], (R, E)), rtol=1e-12, atol=1e-13)
    ns = m.node_states()
    edge = np.asarray(z["edge"])
    assert np.array_equal(ns[:, :, 0], nodes[:, edge[:, 0] - 1]) and np.array_equal(ns[:, :, 1], nodes[:, edge[:, 1] - 1])
    T = tips.shape[1]
    tip_rows = edge[:, 1] <= T
    assert np.array_equal(ns[:, tip_rows, 1], tips[:, edge[tip_rows, 1] - 1])
    _tampered(L.phm_simulate_histories_maps, args, m, row=5 * E + 777)


def test_c3_exp_maps_1024():
    z, Q, pid, _ = synth.config_problem(3)
    n, N = 4, 1024
    E = z["edge"].shape[0]
    L = _lib.load()
    args, outs, keep = _exp_args(z, Q, pid, N, 0xC31, rescale=True)
    (out,), m = _two_phase(L.phm_maketreelistEXP_maps, args, outs, N, E)
    assert np.array_equal(out, api.sumstatEXP(z, Q, pid, N, seed=0xC31, rescale=True))
    h, a, b = _pairs(m)
    assert np.all(a != b)
    col = a * (n - 1) + np.where(b > a, b - 1, b)
    cnt = np.bincount(h * n * (n - 1) + col, minlength=N * n * (n - 1)).reshape(N, n * (n - 1))
    assert np.array_equal(cnt.astype(np.float64), out[:, n:])
    # the kernel sums dwell in 64-bit fixed point (scale 2^(61 - e), tree length < 2^e): rebuilt the same way, bit for bit
    length = sum(float(x) for x in z["edge.length"])                       # the host's sum, edge-row order
    ex = math.frexp(max(length, 1.0))[1]
    fx = np.rint(m.dwell * 2.0 ** (61 - ex)).astype(np.int64)
    acc = np.zeros((N, n), dtype=np.int64)
    np.add.at(acc, (np.repeat(np.arange(N * E) // E, np.diff(m.off)), m.state.astype(np.int64) - 1), fx)
    assert np.array_equal(acc.astype(np.float64) * 2.0 ** (ex - 61), out[:, :n])
    me = m.mapped_edge(n).astype(np.longdouble).sum(axis=1)                # and the plain sums, to 1e-15 of the tree length
    assert np.max(np.abs(me - out[:, :n])) <= 1e-15 * length
    np.testing.assert_allclose(_row_sums(m), np.broadcast_to(z["edge.length"], (N, E)), rtol=1e-12)
    ns = m.node_states()
    edge = np.asarray(z["edge"])
    T = len(z["states"])
    tip_rows = edge[:, 1] <= T
    assert np.all(ns[:, tip_rows, 1] == np.asarray(z["states"])[edge[tip_rows, 1] - 1][None, :])
    into = np.full(2 * T, -1)
    into[edge[:, 1]] = np.arange(E)                                         # the edge row that ends at each node
    inner = into[edge[:, 0]] >= 0
    assert np.array_equal(ns[:, inner, 0], ns[:, into[edge[inner, 0]], 1])  # a branch starts where its parent branch ends
    _tampered(L.phm_maketreelistEXP_maps, args, m, row=3 * E + 12345)


def test_two_devices_give_the_one_device_maps():
    Q = _model(4)
    z = _tree(200, 0x6D, True)
    pid = np.full(4, 0.25)
    one = api.simulate_histories(z, Q, pid, 300, nodes=True, maps=True, seed=5)
    two = api.simulate_histories(z, Q, pid, 300, nodes=True, maps=True, seed=5, devices=[0, 0])
    for a, b in zip(one[:3], two[:3]):
        assert np.array_equal(a, b)
    _same_maps(two[3], (one[3].off, one[3].dwell, one[3].state))
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    ze = synth.make_tree(200, Q, Omega, 0x6E)
    o1, m1 = api.sumstatEXP(ze, Q, pid, 300, maps=True, seed=6)
    o2, m2 = api.sumstatEXP(ze, Q, pid, 300, maps=True, seed=6, devices=[0, 0])
    assert np.array_equal(o1, o2)
    _same_maps(m2, (m1.off, m1.dwell, m1.state))


def test_exp_maps_per_branch_means_match_exact():
    n = 4
    Q = synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0) * 0.5
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    pid = np.full(n, 1.0 / n)
    z = synth.make_tree(40, Q, Omega, 0x40A, pid, init_segments=n)
    N = 4096
    _, m = api.sumstatEXP(z, Q, pid, N, maps=True, seed=0x40B)
    _, _, exact = api.expected_sumstat(z, Q, pid, per_branch=True)
    exact = exact[0]                                                        # [E, n + n(n-1)]
    E = m.n_edge
    per = np.zeros((N, E, n + n * (n - 1)))
    per[:, :, :n] = m.mapped_edge(n)
    h, a, b = _pairs(m)
    row = np.repeat(np.arange(m.off.size - 1), np.diff(m.off))
    same = row[:-1] == row[1:]
    br = row[:-1][same] % E
    col = a * (n - 1) + np.where(b > a, b - 1, b)
    np.add.at(per, (h, br, n + col), 1.0)
    mean, sd = per.mean(axis=0), per.std(axis=0, ddof=1)
    se = np.sqrt(np.maximum(sd ** 2, np.where(sd == 0, exact, 0.0)) / N)   # a column never seen: a Poisson bound
    z_ = np.abs(mean - exact) / np.maximum(se, 1e-300)
    z_[(se == 0) & (exact == 0)] = 0.0
    assert np.max(z_) < 5, (np.max(z_), np.unravel_index(np.argmax(z_), z_.shape))


def test_exp_draw_starts_a_chain():
    n = 4
    Q = synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0)
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    pid = np.full(n, 1.0 / n)
    z = synth.make_tree(60, Q, Omega, 0x51A, pid)
    _, m = api.sumstatEXP(z, Q, pid, 8, maps=True, seed=0x51B)
    zt = history_tree(z, m, 3, n=n)
    assert np.array_equal(zt["states"], z["states"])
    out = api.sumstatMCMC(zt, Q, pid, Omega, 300, seed=0x51C)
    assert out.shape[0] == 300 and np.all(np.isfinite(out))
    out2 = api.sumstatEXP(zt, Q, pid, 16, seed=0x51D)
    assert np.all(np.isfinite(out2))
