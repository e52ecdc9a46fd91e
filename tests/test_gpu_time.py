"""Exact expectations through time on the device (phm_expected_through_time) against the Python twin (tests/timeref.py), against
phm_expected_stats' node posteriors, totals and loglik, under chunking and devices, and against sumstatEXP's sampled maps binned
by Maps.through_time."""
import numpy as np
import pytest

import timeref
from phylomap_amd import api, synth
from phylomap_amd.maps import node_depths

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
    lens = lens.copy()
    lens[3] = 0.0                                                           # a zero-length branch
    if shuffled:
        perm = np.random.default_rng(seed).permutation(edge.shape[0])
        edge, lens = edge[perm], lens[perm]
    return {"edge": edge, "edge.length": lens, "Nnode": T - 1, "states": np.ones(T, dtype=np.int32)}


def _tips(z, Q, pid, S, seed, observe=None, missing=0.1):
    tips, _ = api.simulate_histories(z, Q, pid, S, observe=observe, seed=seed)
    rs = np.random.default_rng(seed)
    tips[rs.random(tips.shape) < missing] = 0
    return tips


def _bounds(z):
    """0, internal node depths, points between them, the largest depth and beyond"""
    d = node_depths(z)
    inner = np.sort(d[len(z["states"]):])
    return np.unique(np.concatenate([[0.0], inner[1:6], 0.5 * (inner[1:4] + inner[2:5]), [d.max(), 1.2 * d.max()]]))


def _points(z):
    """every edge row at 0, at t_b and inside"""
    el = np.asarray(z["edge.length"])
    E = el.size
    return np.concatenate([np.arange(E)] * 3), np.concatenate([np.zeros(E), el, 0.4 * el])


def _close(got, want, rtol, atol):
    err = np.abs(got - want)
    assert np.all(err <= rtol * np.abs(want) + atol), (err.max(), np.max(err / np.maximum(np.abs(want), 1e-300)))


@pytest.mark.parametrize("n", [2, 3, 4, 8, 20, 61])
@pytest.mark.parametrize("shuffled", [False, True])
def test_against_the_twin(n, shuffled):
    Q = _model(n)
    z = _tree(16, 0x7E00 + n, shuffled)
    pid = np.arange(1.0, n + 1.0)
    bounds, points = _bounds(z), _points(z)
    E = len(z["edge.length"])
    length = float(np.sum(z["edge.length"]))
    for S, observed in ((1, False), (63, True), (64, False), (130, True)):
        observe = (np.arange(n) % 2 + 1) if observed else None
        tips = _tips(z, Q, pid, S, seed=100 * n + S, observe=observe)
        got = api.expected_through_time(z, Q, pid, bounds=bounds, points=points, sites=tips, observe=observe)
        want = timeref.through_time(z["edge"], z["edge.length"], Q, pid, tips, bounds=bounds, points=points, observe=observe)
        _close(got["occupancy"], want["occupancy"], 0.0, 1e-12)
        _close(got["points"], want["points"], 0.0, 1e-12)
        _close(got["bins"], want["bins"], 1e-12, 1e-14 * length)
        st, ll, post = api.expected_sumstat(z, Q, pid, sites=tips, observe=observe, nodes=True)
        assert np.array_equal(got["loglik"], ll)
        _close(got["points"][:, E:2 * E], post[:, np.asarray(z["edge"])[:, 1] - 1], 0.0, 1e-14)     # pi(t_b): the child's posterior
        np.testing.assert_allclose(got["occupancy"].sum(axis=2), np.broadcast_to(timeref.lineages(z["edge"], z["edge.length"], bounds),
                                                                                (S, bounds.size)), rtol=0, atol=1e-12)
    only = api.expected_through_time(z, Q, pid, points=points, sites=tips, observe=observe)    # one output alone: the same bits
    assert sorted(only) == ["loglik", "points"] and np.array_equal(only["points"], got["points"])


def test_c3_bins_sum_to_the_totals_and_lineages_add_up():
    z, Q, pid, _ = synth.config_problem(3)                                  # 10 000 tips, 4 states
    tips = _tips(z, Q, pid, 1024, seed=0xC3)
    d = node_depths(z)
    bounds = np.linspace(0.0, d.max(), 101)                                # 100 equal bins over the depth
    got = api.expected_through_time(z, Q, pid, bounds=bounds, sites=tips)
    st, ll = api.expected_sumstat(z, Q, pid, sites=tips)
    length = float(np.sum(z["edge.length"]))
    _close(got["bins"].sum(axis=1), st, 1e-11, 1e-14 * length)
    assert np.array_equal(got["loglik"], ll)
    edge = np.asarray(z["edge"])
    dp, dc = d[edge[:, 0] - 1], d[edge[:, 1] - 1]
    alive = np.array([np.sum((dp < t) & (t <= dc)) + (t == 0.0) for t in bounds], dtype=float)
    _close(got["occupancy"].sum(axis=2), np.broadcast_to(alive, (1024, bounds.size)), 1e-12, 0.0)


def test_devices_and_chunks_change_nothing():
    Q = _model(8)
    z = _tree(40, 11, True)
    pid = np.ones(8)
    tips = _tips(z, Q, pid, 130, seed=12)
    args = dict(bounds=_bounds(z), points=_points(z), sites=tips)
    whole = api.expected_through_time(z, Q, pid, **args)
    for opt in ({"devices": [0, 0]}, {"expect_chunk": 5}, {"expect_chunk": 1, "devices": [0, 0]}):
        got = api.expected_through_time(z, Q, pid, **args, **opt)
        for k in whole:
            assert np.array_equal(whole[k], got[k]), (opt, k)


def test_exp_maps_through_time_match_the_exact_values():
    n = 4
    Q = synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0) * 0.5
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    pid = np.full(n, 1.0 / n)
    z = synth.make_tree(40, Q, Omega, 0x40A, pid, init_segments=n)
    N = 4096
    _, m = api.sumstatEXP(z, Q, pid, N, maps=True, seed=0x40B)
    d = node_depths(z)
    bounds = np.unique(np.concatenate([np.linspace(0.0, d.max(), 9), np.sort(d[40:])[1:4]]))
    exact = api.expected_through_time(z, Q, pid, bounds=bounds)
    occ, bins = m.through_time(z, bounds, n)
    for name, draws, ex in (("occupancy", occ, exact["occupancy"][0]), ("bins", bins, exact["bins"][0])):
        mean, sd = draws.mean(axis=0), draws.std(axis=0, ddof=1)
        se = np.sqrt(np.maximum(sd ** 2, np.where(sd == 0, ex, 0.0)) / N)        # a column never seen: a Poisson bound
        z_ = np.abs(mean - ex) / np.maximum(se, 1e-300)
        z_[(se == 0) & (np.abs(mean - ex) < 1e-9)] = 0.0
        assert np.max(z_) < 5, (name, np.max(z_), np.unravel_index(np.argmax(z_), z_.shape))
