"""Exact expectations through time under many rate matrices on the device (phm_expected_through_time_models, DESIGN.md section
28) against the Python twin (tests/timeref_models.py: tests/timeref.py per model) with section 16's own bars, against
loglik_models, expected_sumstat_models and ancestral_states_models, across lanes, chunks and devices, at the special evaluations,
through the 9..64-state route and past 65 535 items of one launch.

The trees are small, because that is where the kernels can go wrong: a 9-tip tree with its edge rows shuffled and a branch of
length 0 (E = 16), and the 6-tip tree of ``manymodelscases`` (E = 10).  The twin of a state count is computed once for 130 models
x 3 sites and shared: a call of K models is compared with its first K, a call of one site with its first, a paired call with its
(model, site) entries."""
import functools

import numpy as np
import pytest

import branchrowscases as bc
import exactref
import timeref
import timeref_models
from phylomap_amd import api, synth

pytestmark = pytest.mark.gpu

STATES = [2, 3, 4, 5, 8]                                                      # both register classes (n <= 4, 5..8) and their edges
KS = [1, 63, 64, 65, 130]                                                     # lane padding and a second wave
T9 = 9
ZERO_EDGE = 3


@functools.lru_cache(maxsize=None)
def tree9():
    edge, lens = synth.random_tree(T9, 1.0, 0x7A9)
    perm = np.random.default_rng(0x7A9).permutation(edge.shape[0])
    edge, lens = edge[perm], lens[perm].copy()
    lens[ZERO_EDGE] = 0.0
    return {"edge": edge, "edge.length": lens, "Nnode": T9 - 1, "states": np.ones(T9, dtype=np.int32)}


def bounds_of(z):
    """0, exactly on two node depths, inside, the largest depth and past it"""
    d = timeref.depths(z["edge"], z["edge.length"])
    inner = np.unique(d[len(z["states"]):])
    inner = inner[inner > 0.0]
    return np.unique(np.concatenate([[0.0], inner[:2], [0.5 * (inner[0] + inner[1]), 0.37 * d.max(), d.max(), 1.2 * d.max()]]))


def points_of(z):
    """every edge row at 0, at t_b and inside"""
    el = np.asarray(z["edge.length"])
    E = el.size
    return np.concatenate([np.arange(E)] * 3).astype(np.int32), np.concatenate([np.zeros(E), el, 0.4 * el])


@functools.lru_cache(maxsize=None)
def case(n):
    """(z, Qs [130], pid [130, n], tips [3, T], bounds, points, twin) of a state count; the twin is shared and never changed"""
    z = tree9()
    Qs, pid = bc.models(n, 130)
    tips = bc.sites(n, T9, S=3)
    bounds, points = bounds_of(z), points_of(z)
    twin = timeref_models.through_time_models(z["edge"], z["edge.length"], Qs, pid, tips, bounds=bounds, points=points)
    for v in twin.values():
        v.setflags(write=False)
    return z, Qs, pid, tips, bounds, points, twin


def errors(got, want, z, what=""):
    """the three figures of section 16's bars, each as error / allowance (<= 1 passes); printed before anything is asserted"""
    length = float(np.sum(z["edge.length"]))
    occ = float(np.max(np.abs(got.occupancy - want["occupancy"]))) / 1e-12
    pts = float(np.max(np.abs(got.point_post - want["points"]))) / 1e-12
    bins = float(np.max(np.abs(got.bins - want["bins"]) / (1e-12 * np.abs(want["bins"]) + 1e-14 * length)))
    print(f"{what}: occupancy {occ:.3g}, points {pts:.3g}, bins {bins:.3g} of the allowance")
    return occ, pts, bins


def check(got, want, z, what=""):
    occ, pts, bins = errors(got, want, z, what)
    assert occ <= 1.0 and pts <= 1.0 and bins <= 1.0, (what, occ, pts, bins)


def same(a, b, what=""):
    for name in a._fields:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert np.array_equal(x, y, equal_nan=True), (what, name)


@pytest.mark.parametrize("n", STATES)
def test_against_the_twin(n):
    z, Qs, pid, tips, bounds, points, twin = case(n)
    lineages = timeref.lineages(z["edge"], z["edge.length"], bounds)
    for K in KS:
        for S in (1, 3):
            got = api.expected_through_time_models(z, Qs[:K], pid[:K], sites=tips[:S], bounds=bounds, points=points)
            assert got.loglik.shape == (K, S) and got.occupancy.shape == (K, S, bounds.size, n)
            assert got.bins.shape == (K, S, bounds.size - 1, n * n) and got.point_post.shape == (K, S, points[0].size, n)
            check(got, {k: v[:K, :S] for k, v in twin.items()}, z, f"n={n} K={K} S={S} cross")
            np.testing.assert_allclose(got.loglik, twin["loglik"][:K, :S], rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(got.occupancy.sum(axis=-1), np.broadcast_to(lineages, (K, S, bounds.size)), rtol=0, atol=1e-12)
        som = bc.owner(K, 3)
        got = api.expected_through_time_models(z, Qs[:K], pid[:K], sites=tips, site_of_model=som, bounds=bounds, points=points)
        assert got.loglik.shape == (K,) and got.bins.shape == (K, bounds.size - 1, n * n)
        check(got, {k: v[np.arange(K), som] for k, v in twin.items()}, z, f"n={n} K={K} paired")


def test_against_the_twin_behind_an_observe_map():
    """a parity ``observe`` map, a missing tip in every site, a prior shared by the models"""
    n, K = 4, 65
    z, Qs, pid, _, bounds, points, _ = case(n)
    observe = bc.parity(n)
    tips = bc.sites(n, T9, S=3, observe=observe, seed=1)
    tips[:, 4] = 0
    want = timeref_models.through_time_models(z["edge"], z["edge.length"], Qs[:K], pid[0], tips, bounds=bounds, points=points, observe=observe)
    got = api.expected_through_time_models(z, Qs[:K], pid[0], sites=tips, observe=observe, bounds=bounds, points=points)
    check(got, want, z, "observe")


@pytest.mark.parametrize("n", STATES)
def test_identities(n):
    K, S = 65, 3
    z, Qs, pid, tips, bounds, points, _ = case(n)
    Qs, pid = Qs[:K], pid[:K]
    E = len(z["edge.length"])
    length = float(np.sum(z["edge.length"]))
    got = api.expected_through_time_models(z, Qs, pid, sites=tips, bounds=bounds, points=points)
    # 1. loglik is loglik_models' bit for bit
    assert np.array_equal(got.loglik, api.loglik_models(z, Qs, pid, sites=tips))
    # 2. one bin over the whole depth: the totals of expected_sumstat_models (another order of addition)
    dmax = float(timeref.depths(z["edge"], z["edge.length"]).max())
    whole = api.expected_through_time_models(z, Qs, pid, sites=tips, bounds=[0.0, 1.2 * dmax])
    assert whole.point_post is None and whole.bins.shape == (K, S, 1, n * n)
    stats, ll = api.expected_sumstat_models(z, Qs, pid, sites=tips)
    err = np.abs(whole.bins[:, :, 0] - stats) / (1e-12 * np.abs(stats) + 1e-14 * length)
    print(f"n={n}: one bin against the totals: {np.max(err):.3g} of the allowance")
    assert np.max(err) <= 1.0 and np.array_equal(whole.loglik, ll)
    np.testing.assert_allclose(whole.occupancy[:, :, 0].sum(axis=-1), 1.0, rtol=0, atol=1e-12)       # the root, one lineage
    # 3. the lineages add up, and pi at the ends of a branch is the marginal posterior of the node there
    np.testing.assert_allclose(got.occupancy.sum(axis=-1), np.broadcast_to(timeref.lineages(z["edge"], z["edge.length"], bounds), (K, S, bounds.size)),
                               rtol=0, atol=1e-12)
    anc = api.ancestral_states_models(z, Qs, pid, sites=tips, joint=False)
    edge = np.asarray(z["edge"])
    at_parent, at_child = got.point_post[:, :, :E], got.point_post[:, :, E:2 * E]
    e0 = float(np.max(np.abs(at_parent - anc.node_post[:, :, edge[:, 0] - 1])))
    e1 = float(np.max(np.abs(at_child - anc.node_post[:, :, edge[:, 1] - 1])))
    print(f"n={n}: pi(0) against the parent's posterior {e0:.3g}, pi(t_b) against the child's {e1:.3g}")
    assert e0 <= 1e-14 and e1 <= 1e-14
    # 5. chunks of models, sites and items, and two shards, change no bit
    for opt in ({"expect_chunk": 1}, {"expect_chunk": 5}, {"devices": [0, 0]}):
        same(api.expected_through_time_models(z, Qs, pid, sites=tips, bounds=bounds, points=points, **opt), got, str(opt))
    # one output alone: the same bits
    only = api.expected_through_time_models(z, Qs, pid, sites=tips, points=points)
    assert only.occupancy is None and only.bins is None and np.array_equal(only.point_post, got.point_post)


@pytest.mark.parametrize("n", STATES)
def test_a_lane_does_not_depend_on_its_neighbours(n):
    """4. row k of a call of 130 models is the call on model k alone, bit for bit"""
    z, Qs, pid, tips, bounds, points, _ = case(n)
    many = api.expected_through_time_models(z, Qs, pid, sites=tips, bounds=bounds, points=points)
    for k in (0, 63, 64, 129):
        one = api.expected_through_time_models(z, Qs[k:k + 1], pid[k:k + 1], sites=tips, bounds=bounds, points=points)
        for name in many._fields:
            assert np.array_equal(getattr(many, name)[k], getattr(one, name)[0]), (k, name)


def test_an_impossible_evaluation_and_a_model_that_leaves_no_state():
    n, K, S = 4, 65, 3
    z, Qs, pid, tips, bounds, points, _ = case(n)
    tips = tips.copy()
    tips[0] = 1                                                                # site 0: every tip in state 1, one missing
    tips[0, 2] = 0
    assert len(set(tips[1][tips[1] > 0])) > 1 and len(set(tips[2][tips[2] > 0])) > 1
    still = 40
    Qs = Qs[:K].copy()
    Qs[still] = 0.0                                                            # max(-q_ii) = 0: P = I, impossible on sites 1 and 2
    got = api.expected_through_time_models(z, Qs, pid[:K], sites=tips, bounds=bounds, points=points)
    assert np.isfinite(got.loglik[still, 0]) and np.all(np.isneginf(got.loglik[still, 1:]))
    for x in (got.occupancy, got.bins, got.point_post):
        assert np.all(np.isnan(x[still, 1:])) and np.all(np.isfinite(np.delete(x, still, axis=0))) and np.all(np.isfinite(x[still, 0]))
    keep = np.arange(K) != still                                               # the neighbours: the call without that model, bit for bit
    without = api.expected_through_time_models(z, Qs[keep], pid[:K][keep], sites=tips, bounds=bounds, points=points)
    for name in got._fields:
        assert np.array_equal(getattr(got, name)[keep], getattr(without, name)), name
    # the model that leaves no state on the site it can explain: state 1 everywhere, the dwell of a bin is the length inside it
    assert np.array_equal(got.point_post[still, 0], np.tile([1.0, 0.0, 0.0, 0.0], (points[0].size, 1)))
    assert np.array_equal(got.occupancy[still, 0, :, 0], timeref.lineages(z["edge"], z["edge.length"], bounds))
    assert not np.any(got.occupancy[still, 0, :, 1:]) and not np.any(got.bins[still, 0, :, 1:])
    inside = np.zeros(bounds.size - 1)
    for k, _, s1, s2 in timeref.sub_branches(z["edge"], z["edge.length"], bounds):
        inside[k] += s2 - s1
    np.testing.assert_allclose(got.bins[still, 0, :, 0], inside, rtol=1e-12, atol=0)


def test_a_structurally_zero_rate_gives_an_exact_zero():
    n, K = 4, 65
    z, Qs, pid, tips, bounds, points, _ = case(n)
    Qs = Qs[:K].copy()
    k, i, j = 17, 2, 0
    Qs[k, i, i] += Qs[k, i, j]                                                 # the row still sums to 0
    Qs[k, i, j] = 0.0
    Qs[k + 1, i, j] = max(Qs[k + 1, i, j], 0.05)
    Qs[k + 1, i, i] = 0.0
    Qs[k + 1, i, i] = -Qs[k + 1, i].sum()
    got = api.expected_through_time_models(z, Qs, pid[:K], sites=tips, bounds=bounds, points=points)
    col = n + exactref.columns(n).index((i, j))
    assert np.all(got.bins[k, :, :, col] == 0.0) and np.all(got.bins[k + 1, :, :-1, col] > 0.0)
    want = timeref_models.through_time_models(z["edge"], z["edge.length"], Qs[k:k + 2], pid[k:k + 2], tips, bounds=bounds, points=points)
    check(api.ThroughTimeModels(*(x[k:k + 2] for x in got)), want, z, "zero rate")


def test_a_fast_branch_runs_the_rescaling_and_the_stopping_rule():
    """max(-q_ii) t_b near 2 000 on the longest branch: the weights pass 2^512 several times before the sum ends"""
    n = 4
    z, Qs, pid, tips, bounds, points, _ = case(n)
    Qs = Qs[:2].copy()
    Qs[1] *= 2000.0 / (float(np.max(-np.diag(Qs[1]))) * float(np.max(z["edge.length"])))
    want = timeref_models.through_time_models(z["edge"], z["edge.length"], Qs, pid[:2], tips, bounds=bounds, points=points)
    got = api.expected_through_time_models(z, Qs, pid[:2], sites=tips, bounds=bounds, points=points)
    check(got, want, z, "mu t = 2000")


@pytest.mark.parametrize("n", [9, 20])
def test_wide_states_are_served_model_by_model(n):
    """9..64 states: each model's values are expected_through_time's bit for bit (the same machinery)"""
    z = bc.tree6()
    K = 3
    Qs, pid = bc.models(n, K)
    tips = bc.sites(n, 6, S=3)
    bounds, points = bounds_of(z), points_of(z)
    got = api.expected_through_time_models(z, Qs, pid, sites=tips, bounds=bounds, points=points)
    som = np.array([2, 0, 2], dtype=np.int32)
    paired = api.expected_through_time_models(z, Qs, pid, sites=tips, site_of_model=som, bounds=bounds, points=points)
    for k in range(K):
        one = api.expected_through_time(z, Qs[k], pid[k], bounds=bounds, points=points, sites=tips)
        for name, key in (("loglik", "loglik"), ("occupancy", "occupancy"), ("bins", "bins"), ("point_post", "points")):
            assert np.array_equal(getattr(got, name)[k], one[key]), (k, name)
            assert np.array_equal(getattr(paired, name)[k], one[key][som[k]]), (k, name)


def test_items_past_one_launch():
    """66 000 caller's points on the 6-tip tree: the second launch starts at item 65 535.  The points repeat with period 30, so
    every posterior of the second launch has a bit-identical copy in the first; the twin is asked at the first, the last and the
    points on both sides of the launch boundary"""
    n, P, period = 3, 66000, 30
    z = bc.tree6()
    Qs, pid = bc.models(n, 1)
    tips = bc.sites(n, 6, S=1)
    base = points_of(z)
    assert base[0].size == period
    pe, pp = np.resize(base[0], P), np.resize(base[1], P)
    got = api.expected_through_time_models(z, Qs, pid, sites=tips, points=(pe, pp))
    assert got.point_post.shape == (1, 1, P, n) and got.occupancy is None and got.bins is None
    post = got.point_post[0, 0]
    assert np.array_equal(post, np.resize(post[:period], (P, n)))
    at = np.array([0, 65533, 65534, 65535, 65536, P - 1])
    want = timeref.through_time(z["edge"], z["edge.length"], Qs[0], pid[0], tips, points=(pe[at], pp[at]))["points"][0]
    err = float(np.max(np.abs(post[at] - want)))
    print(f"points past one launch: {err:.3g} against 1e-12")
    assert err <= 1e-12
