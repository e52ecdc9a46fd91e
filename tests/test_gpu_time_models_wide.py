"""Exact expectations through time under many rate matrices at 9..64 states, batched over the models on the device
(phm_expected_through_time_models_wide behind ``api.expected_through_time_models(batched=True)``) against
the Python twin (tests/timeref_models.py: tests/timeref.py per model) with section 16's own bars, against loglik_models,
expected_sumstat_models and ancestral_states_models, across chunks and devices, in both forms of the branch stage, at the special
evaluations, with labels, past 65 535 items of one launch and against the model-by-model route.

The trees are small, because that is where the kernels can go wrong: the 9-tip tree of test_gpu_time_models.py with its edge rows
shuffled and a branch of length 0 (E = 16), and the 6-tip tree of ``manymodelscases`` (E = 10).  The twin of a state count is
computed once for 3 models x the sites its class needs and shared: a call of K models is compared with its first K, a call of S
sites with its first S, a paired call with its (model, site) entries."""
import functools
import os
import re

import numpy as np
import pytest

import branchrowscases as bc
import exactref
import timeref
import timeref_models
from phylomap_amd import api, ratemodel, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = [9, 16, 17, 32, 33, 61, 64]                                          # the first and the unpadded last of each lane class, the codon size
PAST_TILE = (9, 17, 33)                                                       # one n of each class also runs past a workgroup's site tile
T9 = 9
ZERO_EDGE = 3


def lanes(n):
    return 16 if n <= 16 else 32 if n <= 32 else 64


@functools.lru_cache(maxsize=None)
def site_tile(NP):
    """sites of a workgroup of the along and branch stages, G x TMW_SITES, read from the kernels' constants"""
    src = open(os.path.join(ROOT, "phylomap_amd", "csrc", "phm_time_models_wide.h")).read()
    walk = int(re.search(r"constexpr int TMW_SITES = (\d+);", src).group(1))
    m = re.search(r"inline int tmw_groups\(int NP\) \{ return NP == 16 \? (\d+) : (\d+); \}", src)
    return (int(m.group(1)) if NP == 16 else int(m.group(2))) * walk


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
    """(z, Qs [3], pid [3, n], tips [S, T], bounds, points, twin) of a state count; the twin is shared and never changed"""
    z = tree9()
    Qs, pid = bc.models(n, 3)
    S = site_tile(lanes(n)) + 1 if n in PAST_TILE else 3
    tips = bc.sites(n, T9, S=S)
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


def check(got, want, z, what="", bars=1.0):
    occ, pts, bins = errors(got, want, z, what)
    assert occ <= bars and pts <= bars and bins <= bars, (what, occ, pts, bins)


def same(a, b, what=""):
    for name in a._fields:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert np.array_equal(x, y, equal_nan=True), (what, name)


def batched(*args, **kw):
    return api.expected_through_time_models(*args, batched=True, **kw)


@pytest.mark.parametrize("n", STATES)
def test_against_the_twin(n):
    z, Qs, pid, tips, bounds, points, twin = case(n)
    lineages = timeref.lineages(z["edge"], z["edge.length"], bounds)
    site_counts = (1, 3) + ((tips.shape[0],) if n in PAST_TILE else ())
    assert tips.shape[0] == (site_tile(lanes(n)) + 1 if n in PAST_TILE else 3)
    for K in (1, 2, 3):
        for S in site_counts:
            got = batched(z, Qs[:K], pid[:K], sites=tips[:S], bounds=bounds, points=points)
            assert got.loglik.shape == (K, S) and got.occupancy.shape == (K, S, bounds.size, n)
            assert got.bins.shape == (K, S, bounds.size - 1, n * n) and got.point_post.shape == (K, S, points[0].size, n)
            check(got, {k: v[:K, :S] for k, v in twin.items()}, z, f"n={n} K={K} S={S} cross")
            np.testing.assert_allclose(got.loglik, twin["loglik"][:K, :S], rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(got.occupancy.sum(axis=-1), np.broadcast_to(lineages, (K, S, bounds.size)), rtol=0, atol=1e-12)
        som = bc.owner(K, 3)
        got = batched(z, Qs[:K], pid[:K], sites=tips[:3], site_of_model=som, bounds=bounds, points=points)
        assert got.loglik.shape == (K,) and got.bins.shape == (K, bounds.size - 1, n * n)
        check(got, {k: v[np.arange(K), som] for k, v in twin.items()}, z, f"n={n} K={K} paired")


def test_against_the_twin_behind_an_observe_map():
    """a parity ``observe`` map, a missing tip in every site, a prior shared by the models"""
    n, K = 20, 3
    z, Qs, pid, _, bounds, points, _ = case(n)
    observe = bc.parity(n)
    tips = bc.sites(n, T9, S=3, observe=observe, seed=1)
    tips[:, 4] = 0
    want = timeref_models.through_time_models(z["edge"], z["edge.length"], Qs[:K], pid[0], tips, bounds=bounds, points=points, observe=observe)
    got = batched(z, Qs[:K], pid[0], sites=tips, observe=observe, bounds=bounds, points=points)
    check(got, want, z, "observe")


@pytest.mark.parametrize("n", STATES)
def test_identities(n):
    K, S = 3, 3
    z, Qs, pid, tips, bounds, points, _ = case(n)
    tips = tips[:S]
    E = len(z["edge.length"])
    assert E == 16                                                             # one run of the totals: the same order of addition
    got = batched(z, Qs, pid, sites=tips, bounds=bounds, points=points)
    # loglik is loglik_models' bit for bit
    assert np.array_equal(got.loglik, api.loglik_models(z, Qs, pid, sites=tips))
    # one bin over the whole depth: the totals of expected_sumstat_models bit for bit (the restated body and the form rule)
    dmax = float(timeref.depths(z["edge"], z["edge.length"]).max())
    whole = batched(z, Qs, pid, sites=tips, bounds=[0.0, 1.2 * dmax])
    assert whole.point_post is None and whole.bins.shape == (K, S, 1, n * n)
    stats, ll = api.expected_sumstat_models(z, Qs, pid, sites=tips)
    differ = int(np.sum(whole.bins[:, :, 0] != stats))
    print(f"n={n}: one bin against the totals: {differ} of {stats.size} values differ")
    assert differ == 0 and np.array_equal(whole.loglik, ll)
    np.testing.assert_allclose(whole.occupancy[:, :, 0].sum(axis=-1), 1.0, rtol=0, atol=1e-12)       # the root, one lineage
    # the lineages add up, and pi at the ends of a branch is the marginal posterior of the node there
    np.testing.assert_allclose(got.occupancy.sum(axis=-1), np.broadcast_to(timeref.lineages(z["edge"], z["edge.length"], bounds), (K, S, bounds.size)),
                               rtol=0, atol=1e-12)
    anc = api.ancestral_states_models(z, Qs, pid, sites=tips, joint=False)
    edge = np.asarray(z["edge"])
    at_parent, at_child = got.point_post[:, :, :E], got.point_post[:, :, E:2 * E]
    e0 = float(np.max(np.abs(at_parent - anc.node_post[:, :, edge[:, 0] - 1])))
    e1 = float(np.max(np.abs(at_child - anc.node_post[:, :, edge[:, 1] - 1])))
    print(f"n={n}: pi(0) against the parent's posterior {e0:.3g}, pi(t_b) against the child's {e1:.3g}")
    assert e0 <= 1e-14 and e1 <= 1e-14
    # chunks of models, sites and items, and two shards, change no bit
    for opt in ({"expect_chunk": 1}, {"expect_chunk": 5}, {"devices": [0, 0]}):
        same(batched(z, Qs, pid, sites=tips, bounds=bounds, points=points, **opt), got, str(opt))
    # one output alone: the same bits
    only = batched(z, Qs, pid, sites=tips, points=points)
    assert only.occupancy is None and only.bins is None and np.array_equal(only.point_post, got.point_post)
    only = batched(z, Qs, pid, sites=tips, bounds=bounds)
    assert only.point_post is None and np.array_equal(only.bins, got.bins) and np.array_equal(only.occupancy, got.occupancy)
    # row k of the call of three models is the call on model k alone
    for k in range(K):
        one = batched(z, Qs[k:k + 1], pid[k:k + 1], sites=tips, bounds=bounds, points=points)
        for name in got._fields:
            assert np.array_equal(getattr(got, name)[k], getattr(one, name)[0]), (k, name)


@pytest.mark.parametrize("n", [9, 33])
def test_both_forms_of_the_branch_stage(n):
    """max(-q_ii) t on the longest branch just below and just above the switch between the short and the long form (17.1), and
    near 2 000, where the weights of both kernels pass 2^512 several times before their sums end"""
    z, Qs, pid, tips, bounds, points, _ = case(n)
    tips = tips[:3]
    longest = float(np.max(z["edge.length"]))
    Qs = Qs.copy()
    for k, x in enumerate((17.0, 17.2, 2000.0)):
        Qs[k] *= x / (float(np.max(-np.diag(Qs[k]))) * longest)
    dmax = float(timeref.depths(z["edge"], z["edge.length"]).max())
    whole = np.array([0.0, 1.2 * dmax])                                        # whole branches: h = t_b, the longest on either side
    want = timeref_models.through_time_models(z["edge"], z["edge.length"], Qs, pid, tips, bounds=bounds, points=points)
    got = batched(z, Qs, pid, sites=tips, bounds=bounds, points=points)
    for k, x in enumerate((17.0, 17.2, 2000.0)):
        check(api.ThroughTimeModels(*(v[k:k + 1] for v in got)), {key: v[k:k + 1] for key, v in want.items()}, z, f"n={n} mu t = {x}")
    want = timeref_models.through_time_models(z["edge"], z["edge.length"], Qs, pid, tips, bounds=whole, points=points)
    got = batched(z, Qs, pid, sites=tips, bounds=whole, points=points)
    check(got, want, z, f"n={n} whole branches")
    stats, _ = api.expected_sumstat_models(z, Qs, pid, sites=tips)             # both forms are the totals' forms, bit for bit
    assert np.array_equal(got.bins[:, :, 0], stats)


def test_an_impossible_evaluation_and_a_model_that_leaves_no_state():
    n, K, S = 9, 3, 3
    z, Qs, pid, tips, bounds, points, _ = case(n)
    tips = tips[:S].copy()
    tips[0] = 1                                                                # site 0: every tip in state 1, one missing
    tips[0, 2] = 0
    assert len(set(tips[1][tips[1] > 0])) > 1 and len(set(tips[2][tips[2] > 0])) > 1
    still = 1
    Qs = Qs.copy()
    Qs[still] = 0.0                                                            # max(-q_ii) = 0: P = I, impossible on sites 1 and 2
    got = batched(z, Qs, pid, sites=tips, bounds=bounds, points=points)
    assert np.isfinite(got.loglik[still, 0]) and np.all(np.isneginf(got.loglik[still, 1:]))
    for x in (got.occupancy, got.bins, got.point_post):
        assert np.all(np.isnan(x[still, 1:])) and np.all(np.isfinite(np.delete(x, still, axis=0))) and np.all(np.isfinite(x[still, 0]))
    keep = np.arange(K) != still                                               # the neighbours: the call without that model, bit for bit
    without = batched(z, Qs[keep], pid[keep], sites=tips, bounds=bounds, points=points)
    for name in got._fields:
        assert np.array_equal(getattr(got, name)[keep], getattr(without, name)), name
    # the model that leaves no state on the site it can explain: state 1 everywhere, the dwell of a bin is the length inside it
    unit = np.zeros(n)
    unit[0] = 1.0
    assert np.array_equal(got.point_post[still, 0], np.tile(unit, (points[0].size, 1)))
    assert np.array_equal(got.occupancy[still, 0, :, 0], timeref.lineages(z["edge"], z["edge.length"], bounds))
    assert not np.any(got.occupancy[still, 0, :, 1:]) and not np.any(got.bins[still, 0, :, 1:])
    inside = np.zeros(bounds.size - 1)
    for k, _, s1, s2 in timeref.sub_branches(z["edge"], z["edge.length"], bounds):
        inside[k] += s2 - s1
    np.testing.assert_allclose(got.bins[still, 0, :, 0], inside, rtol=1e-12, atol=0)


def test_a_structurally_zero_rate_gives_an_exact_zero():
    n = 9
    z, Qs, pid, tips, bounds, points, _ = case(n)
    tips = tips[:3]
    Qs = Qs.copy()
    k, i, j = 0, 2, 0
    Qs[k, i, i] += Qs[k, i, j]                                                 # the row still sums to 0
    Qs[k, i, j] = 0.0
    Qs[k + 1, i, j] = max(Qs[k + 1, i, j], 0.05)
    Qs[k + 1, i, i] = 0.0
    Qs[k + 1, i, i] = -Qs[k + 1, i].sum()
    got = batched(z, Qs, pid, sites=tips, bounds=bounds, points=points)
    col = n + exactref.columns(n).index((i, j))
    assert np.all(got.bins[k, :, :, col] == 0.0) and np.all(got.bins[k + 1, :, :-1, col] > 0.0)
    want = timeref_models.through_time_models(z["edge"], z["edge.length"], Qs, pid, tips, bounds=bounds, points=points)
    check(got, want, z, "zero rate")


@pytest.mark.parametrize("n", [20, 61])
def test_labelled_bins_are_the_column_loop_over_the_full_rows(n):
    K, S = 3, 3
    z = tree9()
    Qs, pid = bc.models(n, K)
    tips = bc.sites(n, T9, S=S)
    bounds = bounds_of(z)
    if n == 20:
        rs = np.random.default_rng(0xB29 + n)
        labels = np.stack([rs.uniform(-1.0, 1.0, (n, n)), rs.uniform(0.0, 1.0, (n, n))])
    else:                                                                      # what a codon model is asked for: counts of chosen changes
        labels = np.stack([ratemodel.count_labels(n, [(0, 1), (1, 0), (5, 60), (60, 60)]), ratemodel.observed_change_labels(bc.parity(n))])
    full = batched(z, Qs, pid, sites=tips, bounds=bounds)
    got = batched(z, Qs, pid, sites=tips, bounds=bounds, labels=labels)
    assert got.bins.shape == (K, S, bounds.size - 1, 2) and np.array_equal(got.occupancy, full.occupancy)
    assert np.array_equal(got.loglik, full.loglik)
    assert np.array_equal(got.bins, bc.label_reduce(full.bins, labels))
    som = bc.owner(K, S)
    paired = batched(z, Qs, pid, sites=tips, site_of_model=som, bounds=bounds, labels=labels[1])
    assert paired.bins.shape == (K, bounds.size - 1, 1)
    assert np.array_equal(paired.bins[..., 0], got.bins[np.arange(K), som][..., 1])
    for opt in ({"expect_chunk": 1}, {"devices": [0, 0]}):
        same(batched(z, Qs, pid, sites=tips, bounds=bounds, labels=labels, **opt), got, str(opt))


def test_items_past_one_launch():
    """66 000 caller's points on the 6-tip tree: the second launch starts at item 65 535.  The points repeat with period 30, so
    every posterior of the second launch has a bit-identical copy in the first; the twin is asked at the first, the last and the
    points on both sides of the launch boundary"""
    n, P, period = 9, 66000, 30
    z = bc.tree6()
    Qs, pid = bc.models(n, 1)
    tips = bc.sites(n, 6, S=1)
    base = points_of(z)
    assert base[0].size == period
    pe, pp = np.resize(base[0], P), np.resize(base[1], P)
    got = batched(z, Qs, pid, sites=tips, points=(pe, pp))
    assert got.point_post.shape == (1, 1, P, n) and got.occupancy is None and got.bins is None
    post = got.point_post[0, 0]
    assert np.array_equal(post, np.resize(post[:period], (P, n)))
    at = np.array([0, 65533, 65534, 65535, 65536, P - 1])
    want = timeref.through_time(z["edge"], z["edge.length"], Qs[0], pid[0], tips, points=(pe[at], pp[at]))["points"][0]
    err = float(np.max(np.abs(post[at] - want)))
    print(f"points past one launch: {err:.3g} against 1e-12")
    assert err <= 1e-12


@pytest.mark.parametrize("n", [9, 20])
def test_against_the_model_by_model_route(n):
    """the link between the two routes: each is within one bar of the twin, and they are within two bars of each other"""
    z, Qs, pid, tips, bounds, points, twin = case(n)
    tips = tips[:3]
    want = {k: v[:, :3] for k, v in twin.items()}
    new = batched(z, Qs, pid, sites=tips, bounds=bounds, points=points)
    old = api.expected_through_time_models(z, Qs, pid, sites=tips, bounds=bounds, points=points)
    check(new, want, z, f"n={n} batched against the twin")
    check(old, want, z, f"n={n} model by model against the twin")
    check(new, {"occupancy": old.occupancy, "bins": old.bins, "points": old.point_post}, z, f"n={n} batched against model by model", bars=2.0)
    np.testing.assert_allclose(new.loglik, old.loglik, rtol=1e-12, atol=1e-12)
