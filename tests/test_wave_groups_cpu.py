"""What the shapes of tests/test_gpu_wave_groups.py reach in the persistent kernels (tests/wavegroups.py restates the host's
formulas): a wave item of several branches, a last item cut short, a second trip of the persistent loop -- and that no other exact
test reaches any of them.  The formulas are pinned to their values at the time of writing: if one of these tests fails after a
heuristic was retuned, move the shapes in wavegroups.py until the properties asserted here hold again; do not relax them."""
import numpy as np
import pytest

import samplecases as sc
import wavegroups as wg
from phylomap_amd import synth


def test_the_formulas_at_their_corners():
    assert wg.sampler_launch(46, 1)["group"] == 1 and wg.sampler_launch(46, 178)["group"] == 1
    assert wg.sampler_launch(46, 179)["group"] == 1 and wg.sampler_launch(46, 357)["group"] == 2      # 46 * 357 = 16 422 >= 16 384
    assert wg.sampler_launch(46, 356)["group"] == 1
    assert wg.sampler_launch(46, 100000)["group"] == 16
    assert wg.sampler_launch(46, 1)["waves"] == 48 and wg.sampler_launch(46, 178)["waves"] == 8188
    assert wg.sampler_launch(46, 179)["waves"] == 8192 and wg.sampler_launch(46, 179)["second_trip"]  # 8 234 items, group still 1
    assert wg.group_sizes(46, 3) == [3] * 15 + [1] and wg.group_sizes(32, 3) == [3] * 10 + [2] and wg.group_sizes(10, 9) == [9, 1]
    lv = wg.simulate_launches([32], 64 * 512)
    assert lv[0]["group"] == 2 and not lv[0]["short_last"] and lv[0]["waves"] == lv[0]["items"] == 16 * 512
    assert wg.simulate_launches([32], 64 * 774, expect_chunk=2)[0]["group"] == 2


@pytest.mark.parametrize("paired", [False, True])
def test_sample_histories_shape(paired):
    K, S = wg.SAMPLE_KS[paired]
    D = wg.SAMPLE_D
    n_eval = K if paired else K * S                        # site_of_model: one evaluation per model
    E = sc.tree()[0].shape[0]
    assert E == 46 and D % 64 == 14 and n_eval == 10
    tiles = wg.tiles_of_sample(n_eval, D)
    assert tiles == [550]
    a = wg.sampler_launch(E, tiles[0])
    assert a["group"] == 3 and a["sizes"] == [3] * 15 + [1] and a["short_last"]
    assert a["items"] == 8800 and a["waves"] == 8192 and a["second_trip"] and a["second_items"] == 608
    chunks = wg.tiles_of_sample(n_eval, D, wg.CHUNK_SAMPLE)
    assert chunks == [64] * 8 + [38]
    for t in chunks:                                       # what it is compared with: one branch per item, one item per wave
        b = wg.sampler_launch(E, t)
        assert b["group"] == 1 and not b["second_trip"]


def test_long_branch_shape():
    edge, _ = synth.random_tree(6, 0.3, 9)
    E = edge.shape[0]
    assert E == 10
    tiles = wg.tiles_of_sample(3, wg.LONG_D)
    assert len(tiles) == 1
    a = wg.sampler_launch(E, tiles[0])
    assert a["group"] >= 3 and a["short_last"] and a["second_trip"]
    assert wg.LONG_D != 160000 or (tiles == [7500] and a["group"] == 9 and a["sizes"] == [9, 1] and a["items"] == 15000)
    for t in wg.tiles_of_sample(3, wg.LONG_D, wg.CHUNK_SAMPLE):
        b = wg.sampler_launch(E, t)
        assert b["group"] == 1 and not b["second_trip"]


def test_posterior_rates_shape():
    tiles = wg.tiles_of_gibbs(wg.GIBBS_CHAINS, wg.GIBBS_SITES)
    assert tiles == [537] and 179 * 64 - wg.GIBBS_CHAINS == 36
    a = wg.sampler_launch(46, tiles[0])
    assert a["group"] == 3 and a["sizes"][-1] == 1 and a["short_last"]
    assert a["items"] == 8592 and a["waves"] == 8192 and a["second_trip"]
    chunks = wg.tiles_of_gibbs(wg.GIBBS_CHAINS, wg.GIBBS_SITES, wg.CHUNK_GIBBS)
    assert chunks == [96] * 5 + [57]
    for t in chunks:
        b = wg.sampler_launch(46, t)
        assert b["group"] == 1 and not b["second_trip"]


@pytest.mark.parametrize("shuffle", [False, True])
def test_complete_tree_and_the_simulation_shape(shuffle):
    edge, lens = wg.complete_tree(shuffle=shuffle)
    T = 32
    assert edge.shape == (62, 2) and lens.shape == (62,) and np.sum(lens == 0.0) == 1 and lens.min() == 0.0
    assert len(np.unique(np.round(lens, 12))) == 62
    assert sorted(edge[:, 1].tolist()) == [v for v in range(1, 64) if v != T + 1]       # every node but the root is a child once
    assert np.all(np.bincount(edge[:, 0], minlength=64)[T + 1:] == 2) and np.all(edge[:, 0] > T)
    levels = wg.level_counts(edge)
    assert levels == [2, 4, 8, 16, 32]
    plain = wg.complete_tree()
    if shuffle:
        assert not np.array_equal(edge, plain[0])
        assert sorted(map(tuple, np.column_stack([edge, lens]).tolist())) == sorted(map(tuple, np.column_stack(plain).tolist()))
    else:                                                  # pre-order: every parent is the root or the child of an earlier row
        seen = {T + 1}
        for p, c in edge.tolist():
            assert p in seen
            seen.add(c)
        assert edge[0].tolist() == [T + 1, T + 2] and lens[5] == 0.0
    K, R = wg.SIM_KR
    assert K * R == 49500 and R % 64 != 0
    lv = wg.simulate_launches(levels, K * R)
    assert [x["group"] for x in lv] == [1, 1, 1, 1, 3]
    assert lv[4]["sizes"] == [3] * 10 + [2] and lv[4]["short_last"] and lv[4]["items"] == 11 * 774
    assert not any(x["second_trip"] for x in lv)           # the level grid covers its items up to 262 144 of them
    for x in wg.simulate_launches(levels, wg.CHUNK_SIM, wg.CHUNK_SIM):
        assert x["group"] == 1 and not x["second_trip"]


def test_every_other_exact_shape_is_ungrouped():
    """the gap the shapes above close: 46 edges and at most 30 tiles, or levels of at most about ten edges"""
    for t in range(1, 31):
        a = wg.sampler_launch(46, t)
        assert a["group"] == 1 and not a["second_trip"]
    a = wg.sampler_launch(10, 3)                           # test_long_branch: 3 models x 64 draws
    assert a["group"] == 1 and not a["second_trip"]
    for shuffle in (False, True):
        levels = wg.level_counts(sc.tree(shuffle=shuffle)[0])
        assert sum(levels) == 46 and max(levels) <= 12
        for h in (1, 65, 130, 210):                        # test_gpu_simulate_models.KR: K * R histories
            assert all(x["group"] == 1 and not x["second_trip"] for x in wg.simulate_launches(levels, h))
    levels = wg.level_counts(synth.random_tree(40, 1.0, 0x40)[0])                       # the closed-form test: 3 x 4 096 histories
    assert all(x["group"] == 1 for x in wg.simulate_launches(levels, 3 * 4096))
    # Grouped sampler calls before these tests.  test_statistics_on_the_device, 78 edges x 512 tiles: held to z-scores only.
    assert wg.sampler_launch(78, 4 * 128)["group"] == 4
    # test_fit_to_models_to_maps_to_a_chain, 200 tips x 64 evaluations of one draw: held to the sum of its dwell columns only.
    assert wg.sampler_launch(398, 64)["group"] == 3
    # test_gpu_gibbs.check_rows replaying 130 joint chains x 3 sites at D = 1: 390 tiles of ONE valid lane each, pairs of branches
    # without a remainder, held to the packed form (9 tiles, ungrouped) in counts and dwell sums, not in nodes or maps.
    a = wg.sampler_launch(46, 130 * 3)
    assert a["group"] == 2 and not a["short_last"] and wg.sampler_launch(46, wg.tiles_of_gibbs(130, 3)[0])["group"] == 1
