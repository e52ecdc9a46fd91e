"""What tests/test_gpu_mcmc_maps_classes.py relies on, checked without a GPU: the cases of tests/mcmcmapsclasses.py are cases -- the
oracle's maps of the compared replicas hold interior segments (drawn states, neither end of their branch) in every block of eight
states the replay's block scan can land in and in state n - 1, so a replay that scans or walks wrongly cannot agree by having
nothing to draw; every case lands in the wt_branch_kernel instantiation it is listed for and all ten are reached; the new cases are
what they are named for; and the Python twin equals the oracle's maps where the twin is affordable."""
import numpy as np
import pytest

import mcmcmapsclasses as M
import rateupdatecases as RC
import wtilesclasses as W

ALL = M.all_cases()
IDS = [c.name for c in ALL]


def test_case_list_is_the_class_files_and_four_more():
    names = [c.name for c in ALL]
    assert len(names) == len(set(names)) == 86
    want = {c.name for c in W.all_cases() if not c.name.endswith("ladder")}
    assert len(want) == 78 and want <= set(names)
    assert sorted(c.name for c in ALL if c.family == "ladder") == ["band1_n29_ladder", "band1_n32_ladder", "band2_n12_ladder", "band2_n9_ladder"]
    assert [c.name for c in ALL[-4:]] == ["sparse_mixed_n12", "sparse_mixed_n36", "long_n17", "long_n40"]
    for c in ALL:
        assert all("reduce" not in r for r in c.runs) and len(c.runs) >= 1
        assert c.S in (70, 150) and c.replicas[-1] == c.S - 1 and {0, 63, 64} <= set(c.replicas)       # a full tile and a short last one
        assert 11 <= len(c.z["states"]) <= 14 or (c.family == "ladder" and len(c.z["states"]) == 300)
    for c in ALL:
        if c.family == "b2l":
            assert [r["branch_group"] for r in c.runs] == [1, 4, 64] and c.n_edge == 26 and c.n_edge % 4 == 2
    assert {c.n for c in ALL if c.family == "dense"} >= {9, 17, 33, 57, 16, 32, 64}                  # one state, eight states in the last block


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_case_lands_in_the_branch_kernel_it_is_listed_for(case):
    assert len(case.listed) == len(case.runs)
    for run, name in zip(case.runs, case.listed):
        assert name in W.ALL_CLASSES and case.n in W.ALL_CLASSES[name]
        ks = case.kernels(run)
        assert name in ks and sum(k.startswith("wt_branch_kernel") for k in ks) == 1, (case.name, run, sorted(ks))


def test_all_ten_branch_kernels_are_reached():
    ten = {k for k in W.ALL_CLASSES if k.startswith("wt_branch_kernel")}
    assert len(ten) == 10
    assert {name for c in ALL for name in c.listed} == ten


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_oracle_maps_hold_drawn_states_in_every_block_of_eight(case):
    """over the compared replicas and all iterations: interior segments in every block of eight states, state n - 1 among them
    beyond eight states (band1_n5_random never draws state 4; five states are one block), at least 100 of them; and one-segment
    branches, which the replay copies"""
    n, E = case.n, case.n_edge
    inter, singles = [], 0
    for r in case.replicas:
        maps = M.oracle_maps(case.case, r)
        assert len(maps) == case.N
        for off, dwell, state, raw in maps:
            assert off.size == E + 1 and off[-1] == dwell.size == state.size and np.all(np.diff(off) >= 1)
            assert np.all(np.diff(off) <= raw) and state.min() >= 0 and state.max() < n and np.all(dwell > 0.0)
            row = np.repeat(np.arange(E), np.diff(off))
            assert np.all(state[1:][row[1:] == row[:-1]] != state[:-1][row[1:] == row[:-1]])           # merged: no state repeats
            rs = np.zeros(E)
            np.add.at(rs, row, dwell)
            np.testing.assert_allclose(rs, case.z["edge.length"], rtol=1e-12)
            inter.append(M.interior(off, state))
        # A branch that a sweep left in one segment is replayed by the next as one segment: its ends were drawn zero steps apart, so
        # parent and child state are equal there and ``(m == 1) ? cs : ps`` of the replay never has to choose.  Every case has some.
        one = [(it, b) for it in range(case.N - 1) for b in np.nonzero(maps[it][3] == 1)[0]]
        assert all(maps[it + 1][0][b + 1] - maps[it + 1][0][b] == 1 for it, b in one)
        singles += len(one)
    assert singles > 0
    inter = np.concatenate(inter)
    assert set((inter // 8).tolist()) == set(range(W.ceil_div(n, 8))), sorted(set((inter // 8).tolist()))
    if n > 8:
        assert np.any(inter == n - 1)
    assert inter.size >= 100, inter.size


def test_long_branch_cases_hold_a_branch_beyond_64_segments_after_every_sweep():
    for n in M.LONG_NS:
        c = M.long_case(n)
        assert len(c.z["maps"][0]) == M.LONG_SEGMENTS == 100 and c.S == 70 and RC.band_class(c.B) == 0
        np.testing.assert_allclose(c.z["edge.length"][0] * c.Omega, 90.0, rtol=1e-12)
        for r in c.replicas:
            assert W.oracle_walk(c, r)[0] > 64
            for _, _, _, raw in M.oracle_maps(c, r):
                assert raw[0] > 64, raw
    assert [c.long_branch for c in ALL] == [False] * 82 + [False, False, True, True]


def test_sparse_cases_prune_with_a_band_and_draw_without():
    c = M.sparse_case(12)
    Bc = W.chain_matrix(c.B, "sparse")
    assert RC.band_class(Bc) == 1 and RC.band_class(c.B) == 0 and 0.0 < c.B[0, 11] < 1e-7 and Bc[0, 11] == 0.0
    assert c.kernels({}) >= {"wt_up_band_kernel<12, 1>", "wt_branch_kernel<false, true, true, 0>"}
    c = M.sparse_case(36)
    Bc = W.chain_matrix(c.B, "sparse")
    assert RC.half_bandwidth(Bc) == 1 and RC.half_bandwidth(c.B) == 35 and 0.0 < c.B[0, 35] < 1e-7
    assert c.kernels({}) >= {"wt_up_msplit_kernel<3>", "wt_down1_kernel<3>", "wt_branch_kernel<false, false, false, 0>"}
    for n in M.SPARSE_NS:
        c = M.sparse_case(n)
        assert c.variant == "sparse" and c.S == 70 and c.replicas == W.REPLICAS_2_TILES and len(c.z["states"]) == 12
        assert all(len(m) == n for m in c.z["maps"]) and {1, n} <= set(c.z["states"].tolist()) and np.ptp(c.pid) > 0
        np.testing.assert_allclose(c.Q.sum(1), 0.0, atol=1e-15)
        for r in c.replicas:
            rows, rc = W.oracle_rows(c, r)
            assert rc == 0
            np.testing.assert_allclose(rows[:, :n].sum(1), c.length, rtol=1e-11)


TWIN = [c for c in ALL if c.twin]


@pytest.mark.parametrize("case", TWIN, ids=[c.name for c in TWIN])
def test_twin_equals_the_oracle_maps(case):
    """replica S - 1, every iteration and edge row: states equal, dwell within the bar of mcmcmapsclasses.dwell_bar"""
    assert case.n <= 17
    r = case.S - 1
    rows = M.twin_rows(case.case, r)
    bar, worst = M.dwell_bar(case.case), 0.0
    for it, (off, dwell, state, _) in enumerate(M.oracle_maps(case.case, r)):
        for b in range(case.n_edge):
            want_d, want_s = dwell[off[b]:off[b + 1]], state[off[b]:off[b + 1]]
            got = rows[(it, b)]
            assert [s for _, s in got] == want_s.tolist(), (it, b)
            worst = max(worst, float(np.max(np.abs(np.array([d for d, _ in got]) - want_d) / want_d)))
    print(f"{case.name}: worst dwell error {worst:.3g}, {worst / bar:.3g} of the bar {bar:.3g}")
    assert worst <= bar
