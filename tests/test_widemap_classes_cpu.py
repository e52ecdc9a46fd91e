"""The cases of tests/widemapclasses.py pinned to the paths of phm_wide.hip and phm_wbranch.hip they are there for, through the
host's rules restated there -- no GPU needed.  tests/test_gpu_widemap_classes.py runs them."""
import numpy as np
import pytest

import widemapclasses as C


def test_constants_read_from_the_sources():
    assert (C.WIDE_BLOCK, C.WIDE_MAXSEG, C.WIDE_MAXSEG_BIG_N, C.WB_ELL_MAX, C.WB_BLOCK) == (384, 128, 128, 16, 256)
    assert (C.WB_MERGED_LDS, C.WB_FLUSH, C.WB_VARIATES, C.WB_B2_LDS_WAVES) == (192, 64, 64, 32768)
    assert (C.WB_WALK_LDS_NODES, C.WB_DMAP_BYTES, C.WIDE_TARGET_TILES) == (61440, 256 << 20, 8192)
    assert (C.WIDE_LDS_DEFAULT, C.WB_LDS_DEFAULT) == (64 * 1024, 48 * 1024)


def test_rep_stride_restated():
    for S, want in C.MULTI_STRIDE.items():
        assert C.rep_stride(S) == want, S
    assert [C.rep_stride(S) for S in (1, 330, 4096, 16384, 32768, 32769, 65537, 262144, 1 << 20)] == [1, 1, 1, 2, 4, 8, 16, 32, 64]


@pytest.mark.parametrize("S", C.MULTI_S)
def test_multi_replica_cases_fill_their_waves(S):
    """A: every run has more than one replica in a wave, a last tile that is partly filled, and compared replicas in lane 0, in
    lane 1, in the last lane of the first tile, in the first lane of the second and in the last tile"""
    st = C.rep_stride(S)
    tiles = C.ceil_div(S, st)
    last = S - (tiles - 1) * st
    assert st >= 2 and 1 <= last < st
    assert last == 1                                            # every S here is 2^k + 1: the last tile holds one replica
    reps = C.multi_replicas(S)
    assert {0, 1, st - 1, st, S - 2, S - 1} <= set(reps) and len(reps) >= 6
    mid = C.middle_replica(S)
    assert mid in reps and mid % st != 0 and 0 < mid // st < tiles - 1
    assert (S - 2) // st == tiles - 2 and (S - 2) % st == st - 1      # the last lane of the last full tile
    for n in C.MULTI_NS:
        c = C.multi_case(n, S)
        assert c.n == n and c.T == C.MULTI_TIPS and c.N == C.MULTI_SWEEPS and c.mapping == "replicas"
    sites = C.multi_sites(C.multi_case(5, S))
    assert sites.shape == (S, C.MULTI_TIPS) and sites.min() == 1 and sites.max() == 5
    assert len({sites[r].tobytes() for r in reps}) == len(reps)       # the compared replicas see different tips


def test_multi_replica_waves_differ_between_lanes():
    """the wave maximum of the segment counts and the rows a branch consumes are taken over lanes that differ: on the oracle the
    replicas of one tile leave different segment counts on some branch after the first sweep"""
    c = C.multi_case(20, 262145)
    counts = np.array([C.oracle_dump(c, r)[1].seg_count for r in (0, 1, 63)])
    assert np.any(counts.max(0) != counts.min(0))
    assert np.any(counts.argmax(0) != 0)                       # lane 0 is not always the longest


def test_list_problem_puts_several_replicas_of_a_tree_in_one_tile():
    Q, pid, Omega, trees = C.list_problem()
    assert Q.shape[0] == C.LIST_N and len(trees) == C.LIST_TREES and 1 < C.LIST_S < 64


@pytest.mark.parametrize("case", C.edge_cases(), ids=[c.name for c in C.edge_cases()])
def test_edge_cases_sit_on_their_edges(case):
    """B: dense rows on both matrices, every state count on its side of the LDS sizes that cross a launch default"""
    n, sparse = case.n, case.sparse
    ell_w, ell2_w, hb = case.classes()
    assert (ell_w, ell2_w, hb) == (0, 0, 0)
    assert np.all(case.B > 1e-7) and (np.count_nonzero(case.B, axis=1).min() > C.WB_ELL_MAX or n <= C.WB_ELL_MAX)
    assert np.array_equal(C.chain_matrix(case.B, sparse), case.B)
    if case.mapping == "replicas":
        over = C.wide_lds_bytes(n, sparse) > C.WIDE_LDS_DEFAULT
        assert over == (n >= (32 if sparse else 45))
        assert C.rep_stride(case.S) == 1
    else:
        over = C.wbranch_lds_bytes(n, sparse) > C.WB_LDS_DEFAULT
        assert over == (sparse and n >= 56)
        assert C.b2_in_lds(case.S, case.E, ell2_w) and C.uses_dmap(case.S, case.E, n) and C.walk_uses_lds(case.T - 1)
        kinds = {k for _, _, k in C.pruning_launches(C.height_level_sizes(case.z), dense=True)}
        assert kinds == {"run", "level"}                        # wb_up_kernel and wb_up_run_kernel<512, true> both stage the model


def test_edge_state_counts():
    assert {64 - n for n in C.EDGE_DENSE_NS} >= {59, 1, 0}
    assert (C.wide_lds_bytes(44, False), C.wide_lds_bytes(45, False)) == (65344, 65712)
    assert (C.wide_lds_bytes(31, True), C.wide_lds_bytes(32, True)) == (64776, 66304)
    assert (C.wbranch_lds_bytes(55, True), C.wbranch_lds_bytes(56, True)) == (48840, 51520)


def test_pruning_launch_rule_restated():
    assert C.pruning_launches([6, 4, 2, 1], True) == [(0, 1, "level"), (1, 4, "run")]
    assert C.pruning_launches([6, 4, 5, 4, 1], True) == [(0, 1, "level"), (1, 2, "level"), (2, 3, "level"), (3, 5, "run")]
    assert C.pruning_launches([9, 8, 5, 1], False) == [(0, 1, "level"), (1, 4, "run")]
    assert C.pruning_launches([3], True) == [(0, 1, "level")]


@pytest.mark.parametrize("k", range(len(C.ELL_PAIRS) // 2))
def test_ellpack_pairs_straddle_the_rule(k):
    """C: in each pair one side takes ELLPACK rows and the other dense ones; unbanded, asymmetric, one row short"""
    (n1, w1), (n2, w2) = C.ELL_PAIRS[2 * k], C.ELL_PAIRS[2 * k + 1]
    a, b = C.ell_case(n1, w1), C.ell_case(n2, w2)
    assert a.classes() == (w1, w1, 0)
    assert b.classes() == (0, 0, 0)
    for c, w in ((a, w1), (b, w2)):
        nz = np.count_nonzero(c.B, axis=1)
        assert nz.max() == w and sorted(nz)[1] == w and (nz.min() == w - 1 or w == 2)
        assert not np.array_equal(c.B != 0, (c.B != 0).T)
        assert C.RC.half_bandwidth(c.B) > 2 or c.n <= 6
    assert (3 * w1 <= n1 and w1 <= C.WB_ELL_MAX) and (3 * w2 > n2 or w2 > C.WB_ELL_MAX)


def test_band_case_with_and_without_shifts():
    c = C.band16_case()
    assert c.classes() == (5, 5, 2) and c.classes(sparse_chains=2) == (5, 5, 0)


@pytest.mark.parametrize("model", C.THRESHOLD_MODELS)
def test_threshold_cases_have_two_different_matrices(model):
    c = C.threshold_case(model, True)
    Bc = C.chain_matrix(c.B, True)
    assert not np.array_equal(Bc, c.B) and np.all(c.B[Bc == 0] <= 1e-7) and np.all(Bc[Bc != 0] > 1e-7)
    ell_w, ell2_w, hb = c.classes()
    want = {"corner12": (3, 3, 1), "corner36": (3, 3, 1), "under12": (3, 0, 1), "under36": (3, 0, 1), "tiny10": (0, 0, 0),
            "ell6over4": (4, 6, 0)}[model]
    assert (ell_w, ell2_w, hb) == want
    if model == "tiny10":                                       # dense rows on both sides, different numbers (and in s_Bc / s_B2 of phm_wide.hip)
        assert np.count_nonzero(Bc) < np.count_nonzero(c.B) == c.n * c.n


def test_threshold_cases_survive_where_they_are_run_unscaled():
    """the reference's SPARSE driver does not rescale: the models run without it are those the oracle finishes"""
    for model in C.THRESHOLD_MODELS:
        c = C.threshold_case(model, False)
        for r in c.replicas:
            assert C.oracle_rows(c, r)[1] == 0, (model, r)


@pytest.mark.parametrize("case", C.window_cases(), ids=[c.name for c in C.window_cases()])
def test_window_cases_pass_every_window_on_the_oracle(case):
    """D: in some sweep of a compared replica a branch holds more than 192 merged segments, notes more than 64 transitions and
    takes more than 64 exponential draws; one branch starts with exactly 192 segments and one with 193"""
    lens = sorted(len(m) for m in case.z["maps"])
    assert lens[-3:] == [C.WB_MERGED_LDS, C.WB_MERGED_LDS + 1, C.WINDOW_SEGMENTS]
    assert case.classes()[:2] == (0, 0) and C.b2_in_lds(case.S, case.E, 0) and C.uses_dmap(case.S, case.E, case.n)
    best = np.max([C.oracle_windows(case, r) for r in case.replicas], axis=(0, 1))
    assert best[0] > C.WB_MERGED_LDS and best[1] > C.WB_FLUSH and best[2] > C.WB_VARIATES, best
    for r in case.replicas:                                     # ... every replica spills merged segments in some sweep, and in
        wins = C.oracle_windows(case, r)                        # EVERY sweep flushes and refills more than twice on some branch
        assert max(w[0] for w in wins) > C.WB_MERGED_LDS, (r, wins)
        assert all(w[1] > 2 * C.WB_FLUSH and w[2] > 2 * C.WB_VARIATES for w in wins), (r, wins)


def test_window_case_with_the_forward_matrix_in_global_memory():
    c = C.window_case("bigtree", 20, C.WINDOW_BIG_S)
    assert c.S * c.E == 32780 > C.WB_B2_LDS_WAVES and not C.b2_in_lds(c.S, c.E, 0)
    assert C.b2_in_lds(C.WINDOW_S, c.E, 0) and c.replicas == (0, 63, c.S - 1)


def test_fallback_cases_cross_their_thresholds():
    """E, by shape alone (the trees are built on the GPU side of the tests: here only their sizes)"""
    E = 2 * C.LEVELS_TIPS - 2
    assert C.LEVELS_S * E * C.LEVELS_N > C.WB_DMAP_BYTES >= (C.LEVELS_S - 1) * E * C.LEVELS_N and C.LEVELS_S <= 65535
    assert not C.uses_dmap(C.LEVELS_S, E, C.LEVELS_N)
    assert not C.walk_uses_lds(C.WALK_TIPS - 1) and C.walk_uses_lds(C.WB_WALK_LDS_NODES)
    assert C.uses_dmap(1, 2 * C.WALK_TIPS - 2, C.WALK_N)


@pytest.mark.parametrize("n", C.LIMIT_NS)
def test_limit_cases(n):
    """F: exactly the limit, one beyond, and a chain whose first sweep leaves more than the limit"""
    at, over, grow = C.limit_case(n, 0), C.limit_case(n, 1), C.outgrow_case(n)
    assert max(len(m) for m in at.z["maps"]) == C.wide_maxseg(n) == max(len(m) for m in over.z["maps"]) - 1
    assert max(len(m) for m in grow.z["maps"]) < C.wide_maxseg(n)
    for r in grow.replicas:
        _, rc, dump = grow.oracle(r, dump=True, N=1)
        assert rc == 0 and dump.seg_count[0] > C.wide_maxseg(n)
    for r in at.replicas:
        assert C.oracle_rows(at, r)[1] == 0
