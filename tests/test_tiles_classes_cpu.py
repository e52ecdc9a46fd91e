"""What tests/test_gpu_tiles_classes.py relies on, checked without a GPU: every case of tests/tilesclasses.py lands in the class it was
chosen for under the host's rules restated there (group, ragged last group, chunks, counter copies, form, clusters or levels, parts),
the cases between them reach every instantiation of the branch kernel under every kind of group and every instantiation of the
cluster pruning kernel, and the oracle's runs hold what the cases are there to provoke."""
import numpy as np
import pytest

import tilesclasses as T


def test_the_restated_rules_at_their_documented_points():
    """the examples the engine's comments and the existing tests name: C2 at 66 tiles has group 2, C3 at 16 tiles 4, C2 at 256 tiles 7,
    C3 at 256 tiles the cap of 16; 512 counter sets however few the tiles; a forced group clamps at 64"""
    assert T.group(66, 1998) == 2 and T.group(16, 19998) == 4 and T.group(256, 1998) == 7 and T.group(256, 19998) == 16
    assert T.group(1, 10) == 1 and T.group(256, 19998, 3) == 3 and T.group(1, 10, 1000) == 64
    assert [T.cnt_copies(t) for t in (1, 2, 5, 8, 9, 16, 66, 255, 256, 511, 512, 1000)] == [64, 64, 64, 64, 64, 32, 8, 4, 2, 2, 1, 1]
    assert T.parts(256, 19998, 16) == 2 and T.parts(16, 19998, 4) == 2 and T.parts(5, 78, 1) == 1 and T.parts(5, 78, 1, forced=3) == 3
    assert T.parts(2, 78, 1, forced=3) == 2 and T.parts(256, 19998, 16, clustered=True) == 1 and T.parts(256, 19998, 16, recorded=True) == 1
    assert T.clusters(64, 1024) and not T.clusters(64, 1025) and T.clusters(64, 1025, deep=True) and not T.clusters(1, 5, level_groups=1)
    assert T.poisson_capacity(0.0, 1e-9) == 1 and T.poisson_capacity(0.1, 0.01) == 3


def test_instantiation_tables():
    assert len(set(T.BRANCH_KERNELS)) == 12 and len(set(T.UP_CLUSTER_KERNELS)) == 6


def test_family_a_reaches_every_branch_kernel_with_every_kind_of_group():
    """each of the 12 tiles_branch_kernel<NS, KS, LONG> with one branch per wave, a ragged last group and one wave for the whole tree;
    each of the 6 tiles_up_cluster_kernel<NS, ASYNC>; and the long kind also with a launch per level (no cluster kernel)"""
    seen, up = {}, set()
    for c in T.cases_a():
        assert c.S == 70 and c.tiles == 2 and c.S - 64 == 6 and c.runs == (1, 3) and c.replicas == (0, 63, 64, 69)
        assert c.E == (22 if c.long else 46) and c.groups == (1, 3, 64)
        kinds = set()
        for g in c.groups:
            gg = c.group(g)
            if gg == 1:
                kinds.add("one")
            elif gg >= c.E:
                kinds.add("tree")
                assert T.n_groups(c.E, gg) == 1
            elif c.E % gg:
                kinds.add("ragged")
                assert c.E % gg == 1                      # a last group of one branch
        seen.setdefault(c.branch_kernel(), set()).update(kinds)
        assert c.clusters() and not c.clusters(level_groups=1)
        up.add(c.up_cluster_kernel())
        assert c.up_cluster_kernel(level_groups=1) is None
    assert set(seen) == set(T.BRANCH_KERNELS)
    assert all(k == {"one", "ragged", "tree"} for k in seen.values()), seen
    assert up == set(T.UP_CLUSTER_KERNELS)
    # the ks sweep shares <4, true, LONG> with the bf sweep and adds the parity tip masks
    assert {(c.variant, c.n) for c in T.cases_a()} == set(T.SWEEPS_A)


@pytest.mark.parametrize("case", [c for c in T.cases_a() if c.long], ids=repr)
def test_family_a_long_paths_outgrow_the_packed_form_in_the_oracle(case):
    """more than 64 segments on some branch after sweep 1: two registers of 2-bit states could not hold them"""
    for r in case.replicas:
        assert T.oracle_longest(case, r) > 64


def test_family_b_chunks():
    c = T.case_b()
    assert c.n == 2 and c.E == 198 and not c.long
    assert (T.n_groups(198, 3), T.n_chunks(198, 3), 66 - 64) == (66, 2, 2)
    assert (T.n_groups(198, 1), T.n_chunks(198, 1), 198 - 3 * 64) == (198, 4, 6)


def test_family_c_form_rule_and_table_edge():
    """the form by the caller's segments alone (no branch is expected to hold 48 in stationarity); the first draw of a branch of m
    segments reads chain row m - 2: 23 is the last row in LDS, 24 the first in global memory"""
    for segs, c in zip(T.SEGMENTS_C, T.cases_c()):
        assert c.n == 4 and c.E == 18 and max(1.0 + c.Omega * float(sum(m)) for m in c.z["maps"]) < T.LONG_SEGMENTS
        assert all(len(m) == segs for m in c.z["maps"])
        assert c.long == (segs > 48), segs
        assert c.branch_kernel() == (4, False, segs > 48)
        assert (segs - 2 >= T.KTAB) == (segs != 25)
        assert min(T.slot_caps(c.z, c.Omega, c.S, c.N)) + 1 > segs - 2     # klong: the table holds the row
    assert T.SEGMENTS_C == (25, 48, 49, 64, 65) and 25 - 2 == T.KTAB - 1


def test_family_c_rows_23_and_24_differ_under_the_slow_chain():
    """a draw from row 23 where row 24 is due -- the table edge off by one -- must change paths, not the ninth digit of a probability"""
    for segs, c in zip(T.SEGMENTS_C_SLOW, T.cases_c_slow()):
        assert c.n == 2 and c.E == 18 and all(len(m) == segs for m in c.z["maps"]) and c.long == (segs > 48)
        assert max(1.0 + c.Omega * float(sum(m)) for m in c.z["maps"]) < T.LONG_SEGMENTS
        p23, p24 = np.linalg.matrix_power(c.B, T.KTAB - 1), np.linalg.matrix_power(c.B, T.KTAB)
        assert np.min(np.abs(p24 - p23)) > 0.35
        assert (segs - 2 >= T.KTAB) == (segs >= 26)
        for r in c.replicas:
            assert np.all(T.oracle_rows(c, r)[:, c.n:].sum(0) > 0)
    slow = np.linalg.matrix_power(T.case_c(48).B, T.KTAB) - np.linalg.matrix_power(T.case_c(48).B, T.KTAB - 1)
    assert np.max(np.abs(slow)) < 1e-3                # the family's first model: neighbouring rows nearly agree


def test_family_d_one_lane_counts_past_16_bits():
    """sweep 1 of every compared replica counts more than 65 535 (1, 1) pairs; with branch_group 64 one wave walks all ten branches,
    and the three long ones come first in the order (largest slot first), so the third passes 65 535 pending segments"""
    c = T.case_d()
    assert c.n == 2 and c.E == 10 and c.group(64) == 64 and T.n_groups(c.E, 64) == 1 and c.long and c.branch_kernel() == (2, True, True)
    assert sorted(len(m) for m in c.z["maps"])[-3:] == [30000] * 3 and sorted(len(m) for m in c.z["maps"])[:7] == [2] * 7
    assert np.all(c.z["states"] == 1) and all(np.all(m == 1) for m in c.z["mapnames"])
    caps = T.slot_caps(c.z, c.Omega, c.S, c.N)
    assert max(caps) < 65535 and sorted(np.argsort(-np.asarray(caps), kind="stable")[:3]) == sorted(np.argsort([-len(m) for m in c.z["maps"]], kind="stable")[:3])
    assert 2 * 30000 <= 65535 < 3 * 30000
    for r in T.D_REPLICAS:
        rows = T.oracle_rows(c, r)
        assert 86736 <= rows[0, c.n + 0] <= 86894, rows[0]
        assert rows[0, c.n + 0] > 65535
    assert c.bytes(64) < 0.25 * T.GIB


def test_family_e_counter_copies():
    for S, c in zip(T.REPLICAS_E, T.cases_e()):
        assert c.variant == "ks" and c.ncnt == 16 and c.E == 38 and c.E % 3 == 2
        assert T.cnt_copies(c.tiles) == T.REPLICAS_E[S]
    assert [c.tiles for c in T.cases_e()] == [1, 9, 33, 129, 512]
    assert [T.cnt_copies(t) for t in (1, 9, 33, 129, 512)] == [64, 64, 16, 4, 1]
    # groups of 3: 13 groups over min(copies, 13) copies -- more than one copy in use wherever there is more than one
    assert T.n_groups(38, 3) == 13 and [len({g & (k - 1) for g in range(13)}) for k in (64, 16, 4, 1)] == [13, 13, 4, 1]


def test_family_f_parts_on_an_uneven_split():
    for c in (T.case_f(4), T.case_f(2)):
        assert c.tiles == 5 and c.S - 4 * 64 == 54 and not c.clusters() and c.E == 78
        for g in c.groups:
            assert [T.parts(c.tiles, c.E, g, forced=p) for p in T.PARTS_F] == [1, 2, 3]
        assert T.parts(c.tiles, c.E, 1) == 1          # automatically a tree this small keeps one part
        assert 5 % 2 and 5 % 3


def test_families_g_h_i():
    g = T.case_g_sites()
    assert g.tiles == 3 and g.sites.shape == (130, 30) and g.E == 58 and g.E % 3 == 1
    o = T.case_g_offset()
    assert o.base["replica_offset"] == 1000 and o.E % 3 == 1
    assert [(c.n, c.long) for c in T.cases_h()] == [(2, False), (2, True), (3, False), (3, True), (4, False), (4, True)]
    assert all(T.parts(c.tiles, c.E, 1, recorded=True) == 1 for c in T.cases_h())
    i = T.case_i()
    assert i.base["cap_tail"] == 0.9 and i.tiles == 4 and 3 in i.groups


@pytest.mark.parametrize("tips,want", [(1024, 1), (1025, 2)])
def test_j1_the_edge_of_the_automatic_group(tips, want):
    c = T.case_j1(tips)
    assert c.tiles == 64 and c.E == 2 * tips - 2 and c.group(0) == want and c.groups == (0,)
    assert (c.tiles * c.E) // T.GROUP_WAVES == want
    assert c.bytes() <= T.BYTES_CAP
    assert set(T.slot_caps(c.z, c.Omega, c.S, c.N, T.J_CAP_TAIL)) == {T.J_ROWS_FLOOR}
    for r in c.replicas:                                  # the shrunk branches still show every count column
        assert np.all(T.oracle_rows(c, r)[:, c.n:] > 0)


def test_j2_the_class_of_the_headline():
    c = T.case_j2()
    assert c.n == 4 and c.tiles == 256 and c.S == 16374 and 16374 - 255 * 64 == 54 and c.E == 4198 and c.runs == (1, 2)
    g = c.group(0)
    assert g == 16 and c.E % 16 == 6 and T.n_groups(c.E, g) == 263 and T.n_chunks(c.E, g) == 5 and 263 - 4 * 64 == 7
    assert T.cnt_copies(c.tiles) == 2 and not c.clusters() and not c.long
    assert c.tiles * 263 >= 65536 and T.parts(c.tiles, c.E, g) == 2
    for r in c.replicas:                                  # every count column the model allows (B's zeros stay zero)
        cnt = T.oracle_rows(c, r)[:, c.n:].sum(0)
        possible = np.array([c.B[a, b] != 0 for a in range(4) for b in range(4) if a != b])
        assert np.array_equal(cnt > 0, possible), cnt
        assert possible.sum() == 8


def test_j2_bytes_sit_at_the_floor_of_its_class():
    """The cap of 8 GiB cannot hold for this class: group 16 needs 2^20 (tile, branch) pairs, i.e. 2^26 (lane, branch) pairs, and the
    engine keeps for each at least 2 x 6 rows x 8 B of dwell times (plan_slots gives a two-segment path of positive length no fewer
    than 6 rows), 4 x 8 B of partial dwell sums, half of 4 x 8 B of partial likelihoods and 2 B of counts: 146 B, 9.1 GiB.  The case
    is held to that floor instead -- every slot at 6 rows -- and to within 4 % of the bound just derived."""
    c = T.case_j2()
    assert set(T.slot_caps(c.z, c.Omega, c.S, c.N, T.J_CAP_TAIL)) == {T.J_ROWS_FLOOR}
    floor = (1 << 26) * (2 * T.J_ROWS_FLOOR * 8 + 4 * 8 + 4 * 8 // 2 + 2)
    assert floor > T.BYTES_CAP
    assert floor <= c.bytes() <= 1.04 * floor, (c.bytes() / T.GIB, floor / T.GIB)
