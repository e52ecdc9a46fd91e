"""What tests/test_gpu_wtiles_classes.py relies on, checked without a GPU: the cases of tests/wtilesclasses.py between them reach every
kernel instantiation the launchers of phm_wtiles.hip can launch (by the host's dispatch rules restated there), every case is the
input it was chosen to be, and the oracle accepts it, keeps its branches on the branch kernel's first pass and draws from every
state."""
import numpy as np
import pytest

import rateupdatecases as RC
import wtilesclasses as W

ALL = W.all_cases()
IDS = [c.name for c in ALL]


def test_class_table_counts_and_ranges():
    """the table against the counts the kernel file's launchers spell out, and every n from 5 to 64 in exactly one class per family"""
    fam = {}
    for name, ns in W.ALL_CLASSES.items():
        fam.setdefault(name.split("<")[0], []).append((name, ns))
    assert {k: len(v) for k, v in fam.items()} == {
        "wt_root_kernel": 1, "wt_stats_kernel": 1, "wt_up_kernel": 4, "wt_up_blocks_kernel": 1, "wt_up_msplit_kernel": 3, "wt_up2_kernel": 12,
        "wt_up_band_kernel": 14, "wt_up_band_cluster_kernel": 14, "wt_down1r_kernel": 7, "wt_down1r_cluster_kernel": 7, "wt_down1_kernel": 2,
        "wt_branch_kernel": 10}
    assert len(W.ALL_CLASSES) == 76 and W.REACHABLE == set(W.ALL_CLASSES)
    for k, lo, hi in (("wt_up_kernel", 5, 64), ("wt_up_blocks_kernel", 5, 16), ("wt_up_msplit_kernel", 17, 64), ("wt_up2_kernel", 17, 64),
                      ("wt_down1r_kernel", 5, 32), ("wt_down1r_cluster_kernel", 5, 32), ("wt_down1_kernel", 33, 64)):
        assert sorted(n for _, ns in fam[k] for n in ns) == list(range(lo, hi + 1)), k
    for name, ns in fam["wt_up2_kernel"]:
        mt, ksu = (int(a) for a in name[name.index("<") + 1:-1].split(","))
        assert all(W.ceil_div(n, 4) == ksu and W.ceil_div(n, 16) == mt for n in ns), name
    for k in ("wt_up_band_kernel", "wt_up_band_cluster_kernel"):
        for name, ns in fam[k]:
            npad, hb = (int(a) for a in name[name.index("<") + 1:-1].split(","))
            assert all(4 * W.ceil_div(n, 4) == npad and 2 * hb + 1 < n for n in ns) and (ns[0] == npad - 3 or 2 * hb + 1 >= npad - 3), name


def test_cases_cover_every_reachable_instantiation():
    """no entry of the table -- every instantiation the kernel file holds -- without a case whose dispatch names it, no answer of the
    dispatch outside the table, and every case at an n its kernels are listed for"""
    seen = {}
    for c in ALL:
        for run in c.runs:
            for k in c.kernels(run):
                assert k in W.ALL_CLASSES, (c.name, run, k)
                assert c.n in W.ALL_CLASSES[k], (c.name, k)
                seen.setdefault(k, set()).add(c.n)
    assert set(seen) == W.REACHABLE, sorted(W.REACHABLE - set(seen))
    # the instantiations the suite had never run, by name
    for k, ns in (("wt_up2_kernel<2, 7>", {25, 28}), ("wt_up2_kernel<3, 11>", {41, 44}), ("wt_up2_kernel<4, 13>", {49, 52}),
                  ("wt_up2_kernel<4, 14>", {53, 56}), ("wt_up2_kernel<4, 15>", {57, 60}), ("wt_up_band_kernel<16, 1>", {13, 16}),
                  ("wt_up_band_kernel<28, 1>", {25, 28}), ("wt_up_band_cluster_kernel<8, 2>", {6, 8}),
                  ("wt_up_band_cluster_kernel<16, 2>", {13, 16}), ("wt_up_band_cluster_kernel<20, 2>", {17, 20}),
                  ("wt_up_band_cluster_kernel<28, 2>", {25, 28})):
        assert ns <= seen[k], (k, seen[k])


def test_trace_names_reads_a_statistics_line():
    line = '"void phm::(anonymous namespace)::wt_up2_kernel<2, 7>(phm::WtParams, int, int)",12\n' \
           '"void phm::(anonymous namespace)::wt_branch_kernel<false,true,true,1>(phm::WtParams, int)",3\nphm::wt_root_kernel(phm::WtParams, int)'
    assert W.trace_names(line) == {"wt_up2_kernel<2, 7>", "wt_branch_kernel<false, true, true, 1>", "wt_root_kernel"}


def test_dense_cases_sit_on_the_class_edges():
    assert W.DENSE_NS == (5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 32, 33, 36, 37, 40, 41, 44, 45, 48, 49, 52, 53, 56, 57, 60, 61, 64)
    for n in W.DENSE_NS:
        c = W.dense_case(n)
        ksu = W.ceil_div(n, 4)
        assert n % 4 in (1, 0) and W.ceil_div(n - 1, 4) == ksu - (n % 4 == 1) and W.ceil_div(n + 1, 4) == ksu + (n % 4 == 0)
        assert RC.band_class(c.B) == 0 and np.count_nonzero(c.B) == n * n          # dense: matrix cores, no generated kernel
        slots = n * (n - 1) if n <= 10 else 0                                          # 90 pairs at n = 10 are the last to fit the LDS slots
        assert W.plain_slot_class(c.B) == slots and W.branch_paths(n, c.B, c.variant, True) == (slots, slots == 0, n > 32)
        assert c.tiles == 3 and c.S % 64 == 22 and c.replicas[-1] == c.S - 1 and c.N == 6
        for run in c.runs:
            f, ks = run["pruning_form"], c.kernels(run)
            mt = W.ceil_div(n, 16)
            up = {0: "wt_up_msplit_kernel<%d>" % mt if mt > 1 else "wt_up_blocks_kernel<1>", 1: "wt_up_kernel<%d>" % mt,
                  2: "wt_up_msplit_kernel<%d>" % mt if mt > 1 else "wt_up_blocks_kernel<1>", 3: "wt_up2_kernel<%d, %d>" % (mt, ksu)}[f]
            assert up in ks, (n, f, ks)
            assert ("wt_down1_kernel<%d>" % mt if mt >= 3 else "wt_down1r_kernel<%d>" % (4 * ksu)) in ks
            assert "wt_branch_kernel<false, %s, %s, 0>" % (("true", "true") if n <= 32 else ("false", "false")) in ks
    # the block scan of a dense draw: every nblk from 1 to 8, both parities of n, n = 8 q + 1 (one state in the last block) and 8 q
    assert {W.ceil_div(n, 8) for n in W.DENSE_NS} == set(range(1, 9))
    assert {49, 52, 53, 56} <= set(W.DENSE_NS) and all(W.ceil_div(n, 8) == 7 for n in (49, 52, 53, 56))
    assert {n % 8 for n in W.DENSE_NS} == {0, 1, 4, 5}
    assert all(W.dense_case(n, "plain").variant == "plain" and n % 4 == 1 for n in W.DENSE_PLAIN_NS)
    # wt_up2_kernel's last chunk of eight fragments, per class of the new cases: NF = MT * KSU
    last = {n: (W.ceil_div(n, 16) * W.ceil_div(n, 4) - 1) % 8 + 1 for n in (25, 41, 49, 53, 57)}
    assert last == {25: 6, 41: 1, 49: 4, 53: 8, 57: 4}


@pytest.mark.parametrize("npad,hb", W.BAND_CLASSES)
def test_band_cases_sit_on_the_class_edges(npad, hb):
    lo, hi = W.band_ns(npad, hb)
    assert (lo, hi) == (max(npad - 3, 2 * hb + 2), npad) and lo in W.ALL_CLASSES["wt_up_band_kernel<%d, %d>" % (npad, hb)]
    assert lo - 1 not in W.ALL_CLASSES["wt_up_band_kernel<%d, %d>" % (npad, hb)]
    if npad == 8:
        assert lo == {1: 5, 2: 6}[hb]                     # the smallest n the host rule accepts
    else:
        assert lo % 2 == 1                                # an odd bottom: n - 1 pairs of a row and one padded entry
    for n in (lo, hi):
        for tree in ("random", "ladder"):
            c = W.band_case(n, hb, tree)
            assert RC.half_bandwidth(c.B) == hb == RC.band_class(c.B) and RC.band_class(c.B[:2 * hb + 1, :2 * hb + 1]) == 0
            full = sum(min(n - 1, i + hb) - max(0, i - hb) for i in range(n))
            assert np.count_nonzero(c.B) - n == full - (1 if hb == 1 else 0) and (c.B[3, 4] == 0.0) == (hb == 1)
            assert W.plain_slot_class(c.B) == (full - (hb == 1) if full - (hb == 1) <= 96 else 0)
            assert np.ptp(c.pid) > 0 and abs(c.pid.sum() - 1) < 1e-12
            assert all(len(m) == n for m in c.z["maps"]) and {1, n} <= set(c.z["states"].tolist())
            assert c.S == 70 and c.tiles == 2 and c.replicas == (0, 63, 64, 69)
            ks = [c.kernels(run) for run in c.runs]
            if tree == "random":
                assert len(c.z["states"]) == 12 and [r["level_groups"] for r in c.runs] == [1]
                assert {"wt_up_band_kernel<%d, %d>" % (npad, hb), "wt_down1r_kernel<%d>" % npad} <= ks[0]
            else:
                assert len(c.z["states"]) == 300 and c.N == 4 and [r["level_groups"] for r in c.runs] == [1, 2, 0] and c.deep
                levels = len(RC.height_level_sizes(c.z["edge"]))
                assert levels == 299 > 4 * 9 + 32                                   # deep_tree (phm_engine.cpp): the automatic choice
                assert {"wt_up_band_kernel<%d, %d>" % (npad, hb), "wt_down1r_kernel<%d>" % npad} <= ks[0]
                assert {"wt_up_band_cluster_kernel<%d, %d>" % (npad, hb), "wt_down1r_cluster_kernel<%d>" % npad} <= ks[1] == ks[2]
            assert all("wt_branch_kernel<false, true, true, %d>" % hb in k for k in ks)


def test_b2l_slot_and_ks_cases_are_what_they_are_named_for():
    for v, n in W.B2L_CASES:
        c = W.b2l_case(v, n)
        assert n > 32 and len(c.z["states"]) == 14 and W.branch_group(c.tiles, c.n_edge) == 1
        on = "wt_branch_kernel<%s, false, true, 0>" % ("true" if v == "ks" else "false")
        assert [on in c.kernels(r) for r in c.runs] == [False, False, True, True]
        assert [(r["branch_group"], r["reduce"]) for r in c.runs] == [(1, False), (1, True), (4, False), (4, True)]
        assert W.branch_paths(n, c.B, v, True) == (0, True, True)
        if v == "ks":
            assert RC.half_bandwidth(c.B) == 2 and RC.band_class(c.B) == 0 and set(c.z["states"].tolist()) <= {1, 2}
    want = {(10, 0): 90, (11, 0): 0, (25, 2): 94, (26, 2): 0}
    pairs = {(10, 0): 90, (11, 0): 110, (25, 2): 94, (26, 2): 98}
    for n, hb in W.SLOT_CASES:
        c = W.slot_case(n, hb)
        assert np.count_nonzero(c.B) - n == pairs[n, hb] and W.plain_slot_class(c.B) == want[n, hb] and RC.band_class(c.B) == hb
        assert W.branch_paths(n, c.B, c.variant, True) == (want[n, hb], want[n, hb] == 0, False)
        assert [r["reduce"] for r in c.runs] == [False, True]
    for (kind, n), (band, slots) in zip(W.KS_SMALL_CASES, ((2, 4 * 12 - 4), (1, 2 * 8), (0, 4 * 12 - 4))):
        c = W.ks_small_case(kind, n)
        assert RC.slot_class(c.B) == slots == W.slot_count(c.B, "ks")
        assert all("wt_branch_kernel<true, true, true, %d>" % band in c.kernels(r) for r in c.runs)
    # mask tip rows in every pruning form: the matrix-core kernels of one and of three row blocks, none replaced by a band kernel
    up = {12: ("wt_up_blocks_kernel<1>", "wt_up_kernel<1>", "wt_up_blocks_kernel<1>"),
          34: ("wt_up_msplit_kernel<3>", "wt_up_kernel<3>", "wt_up_msplit_kernel<3>", "wt_up2_kernel<3, 9>")}
    for n in W.KS_FORM_NS:
        c = W.ks_form_case(n)
        assert c.ks and c.S == 70 and c.N == 6 and len(c.z["states"]) == 14 and set(c.z["states"].tolist()) <= {1, 2}
        assert [r["pruning_form"] for r in c.runs] == list(W.dense_forms(n)) and len(up[n]) == len(c.runs)
        assert all(k in c.kernels(r) for k, r in zip(up[n], c.runs)), [sorted(c.kernels(r)) for r in c.runs]


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_oracle_accepts_the_case_and_draws_from_every_state(case):
    """status 0 on the compared replicas; no branch beyond 64 segments after any sweep (the branch kernel's first pass; the loop
    beyond has tests of its own); every state is the previous state of a forward draw somewhere in the run, so the draws at
    states 0 and n - 1 -- the clamped columns of a banded draw -- are made and not assumed"""
    longest, parents = 0, set()
    for r in case.replicas:
        rows, rc = W.oracle_rows(case, r)
        assert rc == 0 and rows.shape == (case.N, case.n + case.ncnt + (2 + 3 * (case.n // 2 - 1) + 1 if case.ks else 0))
        np.testing.assert_allclose(rows[:, :case.n].sum(1), case.length, rtol=1e-11)
        l, p = W.oracle_walk(case, r)
        longest, parents = max(longest, l), parents | p
    assert longest <= 64, longest
    assert parents == set(range(case.n)), sorted(set(range(case.n)) - parents)
