"""What tests/test_gpu_narrow_classes.py relies on, checked without a GPU: every case of tests/narrowclasses.py lands in the class its name
says under the rules restated there (wave-wide branches, waves and group positions, pruning form, window shares), the oracle's chain
states before and after every sweep show that the case reaches what it is there to reach (window sums, refills, allotments, output
stages, blocks of the wave-wide walk, overflowing slots) -- a case that stops reaching its class after a change of seed or constant
fails here, not silently on the GPU -- and build_cluster_plan / build_band_plan hold their invariants on the trees of the cases, in a
stand-alone program (tests/native/cluster_plan_check.cpp) built with phm_sched.cpp under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import narrowclasses as NC
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake(counts, steps=0.0):
    """a tree of which only the paths matter: segment counts per branch, Omega t_b = steps at Omega = 1"""
    return {"maps": [np.full(m, steps / m) for m in counts]}


def test_the_restated_rules_at_their_documented_points():
    """the examples the engine's comments and the issue name: min(E / 16, 128) gives 127 wave-wide branches at 1 024 tips and 128 at
    1 025, none at E = 14 and one at E = 16; a branch expected to hold 96 segments is wave-wide and turns the automatic pruning form,
    one of 95 is not and does not; group g of eight-lane wave k sits at n_long + g n_waves8 + k; windows of 192 and 256"""
    assert NC.n_wide(_fake([2] * 2046), 1.0) == 127 and NC.n_wide(_fake([2] * 2048), 1.0) == 128 and NC.n_wide(_fake([2] * 6144), 1.0) == 128
    assert NC.n_wide(_fake([2] * 14), 1.0) == 0 and NC.n_wide(_fake([2] * 16), 1.0) == 1 and NC.n_wide(_fake([2] * 2), 1.0) == 0
    assert NC.n_wide(_fake([2] * 7 + [96]), 1.0) == 1 and NC.n_wide(_fake([2] * 7 + [95]), 1.0) == 0
    assert NC.n_wide(_fake([1] * 8, 95.0), 1.0) == 8 and NC.n_wide(_fake([1] * 8, 94.0), 1.0) == 0      # clipped to E
    assert NC.dependency_driven(_fake([2] * 7 + [96]), 1.0) and not NC.dependency_driven(_fake([2] * 7 + [95]), 1.0)
    assert NC.dependency_driven(_fake([2] * 8), 1.0, 2) and not NC.dependency_driven(_fake([96] * 8), 1.0, 1)
    assert NC.n_waves(8, 0) == 1 and NC.n_waves(16, 1) == 3 and NC.n_waves(19998, 128) == 128 + 2484 and NC.n_waves(2, 0) == 1
    assert NC.wave_positions(8, 0) == [list(range(8))]
    assert NC.wave_positions(16, 1) == [[1, 3, 5, 7, 9, 11, 13, 15], [2, 4, 6, 8, 10, 12, 14]]            # the last wave is ragged
    assert NC.wave_positions(4, 0) == [[0, 1, 2, 3]] and NC.wave_positions(10, 1) == [[1, 3, 5, 7, 9], [2, 4, 6, 8]]
    assert NC.branch_order([5, 9, 5, 9, 7]) == [1, 3, 4, 0, 2]
    # windows: wb[g + 1] = min(wb[g] + m_g - 1, 192), eb[g + 1] = min(eb[g] + m_g + 8, 256); a group without a branch counts as m = 1
    assert NC.windows([2] * 8) == [(g, 1, 10 * g, 10) for g in range(8)]
    assert NC.windows([100, 100, 5]) == [(0, 99, 0, 108), (99, 93, 108, 108), (192, 0, 216, 13), (192, 0, 229, 9), (192, 0, 238, 9),
                                         (192, 0, 247, 9), (192, 0, 256, 0), (192, 0, 256, 0)]
    assert NC.windows([300])[0] == (0, 192, 0, 256)
    assert (NC.OUT_STAGE, NC.CLUSTER_NODES, NC.CLUSTER_PASS, NC.CLUSTER_STRIDE) == (32, 256, 64, 16)
    assert (NC.WALK_BLOCK, NC.WALK_RING, NC.WALK_AHEAD, NC.LDS_NODES) == (1024, 4, 2 * 4 + 1, 60 * 1024)
    assert NC.stat_cols(4, False) == 17 and NC.stat_cols(4, True) == 21 and NC.stat_cols(2, False) == 5 and (NC.STATS_RIDING, NC.STATS_OWN) == (512, 256)


def test_case_names_are_unique_and_every_case_runs_clean_in_the_oracle():
    cases = NC.all_cases()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        for chain in sorted({0, c.S - 1}):
            assert NC.oracle_state(c, chain, c.N).rc == 0, c
        assert c.n_long == len(c.wide) and c.n_waves == c.n_long + len(c.waves) and sorted(c.wide + sum(c.waves, [])) == list(range(c.E))
        sizes = [len(w) for w in c.waves]                   # the missing groups are the last ones of the later waves
        assert sizes == sorted(sizes, reverse=True) and max(sizes) - min(sizes) <= 1 and 1 <= min(sizes) and max(sizes) <= 8


# ---------------------------------------------------------------------------------------------------------------------------
# cluster plans
# ---------------------------------------------------------------------------------------------------------------------------
def _tiers(text):
    return [[int(v) for v in tier.split(",")] for tier in text.split("|")]


def test_cluster_plans_under_sanitizers(tmp_path):
    """build_cluster_plan(s, 256) and build_band_plan(s, 8) on the 2-tip tree, ladders, balanced trees, a random tree and the
    cherry-bottom trees of the cases: the program checks the invariants of each plan and prints its tier and cluster sizes, which must
    be those the restated rules derive"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "cluster_plan_check")
    csrc = os.path.join(ROOT, "phylomap_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "native", "cluster_plan_check.cpp"), os.path.join(csrc, "phm_sched.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ok", run.stdout
    got = {name: _tiers(sizes) for name, sizes in (line.split(":") for line in lines[:-1])}
    assert len(got) == 2 * len(NC.PLAN_TREES)
    for name, make in NC.PLAN_TREES:
        shape = make()
        assert got[name + " clusters"] == NC.cluster_tiers(shape), name
        assert got[name + " bands"] == NC.band_tiers(shape), name
    # the sizes the documents name
    assert got["ladder 2 clusters"] == [[1]] and got["ladder 257 clusters"] == [[256]] and got["ladder 258 clusters"] == [[256], [1]]
    assert got["ladder 700 clusters"] == [[256], [256], [187]]
    assert got["balanced 257 clusters"] == [[256]] and got["balanced 258 clusters"] == [[128, 128], [1]]
    assert got["balanced 1024 clusters"] == [[255] * 4, [3]]
    assert got["ladder 700 bands"] == [[8]] * 87 + [[3]] and got["balanced 258 bands"] == [[128, 128], [1]]
    assert got["cherries 2048 1025 clusters"] == [[256] + [255] * 11, [11]]


# ---------------------------------------------------------------------------------------------------------------------------
# tree passes and walk
# ---------------------------------------------------------------------------------------------------------------------------
def test_tree_pass_cases_land_in_their_classes():
    by = {c.name: c for c in NC.cases_tree()}
    for name, tips in (("P_tips2", 2), ("P_tips3", 3)):
        c = by[name]
        up, down = NC.level_sizes(c.z)
        assert c.tips == tips and c.n_long == 0 and c.n_waves == 1 and len(c.waves[0]) == 2 * tips - 2 < 8
        assert sum(down) == tips - 2 and len([d for d in down if d]) == (tips - 2)      # no walk level at 2 tips, one edge at 3
    assert NC.level_sizes(by["P_tips2"].z)[1] == []
    # a height level of exactly 64 (one pass), 65 (a ragged second pass: one live group of 64) and 128 nodes (two full passes) in one cluster
    for name, level in (("P_level64", 64), ("P_level65", 65), ("P_level128", 128)):
        c = by[name]
        assert len(NC.cluster_tiers(c.shape)) == 1 and len(NC.cluster_tiers(c.shape)[0]) == 1
        assert NC.level_sizes(c.z)[0][0] == level and c.tips == 2 * level
        assert NC.ceil_div(level, NC.CLUSTER_PASS) == {64: 1, 65: 2, 128: 2}[level] and level % NC.CLUSTER_PASS == {64: 0, 65: 1, 128: 0}[level]
    assert NC.cluster_tiers(by["P_bushy256"].shape) == [[256]] and NC.cluster_tiers(by["P_bushy257"].shape) == [[128, 128], [1]]
    assert NC.cluster_tiers(by["P_ladder256"].shape) == [[256]] and NC.cluster_tiers(by["P_ladder257"].shape) == [[256], [1]]
    assert (by["P_ladder256"].tips, by["P_ladder257"].tips, by["P_bushy256"].tips, by["P_bushy257"].tips) == (257, 258, 257, 258)
    assert len(NC.level_sizes(by["P_ladder256"].z)[0]) == 256                       # a cluster of 256 levels of one node each
    # chains of 15 .. 17 and 31 .. 33 steps on the edges to internal nodes: either side of one and two strides of the dependency-driven form
    for segs in NC.CHAIN_SEGMENTS:
        c = by[f"P_chain{segs - 1}"]
        assert all(len(m) == segs for m in c.z["maps"]) and np.any(c.z["edge"][:, 1] > c.tips) and c.forms == (1, 2) and c.N == 1
        assert c.dependency_driven(2) and not c.dependency_driven(1) and not c.dependency_driven(0)
    assert [s - 1 for s in NC.CHAIN_SEGMENTS] == [NC.CLUSTER_STRIDE - 1, NC.CLUSTER_STRIDE, NC.CLUSTER_STRIDE + 1,
                                                  2 * NC.CLUSTER_STRIDE - 1, 2 * NC.CLUSTER_STRIDE, 2 * NC.CLUSTER_STRIDE + 1]
    s = by["P_sites"]
    assert s.S == 3 and s.sites.shape == (3, s.tips) and len({tuple(r) for r in s.sites}) == 3
    for name, n in (("P_ks2", 2), ("P_ks4", 4)):
        c = by[name]
        assert c.ks and c.n == n and set(np.unique(c.z["states"])) <= {1, 2} and c.ncnt == n * n
    assert {c.forms for c in by.values()} == {(1, 2)}
    assert {"plain", "bigtree", "ks"} == {c.variant for c in by.values()} and {2, 3, 4} == {c.n for c in by.values()}


def test_walk_cases_land_in_their_classes():
    by = {c.name: c for c in NC.cases_walk()}
    levels = []
    for t in NC.LADDER_TIPS:
        c = by[f"W_ladder{t}"]
        down = NC.level_sizes(c.z)[1]
        assert c.tips == t and down == [1] * (t - 2) and c.N == 3 and c.dump_at == (1, 2, 3)
        levels.append(len(down))
    assert levels == list(range(14)) and {v % NC.WALK_RING for v in levels} == {0, 1, 2, 3} and max(levels) > NC.WALK_AHEAD
    for name, widest in (("W_level63", 63), ("W_level64", 64), ("W_level65", 65), ("W_level1024", 1024), ("W_level1025", 1025)):
        c = by[name]
        assert max(NC.level_sizes(c.z)[1]) == widest, name
        assert c.tips - 1 <= NC.LDS_NODES
    assert by["W_level1025"].tips == 3073 and by["W_level1024"].E >= 2048 and by["W_level1024"].n_long == by["W_level1025"].n_long == NC.LONG
    assert 64 < 65 <= 2 * 64 and NC.WALK_BLOCK < 1025                               # the second wave prefetches; a thread takes a second edge


# ---------------------------------------------------------------------------------------------------------------------------
# the eight-lane walk
# ---------------------------------------------------------------------------------------------------------------------------
def _one_wave(c):
    assert c.E == 8 and c.n_long == 0 and c.n_waves == 1 and max(NC.expected_segments(c.z, c.Omega)) < NC.WIDE_SEGMENTS, c
    return sorted(NC.reached(c, sweep=1, chain=0), key=lambda r: r["group"])


def test_window_cases_reach_their_sums_and_refills():
    for total in (191, 192, 193):
        rs = _one_wave(NC.case_map_window(total))
        assert sum(r["m"] - 1 for r in rs) == total == NC.case_map_window(total).wants["map_sum"]
        assert sum(r["pre"] for r in rs) == min(total, NC.MAP_WINDOW) and [r["beyond"] for r in rs][:7] == [0] * 7
        assert rs[7]["beyond"] == max(0, total - NC.MAP_WINDOW)
    for by in (1, 8, 9):                               # one refill round of one, a full round, two rounds with a ragged second
        rs = _one_wave(NC.case_straddle(by))
        assert [r["beyond"] for r in rs] == [0] * 7 + [by] and rs[7]["pre"] == 10 and rs[7]["wb"] + rs[7]["pre"] == NC.MAP_WINDOW
        assert NC.ceil_div(by, NC.LANES) == {1: 1, 8: 1, 9: 2}[by]
    rs = _one_wave(NC.case_beyond())
    assert [(r["m"], r["wb"], r["pre"]) for r in rs[3:]] == [(6, 192, 0), (2, 192, 0), (1, 192, 0), (1, 192, 0), (1, 192, 0)]
    assert rs[3]["beyond"] == 5 and rs[2]["pre"] == 4 and rs[2]["beyond"] == 6
    assert rs[7]["eb"] + rs[7]["epre"] <= NC.EXP_WINDOW
    for total in (255, 256, 257):
        rs = _one_wave(NC.case_exp_window(total))
        assert sum(r["m"] + NC.EXP_AHEAD for r in rs) == total and sum(r["epre"] for r in rs) == min(total, NC.EXP_WINDOW)
        assert sum(r["m"] - 1 for r in rs) < NC.MAP_WINDOW
        assert rs[7]["epre"] == rs[7]["m"] + NC.EXP_AHEAD - max(0, total - NC.EXP_WINDOW)
    rs = _one_wave(NC.case_cut())
    assert (rs[6]["m"], rs[6]["epre"]) == (30, 28) and rs[6]["new"] > 28 and (rs[7]["m"], rs[7]["epre"], rs[7]["eb"]) == (10, 0, 256) and rs[7]["new"] > 0
    assert not any(r["stuck"] for r in rs)


def test_allotment_and_output_stage_are_reached():
    """L_allot: in some sweep some eight-lane branch with an uncut share consumes exactly m + 8 variates (no refill), m + 9 (one round
    for one), m + 16 (one full round) and m + 17 (a second round), and some branch leaves 31, 32, 33, 64 and 65 pieces (no flush, a
    flush with nothing behind it, one with one piece behind it, two flushes, two and one piece)"""
    c = NC.case_allot()
    _one_wave(c)
    rs = [r for r in NC.reach(c) if not r["wide"] and not r["stuck"]]
    over = {r["new"] - r["m"] - NC.EXP_AHEAD for r in rs if r["epre"] == r["m"] + NC.EXP_AHEAD}
    assert set(c.wants["over_allotment"]) <= over, sorted(over)
    pieces = {r["new"]: r["flushes"] for r in rs}
    assert set(c.wants["pieces"]) <= set(pieces), sorted(pieces)
    assert [pieces[k] for k in (31, 32, 33, 64, 65)] == [0, 1, 1, 2, 2]
    assert any(r["m"] == 1 and 30.0 <= c.Omega * c.z["edge.length"][r["branch"]] <= 36.0 for r in NC.reached(c, sweep=1))      # the issue's starting point


def test_ragged_waves_and_the_e_over_16_rule():
    got = {}
    for tips, long_branch in ((5, False), (9, False), (6, True), (8, False)):
        c = NC.case_ragged(tips, long_branch)
        got[tips] = (c.E, c.n_long, (c.E - c.n_long) % 8, len(c.waves[-1]))
    # E is even, so the edge sits between E = 14 (8 tips: none) and E = 16 (9 tips: one wave-wide branch)
    assert got == {5: (8, 0, 0, 8), 9: (16, 1, 7, 7), 6: (10, 1, 1, 4), 8: (14, 0, 6, 7)}      # 15 = 8 + 7, 9 = 5 + 4, 14 = 7 + 7 branches
    assert max(NC.expected_segments(NC.case_ragged(6, True).z, NC.case_ragged(6, True).Omega)) == 96
    by = {c.name: c for c in NC.cases_lanes()}
    assert (by["L_wide127"].tips, by["L_wide127"].n_long, by["L_wide128"].tips, by["L_wide128"].n_long) == (1024, 127, 1025, 128)
    assert max(NC.expected_segments(by["L_wide128"].z, by["L_wide128"].Omega)) < NC.WIDE_SEGMENTS


def test_expected_95_and_96_segments():
    for through in ("length", "path"):
        lo, hi = NC.case_expected(95, through), NC.case_expected(96, through)
        assert max(NC.expected_segments(lo.z, lo.Omega)) == 95.0 and max(NC.expected_segments(hi.z, hi.Omega)) == 96.0
        assert (lo.n_long, hi.n_long) == (0, 1) and not lo.dependency_driven(0) and hi.dependency_driven(0)
        assert hi.wide == [3] and (len(hi.z["maps"][3]) == 96) == (through == "path") and hi.forms == (0, 1, 2)
        assert hi.n_waves == 2 and len(hi.waves[0]) == 7


# ---------------------------------------------------------------------------------------------------------------------------
# the wave-wide walk
# ---------------------------------------------------------------------------------------------------------------------------
def test_wave_wide_cases_reach_their_blocks():
    """old paths of 1, 2, 64, 65, 66, 129 and 130 segments: m - 1 change points in no block, one lane, 63 lanes, a full block, a full
    block and one lane, two blocks, two blocks and one lane.  Not asserted: where in a block the states change (the reach functions
    cannot see a change at the first or last lane of a block)."""
    blocks = {1: (0, 0), 2: (1, 1), 64: (1, 63), 65: (1, 64), 66: (2, 1), 129: (2, 64), 130: (3, 1)}
    for m0 in NC.WIDE_PATHS:
        for variant, n in NC.WIDE_SWEEPS:
            c = NC.case_wide(m0, variant, n)
            assert c.E == 16 and c.wide == [c.long_branch] and c.n_long == 1 and c.N >= 4 and c.S >= 2 and c.ks == (variant == "ks")
            for chain in range(c.S):
                r, = NC.reached(c, wide=True, sweep=1, chain=chain)
                assert r["m"] == m0 and r["old_blocks"] == blocks[m0][0] and (m0 - 1) - 64 * max(0, blocks[m0][0] - 1) == blocks[m0][1]
                later = NC.reached(c, wide=True, chain=chain, sweep=lambda rec: rec["sweep"] > 1)
                assert len(later) == c.N - 1 and all(rec["m"] > 1 for rec in later)      # later sweeps read what the walk wrote
    assert {(v, n) for v, n in NC.WIDE_SWEEPS} == {("plain", 2), ("plain", 3), ("plain", 4), ("ks", 2), ("ks", 4)}
    for c in (NC.case_wide(130, "plain", 2, zero=True), NC.case_wide(130, "ks", 4, zero=True)):
        r, = NC.reached(c, wide=True, sweep=1, chain=0)
        path = c.z["maps"][c.long_branch]
        assert r["stuck"] and path[70] == 0.0 and np.all(np.delete(path, 70) > 0) and 65 <= 70 < 129      # inside the second block


def test_wave_wide_consumption_and_long_merged_segments():
    c = NC.case_wide_consume()
    assert c.n_long == 2
    used = {r["new"]: r["var_blocks"] for r in NC.reached(c, wide=True, stuck=False)}
    assert set(c.wants["wide_consumes"]) <= set(used), sorted(used)
    assert [used[k] for k in (63, 64, 65, 129)] == [1, 1, 2, 3]
    c = NC.case_wide_run()
    assert c.wide == [int(np.argmax(c.z["edge.length"]))]
    runs = [r["run"] for r in NC.reached(c, wide=True)]
    assert len(runs) == c.S * c.N and min(runs) > c.wants["wide_run_over"], runs


# ---------------------------------------------------------------------------------------------------------------------------
# flags, capacity, statistics
# ---------------------------------------------------------------------------------------------------------------------------
def test_flag_cases():
    c = NC.case_absorbing()
    assert np.array_equal(c.B[2], [0.0, 0.0, 1.0]) and c.n_long == 1 and len(c.z["maps"][c.wide[0]]) == 130
    assert all(NC.oracle_state(c, chain, c.N).rc == 0 for chain in range(c.S))
    assert np.any(c.z["states"] != 3)                  # branches that do not end in the absorbing state: their maps flag the entry of state 3
    bad = NC.case_impossible()
    assert NC.oracle_state(bad, 0, 1).rc & O.ERR_ZERO_PROB
    assert np.all(bad.z["states"] != 3) and np.array_equal(bad.pid, [0.0, 0.0, 1.0])


@pytest.mark.parametrize("kind", ["lanes", "wide"])
def test_capacity_cases_overflow_where_they_say(kind):
    """the first sweep in which a new path outgrows its slot (the slots as plan_slots cuts them at cap_tail = 0.9) holds such a branch
    of the kind the case names; the eight-lane one has written out a full output stage before"""
    c = NC.case_capacity(kind)
    over = [r for r in NC.reach(c) if r["new"] > c.caps[r["branch"]]]
    assert over and c.opt["cap_tail"] == 0.9
    first = min(r["sweep"] for r in over)
    hit = [r for r in over if r["sweep"] == first and r["wide"] == (kind == "wide")]
    assert hit, over[:3]
    if kind == "lanes":
        assert c.n_long == 0 and any(c.caps[r["branch"]] >= NC.OUT_STAGE for r in hit)
    assert first < c.N


def test_statistics_cases():
    rows = [NC.case_stats(t).n_waves for t in NC.STAT_TIPS]
    assert rows == [14, 412, 687] and rows[0] < NC.STATS_OWN < rows[1] <= NC.STATS_RIDING < rows[2]
    assert all(NC.case_stats(t).S == 1 and not NC.case_stats(t).opt for t in NC.STAT_TIPS)
    assert [NC.ceil_div(s, 64) for s in NC.REDUCE_CHAINS] == [1, 2, 3] and [s % 64 for s in NC.REDUCE_CHAINS] == [0, 1, 2]
    for s in NC.REDUCE_CHAINS:
        assert NC.case_reduce(s, "ks").ks and NC.case_reduce(s, "bigtree").tips == 12 and NC.case_reduce(s, "ks").opt == {"reduce": True}
