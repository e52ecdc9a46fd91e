"""The (tile, branch) sweep for 2 to 4 states (phm_tiles.hip, phm_mcmc_maps.hip; tiles_setup, fill_tile_params and tiles_sweep_parts
of phm_engine.cpp) at every group, path and copy class (tests/tilesclasses.py; tests/test_tiles_classes_cpu.py pins every case to
its class): each case against the CPU oracle with the bar of BASELINE.json as test_gpu_parity._same states it -- counts bit for bit,
dwell sums within 1e-10 relative, trailing columns within 1e-9 -- the tree length in every dwell row of every replica, the groups of
a case against each other (counts and integer columns bit for bit: grouping changes only where partial dwell sums are rounded), the
sweep parts against each other bit for bit, the replica-summed output against the sum, and the automatic classes at natural size
against the forced ones and the replica mapping."""
import collections

import numpy as np
import pytest

import tilesclasses as T
from phylomap_amd import _lib, api
from test_gpu_mcmc_maps import _check_history, _twin
from test_gpu_parity import _same

pytestmark = pytest.mark.gpu

_VARIANT = {"plain": _lib.PHM_MCMC, "bigtree": _lib.PHM_MCMC_BIGTREE, "bf": _lib.PHM_MCMC_BF, "ks": _lib.PHM_MCMC_KS}
_API = {"plain": api.sumstatMCMC, "bigtree": api.sumstatMCMC_bigtree, "bf": api.sumstatMCMCbf_sweep, "ks": api.sumstatMCMCks_sweep}

Run = collections.namedtuple("Run", "stats recoveries bytes launches")


def _run(case, group=0, mapping="tiles", **over):
    """the case's run() calls on one engine: the `it & 1` dwell buffers swap across calls"""
    opt = dict(case.base, **over)
    if group:
        opt["branch_group"] = group
    if case.sites is not None:
        opt["tips_per_replica"] = True
    eng = _lib.Engine(case.z, case.Q, case.pid, case.Omega, case.N, variant=_VARIANT[case.variant], states=case.sites, seed=case.seed,
                      n_replicas=case.S, mapping=mapping, **opt)
    try:
        launches = []
        for k in case.runs:
            eng.run(k); eng.sync()
            launches.append(int(eng.info().last_run_launches))
        info = eng.info()
        return Run(np.array(eng.stats(0, case.N)), int(info.recoveries), int(info.device_bytes), tuple(launches))
    finally:
        eng.close()


def _against_oracle(case, run, recoveries=0):
    got = run.stats
    assert got.shape[:2] == (case.S, case.N)
    for r in case.replicas:
        _same(got[r], T.oracle_rows(case, r), case.n, "tiles", ks=case.ks_layout)
    np.testing.assert_allclose(got[:, :, :case.n].sum(2), case.length, rtol=1e-11)      # every replica, every sweep
    assert run.recoveries == recoveries


def _same_across_groups(case, a, b):
    n = case.n
    np.testing.assert_array_equal(a[..., n:], b[..., n:])
    np.testing.assert_allclose(a[..., :n], b[..., :n], rtol=1e-10, atol=0)


def _reduced_is_the_sum(case, red, per):
    n, c = case.n, case.n + case.ncnt
    assert red.shape == per.shape[1:]
    np.testing.assert_array_equal(red[:, n:c], per.sum(0)[:, n:c])
    np.testing.assert_allclose(red[:, :n], per.sum(0)[:, :n], rtol=1e-12, atol=0)


def _oracle_and_groups(case, **over):
    """every group of the case against the oracle, and against the first"""
    runs = {g: _run(case, g, **over) for g in case.groups}
    for g, run in runs.items():
        _against_oracle(case, run)
        _same_across_groups(case, run.stats, runs[case.groups[0]].stats)
    return runs


A = T.cases_a()


@pytest.mark.parametrize("case", A, ids=repr)
def test_every_branch_kernel_at_group_1_3_and_64(case):
    """A: plain, bf and ks sweeps at 2 to 4 states on short (24 tips, the packed form) and 300-segment paths (12 tips, LONG): one
    branch per wave, groups of 3 with a last group of one, one wave for the whole tree; two tiles, the second with 6 live lanes.
    The long kind once more with a launch per level (tiles_up_kernel instead of the ASYNC cluster kernel): the same bits"""
    runs = _oracle_and_groups(case)
    if case.long:
        levels = _run(case, 3, level_groups=1)
        assert levels.recoveries == 0
        np.testing.assert_array_equal(levels.stats, runs[3].stats)


def test_chunks_of_the_dwell_reduction():
    """B: 66 groups = 2 chunks (the second of 2), 198 groups = 4 chunks (the last of 6), per replica and summed over replicas"""
    case = T.case_b()
    runs = _oracle_and_groups(case)
    for g in case.groups:
        red = _run(case, g, reduce=True)
        assert red.recoveries == 0
        _reduced_is_the_sum(case, red.stats, runs[g].stats)


C = T.cases_c() + T.cases_c_slow()


@pytest.mark.parametrize("case", C, ids=repr)
def test_form_rule_and_chain_table_edge(case):
    """C: 25 and 48 caller-supplied segments stay in the packed form and draw from chain rows 23 (the last in LDS) and 24+ (global
    memory); 49, 64 and 65 take the LONG form, whose prefetched rows cross the same edge.  The same at 25, 26 and 49 segments under a
    nearly periodic 2-state chain, where rows 23 and 24 differ by 0.38 in every entry"""
    _oracle_and_groups(case)


def test_counter_hand_over_inside_a_group():
    """D: 90 000 segments in one wave's group; every lane counts about 86 800 (1, 1) pairs in sweep 1, so the 16-bit LDS counters must
    be handed to the global ones before the third long branch -- a hand-over that is missing or resets the wrong thing wraps that
    column.  All replicas of the grouped run against one branch per wave, four against the oracle"""
    case = T.case_d()
    runs = _oracle_and_groups(case)
    assert np.all(runs[64].stats[:, 0, case.n] > 65535)
    assert runs[64].bytes < 0.25 * T.GIB


E = T.cases_e()


@pytest.mark.parametrize("case", E, ids=repr)
def test_counter_copies(case):
    """E: the ks sweep's 16 counters in 64, 16, 4 copies and 1 copy per tile, groups of 3 spread over them; at 512 tiles every
    replica also against the replica mapping"""
    runs = _oracle_and_groups(case)
    if case.tiles == 512:
        rep = _run(case, mapping="replicas")
        _same_across_groups(case, runs[3].stats, rep.stats)


@pytest.mark.parametrize("case", [T.case_f(4), T.case_f(2)], ids=repr)
def test_sweep_parts_with_groups_on_an_uneven_tile_split(case):
    """F: five tiles in parts of 3 + 2 and 2 + 2 + 1 with one and three branches per wave: every column bit for bit as one part"""
    for g in case.groups:
        one = _run(case, g, sweep_parts=1)
        _against_oracle(case, one)
        for p in T.PARTS_F[1:]:
            got = _run(case, g, sweep_parts=p)
            assert got.recoveries == 0
            np.testing.assert_array_equal(got.stats, one.stats, err_msg=f"group {g}, {p} parts")
            assert got.launches == tuple(p * k for k in one.launches)
    _same_across_groups(case, _run(case, 3, sweep_parts=2).stats, _run(case, 1, sweep_parts=1).stats)


@pytest.mark.parametrize("case", [T.case_g_sites(), T.case_g_offset()], ids=repr)
def test_per_replica_tips_and_replica_offsets_with_groups(case):
    """G: 130 alignment sites (tips per replica) and replica_offset = 1000 (oracle replicas 1000 + r), groups of 3 against 1"""
    runs = _oracle_and_groups(case)
    red = _run(case, 3, reduce=True)
    _reduced_is_the_sum(case, red.stats, runs[3].stats)


H = T.cases_h()


@pytest.mark.parametrize("case", H, ids=repr)
def test_maps_replay_with_groups(case):
    """H: mcmc_maps_tiles_kernel walks the branch kernel's groups itself: the maps of sweeps 1 and 3 against the Python twin bit for
    bit on the compared replicas, the same maps from every group, the statistics those of the call without maps"""
    its, E, J = list(T.MAP_ITERS_H), case.E, len(T.MAP_ITERS_H)
    first = None
    for g in case.groups:
        kw = dict(seed=case.seed, n_replicas=case.S, reduce=False, branch_group=g)
        out, m = _API[case.variant](case.z, case.Q, case.pid, case.Omega, case.N, maps=True, map_iters=its, **kw)
        assert m.n_hist == case.S * J and m.n_edge == E
        plain = _API[case.variant](case.z, case.Q, case.pid, case.Omega, case.N, mapping="tiles", **kw)
        np.testing.assert_array_equal(out, plain)
        if first is None:
            first = m
            for r in case.replicas:
                tout, rows = _twin(case.z, case.Q, case.Omega, case.pid, case.N, case.seed, r, case.variant, its)
                for j in range(J):
                    _check_history(m, r * J + j, rows, j, E)
                np.testing.assert_array_equal(out[r][:, case.n:], np.array(tout)[:, case.n:])
        else:
            for a, b in ((m.off, first.off), (m.state, first.state), (m.dwell, first.dwell)):
                np.testing.assert_array_equal(a, b, err_msg=f"group {g}")


def test_capacity_recovery_with_groups():
    """I: slots far too small on purpose (chosen as test_capacity_recovery_replays_through_the_parts chooses them): the rebuilt
    engine replays in groups of 3 and ends where one branch per wave ends"""
    case = T.case_i()
    one, three = _run(case, 1), _run(case, 3)
    assert one.recoveries >= 1 and three.recoveries >= 1
    for run in (one, three):
        _against_oracle(case, run, recoveries=run.recoveries)
    _same_across_groups(case, three.stats, one.stats)


@pytest.mark.parametrize("tips", [1024, 1025])
def test_automatic_group_at_its_1_2_edge(tips):
    """J1: 4 096 replicas of 2 states: 64 x 2 046 (tile, branch) pairs keep one branch per wave, 64 x 2 048 take two.  The automatic
    run equals the run with branch_group set to the restated value in every bit -- and differs in its dwell rounding from the other
    side of the edge, so the observable does tell the two apart -- and every replica equals the replica mapping"""
    case = T.case_j1(tips)
    auto = _run(case)
    _against_oracle(case, auto)
    assert auto.bytes == case.bytes() <= T.BYTES_CAP
    np.testing.assert_array_equal(auto.stats, _run(case, case.group(0)).stats)
    other = _run(case, 3 - case.group(0)).stats
    _same_across_groups(case, auto.stats, other)
    assert not np.array_equal(auto.stats, other)
    _same_across_groups(case, auto.stats, _run(case, mapping="replicas").stats)


def test_the_class_of_the_headline():
    """J2: 256 tiles x 4 198 branches -- group 16 with a last group of 6, 5 chunks, 2 counter copies, one launch per level, two parts
    on streams of their own -- automatically.  Equal in every bit to the run with branch_group = 16, to one part (with the launches
    of two forced parts), and per replica to the replica mapping; 9.41 GiB (tilesclasses.case_j2)"""
    case = T.case_j2()
    auto = _run(case)
    _against_oracle(case, auto)
    assert auto.bytes == case.bytes()
    forced = _run(case, T.group(case.tiles, case.E))
    np.testing.assert_array_equal(auto.stats, forced.stats)
    two, one = _run(case, sweep_parts=2), _run(case, sweep_parts=1)
    assert auto.launches == two.launches == tuple(2 * k for k in one.launches)
    np.testing.assert_array_equal(auto.stats, one.stats)
    np.testing.assert_array_equal(auto.stats, two.stats)
    assert not np.array_equal(auto.stats, _run(case, 8).stats)      # the group is observable at this size
    _same_across_groups(case, auto.stats, _run(case, mapping="replicas").stats)
