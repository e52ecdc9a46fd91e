"""The lane-per-replica sweep kernels for 5 to 64 states (phm_wtiles.hip) at the bottom and the top of every state-count class their
launchers distinguish (tests/wtilesclasses.py; tests/test_wtiles_classes_cpu.py shows that the cases reach every instantiation):
each case against the CPU oracle with the bar of BASELINE.json -- counts bit-exact, dwell sums within 1e-10 relative -- and the chain
state of a replica of the last, partly filled tile bit for bit; the forms of one case against each other, the replica-summed output
against the sum, and the tree length in every dwell row."""
import numpy as np
import pytest

import wtilesclasses as W
from phylomap_amd import _lib, api
from test_gpu_parity import _same

pytestmark = pytest.mark.gpu

_VARIANT = {"plain": _lib.PHM_MCMC, "bigtree": _lib.PHM_MCMC_BIGTREE, "ks": _lib.PHM_MCMC_KS}
_API = {"plain": api.sumstatMCMC, "bigtree": api.sumstatMCMC_bigtree, "ks": api.sumstatMCMCks_sweep}


def _engine_run(case, run, dump_replica=None):
    """(statistics, dump or None) of one engine run of the case under the run's options"""
    eng = _lib.Engine(case.z, case.Q, case.pid, case.Omega, case.N, variant=_VARIANT[case.variant], seed=case.seed, n_replicas=case.S,
                      mapping="tiles", **run)
    try:
        eng.run(case.N); eng.sync()
        return eng.stats(0, case.N), (eng.dump(dump_replica) if dump_replica is not None else None)
    finally:
        eng.close()


def _against_oracle(case, got):
    n = case.n
    for r in case.replicas:
        want, rc = W.oracle_rows(case, r)
        assert rc == 0
        _same(got[r], want, n, "tiles", ks=case.ks)
    # every replica's dwell row adds up to the tree length, on every sweep
    np.testing.assert_allclose(got[:, :, :n].sum(2), case.length, rtol=1e-11)


def _chain_state_is_the_oracles(case, d):
    """seg_count, node_states and the partial likelihoods of replica S - 1 after the last sweep, bit for bit: DESIGN.md section 2
    gives the chain products of every pruning form the oracle's order of fused multiply-adds, the normalisation its four interleaved
    sums and the band kernels the dense sums less their exact zeros, so no form is exempt; the paths themselves likewise"""
    rc, dump = W.oracle_dump(case, case.S - 1)
    assert rc == 0
    np.testing.assert_array_equal(d["seg_count"], dump.seg_count)
    T = len(case.z["states"]) if case.ks else 0          # ks sweep: Engine.dump shows the observed tips, the oracle the re-drawn ones
    np.testing.assert_array_equal(d["node_states"][T:], dump.node_states[T:])
    np.testing.assert_array_equal(d["PL"][T:], dump.PL[T:])
    for b, m in enumerate(dump.seg_count):
        np.testing.assert_array_equal(d["seg_dwell"][b, :m], dump.seg_dwell[b, :m])


def _reduced_is_the_sum(case, red, per):
    n, c = case.n, case.n + case.ncnt
    assert red.shape == per.shape[1:]
    np.testing.assert_array_equal(red[:, n:c], per.sum(0)[:, n:c])
    np.testing.assert_allclose(red[:, :n], per.sum(0)[:, :n], rtol=1e-12, atol=0)
    if case.ks:                                          # parameter columns: plain values; root states: summed
        np.testing.assert_array_equal(red[:, c:-1], per[0][:, c:-1])
        np.testing.assert_array_equal(red[:, -1], per.sum(0)[:, -1])


DENSE = W.dense_cases() + W.ks_form_cases()


@pytest.mark.parametrize("case", DENSE, ids=[c.name for c in DENSE])
def test_dense_every_pruning_form_against_the_oracle_and_each_other(case):
    """bottom and top of every class of ceil(n / 4) from 2 to 16, 150 replicas (22 live lanes in the third tile): the automatic
    form (few tiles: row-split workgroups, or a wave per block up to 16 states), the matrix in registers (1), the split forced (2)
    and, from 17 states, the matrix in LDS (3: wt_up2_kernel<MT, ceil(n / 4)>) -- the same bits from each (phm_wtiles.hip's header).
    The ks sweep at 12 and 34 states likewise (70 replicas): its tips are rows of the parity-mask table in every form"""
    first = None
    for run in case.runs:
        got, d = _engine_run(case, run, dump_replica=case.S - 1)
        _chain_state_is_the_oracles(case, d)
        if first is None:
            first = got
            _against_oracle(case, got)
        else:
            np.testing.assert_array_equal(got, first, err_msg=str(run))


BAND_RANDOM = [c for c in W.band_cases() if c.name.endswith("random")]
BAND_LADDER = [c for c in W.band_cases() if c.name.endswith("ladder")]


@pytest.mark.parametrize("case", BAND_RANDOM, ids=[c.name for c in BAND_RANDOM])
def test_band_kernels_per_level_against_the_oracle(case):
    """wt_up_band_kernel<NP, HB>, wt_down1r_kernel<NP> and the banded draws of the branch kernel at the smallest and the largest n
    of every (NP, HB): tips at both ends of the state space, so the rows whose band is cut by the matrix edge are drawn from"""
    got, d = _engine_run(case, case.runs[0], dump_replica=case.S - 1)
    _against_oracle(case, got)
    _chain_state_is_the_oracles(case, d)


@pytest.mark.parametrize("case", BAND_LADDER, ids=[c.name for c in BAND_LADDER])
def test_band_kernels_over_subtree_clusters_against_the_oracle_and_the_levels(case):
    """the same classes on a 300-tip ladder: a launch per level (level_groups 1), subtree clusters forced (2) and chosen (0)"""
    outs = []
    for run in case.runs:
        got, d = _engine_run(case, run, dump_replica=case.S - 1)
        _chain_state_is_the_oracles(case, d)
        outs.append(got)
    _against_oracle(case, outs[0])
    np.testing.assert_array_equal(outs[1], outs[0])
    np.testing.assert_array_equal(outs[2], outs[0])


GROUPED = W.b2l_cases()


@pytest.mark.parametrize("case", GROUPED, ids=[c.name for c in GROUPED])
def test_rows_of_B_in_lds_beyond_32_states_equal_one_branch_per_wave(case):
    """branch_group = 4 turns on wt_branch_kernel<KS, false, true, 0> on a 14-tip tree (automatically it takes 4 x 65 536 waves):
    against branch_group = 1 and the oracle, per replica and summed over replicas"""
    fn = _API[case.variant]
    out = {(r["branch_group"], r["reduce"]): fn(case.z, case.Q, case.pid, case.Omega, case.N, seed=case.seed, n_replicas=case.S,
                                               mapping="tiles", **r) for r in case.runs}
    _against_oracle(case, out[1, False])
    np.testing.assert_array_equal(out[4, False], out[1, False])
    _reduced_is_the_sum(case, out[1, True], out[1, False])
    np.testing.assert_array_equal(out[4, True], out[1, True])
    _, d = _engine_run(case, {"branch_group": 4}, dump_replica=case.S - 1)
    _chain_state_is_the_oracles(case, d)


COUNTED = W.slot_cases() + W.ks_small_cases()


@pytest.mark.parametrize("case", COUNTED, ids=[c.name for c in COUNTED])
def test_counting_in_lds_slots_and_beside_them(case):
    """either side of WT_MAX_SLOTS = 96 possible transitions (dense 10 | 11 states, half-bandwidth 2 at 25 | 26), and the ks sweep's
    n x n layout at n <= 32 with a band of 2, of 1 and without the band kernels: per replica against the oracle, and the
    replica-summed output (LDS slots, or the workgroup's n x n counters where there are none) against the sum"""
    fn = _API[case.variant]
    per, red = (fn(case.z, case.Q, case.pid, case.Omega, case.N, seed=case.seed, n_replicas=case.S, mapping="tiles", **r) for r in case.runs)
    _against_oracle(case, per)
    _reduced_is_the_sum(case, red, per)
    _, d = _engine_run(case, {k: v for k, v in case.runs[0].items() if k != "reduce"}, dump_replica=case.S - 1)
    _chain_state_is_the_oracles(case, d)
