"""The one-chain branch mapping for 2 to 4 states (phm_narrow.hip; narrow_setup and fill_narrow_params of phm_engine.cpp) at every class
edge (tests/narrowclasses.py; tests/test_narrow_classes_cpu.py pins every case to its class and asserts from the oracle's chain states
that it reaches what it is there to reach): each case through _lib.Engine(..., mapping="branches") against the CPU oracle, chain for
chain -- transition counts, root state and the other integer columns equal, dwell sums within 1e-10 relative (the stated bar of this
mapping), the tree length in every row within 1e-11, and the chain state (segment counts, node states, partial likelihoods and every
dwell piece of every branch) equal after the last sweep and after the sweeps in which a class is reached.  The statistics row hides
most slips -- a wrong piece written at a flush boundary still sums to the right dwell time -- the dwell pieces do not."""
import numpy as np
import pytest

import narrowclasses as NC
from phylomap_amd import _lib

pytestmark = pytest.mark.gpu

_VARIANT = {"plain": _lib.PHM_MCMC, "bigtree": _lib.PHM_MCMC_BIGTREE, "ks": _lib.PHM_MCMC_KS}


def _engine(case, form=0, **over):
    opt = dict(case.opt, **over)
    if case.sites is not None:
        opt["tips_per_replica"] = True
    eng = _lib.Engine(case.z, case.Q, case.pid, case.Omega, case.N, variant=_VARIANT[case.variant], states=case.sites, seed=case.seed,
                      n_replicas=case.S, mapping="branches", pruning_form=form, **opt)
    assert eng.info().mapping == _lib.MAPPING["branches"]
    return eng


def _same_state(case, eng, k, chains=None):
    """eng.dump(r) after k sweeps against the oracle's: segment counts, node states, partial likelihoods, every dwell piece.  Under the
    ks sweep the internal nodes only: phm_engine_dump reports the tips as observed, and the states the sweep re-samples for them are
    held to the oracle's by the dwell pieces and counts of the tip branches they end"""
    for r in range(case.S) if chains is None else chains:
        want, got = NC.oracle_state(case, r, k), eng.dump(r, seg_cap=case.seg_cap)
        assert int(want.seg_count.max()) <= case.seg_cap
        np.testing.assert_array_equal(got["seg_count"], want.seg_count, err_msg=f"{case} chain {r} sweep {k}: segment counts")
        lo = case.tips if case.ks else 0               # ks: the dump's tip rows hold the observed parity, the oracle's the re-sampled tip
        np.testing.assert_array_equal(got["node_states"][lo:], want.node_states[lo:], err_msg=f"{case} chain {r} sweep {k}: node states")
        if k > 0:
            np.testing.assert_array_equal(got["PL"][lo:], want.PL[lo:], err_msg=f"{case} chain {r} sweep {k}: partial likelihoods")
        live = np.arange(case.seg_cap)[None, :] < want.seg_count[:, None]
        np.testing.assert_array_equal(np.where(live, got["seg_dwell"], 0.0), np.where(live, want.seg_dwell, 0.0),
                                      err_msg=f"{case} chain {r} sweep {k}: dwell pieces")


def _same_rows(case, got, want):
    """counts bit for bit, dwell sums within 1e-10 relative, the trailing columns (root state, ...) equal, the tree length in every row"""
    n, c = case.n, case.n + case.ncnt
    assert got.shape == want.shape
    np.testing.assert_array_equal(got[..., n:c], want[..., n:c], err_msg=f"{case}: counts")
    np.testing.assert_allclose(got[..., :n], want[..., :n], rtol=1e-10, atol=0, err_msg=f"{case}: dwell sums")
    np.testing.assert_array_equal(got[..., c:], want[..., c:], err_msg=f"{case}: trailing columns")
    np.testing.assert_allclose(got[..., :n].sum(-1), case.length, rtol=1e-11, err_msg=f"{case}: tree length")


def _oracle_rows(case):
    return np.stack([NC.oracle_state(case, r, case.N).rows for r in range(case.S)])


def _check(case, recoveries=0):
    """the case under each of its pruning forms: the chain state after every sweep of dump_at and all rows against the oracle, and the
    forms against each other bit for bit"""
    first = None
    for form in case.forms:
        eng = _engine(case, form)
        try:
            done = 0
            for k in case.dump_at:
                eng.run(k - done); eng.sync()
                done = k
                _same_state(case, eng, k)
            got = np.array(eng.stats(0, case.N))
            info = eng.info()
            assert (info.recoveries >= 1) if recoveries else (info.recoveries == 0)
        finally:
            eng.close()
        _same_rows(case, got, _oracle_rows(case))
        if first is None:
            first = got
        np.testing.assert_array_equal(got, first, err_msg=f"{case}: pruning_form {form} against {case.forms[0]}")


@pytest.mark.parametrize("case", NC.cases_tree(), ids=repr)
def test_tree_passes(case):
    """2 and 3 tips (no walk level, one ragged wave); a cluster level of 64, 65 and 128 nodes; a cluster of 256 nodes in one tier and 257
    nodes in two, bushy and as a ladder; chains of 15 .. 17 and 31 .. 33 steps either side of the stride of the dependency-driven form
    (PL after one sweep); tips per replica; the ks sweep's parity masks at 2 and 4 states; plain and rescaled pruning -- each with a
    barrier per level and dependency-driven, the two forms equal in every bit"""
    assert case.forms == (1, 2)
    _check(case)


@pytest.mark.parametrize("case", NC.cases_walk(), ids=repr)
def test_walk(case):
    """ladders of 0 .. 13 walk levels (every residue of the ring of four prefetched levels, the first refill of the level boundaries),
    node states after each of three sweeps; a level of 63, 64 and 65 edges (the second wave prefetches or not); a level of 1 024 and
    1 025 edges (a thread takes a second edge of the level)"""
    _check(case)


@pytest.mark.parametrize("case", NC.cases_lanes(), ids=repr)
def test_eight_lane_walk(case):
    """map window sums of 191 .. 193, a branch 1, 8 and 9 old segments past the window, a branch wholly beyond it beside m = 1 branches;
    variate window sums of 255 .. 257, a cut share that is refilled; consumption of exactly m + 8, m + 9, m + 16 and m + 17 variates;
    new paths of 31 .. 33, 64 and 65 pieces; ragged waves; E = 14 and 16; a branch expected to hold 95 and 96 segments, through its
    length and through the caller's path"""
    _check(case)


@pytest.mark.parametrize("case", NC.cases_wide(), ids=repr)
def test_wave_wide_walk(case):
    """old paths of 1, 2, 64, 65, 66, 129 and 130 segments under plain counting at 2 to 4 states and ks counting at 2 and 4, four sweeps
    of two chains; a zero-length segment inside a block; sweeps that consume 63, 64, 65 and 129 variates; merged segments of more than
    64 pieces.  (Not asserted by the CPU test: a state change at the first or last lane of a block.)"""
    _check(case)


def test_absorbing_state_flags_that_never_materialise():
    """a 3-state Q with an absorbing state: the maps carry the "all probabilities zero" flag in the entries of previous states that never
    materialise -- in the down maps, the eight-lane walk and the wave-wide walk's composed maps -- and the call is OK and the oracle's"""
    _check(NC.case_absorbing())


def test_impossible_tips_fail_with_zero_prob():
    case = NC.case_impossible()
    assert NC.oracle_state(case, 0, 1).rc & NC.O.ERR_ZERO_PROB
    with pytest.raises(_lib.PhmError) as e:
        eng = _engine(case)
        try:
            eng.run(1); eng.sync()
        finally:
            eng.close()
    assert e.value.status == 5                         # PHM_ERR_ZERO_PROB


@pytest.mark.parametrize("kind", ["lanes", "wide"])
def test_capacity(kind):
    """cap_tail = 0.9: a slot overflows in an eight-lane branch after a 32-piece flush / in the wave-wide branch; the engine recovers
    and its statistics and chain state are the oracle's; without recovery the same input fails with PHM_ERR_CAPACITY"""
    case = NC.case_capacity(kind)
    _check(case, recoveries=1)
    with pytest.raises(_lib.PhmError) as e:
        eng = _engine(case, recover=False)
        try:
            eng.run(case.N); eng.sync()
        finally:
            eng.close()
    assert e.value.status == 6                         # PHM_ERR_CAPACITY


@pytest.mark.parametrize("tips", NC.STAT_TIPS)
def test_statistics_rows_and_split_calls(tips):
    """14, 412 and 687 wave rows per chain: every sweep's row against the oracle -- the middle sweeps of a call are added up by 512
    threads riding in the next sweep's first launch, the last one by 256 in a launch of its own -- in one call, in N calls of one
    sweep and in two calls; integer columns identical across the three, dwell sums each within the bar of the oracle; and the row a
    one-chain engine leaves in page-locked memory after every call"""
    case = NC.case_stats(tips)
    want = _oracle_rows(case)
    N, a = case.N, 2
    runs = {}
    for name, calls in (("one call", [N]), ("sweep by sweep", [1] * N), ("two calls", [a, N - a])):
        eng = _engine(case)
        try:
            done = 0
            for k in calls:
                eng.run(k); eng.sync()
                done += k
                _same_rows(case, np.array(eng.stats(done - 1, 1)), want[:, done - 1:done])      # the page-locked row of the last sweep
            runs[name] = np.array(eng.stats(0, N))
            _same_state(case, eng, N)
            assert eng.info().recoveries == 0
        finally:
            eng.close()
        _same_rows(case, runs[name], want)
    n = case.n
    for name in ("sweep by sweep", "two calls"):
        np.testing.assert_array_equal(runs[name][..., n:], runs["one call"][..., n:])
        print(f"{case}: dwell sums of '{name}' bit-equal to one call: {np.array_equal(runs[name][..., :n], runs['one call'][..., :n])}")


@pytest.mark.parametrize("variant", ["bigtree", "ks"])
@pytest.mark.parametrize("chains", NC.REDUCE_CHAINS)
def test_rows_summed_over_the_chains_of_a_tile(chains, variant):
    """reduce=True with 64, 65 and 130 chains: the sums over chains against the oracle's rows added in chain order -- counts and the ks
    root-state column equal, dwell sums within the bar -- against the per-chain rows of the same engine without the reduction, and
    the segment counter once per sweep: the segments every sweep read and wrote, from the oracle's chain states"""
    case = NC.case_reduce(chains, variant)
    n, c = case.n, case.n + case.ncnt
    want = np.zeros_like(NC.oracle_state(case, 0, case.N).rows)
    segs = 0
    for r in range(case.S):                            # in chain order
        want = want + NC.oracle_state(case, r, case.N).rows
        segs += sum(int(NC.oracle_state(case, r, k).seg_count.sum()) + int(NC.oracle_state(case, r, k + 1).seg_count.sum()) for k in range(case.N))
    eng = _engine(case)
    try:
        eng.run(case.N); eng.sync()
        red = np.array(eng.stats(0, case.N))
        assert eng.info().seg_read == segs and eng.info().recoveries == 0
        _same_state(case, eng, case.N, chains=sorted({0, 63, case.S - 1}))
    finally:
        eng.close()
    eng = _engine(case, reduce=False)
    try:
        eng.run(1); eng.run(case.N - 1); eng.sync()
        per = np.array(eng.stats(0, case.N))
        assert eng.info().seg_read == segs
    finally:
        eng.close()
    assert red.shape == want.shape and per.shape == (case.S,) + want.shape
    np.testing.assert_array_equal(red[:, n:c], want[:, n:c])
    np.testing.assert_array_equal(red[:, n:c], per.sum(0)[:, n:c])
    np.testing.assert_allclose(red[:, :n], want[:, :n], rtol=1e-10, atol=0)
    np.testing.assert_allclose(red[:, :n], per.sum(0)[:, :n], rtol=1e-12, atol=0)
    np.testing.assert_allclose(red[:, :n].sum(1), case.S * case.length, rtol=1e-11)
    if case.ks:
        np.testing.assert_array_equal(red[:, -1], want[:, -1])             # root states, 0-based, summed over the chains
        np.testing.assert_array_equal(per[:, :, -1], np.stack([NC.oracle_state(case, r, case.N).rows[:, -1] for r in range(case.S)]))
