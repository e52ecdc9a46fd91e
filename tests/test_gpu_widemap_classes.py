"""The replica mapping (phm_wide.hip) and the branch mapping (phm_wbranch.hip) of the 5 to 64 state sweep on the paths that only
a shape reaches (tests/widemapclasses.py; tests/test_widemap_classes_cpu.py pins every case to its path): several replicas taking
turns in one wave, the state counts and LDS sizes at the edges, ELLPACK rows either side of their rule, chain matrices the SPARSE
threshold really changes, the windows of the branch kernel, the tree passes without transition maps and without the LDS copy of
the node states, and the segment limit of the replica mapping.  The bar is test_gpu_parity._same: the replica mapping bit for bit
against the oracle; the branch mapping counts exact, dwell sums within 1e-10, derived columns within 1e-9; every dwell row adds
up to the tree length within 1e-11; the reduced output against the sum of the rows, counts exact and dwell within 1e-12.

Measured on an MI355X (docs/MEASUREMENTS.md, "Replica and branch mappings by class"): see there for the wall time of every test."""
import numpy as np
import pytest

import widemapclasses as C
from phylomap_amd import _lib
from test_gpu_configs import _check_dump
from test_gpu_parity import _same

pytestmark = pytest.mark.gpu


def _run(case, dump=None, S=None, mapping=None, seg_cap=512, **opt):
    """(statistics, chain state of replica ``dump`` or None) of one engine run"""
    eng = case.engine(S=S, mapping=mapping, **opt)
    try:
        eng.run(case.N); eng.sync()
        return eng.stats(0, case.N), (eng.dump(dump, seg_cap=seg_cap) if dump is not None else None)
    finally:
        eng.close()


def _report(case, got, want, mapping):
    """the largest relative dwell error of a compared row, printed before anything is asserted (the branch mapping's figure of
    docs/MEASUREMENTS.md)"""
    if mapping != "replicas":
        n = case.n
        err = float(np.max(np.abs(got[..., :n] - want[..., :n]) / np.where(want[..., :n] != 0, np.abs(want[..., :n]), 1.0)))
        print(f"dwell_error {case.name} {mapping} {err:.3e} = {err / 1e-10:.2e} of the bar")


def _against_oracle(case, got, mapping=None, replicas=None, sites=None):
    mapping = case.mapping if mapping is None else mapping
    for r in (case.replicas if replicas is None else replicas):
        want, rc = C.oracle_rows(case, r) if sites is None else C.oracle_rows_on(case, r, np.ascontiguousarray(sites[r]).tobytes())
        assert rc == 0
        _report(case, got[r], want, mapping)
        _same(got[r], want, case.n, mapping, ks=case.ks)
    np.testing.assert_allclose(got[:, :, :case.n].sum(2), case.length, rtol=1e-11)      # every replica, every sweep


def _chain_state(case, d, replica):
    rc, dump = C.oracle_dump(case, replica)
    assert rc == 0
    if case.ks:                                               # Engine.dump shows the observed tips, the oracle the re-drawn ones
        T = case.T
        d = dict(d, node_states=np.concatenate([dump.node_states[:T], d["node_states"][T:]]), PL=np.concatenate([dump.PL[:T], d["PL"][T:]]))
    _check_dump(d, dump)


def _reduced_is_the_sum(case, red, per):
    """counts exact, dwell sums within 1e-12.  The sum of up to 262 145 rows is formed in extended precision: numpy adds the rows
    of the replica axis one after the other, and in double precision that reference alone drifts by some 1e-12 at this count."""
    n, c = case.n, case.n + case.ncnt
    assert red.shape == per.shape[1:]
    np.testing.assert_array_equal(red[:, n:c], per[:, :, n:c].sum(0))
    tot = per[:, :, :n].astype(np.longdouble).sum(0).astype(np.float64)
    print(f"reduced_error {case.name} {float(np.max(np.abs(red[:, :n] - tot) / tot)):.3e}")
    np.testing.assert_allclose(red[:, :n], tot, rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------------------------------------
# A. several replicas in a wave of the replica mapping
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", C.MULTI_S)
@pytest.mark.parametrize("n", C.MULTI_NS)
def test_replicas_taking_turns_in_a_wave(n, S):
    """8 193 to 262 145 replicas on an 8-tip tree: 2, 4, 32 and 64 replicas share a wave, and the last tile holds one.  Replicas
    {0, 1, stride - 1, stride, a middle one, S - 2, S - 1} bit for bit against the oracle, every replica against the tiles mapping"""
    case = C.multi_case(n, S)
    eng = case.engine()
    try:
        padded = eng.info().n_replicas_padded
        assert padded == 64 * C.ceil_div(S, C.rep_stride(S)), (
            f"{padded // 64} tiles for {S} replicas, not the {C.ceil_div(S, C.rep_stride(S))} of stride {C.rep_stride(S)}: the host puts more replicas on a "
            "tile when the padded layout would take over a quarter of the FREE device memory (replicas_setup) -- on a card that other "
            "work has filled this says nothing about the kernel")
        eng.run(case.N); eng.sync()
        got = eng.stats(0, case.N)
    finally:
        eng.close()
    _against_oracle(case, got)
    tiles, _ = _run(case, mapping="tiles")
    _report(case, got, tiles, "tiles")
    _same(got, tiles, n, "branches")


@pytest.mark.parametrize("S", C.MULTI_S_EXTRA)
@pytest.mark.parametrize("n", C.MULTI_NS)
def test_replicas_taking_turns_with_tips_of_their_own_summed_and_dumped(n, S):
    """the same with per-replica tip states (each compared replica against the oracle on its own tips), with the statistics
    summed over replicas by atomics from several lanes, and the chain state of a replica that is not lane 0 of its tile"""
    case = C.multi_case(n, S)
    sites = C.multi_sites(case)
    got, _ = _run(case, tips_per_replica=True, states=sites)
    _against_oracle(case, got, sites=sites)
    per, d = _run(case, dump=C.middle_replica(S))
    _chain_state(case, d, C.middle_replica(S))
    red, _ = _run(case, reduce=True)
    _reduced_is_the_sum(case, red, per)


@pytest.mark.parametrize("S", C.MULTI_S_EXTRA)
def test_replicas_taking_turns_in_the_ks_layout(S):
    """hidden-rates Q at 8 states, parity tips: the tip draws against the parity mask and the n x n counters with r > 0"""
    case = C.multi_case(8, S, ks=True)
    got, d = _run(case, dump=C.middle_replica(S))
    _against_oracle(case, got)
    _chain_state(case, d, C.middle_replica(S))


def test_list_engine_with_several_replicas_of_a_tree_in_one_tile():
    """three trees, five replicas each, 12 states: a tile per tree with five live lanes (stride 64), Philox replica word
    64 j + c -- the multi-tree drivers themselves return one row per iteration and take no replica count, so the engine over the
    list is asked directly"""
    import oracle_lib as O
    import wtilesclasses as W
    Q, pid, Omega, trees = C.list_problem()
    n, S, N = C.LIST_N, C.LIST_S, C.LIST_SWEEPS
    eng = _lib.Engine(trees, Q, pid, Omega, N, variant=_lib.PHM_MCMC_BIGTREE, seed=5, n_replicas=S, mapping="replicas")
    try:
        eng.run(N); eng.sync()
        got = eng.stats(0, N)
        assert got.shape == (len(trees) * S, N, n * n)
        for j, z in enumerate(trees):
            nen, nodelist, root = W.orders(z)
            for c in range(S):
                want, rc, dump = O.maketreelistMCMC(z, Q, pid, np.eye(n) + Q / Omega, Omega, nen, nodelist, root, N, variant=O.BIGTREE, seed=5,
                                                    replica=64 * j + c, dump=True)
                assert rc == 0
                np.testing.assert_array_equal(got[j * S + c], want)
                if c in (1, S - 1):
                    _check_dump(eng.dump(j * S + c), dump)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------------
# B. state-count and LDS edges
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.edge_cases(), ids=[c.name for c in C.edge_cases()])
def test_state_count_and_lds_edges(case):
    """dense rows at 5 | 44 | 45 | 63 | 64 states, and the SPARSE driver with two LDS copies of B at 31 | 32 | 55 | 56 | 64: the
    replica mapping crosses 64 KiB of dynamic LDS at 45 (32 SPARSE), the pruning kernels of the branch mapping 48 KiB at 56 SPARSE"""
    got, d = _run(case, dump=case.S - 1)
    _against_oracle(case, got)
    _chain_state(case, d, case.S - 1)


# ---------------------------------------------------------------------------------------------------------------------------
# C. the ELLPACK rule, and chain matrices the threshold changes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,w", C.ELL_PAIRS)
@pytest.mark.parametrize("mapping", ["branches", "replicas"])
def test_ellpack_rows_either_side_of_the_rule(mapping, n, w):
    """unbanded rows of w non-zeros: ELLPACK at (6, 2), (12, 4), (48, 16), (64, 16), dense at (5, 2), (11, 4), (47, 16), (64, 17)"""
    case = C.ell_case(n, w, mapping)
    got, d = _run(case, dump=1)
    _against_oracle(case, got)
    _chain_state(case, d, 1)


def test_band_of_two_with_shifts_and_with_ellpack_rows():
    """16 states, half-bandwidth 2: sparse_chains = 2 switches the wave shifts off and leaves the ELLPACK rows -- the same bits"""
    case = C.band16_case()
    got, d = _run(case, dump=1)
    _against_oracle(case, got)
    _chain_state(case, d, 1)
    got2, d2 = _run(case, dump=1, sparse_chains=2)
    np.testing.assert_array_equal(got2, got)
    for k in ("seg_count", "node_states", "PL", "seg_dwell"):
        np.testing.assert_array_equal(d2[k], d[k])


@pytest.mark.parametrize("rescale", [False, True], ids=["unscaled", "rescaled"])
@pytest.mark.parametrize("model", C.THRESHOLD_MODELS)
@pytest.mark.parametrize("mapping", ["branches", "replicas"])
def test_sparse_driver_with_a_chain_matrix_the_threshold_changes(mapping, model, rescale):
    """Bc != B2: ELLPACK pruning under forward rows of another width or dense ones (branches), two different LDS matrices
    (replicas); with the reference's unscaled pruning and rescaled"""
    case = C.threshold_case(model, rescale, mapping)
    got, d = _run(case, dump=1)
    _against_oracle(case, got)
    _chain_state(case, d, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# D. the windows of wb_branch_kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.window_cases(), ids=[c.name for c in C.window_cases()])
def test_branch_kernel_windows(case):
    """branches of 192, 193 and 400 initial segments and 330 expected jumps: merged segments beyond the 192 kept in LDS, several
    flushes of 64 noted transitions and several refills of 64 variates on one branch, in every sweep"""
    got, d = _run(case, dump=1)
    _against_oracle(case, got)
    _chain_state(case, d, 1)


def test_branch_kernel_windows_with_the_forward_matrix_in_global_memory():
    """the 20-state case at 1 490 replicas: S E = 32 780 waves, B2 is read from global memory"""
    case = C.window_case("bigtree", 20, C.WINDOW_BIG_S)
    got, _ = _run(case)
    _against_oracle(case, got)
    tiles, _ = _run(case, mapping="tiles")
    _report(case, got, tiles, "tiles")
    _same(got, tiles, case.n, "branches")


# ---------------------------------------------------------------------------------------------------------------------------
# E. the tree-pass fallbacks of the branch mapping
# ---------------------------------------------------------------------------------------------------------------------------
def test_level_launches_beyond_256_mib_of_transition_maps():
    """64 states, 600 tips, 3 502 replicas: S E n = 268 505 344 > 2^28 -- wb_root_kernel and a wb_down_kernel launch per level"""
    case = C.levels_case()
    assert not C.uses_dmap(case.S, case.E, case.n) and case.E == 2 * C.LEVELS_TIPS - 2
    got, _ = _run(case)
    _against_oracle(case, got)
    tiles, _ = _run(case, mapping="tiles")
    _report(case, got, tiles, "tiles")
    _same(got, tiles, case.n, "branches")


def test_walk_without_the_lds_copy_of_the_node_states():
    """one chain at 5 states on 61 442 tips: 61 441 internal nodes, one beyond the 61 440 the walk keeps in LDS (62 000 tips took
    3.0 s beside the 2.8 s of the 70 000-tip test at 4 states, so the tree is the smallest that crosses)"""
    case = C.walk_case()
    assert not C.walk_uses_lds(case.T - 1) and C.uses_dmap(1, case.E, case.n)
    got, _ = _run(case)
    want, rc = C.oracle_rows(case, 0)
    assert rc == 0
    _report(case, got[0], want, "branches")
    _same(got[0], want, case.n, "branches")
    np.testing.assert_allclose(got[0][:, :case.n].sum(1), case.length, rtol=1e-11)


# ---------------------------------------------------------------------------------------------------------------------------
# F. the segment limit of the replica mapping
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.LIMIT_NS)
def test_segment_limit_of_the_replica_mapping(n):
    """exactly wide_maxseg(n) initial segments on a branch: accepted, the first sweep is the oracle's; one more: refused; a chain
    that outgrows the limit while it runs: the capacity status (the kernel clamps and stays in bounds)"""
    case = C.limit_case(n, 0)
    got, d = _run(case, dump=2)
    _against_oracle(case, got)
    _chain_state(case, d, 2)
    with pytest.raises(_lib.PhmError) as e:
        C.limit_case(n, 1).engine()
    assert e.value.status == C.ST_UNSUPPORTED
    grow = C.outgrow_case(n)
    with pytest.raises(_lib.PhmError) as e:
        eng = grow.engine()
        try:
            eng.run(grow.N); eng.sync()
        finally:
            eng.close()
    assert e.value.status == C.ST_CAPACITY
