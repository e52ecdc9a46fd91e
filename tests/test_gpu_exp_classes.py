"""The matrix-exponential path (phm_exp.hip) at every class edge: the sumstatEXP sampler in both mappings at the state counts,
sample counts, branch groups and branch lengths where it takes another path, and the four transition-matrix kernels at the edges of
their workgroup shares.  tests/test_exp_classes_cpu.py asserts what each case below reaches (tests/expclasses.py).

The bars are the project's: counts bit for bit in both mappings; dwell columns bit for bit with the oracle in the replicas mapping
and to rtol = 1e-10 in the tiles mapping, plus, per sample, segments * 2^(fx_exp - 62): the tiles mapping rounds every segment to
the nearest multiple of 2^(fx_exp - 61) before its exact fixed-point sum (exp_prepare; a sample has jumps + edges segments), and
the cases here put thousands of segments into one sum.  Per sample the dwell columns add up to the tree length to 1e-12."""
import functools

import numpy as np
import pytest

import expclasses as xc
import oracle_lib as O
from phylomap_amd import _lib, api
from test_exp_classes_cpu import SEED, oracle_exp, twin_exp

pytestmark = pytest.mark.gpu

MAPPINGS = ["replicas", "tiles"]      # one wave per tile of 64 samples walks the tree / one wave per (tile, group of branches)


def same(got, want, z, n, mapping):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got[:, n:], want[:, n:])
    if mapping == "replicas":
        np.testing.assert_array_equal(got[:, :n], want[:, :n])
    else:
        bound = 1e-10 * np.abs(want[:, :n]) + xc.tiles_atol(want, z, n)[:, None]
        err = np.abs(got[:, :n] - want[:, :n])
        assert np.all(err <= bound), (err.max(), np.argwhere(err > bound)[:3])
    np.testing.assert_allclose(got[:, :n].sum(1), np.sum(z["edge.length"]), rtol=1e-12, atol=0)


def same_maps(m, want):
    off, dwell, state = want
    assert np.array_equal(m.off, off) and np.array_equal(m.state, state) and np.array_equal(m.dwell, dwell)


def stats_of_maps(m, n):
    """(dwell sums per state [N, n], transition counts [N, n (n - 1)]) rebuilt from the segments"""
    N, E = m.n_hist, m.n_edge
    row = np.repeat(np.arange(N * E), np.diff(m.off))
    dw = np.zeros((N, n))
    np.add.at(dw, (row // E, m.state.astype(np.int64) - 1), m.dwell)
    pair = row[:-1] == row[1:]
    a, b = m.state[:-1][pair].astype(np.int64) - 1, m.state[1:][pair].astype(np.int64) - 1
    assert np.all(a != b)
    ct = np.zeros((N, n * (n - 1)))
    np.add.at(ct, (row[:-1][pair] // E, a * (n - 1) + np.where(b > a, b - 1, b)), 1.0)
    return dw, ct


@functools.lru_cache(maxsize=None)
def state_oracle(n, rescale):
    z, Q, pid = xc.state_case(n)
    want, rc = oracle_exp(z, Q, pid, xc.STATE_N, rescale=rescale)
    assert rc == 0
    return want


# ---- 1. state counts --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("mapping", MAPPINGS)
@pytest.mark.parametrize("n", xc.STATE_COUNTS)
def test_state_counts(n, mapping, rescale):
    """exp_sample_kernel<3> and NS = 3; the run-time forms at 6, 33 and 64 states (a full wave of rows in exp_pl_nodes_kernel)"""
    z, Q, pid = xc.state_case(n)
    got = api.sumstatEXP(z, Q, pid, xc.STATE_N, seed=SEED, mapping=mapping, rescale=rescale)
    same(got, state_oracle(n, rescale), z, n, mapping)


# ---- 2. sample counts -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sample_oracle(n):
    z, Q, pid = xc.state_case(n)
    want, rc = oracle_exp(z, Q, pid, max(xc.SAMPLE_COUNTS))
    assert rc == 0
    return want


@pytest.mark.parametrize("mapping", MAPPINGS)
@pytest.mark.parametrize("N", xc.SAMPLE_COUNTS)
@pytest.mark.parametrize("n", xc.SAMPLE_STATES)
def test_sample_counts(n, N, mapping):
    """one sample, exactly one tile, one lane into a second tile, a second workgroup; samples are addressed by their index, so the
    oracle's first N rows are the N-sample call"""
    z, Q, pid = xc.state_case(n)
    got = api.sumstatEXP(z, Q, pid, N, seed=SEED, mapping=mapping)
    same(got, sample_oracle(n)[:N], z, n, mapping)


@pytest.mark.parametrize("N", xc.SAMPLE_MAPS_N)
@pytest.mark.parametrize("n", xc.SAMPLE_STATES)
def test_sample_counts_with_maps(n, N):
    z, Q, pid = xc.state_case(n)
    out, m = api.sumstatEXP(z, Q, pid, N, maps=True, seed=SEED)
    want, wm = twin_exp(z, Q, pid, N)
    same_maps(m, wm)
    same(out, sample_oracle(n)[:N], z, n, "tiles")
    np.testing.assert_array_equal(out[:, n:], want[:, n:])
    np.testing.assert_array_equal(out, api.sumstatEXP(z, Q, pid, N, seed=SEED))


# ---- 3. branch groups -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(xc.GROUP_CASES))
def test_branch_groups(name):
    """items of 2, 5 and 16 branches, a short last item, waves on a second item: against the oracle over all N, and the replicas
    mapping (no groups) against the oracle bit for bit"""
    z, Q, pid, N = xc.group_case(name)
    n = Q.shape[0]
    want, rc = oracle_exp(z, Q, pid, N)
    assert rc == 0
    same(api.sumstatEXP(z, Q, pid, N, seed=SEED, mapping="tiles"), want, z, n, "tiles")
    same(api.sumstatEXP(z, Q, pid, N, seed=SEED, mapping="replicas"), want, z, n, "replicas")


# ---- 4. branch groups with maps ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", xc.GROUP_MAPS_CASES)
def test_branch_groups_with_maps(name):
    """the map cursor per branch inside an item, in the sizing and in the filling form"""
    z, Q, pid, N = xc.group_case(name, maps=True)
    n, E = Q.shape[0], len(z["edge.length"])
    out, m = api.sumstatEXP(z, Q, pid, N, maps=True, seed=SEED)
    np.testing.assert_array_equal(out, api.sumstatEXP(z, Q, pid, N, seed=SEED))
    want, rc = oracle_exp(z, Q, pid, N)
    assert rc == 0
    same(out, want, z, n, "tiles")
    dw, ct = stats_of_maps(m, n)
    np.testing.assert_array_equal(ct, out[:, n:])
    assert np.array_equal(np.diff(m.off).reshape(N, E).sum(1), out[:, n:].sum(1) + E)
    bound = 1e-10 * np.abs(out[:, :n]) + xc.tiles_atol(out, z, n)[:, None]
    assert np.all(np.abs(dw - out[:, :n]) <= bound)
    # samples are addressed by their index: the first 64 are the 64-sample call, one branch per item, which the twin checks
    out64, m64 = api.sumstatEXP(z, Q, pid, 64, maps=True, seed=SEED)
    k = int(m.off[64 * E])
    assert np.array_equal(m.off[:64 * E + 1], m64.off) and np.array_equal(m.dwell[:k], m64.dwell) and np.array_equal(m.state[:k], m64.state)
    np.testing.assert_array_equal(out[:64], out64)
    twin_out, wm = twin_exp(z, Q, pid, 64)
    same_maps(m64, wm)
    np.testing.assert_array_equal(out64[:, n:], twin_out[:, n:])


# ---- 5. long branches -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mapping", MAPPINGS)
@pytest.mark.parametrize("n", xc.LONG_STATES)
def test_long_branches(n, mapping):
    """rate * t from 0 to 230 on 14 edges: jump times in LDS and in the scratch rows lane by lane, the upper rows of the B^k e_j
    table, scratch rows up to the cap"""
    z, Q, pid, heavy = xc.long_case(n)
    N = xc.long_N(n)
    want, rc = oracle_exp(z, Q, pid, N)
    assert rc == 0
    assert want[:, n:].sum(1).max() >= xc.HEAVY_JUMPS
    same(api.sumstatEXP(z, Q, pid, N, seed=SEED, mapping=mapping), want, z, n, mapping)


@pytest.mark.parametrize("n", xc.LONG_STATES)
def test_long_branches_with_maps(n):
    z, Q, pid, heavy = xc.long_case(n)
    N = xc.LONG_TWIN_N
    out, m = api.sumstatEXP(z, Q, pid, N, maps=True, seed=SEED)
    want, wm = twin_exp(z, Q, pid, N)
    same_maps(m, wm)
    np.testing.assert_array_equal(out[:, n:], want[:, n:])
    np.testing.assert_array_equal(out, api.sumstatEXP(z, Q, pid, N, seed=SEED))
    assert np.diff(m.off).reshape(N, 14)[:, heavy].max() - 1 >= xc.HEAVY_JUMPS


# ---- 6. the cap -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", xc.LONG_STATES)
def test_the_jump_cap_is_an_error_and_not_sticky(n):
    """rate * t = 400 on one branch: every sample runs into the 300-jump cap there, as in the oracle; the next call is clean"""
    z, Q, pid, heavy = xc.long_case(n, xc.CAP_RT)
    _, rc = oracle_exp(z, Q, pid, 64)
    assert rc == O.ERR_UNIF_CAP
    for kw in (dict(mapping="replicas"), dict(mapping="tiles"), dict(maps=True)):
        with pytest.raises(_lib.PhmError, match="PHM_ERR_UNIF_CAP"):
            api.sumstatEXP(z, Q, pid, 64, seed=SEED, **kw)
        zs, Qs, pids = xc.state_case(n)
        got = api.sumstatEXP(zs, Qs, pids, xc.STATE_N, seed=SEED, mapping=kw.get("mapping", "tiles"))
        same(got, state_oracle(n, False), zs, n, kw.get("mapping", "tiles"))


@pytest.mark.parametrize("n", xc.LONG_STATES)
def test_exactly_the_cap_is_legal(n):
    """one sample whose heavy branch takes exactly 300 jumps: no error, the oracle's row, the twin's map"""
    z, Q, pid, heavy = xc.long_case(n, xc.BRINK_RT)
    want, rc = oracle_exp(z, Q, pid, 1, seed=xc.BRINK_SEED)
    assert rc == 0
    for mapping in MAPPINGS:
        same(api.sumstatEXP(z, Q, pid, 1, seed=xc.BRINK_SEED, mapping=mapping), want, z, n, mapping)
    out, m = api.sumstatEXP(z, Q, pid, 1, maps=True, seed=xc.BRINK_SEED)
    same_maps(m, twin_exp(z, Q, pid, 1, seed=xc.BRINK_SEED)[1])
    same(out, want, z, n, "tiles")


@pytest.mark.parametrize("mapping", MAPPINGS)
def test_node_draw_on_the_boundary_of_its_running_sum(mapping):
    """a 600-tip ladder whose unscaled pruning pass ends in denormal weights at the root: u * total equals a running sum in one
    sample of ten, and the draw takes the first state with thr <= cum as the oracle does"""
    z, Q, pid = xc.ladder_case()
    want, rc = oracle_exp(z, Q, pid, xc.TIE_N)
    assert rc == 0
    same(api.sumstatEXP(z, Q, pid, xc.TIE_N, seed=SEED, mapping=mapping), want, z, xc.TIE_STATES, mapping)


# ---- 7. the exact transition-matrix kernels ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", xc.EIGEN_STATES)
def test_expm_eigen_workgroup_shares(n):
    """mpb = 256 / n^2 matrices per workgroup: batches on either side of one and of two workgroups' shares, up to 256 states"""
    Q = xc.model(n)
    lefts, rights, d = api.eigen_decompose(Q)
    dv = np.diag(d)
    for n_t in xc.eigen_batches(n):
        t = xc.eigen_times(n, n_t)
        P, _ = api.expm_eigen(lefts, rights, d, t)
        assert P.shape == (n_t, n, n)
        for b in range(n_t):
            np.testing.assert_array_equal(P[b], O.matexp(lefts, rights, dv, t[b]))


@pytest.mark.parametrize("n", xc.PADE_STATES)
def test_expm_pade_up_to_128_states(n):
    Q = xc.pade_model(n)
    t = xc.pade_times(Q)
    P, _ = api.expm_pade(Q, t)
    for b in range(t.size):
        want, rc = O.expmat_pade(Q * t[b])
        assert rc == 0
        np.testing.assert_array_equal(P[b], want)


def test_expm_refusals():
    for n, call in ((xc.EIGEN_N_MAX + 1, lambda I: api.expm_eigen(I, I, -I, [1.0])), (xc.PADE_N_MAX + 1, lambda I: api.expm_pade(-I, [1.0]))):
        with pytest.raises(_lib.PhmError, match="PHM_ERR_BAD_INPUT"):
            call(np.eye(n))


# ---- 8. the matrix-core kernels: a second matrix per workgroup --------------------------------------------------------------------

@pytest.mark.parametrize("n", xc.MFMA_STATES)
def test_expm_eigen_on_matrix_cores_second_matrix(n):
    Q = xc.model(n)
    lefts, rights, d = api.eigen_decompose(Q)
    t = xc.mfma_times("eigen", n)
    grid = xc.mfma_grid("eigen", t.size)
    P, _ = api.expm_eigen(lefts, rights, d, t, mfma=True)
    exact, _ = api.expm_eigen(lefts, rights, d, t)
    np.testing.assert_allclose(P, exact, rtol=0, atol=1e-13)
    for b0 in (grid, t.size - 3):                              # as a workgroup's first matrix
        first, _ = api.expm_eigen(lefts, rights, d, t[b0:b0 + 3], mfma=True)
        np.testing.assert_array_equal(P[b0:b0 + 3], first)
    for b in (0, 1, grid - 1, grid, grid + 1, t.size - 1):
        np.testing.assert_array_equal(P[b], O.matexp_fma(lefts, rights, np.diag(d), t[b]))


@pytest.mark.parametrize("n", xc.MFMA_STATES)
def test_expm_pade_on_matrix_cores_second_matrix(n):
    Q = xc.pade_model(n)
    t = xc.mfma_times("pade", n)
    grid = xc.mfma_grid("pade", t.size)
    P, _ = api.expm_pade(Q, t, mfma=True)
    exact, _ = api.expm_pade(Q, t)
    np.testing.assert_allclose(P, exact, rtol=0, atol=2e-13)
    for b0 in (grid, t.size - 3):
        first, _ = api.expm_pade(Q, t[b0:b0 + 3], mfma=True)
        np.testing.assert_array_equal(P[b0:b0 + 3], first)
    np.testing.assert_array_equal(P[grid:grid + 3], P[:3])     # the same three times as first matrices of this very launch
