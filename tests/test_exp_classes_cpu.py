"""What the cases of tests/test_gpu_exp_classes.py reach in phm_exp.hip (tests/expclasses.py restates the host's formulas): items of
several branches with a short last one and a second trip of the persistent loop, every (NS, MODE) form of the branch kernel, jump
times beyond the LDS slots next to lanes within them, a branch of more than 200 jumps, the jump cap, and the workgroup shares of the
transition-matrix kernels.  The formulas are pinned to their values at the time of writing: if one of these tests fails after a
heuristic was retuned, move the shapes in expclasses.py until the properties asserted here hold again; do not relax them."""
import functools

import numpy as np
import pytest

import expclasses as xc
import mapsref
import oracle_lib as O
import pyref
from phylomap_amd import api, treeorder

SEED = 41


def orders(z):
    return treeorder.pruningwiseedgeorder(z), treeorder.makenodelist(z), treeorder.myreorder(z)


def oracle_exp(z, Q, pid, N, seed=SEED, rescale=False):
    """(out, rc) of the CPU oracle with the eigendecomposition api.sumstatEXP computes for itself"""
    nen, nodelist, root = orders(z)
    lefts, rights, d = api.eigen_decompose(Q)
    return O.maketreelistEXP(z, Q, pid, nen, nodelist, root, N, lefts, rights, d, seed=seed, rescale=rescale)


def twin_exp(z, Q, pid, N, seed=SEED, jumps=None):
    """(out [N, cols], (off, dwell, state)) of the Python twin; ``jumps``: a dict for the jumps of every (sample, edge row)"""
    nen, nodelist, root = orders(z)
    lefts, rights, d = api.eigen_decompose(Q)
    out, maps = mapsref.sumstatEXP(z, Q.tolist(), pid.tolist(), N, [int(v) for v in nen], [int(v) for v in nodelist], int(root),
                                   lefts.tolist(), rights.tolist(), np.diag(d).tolist(), seed, 0, jumps=jumps)
    return np.array(out), maps


@functools.lru_cache(maxsize=None)
def long_twin(n):
    z, Q, pid, heavy = xc.long_case(n)
    jumps = {}
    return twin_exp(z, Q, pid, xc.LONG_TWIN_N, jumps=jumps) + (jumps,)


def test_the_formulas_at_their_corners():
    a, b = xc.branch_launch(198, 82 * 64), xc.branch_launch(198, 83 * 64)
    assert a["group"] == 1 and b["group"] == 2                                 # 198 * 83 = 16 434 >= 16 384
    assert xc.branch_launch(198, 82 * 64 + 1)["group"] == 2 and xc.smallest_N(198, 2) == 82 * 64 + 1
    assert xc.branch_launch(198, 661 * 64)["group"] == 15 and xc.branch_launch(198, 662 * 64)["group"] == 16
    assert xc.branch_launch(198, 10 ** 7)["group"] == 16                       # the cap
    assert xc.branch_launch(78, 1)["waves"] == 80 and xc.branch_launch(198, 41 * 64)["waves"] == 8120
    c = xc.branch_launch(198, 42 * 64)                                         # 8 316 items on 8 192 waves, group still 1
    assert c["waves"] == 8192 and c["group"] == 1 and c["second_trip"] and c["second_items"] == 124
    assert not xc.branch_launch(198, 41 * 64)["second_trip"]
    assert xc.group_sizes(198, 16) == [16] * 12 + [6] and xc.group_sizes(78, 5) == [5] * 15 + [3] and xc.group_sizes(198, 2) == [2] * 99
    assert xc.tiles_of(1) == 1 and xc.tiles_of(64) == 1 and xc.tiles_of(65) == 2 and xc.tiles_of(257) == 5
    assert [xc.eigen_mpb(n) for n in (2, 3, 4, 5, 11, 15, 16, 17, 256)] == [64, 28, 16, 10, 2, 1, 1, 1, 1]
    assert xc.eigen_grid(3, 28) == 1 and xc.eigen_grid(3, 29) == 2 and xc.eigen_grid(3, 57) == 3 and xc.eigen_grid(65, 3) == 3
    assert xc.eigen_batches(3) == [1, 27, 28, 29, 57] and xc.eigen_batches(11) == [1, 2, 3, 5] and xc.eigen_batches(16) == [1, 3]
    assert xc.mfma_grid("eigen", 72) == 72 and xc.mfma_grid("eigen", 2053) == 2048
    assert xc.mfma_grid("pade", 43) == 43 and xc.mfma_grid("pade", 1030) == 1024
    assert xc.branch_form(2, False) == (2, (0,)) and xc.branch_form(4, True) == (4, (1, 2)) and xc.branch_form(5, False) == (0, (0,))
    assert xc.replica_form(3) == "exp_sample_kernel<3>" and xc.replica_form(5) == "exp_wide_kernel"
    assert xc.pade_squarings(np.array([[-1.0, 1.0], [1.0, -1.0]]), 0.6) == 0          # log2(1.2) = 0.53 * 2^-1
    assert xc.pade_squarings(np.array([[-1.0, 1.0], [1.0, -1.0]]), 0.5) == 1          # a norm of one: as no norm at all
    assert xc.pade_squarings(np.array([[-1.0, 1.0], [1.0, -1.0]]), 0.0) == 1          # frexp(0) has exponent 0
    assert xc.pade_squarings(np.array([[-1.0, 1.0], [1.0, -1.0]]), 2.0) == 3          # log2(4) = 2 = 0.5 * 2^2


def test_what_the_suite_reached_before():
    """the gap: every oracle-checked call had one branch per item and one item per wave"""
    assert xc.branch_launch(198, 1000)["group"] == 1 and not xc.branch_launch(198, 1000)["second_trip"]      # C1: 16 tiles
    for E, N in ((58, 200), (58, 150), (22, 150), (18, 130)):                  # test_exp_*_matches_oracle, test_exp_maps_against_twin
        a = xc.branch_launch(E, N)
        assert a["group"] == 1 and not a["second_trip"]
    assert xc.branch_launch(98, 20000)["group"] == 3                           # the tutorial's agreement in distribution only


@pytest.mark.parametrize("name", list(xc.GROUP_CASES))
def test_group_cases(name):
    n, tree, group, _ = xc.GROUP_CASES[name]
    z, Q, pid, N = xc.group_case(name)
    E = len(z["edge.length"])
    assert Q.shape == (n, n) and E == {"c1": 198, "t40": 78}[tree]
    a = xc.branch_launch(E, N)
    assert a["group"] == group and a["second_trip"]
    if name == "n2_pairs":
        assert a["tiles"] == 83 and a["sizes"] == [2] * 99 and not a["short_last"] and a["second_items"] == 25
    if name == "n3_pairs":
        assert a["tiles"] == 211 and a["sizes"] == [2] * 39 and a["second_items"] == 37
    if name in ("n4_fives", "n6_fives"):
        assert N == 525 * 64 + 1 and N % 64 == 1 and a["tiles"] == 526
        assert a["sizes"] == [5] * 15 + [3] and a["short_last"] and a["items"] == 16 * 526 and a["second_items"] == 224
    if name == "n2_cap":
        assert a["tiles"] == 662 and a["sizes"] == [16] * 12 + [6] and a["short_last"] and a["items"] == 13 * 662
    if name in xc.GROUP_MAPS_CASES:
        zm, _, _, Nm = xc.group_case(name, maps=True)
        b = xc.branch_launch(E, Nm)
        assert b["group"] == 2 and xc.branch_launch(E, Nm - 1)["group"] == 1 and Nm % 64 == 1
        assert xc.branch_launch(E, 64)["group"] == 1                           # what its first 64 samples are compared with


def test_every_form_and_both_mappings_have_a_case():
    forms = xc.covered_forms()
    assert sorted(forms) == [(ns, m) for ns in (0, 2, 3, 4) for m in (xc.MAPS_OFF, xc.MAPS_COUNT, xc.MAPS_WRITE)]
    assert {xc.replica_form(n) for n in xc.STATE_COUNTS + xc.LONG_STATES + (2, 4)} == {
        "exp_sample_kernel<2>", "exp_sample_kernel<3>", "exp_sample_kernel<4>", "exp_wide_kernel"}
    assert 64 in xc.STATE_COUNTS and any(21 <= n <= 60 for n in xc.STATE_COUNTS)
    assert set(xc.SAMPLE_COUNTS) == {1, 64, 65, 257} and xc.tiles_of(257) > xc.WAVES_PER_BLOCK


def test_with_edge_lengths_keeps_a_valid_tree():
    z, Q, pid, heavy = xc.long_case(3)
    edge = np.asarray(z["edge"])
    assert edge.shape == (14, 2) and edge[heavy, 1] <= 8
    rt = np.asarray(z["edge.length"]) * xc.rate_of(Q)
    np.testing.assert_allclose(sorted(rt), [0, 0.05, 0.3, 1, 2, 3, 6, 10, 12, 13, 16, 25, 40, 230], rtol=1e-14)
    zero = int(np.flatnonzero(z["edge.length"] == 0.0)[0])
    assert edge[zero, 1] > 8 and rt[heavy] == rt.max()                         # the zero-length edge is an internal one
    for r in range(14):
        assert np.sum(z["maps"][r]) == pytest.approx(z["edge.length"][r], rel=1e-15, abs=0) and len(z["maps"][r]) == 2
        assert z["mapnames"][r][-1] == (z["states"][edge[r, 1] - 1] if edge[r, 1] <= 8 else 1)
    assert xc.fx_exp(z) == 11 and xc.fx_exp({"edge.length": np.array([0.2, 0.3])}) == 1


@pytest.mark.parametrize("n", xc.LONG_STATES)
def test_long_branch_case(n):
    """lanes beyond the LDS slots next to lanes within them on one branch of one tile, and 200 real jumps on the heavy branch"""
    z, Q, pid, heavy = xc.long_case(n)
    want, rc = oracle_exp(z, Q, pid, xc.long_N(n))
    assert rc == 0
    out, (off, dwell, state), jumps = long_twin(n)
    np.testing.assert_array_equal(out[:, n:], want[:xc.LONG_TWIN_N, n:])         # the twin draws what the oracle draws
    segs = np.diff(off).reshape(xc.LONG_TWIN_N, 14)
    # segments - 1 <= jumps: 14 segments are more than EXP_KL jump times
    both = [b for b in range(14) if (segs[:, b] >= xc.EXP_KL + 2).any() and (segs[:, b] <= xc.EXP_KL).any()]
    assert both, segs.max(0)
    nj = np.array([[jumps[(it, b)] for b in range(14)] for it in range(xc.LONG_TWIN_N)])
    assert np.all(segs - 1 <= nj) and nj.max() <= xc.UNIF_CAP
    assert [b for b in range(14) if (nj[:, b] > xc.EXP_KL).any() and (nj[:, b] == xc.EXP_KL).any() and (nj[:, b] < xc.EXP_KL).any()]
    assert segs[:, heavy].max() - 1 >= xc.HEAVY_JUMPS, segs[:, heavy].max()
    assert np.all(segs[:, int(np.flatnonzero(z["edge.length"] == 0.0)[0])] == 1)


@pytest.mark.parametrize("n", xc.LONG_STATES)
def test_cap_case(n):
    z, Q, pid, heavy = xc.long_case(n, xc.CAP_RT)
    _, rc = oracle_exp(z, Q, pid, 64)
    assert rc == O.ERR_UNIF_CAP


@pytest.mark.parametrize("n", xc.LONG_STATES)
def test_brink_case(n):
    """one sample that draws exactly UNIF_CAP jumps on the heavy branch: legal, and the last row of the B^k e_j table"""
    z, Q, pid, heavy = xc.long_case(n, xc.BRINK_RT)
    want, rc = oracle_exp(z, Q, pid, 1, seed=xc.BRINK_SEED)
    assert rc == 0
    jumps = {}
    out, _ = twin_exp(z, Q, pid, 1, seed=xc.BRINK_SEED, jumps=jumps)
    assert jumps[(0, heavy)] == xc.UNIF_CAP and max(jumps.values()) == xc.UNIF_CAP
    np.testing.assert_array_equal(out[:, n:], want[:, n:])


def test_tie_case():
    """the root's weights are a few units of the smallest denormal, and some sample's u * total IS one of their running sums: the
    first state with thr <= cum and the first with thr < cum differ there"""
    z, Q, pid = xc.ladder_case()
    n = xc.TIE_STATES
    nen, nodelist, root = orders(z)
    lefts, rights, d = api.eigen_decompose(Q)
    out, rc, db = O.maketreelistEXP(z, Q, pid, nen, nodelist, root, xc.TIE_N, lefts, rights, d, seed=SEED, dump=True)
    assert rc == 0
    w = pid * db.PL[root - 1]
    unit = 2.0 ** -1074
    total = w[0]
    for x in w[1:]:
        total += x
    assert 8 * unit <= total <= 1000 * unit and np.count_nonzero(w) >= 3, w / unit
    cum = np.cumsum(w)                                                         # exact: small multiples of one unit
    rng = pyref.Rng(SEED, 0)
    ties = 0
    for it in range(xc.TIE_N):
        u = rng.u(it, pyref.ENT_NODE | (root - 1), 0)
        thr = u * total
        le = int(np.argmax(thr <= cum))
        lt = int(np.argmax(thr < cum)) if (thr < cum).any() else n - 1
        assert le == pyref.sample(w.tolist(), u)
        ties += le != lt
    assert ties >= 3, ties


@pytest.mark.parametrize("n", xc.EIGEN_STATES)
def test_eigen_cases_against_scipy(n):
    from scipy.linalg import expm
    Q = xc.model(n)
    lefts, rights, d = api.eigen_decompose(Q)
    assert n <= xc.EIGEN_N_MAX
    t = xc.eigen_times(n, 3)
    assert t[0] == 0.0 and t[1] == 1e-6 and xc.eigen_times(n, 1).size == 1 and xc.eigen_times(n, 1)[0] == t[2]
    for tb in t:
        np.testing.assert_allclose(O.matexp(lefts, rights, np.diag(d), tb), expm(Q * tb), rtol=0, atol=1e-10)


@pytest.mark.parametrize("n", xc.PADE_STATES)
def test_pade_cases_against_scipy(n):
    from scipy.linalg import expm
    Q = xc.pade_model(n)
    assert n <= xc.PADE_N_MAX
    t = xc.pade_times(Q)
    s = [xc.pade_squarings(Q, tb) for tb in t]
    assert min(s) == 0 and max(s) >= 6, s
    for tb in t:
        got, rc = O.expmat_pade(Q * tb)
        assert rc == 0
        np.testing.assert_allclose(got, expm(Q * tb), rtol=0, atol=1e-12)


@pytest.mark.parametrize("route", ["eigen", "pade"])
def test_matrix_core_batches(route):
    grid = xc.mfma_grid(route, xc.MFMA_BATCH[route])
    for n in xc.MFMA_STATES:
        t = xc.mfma_times(route, n)
        assert 16 < n <= 64 and t.size == xc.MFMA_BATCH[route] > grid and t.size < 2 * grid
        k = 3 if route == "pade" else 2
        assert np.array_equal(t[:k], t[grid:grid + k]) and t[0] == 0.0 and t[1] == 1e-6 and (route == "eigen" or t[2] == 200.0)
