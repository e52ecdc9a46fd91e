"""Per-branch expectations under many rate matrices on the device (phm_expected_branch_stats_models): full
rows against the Python twin (``exactref.expected(per_branch=True)`` per model) at every register class and lane-group width; the
rows added in run order against ``api.expected_sumstat_models``' totals BIT FOR BIT (what holds the new branch stage to the
existing arithmetic); an edge selection out of order with a repeat; a model's independence from the other lanes of its wave;
chunks and devices; labelled sums against the column loop over the full rows bit for bit; impossible, still and long-branch
models; and the one-model call."""
import functools

import numpy as np
import pytest

import branchrowscases as bc
import stateclasses
from phylomap_amd import _lib, api, ratemodel

pytestmark = pytest.mark.gpu
SW_M_CAP = 63                                                                 # phm_scores_wide_form.h


@pytest.fixture(scope="module", autouse=True)
def one_blas_thread():
    """the twin multiplies n x n matrices thousands of times: a BLAS thread pool only gets in its way"""
    try:
        import threadpoolctl
    except ImportError:
        yield
        return
    with threadpoolctl.threadpool_limits(limits=1):
        yield


def terms(x, cap=1 << 21):
    """section 18's stopping rule restated (tests/test_scores_wide_cpu.py pins the header's function to this text)"""
    r, S = x, 1.0 + x
    for m in range(cap + 1):
        rn = r * (x / (m + 2))
        if x < m + 2 and rn <= 2.0 ** -60 * S * (1.0 - x / (m + 3)):
            return m
        r = rn
        S += r
        if r > 2.0 ** 512:
            r *= 2.0 ** -512
            S *= 2.0 ** -512
    return cap + 1


def _bar(what, got, want, ll_got, ll_want, length):
    """the project's per-branch bar (tests/test_gpu_expected.py): |error| <= 1e-12 |want| + 1e-14 x tree length, loglik <= 1e-12
    max(1, |l|); an evaluation the reference finds impossible is -inf with NaN rows.  Prints the worst error over its allowance."""
    assert got.shape == want.shape and ll_got.shape == ll_want.shape, (got.shape, want.shape)
    ok = np.isfinite(ll_want)
    assert np.array_equal(np.isfinite(ll_got), ok)
    assert np.all(ll_got[~ok] == -np.inf) and np.all(np.isnan(got[~ok]))
    le = np.abs(ll_got[ok] - ll_want[ok]) / (1e-12 * np.maximum(1.0, np.abs(ll_want[ok])))
    err = np.abs(got[ok] - want[ok])
    allow = 1e-12 * np.abs(want[ok]) + 1e-14 * length
    print(f"{what}: error / allowance: per branch {np.max(err / allow) if err.size else 0.0:.3g}, loglik {np.max(le) if le.size else 0.0:.3g}")
    assert np.all(le <= 1.0), le.max()
    assert np.all(err <= allow), (err.max(), np.max(err / allow))


def _same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])


@functools.lru_cache(maxsize=None)
def _problem(n, tree="40"):
    """(z, Qs, pid [K, n], tips [3, T], observe, twin branch [K, 3, E, C], twin loglik [K, 3]) of a state count, computed once
    and never changed: K = 70 at n <= 8 (a full wave and a ragged one; smaller batches are its first models), K = 2 above;
    parity observe at 4, 8, 16 and 61 states; the twin is asked for the 40-tip tree alone"""
    z = bc.tree40() if tree == "40" else bc.tree6()
    T = int(z["Nnode"]) + 1
    K = 70 if n <= 8 else 2
    Qs, pid = bc.models(n, K)
    observe = bc.parity(n) if n in (4, 8, 16, 61) else None
    tips = bc.sites(n, T, 3, observe)
    want = bc.twin(z, Qs, pid, tips, observe) if tree == "40" else (None, None)
    for a in (Qs, pid, tips) + tuple(w for w in want if w is not None):
        a.setflags(write=False)
    return z, Qs, pid, tips, observe, want[0], want[1]


# ---- 1. against the twin ----
NARROW = [(n, K) for n in (2, 3, 4, 5, 8) for K in (1, 63, 64, 70)]
WIDE = [(n, 2) for n in (9, 16, 17, 33, 61)]


@pytest.mark.parametrize("n,K", NARROW + WIDE)
def test_full_rows_against_the_twin(n, K):
    """cross with S = 3 and per-model pid, cross with S = 1 and a shared pid, paired"""
    z, Qs, pid, tips, observe, want, ll_want = _problem(n)
    length = float(np.sum(z["edge.length"]))
    E, C = z["edge"].shape[0], n * n
    br, ll = api.expected_branch_stats_models(z, Qs[:K], pid[:K], sites=tips, observe=observe)
    assert br.shape == (K, 3, E, C) and ll.shape == (K, 3)
    _bar(f"n={n} K={K} S=3 cross", br, want[:K], ll, ll_want[:K], length)
    ok = np.isfinite(ll)
    np.testing.assert_allclose(br[ok][:, :, :n].sum(axis=2), np.broadcast_to(z["edge.length"], (int(ok.sum()), E)), rtol=1e-12, atol=1e-14 * length)
    assert np.all(br[ok][:, bc.ZERO_EDGE] == 0.0)                              # the zero-length branch: a row of exact zeros
    zero = np.array([[Qs[k, i, j] == 0.0 for i in range(n) for j in range(n) if i != j] for k in range(K)])
    counts = br[..., n:]                                                      # a structurally zero q_ij: E[N_ij] = 0 exactly
    assert np.all(counts[np.broadcast_to(zero[:, None, None, :], counts.shape) & ok[..., None, None]] == 0.0)
    # one site, the first model's pid shared by all: pid enters through the root alone, so the twin is asked again for K <= 2
    br1, ll1 = api.expected_branch_stats_models(z, Qs[:K], pid[0], sites=tips[1:2], observe=observe)
    assert br1.shape == (K, 1, E, C) and ll1.shape == (K, 1)
    assert np.array_equal(br1[0, 0], br[0, 1], equal_nan=True) and ll1[0, 0] == ll[0, 1]
    if K <= 2:
        w1, wl1 = bc.twin(z, Qs[:K], pid[0], tips[1:2], observe)
        _bar(f"n={n} K={K} S=1 shared pid", br1, w1, ll1, wl1, length)
    som = bc.owner(K, 3)
    brp, llp = api.expected_branch_stats_models(z, Qs[:K], pid[:K], sites=tips, observe=observe, site_of_model=som)
    assert brp.shape == (K, E, C) and llp.shape == (K,)
    ks = np.arange(K)
    _bar(f"n={n} K={K} paired", brp, want[ks, som], llp, ll_want[ks, som], length)
    assert np.array_equal(brp, br[ks, som], equal_nan=True) and np.array_equal(llp, ll[ks, som])


# ---- 2. totals bit for bit ----
@pytest.mark.parametrize("tree", ["40", "6"])
@pytest.mark.parametrize("n", [4, 8, 20, 61])
def test_rows_in_run_order_are_the_totals_bit_for_bit(n, tree):
    z, Qs, pid, tips, observe, _, _ = _problem(n, tree)
    K = min(len(Qs), 5)
    br, ll = api.expected_branch_stats_models(z, Qs[:K], pid[:K], sites=tips, observe=observe)
    st, ll_tot = api.expected_sumstat_models(z, Qs[:K], pid[:K], sites=tips, observe=observe)
    assert np.all(np.isfinite(ll))
    assert np.array_equal(bc.sum_in_run_order(br), st, equal_nan=True)
    assert np.array_equal(ll, ll_tot)
    assert np.array_equal(ll, api.loglik_models(z, Qs[:K], pid[:K], sites=tips, observe=observe))
    som = bc.owner(K, 3)
    brp, llp = api.expected_branch_stats_models(z, Qs[:K], pid[:K], sites=tips, observe=observe, site_of_model=som)
    stp, llp_tot = api.expected_sumstat_models(z, Qs[:K], pid[:K], sites=tips, observe=observe, site_of_model=som)
    assert np.array_equal(bc.sum_in_run_order(brp), stp, equal_nan=True) and np.array_equal(llp, llp_tot)


# ---- 3. selection ----
@pytest.mark.parametrize("n", [4, 20])
def test_a_selection_out_of_order_with_a_repeat(n):
    z, Qs, pid, tips, observe, _, _ = _problem(n)
    K = min(len(Qs), 5)
    full = api.expected_branch_stats_models(z, Qs[:K], pid[:K], sites=tips, observe=observe)
    got = api.expected_branch_stats_models(z, Qs[:K], pid[:K], sites=tips, observe=observe, edges=bc.EDGE_LIST)
    assert got[0].shape == (K, 3, len(bc.EDGE_LIST), n * n)
    assert np.array_equal(got[0], full[0][:, :, bc.EDGE_LIST], equal_nan=True) and np.array_equal(got[1], full[1])
    som = bc.owner(K, 3)
    brp, llp = api.expected_branch_stats_models(z, Qs[:K], pid[:K], sites=tips, observe=observe, site_of_model=som, edges=bc.EDGE_LIST)
    ks = np.arange(K)
    assert np.array_equal(brp, got[0][ks, som], equal_nan=True) and np.array_equal(llp, got[1][ks, som])
    one = api.expected_branch_stats_models(z, Qs[:K], pid[:K], sites=tips, observe=observe, edges=[bc.ZERO_EDGE])
    assert one[0].shape == (K, 3, 1, n * n) and np.all(one[0] == 0.0)


# ---- 4. independence from the wave's other lanes ----
@pytest.mark.parametrize("n", [3, 8])
def test_a_model_does_not_see_its_waves_other_lanes(n):
    z, Qs, pid, tips, observe, _, _ = _problem(n)
    br, ll = api.expected_branch_stats_models(z, Qs, pid, sites=tips, observe=observe)
    for k in (0, 37, 69):
        alone = api.expected_branch_stats_models(z, Qs[k:k + 1], pid[k:k + 1], sites=tips, observe=observe)
        assert np.array_equal(alone[0][0], br[k], equal_nan=True) and np.array_equal(alone[1][0], ll[k])


# ---- 5. chunks and devices; 6. labels ----
def _labels(n, L):
    """L = 3: all zeros, negative weights, the observed changes behind the parity map; L = 1: negative and positive weights"""
    rs = np.random.default_rng(0xB29 + n)
    mixed = rs.uniform(-1.0, 1.0, (n, n))
    if L == 1:
        return mixed[None]
    return np.stack([np.zeros((n, n)), -rs.uniform(0.1, 1.0, (n, n)), ratemodel.observed_change_labels(bc.parity(n))])


@pytest.mark.parametrize("n", [4, 8, 20])
def test_chunks_and_devices_do_not_change_a_bit(n):
    z, Qs, pid, tips, observe, _, _ = _problem(n)
    K = len(Qs) if n <= 8 else 5
    if n > 8:
        Qs, pid = bc.models(n, K)
    lab = _labels(n, 3)
    som = bc.owner(K, 3)

    def f(**kw):
        return api.expected_branch_stats_models(z, Qs[:K], pid[:K], sites=tips, observe=observe, **kw)

    try:
        for kw in ({}, {"labels": lab}, {"site_of_model": som, "edges": bc.EDGE_LIST}, {"site_of_model": som, "labels": lab}):
            plain = f(**kw)
            for opt in ({"expect_chunk": 64}, {"expect_chunk": 2}, {"devices": [0, 0]}):
                assert _same(f(**kw, **opt), plain), (kw.keys(), opt)
    finally:
        _lib.set_debug_options()


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("n", [4, 20, 61])
def test_labelled_sums_are_the_column_loop_over_the_full_rows(n, L):
    z, Qs, pid, tips, observe, _, _ = _problem(n)
    K = min(len(Qs), 5)
    lab = _labels(n, L)
    full, ll = api.expected_branch_stats_models(z, Qs[:K], pid[:K], sites=tips, observe=observe)
    got, ll_l = api.expected_branch_stats_models(z, Qs[:K], pid[:K], sites=tips, observe=observe, labels=lab if L > 1 else lab[0])
    assert got.shape == full.shape[:-1] + (L,) and np.array_equal(ll, ll_l)
    want = bc.label_reduce(full, lab)
    assert np.array_equal(got, want, equal_nan=True)
    if L == 3:
        assert np.all(got[..., 0] == 0.0) and np.all(got[..., 1] <= 0.0) and np.any(got[..., 1] < 0.0) and np.all(got[..., 2] >= 0.0)
    sel = api.expected_branch_stats_models(z, Qs[:K], pid[:K], sites=tips, observe=observe, labels=lab, edges=bc.EDGE_LIST)
    assert np.array_equal(sel[0], want[:, :, bc.EDGE_LIST], equal_nan=True)


# ---- 7. special lanes ----
@pytest.mark.parametrize("n", [4, 9])
def test_an_impossible_model_among_ordinary_ones(n):
    z = bc.tree40()
    Qs, pid = bc.models(n, 5, seed=7)
    tips = bc.sites(n, 40, 3, seed=7)
    tips[:, 0], tips[:, 1] = 1, n                                             # a tip in each block
    h = n // 2
    Qs[2][:h, h:] = 0.0                                                       # block-diagonal: the two halves never meet
    Qs[2][h:, :h] = 0.0
    idx = np.arange(n)
    Qs[2][idx, idx] = 0.0
    Qs[2][idx, idx] = -Qs[2].sum(axis=1)
    lab = _labels(n, 3)
    for kw in ({}, {"labels": lab}):
        br, ll = api.expected_branch_stats_models(z, Qs, pid, sites=tips, **kw)
        assert np.all(ll[2] == -np.inf) and np.all(np.isnan(br[2]))
        rest = [0, 1, 3, 4]
        assert np.all(np.isfinite(ll[rest])) and np.all(np.isfinite(br[rest]))
        alone = api.expected_branch_stats_models(z, Qs[rest], pid[rest], sites=tips, **kw)
        assert np.array_equal(alone[0], br[rest]) and np.array_equal(alone[1], ll[rest])   # the neighbours: the call without it


@pytest.mark.parametrize("n", [4, 17])
def test_a_model_that_leaves_no_state(n):
    """mu = 0 (P = I): dwell = t_b on the posterior state and no counts, on every branch.  Tips in state 3 or missing"""
    z = bc.tree40()
    lens = z["edge.length"]
    Qs, _ = bc.models(n, 3, seed=8)
    Qs[1] = 0.0
    one = np.full((2, 40), 3, dtype=np.int32)
    one[0, ::3] = 0
    one[1] = 0                                                                # every tip missing: the posterior is pid
    pid = np.arange(1.0, n + 1.0)
    br, ll = api.expected_branch_stats_models(z, Qs, pid, sites=one)
    assert np.all(np.isfinite(br)) and np.all(np.isfinite(ll))
    assert np.all(br[1, :, :, n:] == 0.0)                                      # the counts: exactly 0
    np.testing.assert_allclose(br[1, :, :, :n].sum(axis=2), np.broadcast_to(lens, (2, lens.size)), rtol=1e-13, atol=0)
    want = np.zeros((lens.size, n))
    want[:, 2] = lens
    np.testing.assert_allclose(br[1, 0, :, :n], want, rtol=1e-13, atol=0)
    np.testing.assert_allclose(br[1, 1, :, :n], lens[:, None] * (pid / pid.sum())[None, :], rtol=1e-13, atol=0)
    assert np.all(br[:, :, bc.ZERO_EDGE] == 0.0)
    st, ll_tot = api.expected_sumstat_models(z, Qs, pid, sites=one)
    assert np.array_equal(bc.sum_in_run_order(br), st) and np.array_equal(ll, ll_tot)


@pytest.mark.parametrize("n", [5, 8, 17])
def test_a_long_branch_beside_short_ones(n):
    """mu t_b = 800 on one branch: the 2^-512 rescaling at 5 and 8 states; at 17 states the long form on that edge for two models
    and the short form on every other edge, and on that edge too for the third model, in one call"""
    edge, lens, Q, pid, tips = stateclasses.long_branch(n)
    z = {"edge": edge, "edge.length": lens, "Nnode": 5, "states": np.ones(6, dtype=np.int32)}
    Qs = np.stack([Q, 0.01 * Q, 0.5 * Q])
    x = [float(np.max(-np.diag(q))) * float(lens[stateclasses.B_LONG]) for q in Qs]
    assert x[0] == pytest.approx(800.0)
    assert terms(x[0]) > SW_M_CAP and terms(x[2]) > SW_M_CAP and terms(x[1]) <= SW_M_CAP
    assert all(terms(float(np.max(-np.diag(Q))) * float(t)) <= SW_M_CAP for b, t in enumerate(lens) if b != stateclasses.B_LONG)
    br, ll = api.expected_branch_stats_models(z, Qs, pid, sites=tips)
    want, ll_want = bc.twin(z, Qs, pid, tips)
    _bar(f"n={n} long branch, M = {[terms(v) for v in x]}", br, want, ll, ll_want, float(np.sum(lens)))
    st, ll_tot = api.expected_sumstat_models(z, Qs, pid, sites=tips)
    assert np.array_equal(bc.sum_in_run_order(br), st) and np.array_equal(ll, ll_tot)


# ---- 8. against the one-model call ----
@pytest.mark.parametrize("n", [4, 20])
def test_against_the_one_model_call(n):
    z, Qs, pid, tips, observe, _, _ = _problem(n)
    K = min(len(Qs), 3)
    if n > 8:
        Qs, pid = bc.models(n, 3)
    br, ll = api.expected_branch_stats_models(z, Qs[:K], pid[:K], sites=tips, observe=observe)
    length = float(np.sum(z["edge.length"]))
    for k in range(K):
        _, ll_one, br_one = api.expected_sumstat(z, Qs[k], pid[k], sites=tips, observe=observe, per_branch=True)
        assert np.array_equal(ll[k], ll_one)
        err = np.abs(br[k] - br_one)
        allow = 1e-12 * np.abs(br_one) + 1e-14 * length
        print(f"n={n} model {k}: against expected_sumstat(per_branch=True): error / allowance {np.max(err / allow):.3g}")
        assert np.all(err <= allow)
