"""Expected statistics and log-likelihoods of many rate matrices at 9..64 states on the device (phm_expected_stats_models_wide,
DESIGN.md section 26): the first state count of every lane class, its unpadded last and the codon model's 61; cross and paired
mode, shuffled edge tables with a zero-length branch, observe maps, shared and per-model root priors.  loglik against the C-ABI
phm_loglik_models (the one-model-at-a-time route) and against the call with no statistics asked for BIT FOR BIT; the statistics
against the Python twin (``exactref.expected`` per model) and against the C-ABI phm_expected_stats_models (the parent's loop) under
the project's bar; both forms of the branch stage in one launch and on either side of the threshold between them; an impossible
model and a model that leaves no state; chunks and devices bit for bit; one exact-gradient fit with standard errors."""
import ctypes as C

import numpy as np
import pytest

import exactref
import stateclasses
from phylomap_amd import _lib, api, ratemodel, synth

pytestmark = pytest.mark.gpu
WIDE = "phm_expected_stats_models_wide"
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


def _tree(T, seed, shuffled, mean=0.5):
    """pre-ordered edge table, or shuffled with one zero-length branch"""
    edge, lens = synth.random_tree(T, mean, seed)
    if shuffled:
        rs = np.random.default_rng(seed)
        perm = rs.permutation(edge.shape[0])
        edge, lens = edge[perm], lens[perm].copy()
        lens[int(rs.integers(edge.shape[0]))] = 0.0
    return {"edge": edge, "edge.length": lens, "Nnode": T - 1, "states": np.ones(T, dtype=np.int32)}


def _random_Qs(K, n, rs, lo=0.05, hi=1.0):
    """random non-symmetric rate matrices, a tenth of the entries structurally zero, the rates scaled by 4 / n"""
    Qs = rs.uniform(lo, hi, (K, n, n)) * 4.0 / n
    Qs[rs.random((K, n, n)) < 0.1] = 0.0
    idx = np.arange(n)
    Qs[:, idx, (idx + 1) % n] += 0.05 * 4.0 / n                               # never a whole row of zeros
    Qs[:, idx, idx] = 0.0
    Qs[:, idx, idx] = -Qs.sum(axis=2)
    return Qs


def _tips(z, Q, pid, S, seed, observe=None, missing=0.1):
    tips, _ = api.simulate_histories(z, Q, pid, S, observe=observe, seed=seed)
    rs = np.random.default_rng(seed)
    tips[rs.random(tips.shape) < missing] = 0
    return tips


def _bar(got, want, ll_got, ll_want, length):
    """test_gpu_scores.py's bar restated: stats <= 1e-12 relative with section 13's floor of 1e-14 x tree length, loglik <= 1e-12
    max(1, |l|); an evaluation the reference finds impossible is -inf with a row of NaN.  Returns the largest stats error over its
    allowance."""
    assert got.shape == want.shape and ll_got.shape == ll_want.shape
    ok = np.isfinite(ll_want)
    assert np.array_equal(np.isfinite(ll_got), ok)
    assert np.all(ll_got[~ok] == -np.inf) and np.all(np.isnan(got[~ok]))
    le = np.abs(ll_got[ok] - ll_want[ok]) / np.maximum(1.0, np.abs(ll_want[ok]))
    assert np.all(le <= 1e-12), le.max()
    err = np.abs(got[ok] - want[ok])
    allow = 1e-12 * np.abs(want[ok]) + 1e-14 * length
    assert np.all(err <= allow), (err.max(), np.max(err / allow))
    return float(np.max(err / allow)) if err.size else 0.0


def _twin(z, Qs, pid, tips, observe, som):
    """exactref.expected per model: cross [K, S, cols] and [K, S]; paired (model k on site som[k]) [K, cols] and [K]"""
    pid = np.atleast_2d(np.asarray(pid, dtype=np.float64))
    st, ll = [], []
    for k in range(len(Qs)):
        y = tips if som is None else tips[int(som[k])][None]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            s, l = exactref.expected(z["edge"], z["edge.length"], Qs[k], pid[k if pid.shape[0] > 1 else 0], y, observe)
        l = np.where(np.isfinite(l), l, -np.inf)
        st.append(s if som is None else s[0])
        ll.append(l if som is None else l[0])
    return np.array(st), np.array(ll)


def _c_abi(name, z, Qs, pid, tips, observe, som, stats=True, **opt):
    """one entry point of the C-ABI by name, through _lib: (stats [.., cols] or None, loglik)"""
    L = _lib.load()
    n, a, shape, head = api._models_on_tips(z, Qs, pid, tips, observe, som, opt)
    ll = np.zeros(shape)
    if name == "phm_loglik_models":
        _lib.check(L.phm_loglik_models(*head, C.byref(a.opt), _lib._p(ll, C.c_double)))
        return None, ll
    st = np.zeros((n * n,) + shape) if stats else None
    _lib.check(getattr(L, name)(*head, C.byref(a.opt), _lib._p(st, C.c_double), _lib._p(ll, C.c_double)))
    return (None if st is None else np.moveaxis(st, 0, -1)), ll


def _check(what, z, Qs, pid, tips, observe, som):
    """the checks every shape gets; returns the new entry point's (stats, loglik)"""
    K, n = Qs.shape[0], Qs.shape[1]
    length = float(np.sum(z["edge.length"]))
    got, ll = _c_abi(WIDE, z, Qs, pid, tips, observe, som)
    shape = (K,) if som is not None else (K, tips.shape[0])
    assert got.shape == shape + (n * n,) and ll.shape == shape
    _, ll_old = _c_abi("phm_loglik_models", z, Qs, pid, tips, observe, som)
    assert np.array_equal(ll, ll_old)                                         # bit for bit the one-model-at-a-time route's value
    none, ll_only = _c_abi(WIDE, z, Qs, pid, tips, observe, som, stats=False)
    assert none is None and np.array_equal(ll, ll_only)                       # ... and the call that asks for no statistics
    want, ll_want = _twin(z, Qs, pid, tips, observe, som)
    w_twin = _bar(got, want, ll, ll_want, length)
    ok = np.isfinite(ll)
    np.testing.assert_allclose(got[ok][:, :n].sum(axis=1), length, rtol=1e-12)   # the dwell times fill the tree
    old, ll_o = _c_abi("phm_expected_stats_models", z, Qs, pid, tips, observe, som)
    assert np.array_equal(ll, ll_o)
    w_old = _bar(got, old, ll, ll_o, length)
    zero = np.array([[Qs[k, i, j] == 0.0 for i in range(n) for j in range(n) if i != j] for k in range(K)])
    counts = got[..., n:]                                                     # a structurally zero q_ij: E[N_ij] = 0 exactly
    mask = np.broadcast_to(zero if som is not None else zero[:, None, :], counts.shape) & ok[..., None]
    assert np.all(counts[mask] == 0.0)
    print(f"{what}: stats error / allowance: twin {w_twin:.3g}, the parent's loop {w_old:.3g}")
    return got, ll


# (K, S, paired, shuffled + zero-length branch, parity observe, per-model pid)
SHAPES = [(1, 1, False, False, False, False), (3, 5, False, True, True, True), (5, 3, True, False, False, False)]
MANY = (130, 1, True, True, False, False)                  # more models than any chunk of 64 or 128
CASES = [(n, s) for n in (9, 16, 17, 32, 33, 61, 64) for s in SHAPES] + [(n, MANY) for n in (9, 17, 33)]


def _case(n, K, S, shuffled, observed, per_model_pid, seed):
    rs = np.random.default_rng(seed)
    z = _tree(24, seed, shuffled)
    Qs = _random_Qs(K, n, rs)
    observe = (np.arange(n) % 2 + 1) if observed else None
    pid = rs.uniform(0.1, 1.0, (K, n)) if per_model_pid else np.arange(1.0, n + 1.0)
    tips = _tips(z, Qs[0], np.atleast_2d(pid)[0], S, seed, observe)
    return z, Qs, pid, tips, observe


@pytest.mark.parametrize("n,shape", CASES, ids=lambda v: f"K{v[0]}-S{v[1]}-{'paired' if v[2] else 'cross'}" if isinstance(v, tuple)
                         else f"n{v}")
def test_lane_classes_against_the_twin_and_the_parents_loop(n, shape):
    K, S, paired, shuffled, observed, per_model_pid = shape
    seed = 0xC26 + 100 * n + K + S
    z, Qs, pid, tips, observe = _case(n, K, S, shuffled, observed, per_model_pid, seed)
    som = (np.arange(K) % S).astype(np.int32) if paired else None
    _check(f"n={n} K={K} S={S} {'paired' if paired else 'cross'}", z, Qs, pid, tips, observe, som)


@pytest.mark.parametrize("n", [9, 17, 33])
def test_sites_beyond_a_groups_walk_and_a_workgroups_tile(n):
    """70 sites: the branch stage's tile is 16 (9 states) or 8 sites, the down pass' 64, 32 or 16; the last tile is partly empty"""
    seed = 0xC27 + n
    z, Qs, pid, tips, observe = _case(n, 2, 70, True, False, True, seed)
    got, ll = _check(f"n={n} K=2 S=70 cross", z, Qs, pid, tips, observe, None)
    for k in range(2):                                                        # one model on all 70 sites, paired
        pst, pll = _c_abi(WIDE, z, np.repeat(Qs[k:k + 1], 70, axis=0), np.repeat(pid[k:k + 1], 70, axis=0), tips, observe,
                          np.arange(70, dtype=np.int32))
        assert np.array_equal(pll, ll[k]) and np.array_equal(pst, got[k], equal_nan=True)


@pytest.mark.parametrize("n", [9, 17, 33, 64])
def test_both_forms_in_one_launch(n):
    """mu t_b = 800 on one branch (the long form) for two models, 8 for the third (the short form) on the same edge row"""
    edge, lens, Q, pid, tips = stateclasses.long_branch(n)
    z = {"edge": edge, "edge.length": lens, "Nnode": 5, "states": np.ones(6, dtype=np.int32)}
    Qs = np.stack([Q, 0.01 * Q, 0.5 * Q])
    x = [float(np.max(-np.diag(q))) * float(lens[stateclasses.B_LONG]) for q in Qs]
    assert terms(x[0]) > SW_M_CAP and terms(x[2]) > SW_M_CAP and terms(x[1]) <= SW_M_CAP
    assert all(terms(float(np.max(-np.diag(Q))) * float(t)) <= SW_M_CAP for b, t in enumerate(lens) if b != stateclasses.B_LONG)
    _check(f"n={n} long branch, M = {[terms(v) for v in x]}", z, Qs, pid, tips, None, None)


@pytest.mark.parametrize("n", [9, 33])
def test_either_side_of_the_threshold_between_the_forms(n):
    """one branch with M = SW_M_CAP (the last short item) and its neighbour with M = SW_M_CAP + 1 (the first long one)"""
    lo, hi = 10.0, 30.0
    assert terms(lo) <= SW_M_CAP < terms(hi)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if terms(mid) <= SW_M_CAP else (lo, mid)
    seed = 0xC28 + n
    rs = np.random.default_rng(seed)
    z = _tree(24, seed, False)
    Qs = _random_Qs(2, n, rs)
    Qs[1] = Qs[0]                                                             # the same mu: the same two branches for both
    mu = float(np.max(-np.diag(Qs[0])))
    lens = z["edge.length"].copy()
    lens[5], lens[6] = lo * (1.0 - 1e-9) / mu, hi * (1.0 + 1e-9) / mu
    z["edge.length"] = lens
    assert terms(mu * lens[5]) == SW_M_CAP and terms(mu * lens[6]) == SW_M_CAP + 1
    pid = np.arange(1.0, n + 1.0)
    tips = _tips(z, Qs[0], pid, 3, seed)
    _check(f"n={n} threshold at mu t = {lo:.6f}", z, Qs, pid, tips, None, None)


def test_an_impossible_model_among_five():
    n, seed = 9, 0xC29
    rs = np.random.default_rng(seed)
    z = _tree(24, seed, False)
    Qs = _random_Qs(5, n, rs)
    pid = np.arange(1.0, n + 1.0)
    tips = _tips(z, Qs[0], pid, 3, seed)
    tips[:, 0], tips[:, 1] = 1, 9                                             # a tip in each block
    Qs[2][:4, 4:] = 0.0                                                       # block-diagonal: states 1..4 and 5..9 never meet
    Qs[2][4:, :4] = 0.0
    idx = np.arange(n)
    Qs[2][idx, idx] = 0.0
    Qs[2][idx, idx] = -Qs[2].sum(axis=1)
    for som in (None, np.array([0, 1, 2, 0, 1], dtype=np.int32)):
        got, ll = _check("n=9 impossible model" + (" paired" if som is not None else ""), z, Qs, pid, tips, None, som)
        assert np.all(ll[2] == -np.inf) and np.all(np.isnan(got[2]))
        rest = [0, 1, 3, 4]
        assert np.all(np.isfinite(ll[rest])) and np.all(np.isfinite(got[rest]))
        alone, ll_alone = _c_abi(WIDE, z, Qs[rest], pid, tips, None, None if som is None else som[rest])
        assert np.array_equal(ll[rest], ll_alone) and np.array_equal(got[rest], alone)   # the neighbours: the run without it


def test_a_model_that_leaves_no_state():
    """mu = 0 (P = I): dwell = t_b on the posterior state and no counts.  Tips in state 3 or missing"""
    n = 9
    z = _tree(24, 0xC2A, False)
    length = float(np.sum(z["edge.length"]))
    Qs = _random_Qs(3, n, np.random.default_rng(1))
    Qs[1] = 0.0
    one = np.full((2, 24), 3, dtype=np.int32)
    one[0, ::3] = 0
    one[1] = 0                                                                # every tip missing: the posterior is pid
    pid = np.arange(1.0, n + 1.0)
    st, ll = _c_abi(WIDE, z, Qs, pid, one, None, None)
    assert ll[1, 0] == pytest.approx(np.log(3.0 / 45.0), rel=1e-15) and abs(ll[1, 1]) < 1e-15
    want = np.zeros(n * n)
    want[2] = length
    np.testing.assert_allclose(st[1, 0], want, rtol=1e-13, atol=0)
    np.testing.assert_allclose(st[1, 1, :n], pid / 45.0 * length, rtol=1e-13, atol=0)
    assert np.all(st[1, :, n:] == 0.0) and np.all(np.isfinite(st))
    _, ll_only = _c_abi(WIDE, z, Qs, pid, one, None, None, stats=False)
    assert np.array_equal(ll, ll_only)


@pytest.mark.parametrize("n", [9, 33])
def test_chunks_and_devices_do_not_change_a_bit(n):
    seed = 0xC2B + n
    z, Qs, pid, tips, observe = _case(n, 5, 5, True, True, True, seed)
    som = (np.arange(5) % 5).astype(np.int32)

    def f(som, **opt):
        return _c_abi(WIDE, z, Qs, pid, tips, observe, som, **opt)

    def same(a, b):
        return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])

    plain, plain_p = f(None), f(som)
    try:
        for s, ref in ((None, plain), (som, plain_p)):
            assert same(f(s, expect_chunk=64), ref)
            assert same(f(s, expect_chunk=2), ref)
            assert same(f(s, devices=[0, 0]), ref)
    finally:
        _lib.set_debug_options()
    assert np.array_equal(api.loglik_models(z, Qs, pid, sites=tips, observe=observe), plain[1])
    a = api.expected_sumstat_models(z, Qs, pid, sites=tips, observe=observe)   # the Python layer routes 9..64 states here
    assert np.array_equal(a[0], plain[0]) and np.array_equal(a[1], plain[1])


def test_one_fit_with_the_exact_gradient():
    n, T = 9, 60
    m = ratemodel.er(n)
    edge, lens = synth.random_tree(T, 0.5, 0xC2C)
    z = {"edge": edge, "edge.length": lens, "Nnode": T - 1, "states": np.ones(T, dtype=np.int32)}
    pid = np.full(n, 1.0 / n)
    tips, _ = api.simulate_histories(z, m.Q([0.15]), pid, 1, seed=0xC2C)
    z["states"] = tips[0]
    r = api.fit_ml(z, m, pid, starts=4, gtol=1e-8, gradient="exact", se=True)
    fd = api.fit_ml(z, m, pid, starts=4, gtol=1e-5)
    rel = float(np.max(np.abs(r["theta"] - fd["theta"]) / fd["theta"]))
    print(f"er(9), 60 tips: exact: theta {r['theta']} loglik {r['loglik']:.9f} iterations {r['iterations']} calls {r['calls']} "
          f"evaluations {r['evals']} max |score| {np.max(np.abs(r['grad'])):.3g} se_log {r['se_log']}; fd: theta {fd['theta']} "
          f"evaluations {fd['evals']}; relative difference {rel:.3g}")
    assert r["converged"]
    assert np.max(np.abs(r["grad"])) <= 1e-7
    assert rel <= 1e-5
    assert r["se_ok"]
