"""The Python twin of the exact sampler over many rate matrices (tests/samplemodelsref.py) against the
exact conditional expectations, its jump-count series against P, the invariants of its maps, ``fit.sample_thetas`` and the C-ABI
surface of phm_sample_histories_models without a device.  No GPU needed.

|z| < 5 is a condition, not a measurement: over the few hundred column means and node frequencies compared here a correct sampler
misses it with probability below 1e-4, and the seeds are fixed."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy.linalg import expm

import exactref
import samplecases as sc
import samplemodelsref as ref
from phylomap_amd import _lib, api, fit, synth

D_STAT = 4096


@pytest.fixture(scope="module", autouse=True)
def one_blas_thread():
    try:
        import threadpoolctl
    except ImportError:
        yield
        return
    with threadpoolctl.threadpool_limits(limits=1):
        yield


def z_columns(stats, want):
    """|z| of every column mean of stats [D, cols] against want [cols]; a column without spread must match exactly (1e-9)"""
    D = stats.shape[0]
    m, sd = stats.mean(axis=0), stats.std(axis=0, ddof=1)
    z = np.zeros(stats.shape[1])
    for c in range(stats.shape[1]):
        if sd[c] == 0.0:
            assert abs(m[c] - want[c]) < 1e-9, (c, m[c], want[c])
        else:
            z[c] = abs(m[c] - want[c]) / (sd[c] / math.sqrt(D))
    return z


def z_nodes(nodes, post):
    """|z| of every node's state frequencies, nodes [D, NT] 1-based, post [NT, n]; a state of posterior 0 never appears and a state
    of posterior 1 always does.  The count of a state is Binomial(D, p) exactly, so z is taken from the exact tail: the normal
    quantile of min(P(X <= k), P(X >= k)).  Where D p (1 - p) is large this is (f - p) / sqrt(p (1 - p) / D); where it is not
    (a posterior of 3e-5 gives 0.1 expected draws in 4 096, and two of them would read as z = 5.5) the normal form has no such
    meaning, and |z| < 5 keeps its level of 2.9e-7 per side only in this form."""
    from scipy.stats import binom, norm
    D, n = nodes.shape[0], post.shape[1]
    z = np.zeros(post.shape)
    for s in range(n):
        k = (nodes == s + 1).sum(axis=0)
        p = post[:, s]
        sure = (p <= 0.0) | (p >= 1.0)
        assert np.array_equal(k[sure], D * p[sure])
        tail = np.minimum(binom.cdf(k[~sure], D, p[~sure]), binom.sf(k[~sure] - 1, D, p[~sure]))
        z[~sure, s] = np.maximum(0.0, norm.isf(np.minimum(tail, 0.5)))
    return z


def stat_case(n):
    edge, lens = sc.tree()
    if n == 2:
        Q, obs, pid = sc.random_Q(2, 1), None, np.array([.5, .5])
        tips = sc.tips_for(edge, lens, Q, 3)
    else:
        Q, obs, pid = sc.hidden_Q(), sc.PARITY, np.full(4, .25)
        tips = sc.tips_for(edge, lens, Q, 4, obs, 0.1)
    return edge, lens, Q, pid, tips, obs


@pytest.mark.parametrize("n", [2, 4])
def test_twin_against_the_exact_expectations(n):
    edge, lens, Q, pid, tips, obs = stat_case(n)
    assert lens.min() == 0.0 and lens.max() == 6.0 and (n == 2 or np.sum(tips == 0) >= 2)
    r = ref.sample_evaluation(edge, lens, Q, pid, tips, obs, eval_id=0, D=D_STAT, seed=7 + n)
    want, ll, post = exactref.expected(edge, lens, Q, pid, tips[None], observe=obs, nodes=True)
    assert abs(r["loglik"] - ll[0]) < 1e-12 * abs(ll[0])
    zc = z_columns(r["stats"], want[0])
    zn = z_nodes(r["nodes"], post[0])
    print(f"n={n}: max |z| columns {zc.max():.2f}, nodes {zn.max():.2f}")
    assert zc.max() < 5.0
    assert zn.max() < 5.0


def test_twin_jump_count_series_is_p():
    # S e^-x 2^(512 R) = P[a, e]: two states in closed form up to x = 2 280, four states against scipy's expm
    for a, b, t in ((1.0, 0.4, 0.01), (1.0, 0.4, 3.0), (10.0, 2.5, 80.0), (10.0, 7.0, 228.0)):
        Q = np.array([[-a, a], [b, -b]])
        x = max(a, b) * t
        _, _, beta = ref.model_table(Q, ref.stop_index(x))
        pi = np.array([b, a]) / (a + b)
        dec = math.exp(-(a + b) * t)
        P = np.array([[pi[0] + pi[1] * dec, pi[1] - pi[1] * dec], [pi[0] - pi[0] * dec, pi[1] + pi[0] * dec]])
        for i in range(2):
            for j in range(2):
                S, M, R = ref.jump_count_series(x, beta[:, [i], [j]])
                assert M == ref.stop_index(x)
                assert abs(S[0] * math.exp(-x + 512.0 * R * math.log(2.0)) - P[i, j]) < 1e-12, (x, i, j)
    Q = sc.hidden_Q()
    for t in (0.05, 1.0, 6.0, 40.0):
        x = float(np.max(-np.diag(Q))) * t
        _, _, beta = ref.model_table(Q, ref.stop_index(x))
        P = expm(Q * t)
        for i in range(4):
            for j in range(4):
                S, _, R = ref.jump_count_series(x, beta[:, [i], [j]])
                assert abs(S[0] * math.exp(-x + 512.0 * R * math.log(2.0)) - P[i, j]) < 1e-12
    # the stopping index grows with x (the table of a model is as deep as its longest branch needs)
    xs = np.concatenate([np.linspace(1e-6, 50.0, 400), np.linspace(50.0, 3000.0, 60)])
    Ms = [ref.stop_index(float(x)) for x in xs]
    assert all(m1 >= m0 for m0, m1 in zip(Ms, Ms[1:])) and ref.stop_index(0.0) == 0


def test_twin_maps_invariants():
    edge, lens, Q, pid, tips, obs = stat_case(4)
    D, E, n = 256, edge.shape[0], 4
    r = ref.sample_evaluation(edge, lens, Q, pid, tips, obs, eval_id=3, D=D, seed=21)
    off, dw, st = r["seg_off"], r["seg_dwell"], r["seg_state"]
    assert off[0] == 0 and off[-1] == dw.size == st.size and np.all(np.diff(off) >= 1)
    assert dw.min() >= 0.0
    counts = np.zeros((D, n + n * (n - 1)))
    for d in range(D):
        for b in range(E):
            s, w = st[off[d * E + b]:off[d * E + b + 1]], dw[off[d * E + b]:off[d * E + b + 1]]
            assert abs(w.sum() - lens[b]) <= 1e-12 * max(lens[b], 1e-300) or lens[b] == 0.0 and w.sum() == 0.0
            assert s[0] == r["nodes"][d, edge[b, 0] - 1] and s[-1] == r["nodes"][d, edge[b, 1] - 1]
            assert np.all(s[1:] != s[:-1])
            np.add.at(counts[d], s - 1, w)
            for i, j in zip(s[:-1] - 1, s[1:] - 1):
                counts[d, n + i * (n - 1) + (j - 1 if j > i else j)] += 1
    assert np.array_equal(counts[:, n:], r["stats"][:, n:])
    assert np.max(np.abs(counts[:, :n] - r["stats"][:, :n])) < 1e-12 * lens.sum()
    seen = np.asarray(obs)[r["nodes"][:, :tips.size] - 1]
    assert np.all((seen == tips[None]) | (tips[None] == 0))
    assert len(np.unique(r["nodes"][:, np.flatnonzero(tips == 0)[0]])) > 1       # a missing tip comes out sampled


def fake_fit(bound=False, ok=True):
    theta = np.array([0.4, 0.6, 1.5])
    A = np.array([[0.3, 0.0, 0.0], [0.1, 0.2, 0.0], [-0.05, 0.02, 0.25]])
    cov = A @ A.T
    se = np.sqrt(np.diag(cov))
    if bound:
        cov[1, :] = cov[:, 1] = np.nan
        se[1] = np.nan
    return dict(theta=theta, cov_log=cov, se_log=se, se_ok=ok)


def test_sample_thetas():
    r = fake_fit()
    M = 20000
    th = fit.sample_thetas(r, M, seed=5)
    assert th.shape == (M, 3) and np.all(th > 0)
    assert np.array_equal(th, fit.sample_thetas(r, M, seed=5))                  # bit-reproducible
    assert np.array_equal(th[:100], fit.sample_thetas(r, 100, seed=5))          # draw by draw from one stream
    assert not np.array_equal(th[:100], fit.sample_thetas(r, 100, seed=6))
    x = np.log(th)
    cov = r["cov_log"]
    se_mean = np.sqrt(np.diag(cov) / M)
    assert np.all(np.abs(x.mean(axis=0) - np.log(r["theta"])) < 4 * se_mean)
    sc_ = np.cov(x.T)
    se_cov = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / M)     # of a normal sample's covariance entries
    assert np.all(np.abs(sc_ - cov) < 3 * se_cov), np.abs(sc_ - cov) / se_cov
    rb = fake_fit(bound=True)
    tb = fit.sample_thetas(rb, 2000, seed=5)
    assert np.all(tb[:, 1] == rb["theta"][1]) and tb[:, 0].std() > 0 and tb[:, 2].std() > 0
    free = [0, 2]
    assert np.all(np.abs(np.cov(np.log(tb[:, free]).T) - rb["cov_log"][np.ix_(free, free)]) < 0.02)
    with pytest.raises(ValueError):
        fit.sample_thetas(fake_fit(ok=False), 10, seed=5)


def _raw(z, Qs, pid, draws=2, n_pid=None, S=2, observe=None, som=None, stats=True, ll=True, map_off="none", map_cap=0, fill=False):
    Qs = np.asarray(Qs, dtype=np.float64)
    K, n = Qs.shape[0], Qs.shape[1]
    Qf = np.ascontiguousarray(Qs.transpose(0, 2, 1))
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    pt = _lib.PlainTree(z, np.tile(z["states"], (S, 1)))
    t = pt.c
    obs = None if observe is None else np.ascontiguousarray(observe, dtype=np.int32)
    so = None if som is None else np.ascontiguousarray(som, dtype=np.int32)
    o = _lib.make_options(n_replicas=S, tips_per_replica=True)
    H = K * S * max(draws, 1)
    res = np.zeros(H * n * n) if stats else None
    lik = np.zeros(K * S) if ll else None
    off = None if isinstance(map_off, str) else np.ascontiguousarray(map_off, dtype=np.int64)
    dw = np.zeros(max(map_cap, 1)) if fill else None
    ms = np.zeros(max(map_cap, 1), dtype=np.int32) if fill else None
    L = _lib.load()
    status = L.phm_sample_histories_models(C.byref(t), n, K, _lib._p(Qf, C.c_double), _lib._p(pid, C.c_double),
                                           pid.size // n if n_pid is None else n_pid, _lib._p(obs, C.c_int32), _lib._p(so, C.c_int32),
                                           draws, C.byref(o), _lib._p(res, C.c_double), _lib._p(lik, C.c_double), None,
                                           _lib._p(off, C.c_int64), map_cap, _lib._p(dw, C.c_double), _lib._p(ms, C.c_int32))
    return status, L.phm_last_error().decode()


def test_c_abi_checks_need_no_device():
    L = _lib.load()
    assert "phm_sample_histories_models" in _lib.EXPORTS and hasattr(L, "phm_sample_histories_models")
    assert L.phm_version() == 300 and callable(api.sample_histories)
    z, Q, pid, _ = synth.config_problem(2, n_tips=16)
    Qs = np.stack([Q, 2 * Q, 3 * Q])
    E = 30
    assert _raw(z, Qs, pid, stats=False)[0] == 1                               # NULL stats
    assert _raw(z, Qs, pid, ll=False)[0] == 1
    bad = Qs.copy()
    bad[2, 0, 3], bad[2, 0, 1] = -0.05, bad[2, 0, 1] + 0.05                  # a negative rate in model 2
    st, msg = _raw(z, bad, pid)
    assert st == 1 and msg.startswith("model 2")
    st, msg = _raw(z, Qs, pid, draws=0)
    assert st == 1 and "draws" in msg
    assert _raw(z, Qs, pid, draws=-3)[0] == 1
    assert _raw(z, Qs, pid, som=[0, 1, 2])[0] == 1                            # S = 2
    assert _raw(z, Qs, pid, observe=[1, 2, 1, 5])[0] == 1
    z9 = dict(z, states=np.ones(16, dtype=np.int32))
    Q9 = sc.random_Q(9, 1)
    st, msg = _raw(z9, Q9[None], np.full(9, 1 / 9))
    assert st == 2 and "8 states" in msg
    zl = dict(z, **{"edge.length": z["edge.length"] * (40000.0 / (z["edge.length"].max() * np.max(-np.diag(Qs[1]))))})
    st, msg = _raw(zl, Qs, pid)                                               # model 0 stays below the limit, model 1 does not
    assert st == 2 and "model 1" in msg and "32768" in msg
    # the map_off checks are section 14's
    R = 3 * 2 * 2
    good = np.arange(R * E + 1, dtype=np.int64)
    st, msg = _raw(z, Qs, pid, map_off=np.r_[1, good[1:]], map_cap=int(good[-1]), fill=True)
    assert st == 1 and "map_off[0]" in msg
    dec = good.copy()
    dec[5] = 3
    st, msg = _raw(z, Qs, pid, map_off=dec, map_cap=int(good[-1]), fill=True)
    assert st == 1 and "row 4" in msg
    st, msg = _raw(z, Qs, pid, map_off=good, map_cap=int(good[-1]) - 1, fill=True)
    assert st == 1 and "map_cap" in msg
    st, msg = _raw(z, Qs, pid, map_off="none", map_cap=5, fill=True)          # segment arrays without offsets
    assert st == 1 and "map_off is NULL" in msg
    if L.phm_device_count() == 0:                                              # a valid call gets as far as the device
        assert _raw(z, Qs, pid)[0] == 3
        assert _raw(z, Qs, pid, map_off=np.zeros(R * E + 1, dtype=np.int64))[0] == 3
