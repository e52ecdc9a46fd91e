"""The exact sampler of histories over many rate matrices and sites on the device (phm_sample_histories_models, DESIGN.md section
19) against its Python twin (tests/samplemodelsref.py): node states, counts and map offsets and states exactly, dwell times to
1e-12 of the tree length, the log-likelihood bit for bit with ``api.loglik_models``; a branch at mu t = 2 280; impossible
evaluations and a model that leaves no state; chunking and devices; the two-phase maps contract; the device's own statistics
against the exact expectations; and fit -> models -> maps -> chain end to end.

Why exact: the device's P (Pade) and the twin's (scipy) differ in the last bits, so a draw flips only if a uniform falls within
about 1e-14 relative of a threshold -- about 1e-9 per case.  Should one occur, that case's seed changes and section 19 records it;
no tolerance is added."""
import ctypes as C
import math

import numpy as np
import pytest

import samplecases as sc
import samplemodelsref as ref
from phylomap_amd import _lib, api, fit, ratemodel, synth
from phylomap_amd.maps import history_tree
from test_sample_models_cpu import z_columns, z_nodes

pytestmark = pytest.mark.gpu


def models(n, K, seed, hidden=False):
    if hidden:
        return np.stack([sc.hidden_Q(0.5 + 0.25 * k) for k in range(K)])
    return np.stack([sc.random_Q(n, seed + k, 0.5 + 1.5 * (k % 7) / 7.0) for k in range(K)])


def pids(n, K, per_model, seed):
    if not per_model:
        return np.full(n, 1.0 / n)
    p = np.random.default_rng(seed).uniform(0.2, 1.0, (K, n))
    return p / p.sum(axis=1, keepdims=True)


def check_against_twin(z, Qs, pid, sites, D, observe=None, som=None, seed=1, **opt):
    edge, lens = z["edge"], z["edge.length"]
    E = edge.shape[0]
    n = Qs.shape[1]
    stats, ll, nodes, m = api.sample_histories(z, Qs, pid, D, sites=sites, observe=observe, site_of_model=som, nodes=True, maps=True,
                                               seed=seed, **opt)
    want = ref.sample_models(edge, lens, Qs, pid, sites, D, observe=observe, site_of_model=som, seed=seed,
                             replica_offset=opt.get("replica_offset", 0))
    assert np.array_equal(ll, api.loglik_models(z, Qs, pid, sites=sites, observe=observe, site_of_model=som))
    fin = np.isfinite(ll)
    assert np.array_equal(fin, np.isfinite(want["loglik"]))
    assert np.allclose(ll[fin], want["loglik"][fin], rtol=1e-11, atol=1e-11)
    assert np.array_equal(nodes, want["nodes"])
    assert np.array_equal(stats[..., n:], want["stats"][..., n:], equal_nan=True)
    assert np.array_equal(np.isnan(stats), np.isnan(want["stats"]))
    tol = 1e-12 * float(lens.sum())
    assert np.all(np.abs(stats[..., :n][fin] - want["stats"][..., :n][fin]) <= tol)
    assert np.array_equal(m.off, want["off"])
    assert np.array_equal(m.state, want["state"])
    assert m.dwell.size == want["dwell"].size and (m.dwell.size == 0 or np.max(np.abs(m.dwell - want["dwell"])) <= tol)
    rows = np.bincount(np.repeat(np.arange(m.off.size - 1), np.diff(m.off)), weights=m.dwell, minlength=m.off.size - 1)
    want_rows = np.where(np.repeat(fin.reshape(-1), D)[:, None], lens[None, :], 0.0).reshape(-1)
    assert np.all(np.abs(rows - want_rows) <= 1e-12 * want_rows)              # every row sums to its t_b (an undrawn one is empty)
    return stats, ll, nodes, m


CASES = [
    # n, K, S, D, shuffled, observe, missing, per-model pid, paired
    (2, 1, 1, 130, False, None, 0.0, False, False),
    (3, 3, 2, 63, True, None, 0.1, True, False),
    (4, 3, 2, 64, False, sc.PARITY, 0.1, False, True),
    (8, 3, 1, 64, True, None, 0.0, True, False),
    (2, 65, 1, 1, False, None, 0.1, True, False),
    (4, 65, 2, 1, True, sc.PARITY, 0.1, False, True),
    (3, 1, 2, 130, False, None, 0.0, False, False),
    (5, 3, 2, 64, True, None, 0.1, True, False),           # 5, 6, 7 states: the run-time-n forms below n = 8
    (6, 3, 2, 64, False, None, 0.0, False, False),
    (7, 3, 2, 64, True, None, 0.1, False, False),
]


@pytest.mark.parametrize("n,K,S,D,shuffled,observe,missing,per_model,paired", CASES)
def test_against_the_twin(n, K, S, D, shuffled, observe, missing, per_model, paired):
    edge, lens = sc.tree(shuffle=shuffled)
    assert lens.min() == 0.0
    Qs = models(n, K, 100 * n + K, hidden=observe is not None)
    sites = np.stack([sc.tips_for(edge, lens, Qs[0], 50 + s, observe, missing) for s in range(S)])
    som = [(k + 1) % S for k in range(K)] if paired else None
    z = sc.as_z(edge, lens, sites[0])
    check_against_twin(z, Qs, pids(n, K, per_model, n + K), sites, D, observe=observe, som=som, seed=1000 + n * K + D,
                       replica_offset=3 if n == 3 else 0)


def test_long_branch():
    edge, lens = synth.random_tree(6, 0.3, 9)
    lens = lens.copy()
    b_long = 4
    lens[b_long] = 228.0
    fast = np.array([[-10.0, 10.0], [7.0, -7.0]])
    Qs = np.stack([fast, fast * 0.01, fast * 0.001])
    assert float(np.max(-np.diag(Qs[0]))) * lens.max() == 2280.0
    tips = sc.tips_for(edge, lens, Qs[1], 3)
    z = sc.as_z(edge, lens, tips)
    D = 64
    stats, ll, nodes, m = check_against_twin(z, Qs, [.5, .5], tips[None], D, seed=77)
    E = edge.shape[0]
    seg = m.counts().reshape(3, D, E)[0, :, b_long].astype(np.float64)
    _, _, br = api.expected_sumstat(z, Qs[0], [.5, .5], per_branch=True)
    want = 1.0 + float(br[0, b_long, 2:].sum())
    zed = abs(seg.mean() - want) / (seg.std(ddof=1) / math.sqrt(D))
    print(f"long branch: mean segments {seg.mean():.1f}, exact {want:.1f}, |z| = {zed:.2f}")
    assert seg.mean() > 1000 and zed < 5.0


def test_impossible_evaluation_and_a_model_that_leaves_no_state():
    edge, lens = sc.tree()
    Q = sc.random_Q(3, 5)
    Qs = np.stack([Q, np.zeros((3, 3)), 2.0 * Q])
    varied = sc.tips_for(edge, lens, Q, 8)
    assert len(np.unique(varied)) > 1
    sites = np.stack([varied, np.full(varied.size, 2, dtype=np.int32)])
    z = sc.as_z(edge, lens, varied)
    D, E = 70, edge.shape[0]
    stats, ll, nodes, m = check_against_twin(z, Qs, np.full(3, 1 / 3), sites, D, seed=31)
    assert ll[1, 0] == -np.inf and np.all(np.isfinite(np.delete(ll.reshape(-1), 2)))
    assert np.all(np.isnan(stats[1, 0])) and np.all(nodes[1, 0] == 0)
    cnt = m.counts().reshape(3, 2, D, E)
    assert np.all(cnt[1, 0] == 0)
    # mu = 0 on the constant site: one segment per branch, zero counts, the whole tree in state 2
    assert np.all(cnt[1, 1] == 1) and np.all(stats[1, 1, :, 3:] == 0) and np.all(nodes[1, 1] == 2)
    assert np.allclose(stats[1, 1, :, 1], lens.sum(), rtol=1e-14) and np.all(stats[1, 1, :, [0, 2]] == 0)


@pytest.mark.parametrize("n", [4, 8])
def test_chunking_and_devices_change_no_bit(n):
    edge, lens = sc.tree(shuffle=True)
    K, S, D = 5, 3, 70
    Qs = models(n, K, 7 * n, hidden=False)
    sites = np.stack([sc.tips_for(edge, lens, Qs[0], 60 + s, None, 0.1) for s in range(S)])
    z = sc.as_z(edge, lens, sites[0])
    pid = pids(n, K, True, 3)

    def run(**opt):
        return api.sample_histories(z, Qs, pid, D, sites=sites, nodes=True, maps=True, seed=11, **opt)

    def same(a, b):
        return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and
                np.array_equal(a[3].off, b[3].off) and np.array_equal(a[3].dwell, b[3].dwell) and np.array_equal(a[3].state, b[3].state))

    plain = run()
    som = [2, 0, 1, 1, 0]
    plain_p = run(site_of_model=som)
    try:
        assert same(run(expect_chunk=64), plain)
        assert same(run(expect_chunk=2), plain)
        assert same(run(devices=[0, 0]), plain)
        assert same(run(site_of_model=som, expect_chunk=2), plain_p)
        assert same(run(site_of_model=som, devices=[0, 0]), plain_p)
    finally:
        _lib.set_debug_options()


def test_sizing_and_filling():
    edge, lens = sc.tree()
    n, K, D = 4, 3, 40
    Qs = models(n, K, 3)
    tips = sc.tips_for(edge, lens, Qs[0], 70)
    z = sc.as_z(edge, lens, tips)
    E, NT = edge.shape[0], edge.shape[0] + 1
    H = K * D
    L = _lib.load()
    pt, o = _lib.PlainTree(z, z["states"]), _lib.make_options(seed=19)
    Qf = np.ascontiguousarray(Qs.transpose(0, 2, 1))
    pid = np.full((1, n), 0.25)

    def call(off, cap, dwell, state):
        stats = np.zeros((n * n, H))
        ll = np.zeros(K)
        nodes = np.zeros((H, NT), dtype=np.int32)
        st = L.phm_sample_histories_models(C.byref(pt.c), n, K, _lib._p(Qf, C.c_double), _lib._p(pid, C.c_double), 1, None, None, D,
                                           C.byref(o), _lib._p(stats, C.c_double), _lib._p(ll, C.c_double),
                                           _lib._p(nodes, C.c_int32), _lib._p(off, C.c_int64), cap, _lib._p(dwell, C.c_double),
                                           _lib._p(state, C.c_int32))
        return st, (stats, ll, nodes)

    st, plain = call(None, 0, None, None)
    assert st == 0
    off = np.zeros(H * E + 1, dtype=np.int64)
    st, sized = call(off, 0, None, None)
    assert st == 0 and off[-1] >= H * E and np.all(np.diff(off) >= 1)
    cap, G = int(off[-1]), 64
    dwell = np.full(cap + G, -7.25)
    state = np.full(cap + G, -7, dtype=np.int32)
    st, filled = call(off, cap, dwell, state)
    assert st == 0
    for x, y, w in zip(plain, sized, filled):
        assert np.array_equal(x, y) and np.array_equal(x, w)
    assert np.all(dwell[cap:] == -7.25) and np.all(state[cap:] == -7) and np.all(dwell[:cap] >= 0) and np.all(state[:cap] >= 1)
    row = 17 * E + 5
    bad = off.copy()
    bad[row + 1:] += 1
    cap2 = int(bad[-1])
    dwell = np.full(cap2 + G, -7.25)
    state = np.full(cap2 + G, -7, dtype=np.int32)
    st, _ = call(bad, cap2, dwell, state)
    assert st == 1 and f"row {row} " in L.phm_last_error().decode()
    assert np.all(dwell[cap2:] == -7.25) and np.all(state[cap2:] == -7)


def test_statistics_on_the_device():
    edge, lens = synth.random_tree(40, 0.3, 13)
    m = ratemodel.hidden_rates(1)
    thetas = np.array([[.3, .2, .4, .5, 2.0], [.5, .3, .2, .6, 1.5], [.2, .4, .5, .3, 3.0], [.6, .6, .3, .3, 1.0]])
    Qs = m.Qs(thetas)
    tips = sc.tips_for(edge, lens, Qs[0], 17, sc.PARITY, 0.1)
    z = sc.as_z(edge, lens, tips)
    pid = np.full(4, .25)
    D = 8192
    stats, ll, nodes = api.sample_histories(z, Qs, pid, D, observe=sc.PARITY, nodes=True, seed=23)
    want, ll_want = api.expected_sumstat_models(z, Qs, pid, observe=sc.PARITY)
    assert np.array_equal(ll, ll_want)
    for k in range(4):
        zc = z_columns(stats[k, 0], want[k, 0])
        _, _, post = api.expected_sumstat(z, Qs[k], pid, observe=sc.PARITY, nodes=True)
        zn = z_nodes(nodes[k, 0], np.clip(post[0], 0.0, 1.0))
        print(f"model {k}: max |z| columns {zc.max():.2f}, nodes {zn.max():.2f}")
        assert zc.max() < 5.0 and zn.max() < 5.0
    seen = np.asarray(sc.PARITY)[nodes[:, 0, :, :tips.size] - 1]
    assert np.all((seen == tips) | (tips == 0))


def test_fit_to_models_to_maps_to_a_chain():
    import test_fit_cpu
    edge, lens, tips, model, pid, _, th_want = test_fit_cpu.problem(2)
    z = sc.as_z(edge, lens, tips)
    r = api.fit_ml(z, model, pid, se=True)
    assert r["se_ok"] and np.allclose(r["theta"], th_want, rtol=1e-3)
    thetas = fit.sample_thetas(r, 64, seed=4)
    Qs = model.Qs(thetas)
    stats, ll, m = api.sample_histories(z, Qs, pid, 1, maps=True, seed=5)
    assert stats.shape == (64, 1, 1, 4) and np.all(np.isfinite(stats)) and len(m) == 64
    assert np.allclose(stats[..., :2].sum(axis=-1), lens.sum(), rtol=1e-12)
    zt = history_tree(z, m, 37, n=2)
    assert np.array_equal(zt["states"], tips)
    Omega = 1.25 * float(np.max(np.abs(np.diag(Qs[37]))))
    out = api.sumstatMCMC(zt, Qs[37], np.asarray(pid, dtype=np.float64), Omega, 200, seed=6)
    assert out.shape[0] == 200 and np.all(np.isfinite(out))
