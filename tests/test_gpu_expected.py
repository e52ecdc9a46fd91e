"""Exact conditional expectations on the device (phm_expected_stats) against the two routes of the Python twin
(tests/exactref.py), invariances and error paths, large trees, and the point of the feature: per-dataset pins of the samplers
(the posterior mean of a sampler's rows on ONE tip vector against the exact expectation)."""
import os

import numpy as np
import pytest

import exactref
from phylomap_amd import _lib, api, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(n):
    if n == 2:
        return np.array([[-0.6, 0.6], [0.9, -0.9]])
    if n == 3:
        return np.array([[-0.5, 0.3, 0.2], [0.1, -0.4, 0.3], [0.6, 0.0, -0.6]])
    if n == 4:
        return synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0)
    if n == 20:
        return synth.tridiagonal_Q(20, 0.4)
    return synth.dense_Q(n, 0.01, 0.04)


def _tree(T, seed, shuffled):
    edge, lens = synth.random_tree(T, 1.0, seed)
    if shuffled:
        perm = np.random.default_rng(seed).permutation(edge.shape[0])
        edge, lens = edge[perm], lens[perm]
    return {"edge": edge, "edge.length": lens, "Nnode": T - 1, "states": np.ones(T, dtype=np.int32)}


def _tips(z, Q, pid, S, seed, observe=None, missing=0.1):
    tips, _ = api.simulate_histories(z, Q, pid, S, observe=observe, seed=seed)
    rs = np.random.default_rng(seed)
    tips[rs.random(tips.shape) < missing] = 0
    return tips


def _close(got, want, rtol, atol):
    err = np.abs(got - want)
    assert np.all(err <= rtol * np.abs(want) + atol), (err.max(), np.max(err / np.maximum(np.abs(want), 1e-300)))


def _check(z, Q, pid, tips, observe=None, route="unif", rtol=1e-12, what=None):
    st, ll, br, post = api.expected_sumstat(z, Q, pid, sites=tips, observe=observe, per_branch=True, nodes=True)
    ws, wl, wb, wp = exactref.expected(z["edge"], z["edge.length"], Q, pid, tips, observe=observe, route=route,
                                       per_branch=True, nodes=True)
    floor = 1e-14 * float(np.sum(z["edge.length"])) if route == "unif" else rtol * float(np.sum(z["edge.length"]))
    if what is not None:                                   # the figures first: a failing bar is then seen with its size
        with np.errstate(divide="ignore", invalid="ignore"):
            over = [np.nanmax(np.where(g == w, 0.0, np.abs(g - w) / (rtol * np.abs(w) + a)))
                    for g, w, a in ((st, ws, floor), (br, wb, floor), (ll, wl, 0.0))]
        print(f"{what}: error / allowance: totals {over[0]:.3g}, per branch {over[1]:.3g}, loglik {over[2]:.3g}, "
              f"node posteriors {np.max(np.abs(post - wp)) / (1e-13 if route == 'unif' else rtol):.3g}")
    _close(st, ws, rtol, floor)
    _close(br, wb, rtol, floor)
    _close(ll, wl, rtol, 0.0)
    _close(post, wp, 0.0, 1e-13 if route == "unif" else rtol)
    return st, ll, br, post


@pytest.mark.parametrize("n", [2, 3, 4, 8, 20, 61])
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("observed", [False, True])
def test_against_uniformization_twin(n, shuffled, observed):
    Q = _model(n)
    z = _tree(24, 0xE100 + n, shuffled)
    pid = np.arange(1.0, n + 1.0)
    observe = (np.arange(n) % 2 + 1) if observed else None
    for S in (1, 63, 64, 130):
        tips = _tips(z, Q, pid, S, seed=100 * n + S, observe=observe)
        st, ll, br, post = _check(z, Q, pid, tips, observe=observe)
        np.testing.assert_allclose(br.sum(axis=1), st, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(post.sum(axis=2), 1.0, rtol=0, atol=1e-12)
        np.testing.assert_allclose(st[:, :n].sum(axis=1), np.sum(z["edge.length"]), rtol=1e-12)
    # without per-branch / node outputs: the same totals and loglik bit for bit
    st2, ll2 = api.expected_sumstat(z, Q, pid, sites=tips, observe=observe)
    assert np.array_equal(st2, st) and np.array_equal(ll2, ll)


@pytest.mark.parametrize("n", [2, 3, 4, 8])
@pytest.mark.parametrize("shuffled", [False, True])
def test_against_van_loan_twin(n, shuffled):
    Q = _model(n)
    z = _tree(20, 0xE200 + n, shuffled)
    pid = np.ones(n)
    for observe in (None, np.arange(n) % 2 + 1):
        _check(z, Q, pid, _tips(z, Q, pid, 63, seed=7 + n, observe=observe), observe=observe, route="vanloan", rtol=1e-9)


def test_shared_tips_and_z_states():
    Q = _model(4)
    z = _tree(30, 5, False)
    tips = _tips(z, Q, np.ones(4), 1, seed=3)
    z = dict(z, states=tips[0])
    one = api.expected_sumstat(z, Q, np.ones(4))
    shared = api.expected_sumstat(z, Q, np.ones(4), n_replicas=70)          # tips_per_replica = 0: every site the same
    assert np.array_equal(shared[0], np.repeat(one[0], 70, axis=0)) and np.array_equal(shared[1], np.repeat(one[1], 70))


def test_devices_chunks_and_replica_offset_change_nothing():
    Q = _model(8)
    z = _tree(40, 11, True)
    pid = np.ones(8)
    tips = _tips(z, Q, pid, 130, seed=12)
    whole = api.expected_sumstat(z, Q, pid, sites=tips, per_branch=True, nodes=True)
    for opt in ({"devices": [0, 0, 0]}, {"replica_offset": 77}, {"expect_chunk": 64}, {"expect_chunk": 5, "devices": [0, 0]}):
        got = api.expected_sumstat(z, Q, pid, sites=tips, per_branch=True, nodes=True, **opt)
        for a, b in zip(whole, got):
            assert np.array_equal(a, b), opt
    small = api.expected_sumstat(z, Q, pid, sites=tips[:3], devices=[0, 0, 0])
    assert np.array_equal(small[0], whole[0][:3])


def test_impossible_site_is_named():
    Q = np.array([[-0.5, 0.5, 0.0], [0.0, 0.0, 0.0], [0.2, 0.3, -0.5]])    # state 2 absorbing
    z = _tree(16, 3, False)
    tips = np.full((5, 16), 2, dtype=np.int32)
    tips[3, 0] = 1                                                          # site 4: state 1 below an all-2 tree from a root in 2
    with pytest.raises(_lib.PhmError) as e:
        api.expected_sumstat(z, Q, np.array([0.0, 1.0, 0.0]), sites=tips)
    assert e.value.status == 5 and "site 4" in str(e.value)
    api.expected_sumstat(z, _model(2), np.ones(2), sites=np.ones((2, 16)))    # the device is still usable


def test_c3_tree_1024_sites():
    z, Q, pid, _ = synth.config_problem(3)                                  # 10 000 tips, 4 states
    tips = _tips(z, Q, pid, 1024, seed=0xC3)
    st, ll, br = api.expected_sumstat(z, Q, pid, sites=tips, per_branch=True)
    length = float(np.sum(z["edge.length"]))
    np.testing.assert_allclose(st[:, :4].sum(axis=1), length, rtol=1e-12)
    np.testing.assert_allclose(br.sum(axis=1), st, rtol=1e-12, atol=1e-14 * length)
    del br
    pick = [0, 1, 511, 1023]
    ws, wl = exactref.expected(z["edge"], z["edge.length"], Q, pid, tips[pick])
    _close(st[pick], ws, 1e-12, 1e-14 * length)
    _close(ll[pick], wl, 1e-12, 0.0)


def test_squamate_long_branches():
    d = np.load(os.path.join(ROOT, "tests", "golden", "squamate", "seed101_tips.npz"))
    T = len(d["states"])
    z = {"edge": d["edge"], "edge.length": d["edge_length"], "Nnode": T - 1, "states": d["states"]}
    Q = np.array([[-10.0, 10.0], [6.0, -6.0]])                              # mu t_b up to 2 280
    assert 10.0 * d["edge_length"].max() > 2000
    tips = np.stack([d["states"], _tips(z, Q, [0.5, 0.5], 1, seed=4)[0], np.zeros(T, dtype=np.int32)])
    st, ll = api.expected_sumstat(z, Q, [0.5, 0.5], sites=tips)
    ws, wl = exactref.expected(z["edge"], z["edge.length"], Q, [0.5, 0.5], tips)
    length = float(np.sum(z["edge.length"]))
    _close(st, ws, 1e-12, 1e-14 * length)
    _close(ll, wl, 1e-12, 1e-10)                  # site 3 has log p = 0: rows of 7 900 P(t_b) summing to 1 within rounding
    assert abs(ll[2]) < 1e-10                                               # every tip missing: p = 1


# ---- per-dataset pins of the samplers --------------------------------------------------------------------------------------
def _pin(rows, exact, what):
    """rows [K chains, N draws, cols] (post burn-in), exact [cols]: |mean - exact| / SE over the chain means"""
    means = rows.mean(axis=1)
    K = means.shape[0]
    m, se = means.mean(axis=0), means.std(axis=0, ddof=1) / np.sqrt(K)
    flat = se == 0                                       # no chain ever moved off 0: a state / pair of vanishing posterior mass
    assert np.all(np.abs(m[flat] - exact[flat]) < 1e-3), (what, exact[flat])
    keep = ~flat
    z = np.abs(m[keep] - exact[keep]) / se[keep]
    print(f"{what}: max |z| = {z.max():.2f} over {z.size} columns")
    assert z.max() < 4.5, (what, z)


def _dataset(n, Q, T, seed, init_segments, observe=None):
    pid = np.full(n, 1.0 / n)
    Om = 1.25 * float(np.max(np.abs(np.diag(Q))))
    z = synth.make_tree(T, Q, Om, seed, pid, init_segments=init_segments)
    tips, _ = api.simulate_histories(z, Q, pid, 1, observe=observe, seed=seed + 1)
    return z, pid, Om, tips


@pytest.mark.parametrize("fn,n", [("sumstatMCMC", 2), ("sumstatMCMC", 4), ("sumstatMCMC_bigtree", 8), ("SPARSEsumstatMCMC", 20)])
def test_sampler_posterior_mean_matches_exact(fn, n):
    Q = {2: _model(2) * 0.5, 4: synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0) * 0.5, 8: synth.dense_Q(8, 0.03, 0.12),
         20: synth.tridiagonal_Q(20, 0.6)}[n]
    z, pid, Om, tips = _dataset(n, Q, 60, 0xA10 + n, init_segments=n)
    exact, _ = api.expected_sumstat(z, Q, pid, sites=tips)
    K, N, burn = 512, 300, 100
    out = getattr(api, fn)(z, Q, pid, Om, N, sites=np.repeat(tips, K, axis=0), seed=0xA20 + n)     # [K, N, cols]
    _pin(out[:, burn:, :], exact[0], f"{fn} n={n}")


def test_ks_sweep_parity_tips_matches_exact():
    n = 4
    Q = synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0) * 0.5
    z, pid, Om, tips = _dataset(n, Q, 60, 0xA40, init_segments=n, observe=[1, 2, 1, 2])
    exact, _ = api.expected_sumstat(z, Q, pid, sites=tips, observe=[1, 2, 1, 2])
    out = api.sumstatMCMCks_sweep(z, Q, pid, Om, 300, sites=np.repeat(tips, 512, axis=0), seed=0xA41)
    cols = list(range(n)) + [n + a * n + c for a, c in exactref.columns(n)]      # ks layout: n x n counts with self pairs
    _pin(out[:, 100:, cols], exact[0], "ks sweep, parity tips")


def test_sumstat_exp_matches_exact():
    n = 4
    Q = synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0) * 0.5
    z, pid, Om, tips = _dataset(n, Q, 60, 0xA50, init_segments=n)
    exact, _ = api.expected_sumstat(z, Q, pid, sites=tips)
    out = api.sumstatEXP(dict(z, states=tips[0]), Q, pid, 20000, seed=0xA51)        # i.i.d. draws: chains of one draw
    _pin(out[:, None, :], exact[0], "sumstatEXP")


def test_bf_sweep_root_state_matches_node_posterior():
    n = 2
    Q = _model(2) * 0.5
    z, pid, Om, tips = _dataset(n, Q, 60, 0xA60, init_segments=n)
    _, _, post = api.expected_sumstat(z, Q, pid, sites=tips, nodes=True)
    T = tips.shape[1]
    out = api.sumstatMCMCbf_sweep(z, Q, pid, Om, 300, sites=np.repeat(tips, 512, axis=0), seed=0xA61)
    root = out[:, 100:, -1]
    ind = np.stack([root == a for a in range(n)], axis=2).astype(np.float64)
    _pin(ind, post[0, T], "bf sweep root state")
