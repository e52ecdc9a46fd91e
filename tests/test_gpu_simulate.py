"""Forward simulation on the device (phm_simulate_histories) against its Python twin (tests/simref.py) bit for bit, its
invariances, error paths and closed forms at size; then simulation-based calibration of the samplers: datasets simulated
forward, the sampler conditioned on each dataset's tips, the posterior means against the true statistics."""
import numpy as np
import pytest

import simref
from phylomap_amd import _lib, api, synth

pytestmark = pytest.mark.gpu


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


def _check_against_twin(z, Q, pid, R, seed, observe=None, **opt):
    tips, stats, nodes = api.simulate_histories(z, Q, pid, R, observe=observe, nodes=True, seed=seed, **opt)
    wt, ws, wn = simref.simulate(z["edge"], z["edge.length"], Q, pid, R, seed, replica_offset=opt.get("replica_offset", 0),
                                 observe=observe)
    n = Q.shape[0]
    assert np.array_equal(tips, wt)
    assert np.array_equal(nodes, wn)
    assert np.array_equal(stats[:, n:], ws[:, n:])                  # counts and root state
    np.testing.assert_allclose(stats[:, :n], ws[:, :n], rtol=1e-12, atol=0)
    return tips, stats, nodes, ws


@pytest.mark.parametrize("n", [2, 3, 4, 8, 20, 61])
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("observed", [False, True])
def test_bit_exact_against_twin(n, shuffled, observed):
    Q = _model(n)
    z = _tree(24, 0x5100 + n, shuffled)
    pid = np.arange(1.0, n + 1.0)
    observe = (np.arange(n) % 2 + 1) if observed else None
    for R in (1, 63, 64, 130):
        _, stats, _, twin = _check_against_twin(z, Q, pid, R, seed=1000 * n + R, observe=observe)
        if not shuffled:                                            # a pre-order edge table: the twin's dwell sums bit for bit
            assert np.array_equal(stats, twin)


def test_replica_offset_and_devices_give_the_one_call_output():
    Q = _model(4)
    z = _tree(40, 77, False)
    pid = np.ones(4)
    whole = api.simulate_histories(z, Q, pid, 130, nodes=True, seed=9)
    parts = [api.simulate_histories(z, Q, pid, c, nodes=True, seed=9, replica_offset=o) for o, c in ((0, 64), (64, 1), (65, 65))]
    for k in range(3):
        assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts]))
    two = api.simulate_histories(z, Q, pid, 130, nodes=True, seed=9, devices=[0, 0])
    for k in range(3):
        assert np.array_equal(whole[k], two[k])
    small = api.simulate_histories(z, Q, pid, 3, nodes=True, seed=9, devices=[0, 0])      # fewer replicas than 64 per device
    for k in range(3):
        assert np.array_equal(whole[k][:3], small[k])


def test_error_paths_return_their_status():
    z = _tree(16, 3, False)
    fast = np.array([[-1e4, 1e4], [1e4, -1e4]])                     # ~2e4 jumps on a branch of length 2
    zl = dict(z, **{"edge.length": np.full(30, 0.01)})
    zl["edge.length"][5] = 2.0
    with pytest.raises(_lib.PhmError) as e:
        api.simulate_histories(zl, fast, [1, 1], 64, seed=1)
    assert e.value.status == 6 and "edge row 6" in str(e.value)
    with pytest.raises(simref.JumpCapError):
        simref.simulate(zl["edge"], zl["edge.length"], fast, [1, 1], 64, 1)
    with pytest.raises(_lib.PhmError) as e:
        api.simulate_histories(z, _model(4), np.ones(4), 8, observe=[1, 2, 3, 0])
    assert e.value.status == 1
    with pytest.raises(_lib.PhmError) as e:
        api.simulate_histories(z, _model(4), np.zeros(4), 8)
    assert e.value.status == 5
    # an absorbing state is not an error: it keeps the rest of the branch (the reference computes Inf - Inf there)
    Qa = np.array([[-0.5, 0.5, 0.0], [0.0, 0.0, 0.0], [0.2, 0.3, -0.5]])
    _, stats, _, _ = _check_against_twin(z, Qa, np.array([1.0, 0.0, 1.0]), 130, seed=5)
    assert np.all(stats[:, 6:9] == 0.0)
    # the device is still usable after the failed calls
    _check_against_twin(z, _model(2), np.ones(2), 64, seed=6)


def test_c3_tree_16384_replicas_against_closed_forms():
    z, Q, pid, _ = synth.config_problem(3)                          # 10 000 tips, 4 states
    tips, stats = api.simulate_histories(z, Q, pid, 16384, seed=0xC3)
    assert tips.shape == (16384, 10000)
    zs = simref.zscores(tips, stats, z["edge"], z["edge.length"], Q, pid)
    assert zs.max() < 5.0, zs.max()
    np.testing.assert_allclose(stats[:, :4].sum(axis=1), np.sum(z["edge.length"]), rtol=1e-9)


def test_simulate_state_tree_feeds_the_sampler():
    Q = synth.config_Q(1)
    Om = 1.25 * 0.1
    z = synth.make_tree(32, Q, Om, 0x77)
    y = api.simulate_state_tree(z, Q, [0.5, 0.5], seed=4)
    tips, _ = api.simulate_histories(z, Q, [0.5, 0.5], 1, seed=4)
    assert np.array_equal(y["states"], tips[0])
    out = api.sumstatMCMC(y, Q, [0.5, 0.5], Om, 20, seed=1)
    assert out.shape == (20, 4) and np.all(np.isfinite(out))
    y4 = api.simulate_state_tree(z, synth.make2sQ(0.1, 0.1, 0.2, 0.2, 10.0), np.ones(4), observe=[1, 2, 1, 2], seed=4)
    assert set(np.unique(y4["states"])) <= {1, 2}


# ---- simulation-based calibration of the samplers --------------------------------------------------------------------------
def _mcmc_count_col(n, a, c):
    return n + a * (n - 1) + (c - 1 if a < c else c)


def _calibration_z(d):
    """|mean(d)| / (sd(d) / sqrt(S)) per column"""
    S = d.shape[0]
    sd = d.std(axis=0, ddof=1)
    keep = sd > 0
    return np.abs(d.mean(axis=0)[keep]) / (sd[keep] / np.sqrt(S))


def _sites_calibration(fn, n, Q, init_segments, S=512, N=400, burn=100, observe=None, ks=False):
    pid = np.full(n, 1.0 / n)
    Om = 1.25 * float(np.max(np.abs(np.diag(Q))))
    z = synth.make_tree(40, Q, Om, 0xCA1 + n, pid, init_segments=init_segments)
    tips, true = api.simulate_histories(z, Q, pid, S, observe=observe, seed=0x5BC + n)
    out = fn(z, Q, pid, Om, N, sites=tips, seed=0x5BD + n)          # [S, N, cols]
    post = out[:, burn:, :].mean(axis=1)
    cols_true = list(range(n))
    cols_post = list(range(n))
    for a in range(n):
        for c in range(n):
            if a != c:
                cols_true.append(n + a * n + c)
                cols_post.append(n + a * n + c if ks else _mcmc_count_col(n, a, c))
    d = post[:, cols_post] - true[:, cols_true]
    return _calibration_z(d)


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("fn", ["sumstatMCMC", "sumstatMCMC_bigtree"])
def test_calibration_mcmc_sites(fn, n):
    Q = _model(2) * 0.5 if n == 2 else synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0) * 0.5
    zs = _sites_calibration(getattr(api, fn), n, Q, init_segments=n)
    print(f"{fn} n={n}: max |z| = {zs.max():.2f} over {zs.size} columns")
    assert zs.max() < 5.0, zs


def test_calibration_ks_sweep_parity_observe():
    """The ks sweep reads x$states (here the per-site tips) as parity masks (src/phylomap.cpp:1838-1845): true states 1, 3 -> 1
    (odd), 2, 4 -> 2 -- simulate_4_state_tree's map."""
    Q = synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0) * 0.5
    zs = _sites_calibration(api.sumstatMCMCks_sweep, 4, Q, init_segments=4, observe=[1, 2, 1, 2], ks=True)
    print(f"ks sweep, parity tips: max |z| = {zs.max():.2f} over {zs.size} columns")
    assert zs.max() < 5.0, zs


def test_calibration_sumstat_exp():
    n, S, N = 4, 128, 64
    Q = synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0) * 0.5
    pid = np.full(n, 0.25)
    Om = 1.25 * float(np.max(np.abs(np.diag(Q))))
    z = synth.make_tree(40, Q, Om, 0xE4, pid, init_segments=n)
    tips, true = api.simulate_histories(z, Q, pid, S, seed=0xE5)
    cols_true = list(range(n)) + [n + a * n + c for a in range(n) for c in range(n) if a != c]
    cols_post = list(range(n)) + [_mcmc_count_col(n, a, c) for a in range(n) for c in range(n) if a != c]
    d = np.empty((S, len(cols_true)))
    for s in range(S):
        out = api.sumstatEXP(dict(z, states=tips[s]), Q, pid, N, seed=0xE6 + s)
        d[s] = out[:, cols_post].mean(axis=0) - true[s, cols_true]
    zs = _calibration_z(d)
    print(f"sumstatEXP: max |z| = {zs.max():.2f} over {zs.size} columns")
    assert zs.max() < 5.0, zs
