"""Forward simulation under many rate matrices on the device (phm_simulate_histories_models): every history
against the Python twin of the one-model simulator (tests/simref.py) at its global replica word and against
``api.simulate_histories`` itself, model by model -- tips, nodes, counts, root state and maps bit for bit, the fixed-point dwell
sums within 1e-12 of the tree length; model boundaries at lane 0, in mid-wave and nowhere; chunks and devices that change no bit;
the two-phase maps contract; the capacity error; closed forms at 4 096 replicates; ``posterior.predictive`` end to end."""
import ctypes as C

import numpy as np
import pytest

import mapsref
import samplecases as sc
import simref
from phylomap_amd import _lib, api, posterior, ratemodel, synth

pytestmark = pytest.mark.gpu

KR = [(1, 1), (1, 130), (63, 1), (65, 1), (130, 1), (3, 70), (7, 10), (2, 64)]


def _z(shuffle=False):
    edge, lens = sc.tree(shuffle=shuffle)                            # 24 tips, a zero-length branch and one of length 6
    return {"edge": edge, "edge.length": lens, "Nnode": edge.shape[0] // 2}


def _models(n, K, seed):
    """K different generators of n states"""
    if n <= 8:
        return np.stack([sc.random_Q(n, seed + k, 0.4 + 0.15 * (k % 5)) for k in range(K)])
    base = synth.tridiagonal_Q(20, 0.4) if n == 20 else synth.dense_Q(n, 0.01, 0.04)
    return np.stack([base * (1.0 + 0.5 * k) for k in range(K)])


def _pids(n, K, per_model, seed):
    if not per_model:
        return np.arange(1.0, n + 1.0)
    return np.random.default_rng(seed).uniform(0.1, 1.0, (K, n))


def _row_check(m, lens):
    """every map row sums to its branch length"""
    sums = np.add.reduceat(m.dwell, m.off[:-1]).reshape(m.n_hist, m.n_edge)
    assert np.all(np.diff(m.off) >= 1)
    assert np.all(np.abs(sums - lens[None, :]) <= 1e-12 * lens[None, :])


def _check(z, Qs, pids, R, seed, off=0, observe=None, device_twin=True, twin_rows=None, **opt):
    """the batched call against simref.simulate and api.simulate_histories, model by model; ``twin_rows``: the (first replica,
    count) ranges of every model that the Python twin visits (None: all R) -- the device twin always visits them all"""
    Qs = np.asarray(Qs)
    K, n = Qs.shape[0], Qs.shape[1]
    edge, lens = z["edge"], np.asarray(z["edge.length"])
    E, T = edge.shape[0], edge.shape[0] // 2 + 1
    tol = 1e-12 * float(lens.sum())
    tips, stats, nodes, m = api.simulate_histories_models(z, Qs, pids, R, observe=observe, nodes=True, maps=True, seed=seed,
                                                          replica_offset=off, **opt)
    assert tips.shape == (K, R, T) and stats.shape == (K, R, n + n * n + 1) and nodes.shape == (K, R, 2 * T - 1)
    assert m.n_hist == K * R and m.n_edge == E
    _row_check(m, lens)
    pids2 = np.atleast_2d(pids)
    worst = 0.0
    for k in range(K):
        pid = pids2[k if pids2.shape[0] > 1 else 0]
        for r0, cnt in ([(0, R)] if twin_rows is None else twin_rows):
            wt, ws, wn = simref.simulate(edge, lens, Qs[k], pid, cnt, seed, replica_offset=off + k * R + r0, observe=observe)
            rows = slice(r0, r0 + cnt)
            assert np.array_equal(tips[k][rows], wt), k
            assert np.array_equal(nodes[k][rows], wn), k
            assert np.array_equal(stats[k][rows, n:], ws[:, n:]), k     # counts and the root column
            worst = max(worst, float(np.max(np.abs(stats[k][rows, :n] - ws[:, :n]))))
        if device_twin:
            dt, ds, dn, dm = api.simulate_histories(z, Qs[k], pid, R, observe=observe, nodes=True, maps=True, seed=seed,
                                                    replica_offset=off + k * R)
            assert np.array_equal(tips[k], dt) and np.array_equal(nodes[k], dn) and np.array_equal(stats[k][:, n:], ds[:, n:])
            worst = max(worst, float(np.max(np.abs(stats[k][:, :n] - ds[:, :n]))))
            r0, r1 = k * R * E, (k + 1) * R * E
            lo, hi = m.off[r0], m.off[r1]
            assert np.array_equal(m.off[r0:r1 + 1] - lo, dm.off), k
            assert np.array_equal(m.state[lo:hi], dm.state), k
            assert np.array_equal(m.dwell[lo:hi], dm.dwell), k
    print(f"n={n} K={K} R={R}: max |dwell - twin| = {worst:.3e} (bound {tol:.3e})")
    assert worst <= tol
    return tips, stats, nodes, m


@pytest.mark.parametrize("kr", range(len(KR)), ids=[f"K{k}-R{r}" for k, r in KR])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8])
def test_against_both_twins(n, kr):
    K, R = KR[kr]
    # the grid alternates pre-ordered / shuffled edge tables, shared / per-model pid and zero / non-zero replica_offset
    z = _z(shuffle=bool((kr + n) % 2))
    pids = _pids(n, K, bool((kr // 2 + n) % 2), 50 + n)
    _check(z, _models(n, K, 100 * n + kr), pids, R, seed=1000 * n + kr, off=(0 if kr % 3 else 12345 + n))


@pytest.mark.parametrize("K,R", [(2, 3), (1, 65)])
@pytest.mark.parametrize("n", [20, 61, 64])
def test_against_both_twins_wide(n, K, R):
    z = _z(shuffle=(R == 3))
    _check(z, _models(n, K, 0), _pids(n, K, K > 1, 60 + n), R, seed=77 * n + R, off=(9 if K > 1 else 0))


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("per_model", [False, True])
def test_edge_table_orders_and_pid_modes(shuffle, per_model):
    z = _z(shuffle)
    assert np.min(z["edge.length"]) == 0.0
    _check(z, _models(4, 3, 7), _pids(4, 3, per_model, 8), 70, seed=31, off=1 << 20)


def test_maps_against_the_maps_twin():
    z = _z(True)
    Qs, pids = _models(3, 7, 5), _pids(3, 7, True, 6)
    _, _, _, m = _check(z, Qs, pids, 10, seed=8, off=100, device_twin=False)
    E = m.n_edge
    for k in (0, 6):
        off, dwell, state = mapsref.simulate(z["edge"], z["edge.length"], Qs[k], pids[k], 10, 8, replica_offset=100 + 10 * k)[3]
        lo, hi = m.off[k * 10 * E], m.off[(k + 1) * 10 * E]
        assert np.array_equal(m.off[k * 10 * E:(k + 1) * 10 * E + 1] - lo, off)
        assert np.array_equal(m.state[lo:hi], state) and np.array_equal(m.dwell[lo:hi], dwell)


def test_hidden_rates_through_observe():
    Qs = np.stack([sc.hidden_Q(s) for s in (0.5, 1.0, 1.5, 2.0, 3.0)])
    tips, _, nodes, _ = _check(_z(), Qs, np.full(4, 0.25), 30, seed=4, observe=sc.PARITY)
    assert set(np.unique(tips)) <= {1, 2} and np.array_equal(tips, np.asarray(sc.PARITY)[nodes[:, :, :24] - 1])
    assert len(np.unique(nodes)) == 4


def test_absorbing_and_zero_models_share_a_wave_with_ordinary_ones():
    z = _z()
    lens = z["edge.length"]
    Qa = np.array([[-0.5, 0.5, 0.0], [0.0, 0.0, 0.0], [0.2, 0.3, -0.5]])          # state 2 absorbs
    Qs = np.stack([sc.random_Q(3, 1), Qa, np.zeros((3, 3)), sc.random_Q(3, 2), Qa * 4.0, sc.random_Q(3, 3)])
    pids = np.tile([1.0, 0.5, 1.0], (6, 1))
    _, stats, nodes, m = _check(z, Qs, pids, 20, seed=5)                           # 120 histories: models 0 .. 3 in the first wave
    assert np.all(stats[[1, 4]][:, :, 6:9] == 0.0)                                 # no jump out of the absorbing state
    assert np.all(stats[2][:, 3:12] == 0.0)                                        # Q = 0: no jump at all,
    assert np.all(m.counts()[40:60] == 1)                                          # one segment per branch,
    root = stats[2][:, 12].astype(int)
    assert np.all(nodes[2] == root[:, None] + 1)                                   # the root's state everywhere,
    assert np.array_equal(stats[2][np.arange(20), root], np.full(20, stats[2][0, root[0]]))
    assert np.all(np.abs(stats[2][np.arange(20), root] - lens.sum()) <= 1e-12 * lens.sum())
    assert np.any(m.counts()[:40] > 1) and np.any(m.counts()[60:80] > 1)


def _same(a, b):
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert np.array_equal(a[3].off, b[3].off) and np.array_equal(a[3].state, b[3].state) and np.array_equal(a[3].dwell, b[3].dwell)


@pytest.mark.parametrize("n,K,R", [(4, 3, 70), (8, 3, 70), (4, 130, 1)])
def test_chunks_and_devices_change_no_bit(n, K, R):
    z = _z(True)
    Qs, pids = _models(n, K, 3), _pids(n, K, True, 4)
    kw = dict(nodes=True, maps=True, seed=21, replica_offset=5)
    base = api.simulate_histories_models(z, Qs, pids, R, **kw)
    for opt in (dict(expect_chunk=64), dict(expect_chunk=2), dict(devices=[0, 0]), dict(devices=[0, 0], expect_chunk=64)):
        _same(base, api.simulate_histories_models(z, Qs, pids, R, **kw, **opt))
    plain = api.simulate_histories_models(z, Qs, pids, R, seed=21, replica_offset=5, expect_chunk=2)      # no nodes, no maps
    assert np.array_equal(plain[0], base[0]) and np.array_equal(plain[1], base[1])
    api.simulate_histories_models(z, Qs[:1], pids[:1], 1, seed=1)                  # expect_chunk back to its default


def _raw(z, Qs, pid, R, seed, off=None, cap=0, dwell=None, state=None):
    Qs = np.asarray(Qs, dtype=np.float64)
    K, n = Qs.shape[0], Qs.shape[1]
    Qf = np.ascontiguousarray(Qs.transpose(0, 2, 1))
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    pt = _lib.PlainTree(z)
    t, T = pt.c, pt.T
    o = _lib.make_options(seed=seed)
    H = K * R
    tips = np.zeros((H, T), dtype=np.int32)
    nodes = np.zeros((H, 2 * T - 1), dtype=np.int32)
    stats = np.zeros((H, n + n * n + 1), order="F")
    L = _lib.load()
    st = L.phm_simulate_histories_models(C.byref(t), n, K, _lib._p(Qf, C.c_double), _lib._p(pid, C.c_double), 1, None, R, C.byref(o),
                                         _lib._p(tips, C.c_int32), _lib._p(nodes, C.c_int32), _lib._p(stats, C.c_double),
                                         _lib._p(off, C.c_int64), cap, _lib._p(dwell, C.c_double), _lib._p(state, C.c_int32))
    return st, L.phm_last_error().decode(), (tips, nodes, stats)


def test_two_phase_maps_contract():
    z = _z()
    E = z["edge"].shape[0]
    Qs, pid, R = _models(4, 3, 9), np.ones(4), 50
    H = 3 * R
    off = np.full(H * E + 1, -7, dtype=np.int64)
    st, msg, sized = _raw(z, Qs, pid, R, 13, off=off)
    assert st == 0, msg
    assert off[0] == 0 and np.all(np.diff(off) >= 1)
    total = int(off[-1])
    dwell, state = np.full(total + 2, -1.0), np.full(total + 2, -9, dtype=np.int32)      # two guard elements
    st, msg, filled = _raw(z, Qs, pid, R, 13, off=off, cap=total, dwell=dwell, state=state)
    assert st == 0, msg
    for a, b in zip(sized, filled):
        assert np.array_equal(a, b)                                                # the other outputs: bit-identical
    st, msg, plain = _raw(z, Qs, pid, R, 13)
    assert st == 0, msg
    for a, b in zip(sized, plain):
        assert np.array_equal(a, b)
    assert np.all(dwell[total:] == -1.0) and np.all(state[total:] == -9) and np.all(state[:total] >= 1) and np.all(dwell[:total] >= 0.0)
    row = 71 * E + 5                                                               # history 71 (model 1), edge row 6: one segment short
    bad = off.copy()
    bad[row + 1:] -= 1
    assert bad[row + 1] >= bad[row]
    st, msg, _ = _raw(z, Qs, pid, R, 13, off=bad, cap=total, dwell=dwell.copy(), state=state.copy())
    assert st == 1 and f"row {row} " in msg and "history 71" in msg and "edge row 6" in msg, msg


def test_capacity_names_the_model():
    z = _z()
    lens = np.full(46, 0.01)
    lens[5] = 2.0
    zl = dict(z, **{"edge.length": lens})
    slow = np.array([[-0.6, 0.6], [0.9, -0.9]])
    fast = np.array([[-1e4, 1e4], [1e4, -1e4]])                                    # ~2e4 jumps on the branch of length 2
    with pytest.raises(_lib.PhmError) as e:
        api.simulate_histories_models(zl, np.stack([slow, fast, slow]), [1.0, 1.0], 40, seed=1)
    assert e.value.status == 6 and "model 1:" in str(e.value) and "edge row 6" in str(e.value), str(e.value)
    with pytest.raises(simref.JumpCapError):
        simref.simulate(zl["edge"], lens, fast, [1.0, 1.0], 40, 1, replica_offset=40)
    _check(zl, np.stack([slow, slow * 2, slow]), [1.0, 1.0], 40, seed=1)           # the device is still usable, the others are fine


def test_three_models_against_closed_forms():
    edge, lens = synth.random_tree(40, 1.0, 0x40)
    z = {"edge": edge, "edge.length": lens, "Nnode": 39}
    Qs = np.stack([synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0) * 0.5, sc.random_Q(4, 11, 0.6), sc.hidden_Q(1.5)])
    pid = np.array([0.4, 0.3, 0.2, 0.1])
    tips, stats = api.simulate_histories_models(z, Qs, pid, 4096, seed=0x22)
    for k in range(3):
        zs = simref.zscores(tips[k], stats[k], edge, lens, Qs[k], pid)
        print(f"model {k}: max |z| = {zs.max():.2f} over {zs.size} quantities")
        assert zs.max() < 5.0, (k, zs.max())
        assert np.all(np.abs(stats[k][:, :4].sum(axis=1) - lens.sum()) <= 1e-12 * lens.sum())


def test_posterior_predictive_end_to_end():
    model = ratemodel.ard(2)
    Q = model.Q([0.4, 0.7])
    pid = np.array([0.5, 0.5])
    z = synth.make_tree(40, Q, 1.0, 0xAB, pid)
    res = api.posterior_rates(z, model, pid, [1.0, 1.0], 20, chains=4, seed=3)
    assert res["theta"].shape == (20, 4, 2)
    pp = posterior.predictive(res, z, pid, burn=5, seed=0x77, replica_offset=3)
    assert pp["theta"].shape == (60, 2) and pp["tips"].shape == (60, 40) and pp["stats"].shape == (60, 7)
    assert np.array_equal(pp["theta"], res["theta"][5:].reshape(60, 2))
    Qs = posterior.rate_matrices(model, pp["theta"])
    for m in range(60):
        wt, ws, _ = simref.simulate(z["edge"], z["edge.length"], Qs[m], pid, 1, 0x77, replica_offset=3 + m)
        assert np.array_equal(pp["tips"][m], wt[0]), m
        assert np.array_equal(pp["stats"][m, 2:], ws[0, 2:]), m
    thin = posterior.predictive(res, z, pid, burn=5, draws=7, seed=0x77)
    assert np.array_equal(thin["theta"], pp["theta"][(np.arange(7) * 60) // 7]) and thin["tips"].shape == (7, 40)
    t_obs = float(np.sum(np.asarray(z["states"]) == 2))
    p = posterior.ppp(t_obs, np.sum(pp["tips"] == 2, axis=1))
    assert 0.0 <= p <= 1.0
