"""Forward simulation under many rate matrices without a device: every refusal of
phm_simulate_histories_models by status and message, the export, ``posterior.ppp`` on hand-computed numbers and the rows
``posterior.predictive`` simulates under.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from phylomap_amd import _lib, api, posterior, ratemodel, synth


def _raw(z, Qs, pid, R=2, n_pid=None, observe=None, tips=True, stats=True, map_off="none", map_cap=0, fill=False, **opt):
    """the C call with small output buffers where the checks must stop it first; (status, message)"""
    Qs = np.asarray(Qs, dtype=np.float64)
    K, n = Qs.shape[0], Qs.shape[1]
    Qf = np.ascontiguousarray(Qs.transpose(0, 2, 1))
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    pt = _lib.PlainTree(z)
    t, T = pt.c, pt.T
    obs = None if observe is None else np.ascontiguousarray(observe, dtype=np.int32)
    o = _lib.make_options(**opt)
    H = K * max(R, 1) if K * max(R, 1) < 4096 else 1                  # a refused call writes nothing
    tp = np.zeros((H, T), dtype=np.int32) if tips else None
    sb = np.zeros((H, n + n * n + 1), order="F") if stats else None
    off = None if isinstance(map_off, str) else np.ascontiguousarray(map_off, dtype=np.int64)
    dw = np.zeros(max(map_cap, 1)) if fill else None
    ms = np.zeros(max(map_cap, 1), dtype=np.int32) if fill else None
    L = _lib.load()
    status = L.phm_simulate_histories_models(C.byref(t), n, K, _lib._p(Qf, C.c_double), _lib._p(pid, C.c_double),
                                             pid.size // n if n_pid is None else n_pid, _lib._p(obs, C.c_int32), R, C.byref(o),
                                             _lib._p(tp, C.c_int32), None, _lib._p(sb, C.c_double), _lib._p(off, C.c_int64), map_cap,
                                             _lib._p(dw, C.c_double), _lib._p(ms, C.c_int32))
    return status, L.phm_last_error().decode()


def test_export_and_python_entry_point():
    L = _lib.load()
    assert "phm_simulate_histories_models" in _lib.EXPORTS and hasattr(L, "phm_simulate_histories_models")
    assert L.phm_version() == 300                                              # additive: the version stays
    assert callable(api.simulate_histories_models) and callable(posterior.predictive) and callable(posterior.ppp)


def test_c_abi_checks_need_no_device():
    z, Q, pid, _ = synth.config_problem(2, n_tips=16)
    Qs = np.stack([Q, 2 * Q, 3 * Q])
    E = 30
    assert _raw(z, Qs, pid, tips=False)[0] == 1                                # NULL outputs (only nodes and the maps may be NULL)
    assert _raw(z, Qs, pid, stats=False)[0] == 1
    # a bad model is named by its 0-based index
    bad = Qs.copy()
    bad[2, 0, 3], bad[2, 0, 1] = -0.05, bad[2, 0, 1] + 0.05                   # a negative rate in model 2
    st, msg = _raw(z, bad, pid)
    assert st == 1 and msg.startswith("model 2") and "off-diagonal" in msg
    bad = Qs.copy()
    bad[1, 2, 1] -= 0.01                                                       # a row of model 1 does not sum to 0
    st, msg = _raw(z, bad, pid)
    assert st == 1 and msg.startswith("model 1") and "row 3" in msg
    bad = Qs.copy()
    bad[0, 1, 1] = np.nan
    st, msg = _raw(z, bad, pid)
    assert st == 1 and msg.startswith("model 0")
    bad = Qs.copy()                                                            # leaves its state, but only by the 1e-12 slack: no target
    bad[1, 3] = [0.0, 0.0, 0.0, -1e-15]
    bad[1, 0, 0], bad[1, 0, 1] = -1e3, 1e3 - np.sum(Qs[1, 0, 2:])
    bad[1, 0, 2:] = Qs[1, 0, 2:]
    st, msg = _raw(z, bad, pid)
    assert st == 1 and msg.startswith("model 1") and "row 4" in msg and "no target" in msg
    # root priors: one shared column or one per model, each checked and named
    st, msg = _raw(z, Qs, np.tile(pid, 2), n_pid=2)
    assert st == 1 and "n_pid" in msg
    pids = np.tile(pid, (3, 1))
    pids[1] = 0.0
    st, msg = _raw(z, Qs, pids)
    assert st == 5 and msg.startswith("pid column 1")
    pids[1] = [0.5, -0.1, 0.3, 0.3]
    st, msg = _raw(z, Qs, pids)
    assert st == 5 and msg.startswith("pid column 1")
    # replicates, reduce, the replica word
    st, msg = _raw(z, Qs, pid, R=0)
    assert st == 1 and "replicates" in msg
    assert _raw(z, Qs, pid, R=-4)[0] == 1
    st, msg = _raw(z, Qs, pid, reduce=True)
    assert st == 1 and "reduce" in msg
    st, msg = _raw(z, Qs[:2], pid, R=2 ** 30 + 1, replica_offset=2 ** 31 - 1)  # 2^31 - 1 + 2^31 + 2 = 2^32 + 1
    assert st == 1 and "replica word" in msg and str(2 ** 32 + 1) in msg
    if _lib.load().phm_device_count() == 0:                                    # 2^32 - 2 fits: the call gets as far as the device
        st, msg = _raw(z, Qs[:1], pid, R=2 ** 31 - 1, replica_offset=2 ** 31 - 1)
        assert st == 3 and "replica word" not in msg
    # tree, observe, state count
    assert _raw(z, Qs, pid, observe=[1, 2, 1, 5])[0] == 1
    zb = dict(z, **{"edge.length": z["edge.length"].copy()})
    zb["edge.length"][3] = -1.0
    st, msg = _raw(zb, Qs, pid)
    assert st == 1 and "edge row 4" in msg
    zb = dict(z, edge=z["edge"].copy())
    zb["edge"][5, 1] = zb["edge"][6, 1]                                        # a node with two parents
    st, msg = _raw(zb, Qs, pid)
    assert st == 1 and msg.startswith("tree:")
    assert _raw(z, np.zeros((1, 1, 1)), [1.0])[0] == 1                         # n < 2
    Q65 = synth.dense_Q(65, 0.01, 0.02)
    assert _raw(z, Q65[None], np.ones(65))[0] == 1                             # n > 64
    # the map_off checks are section 14's, with R = H
    H = 3 * 2
    good = np.arange(H * E + 1, dtype=np.int64)
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
    st, msg = _raw(z, Qs, pid, map_off=good, map_cap=int(good[-1]), fill=False)
    assert st in (0, 3)                                                        # a sizing call: the offsets are only written
    if _lib.load().phm_device_count() == 0:                                    # a valid call gets as far as the device
        assert _raw(z, Qs, pid)[0] == 3
        assert _raw(z, Qs, np.tile(pid, (3, 1)))[0] == 3
        assert _raw(z, Qs, pid, map_off=np.zeros(H * E + 1, dtype=np.int64))[0] == 3
        with pytest.raises(_lib.PhmError) as e:
            api.simulate_histories_models(z, Qs, pid, 2)
        assert e.value.status == 3


def test_python_wrapper_checks_its_shapes():
    z, Q, pid, _ = synth.config_problem(2, n_tips=16)
    with pytest.raises(ValueError):
        api.simulate_histories_models(z, np.zeros((3, 4, 5)), pid, 1)
    with pytest.raises(ValueError):
        api.simulate_histories_models(z, np.stack([Q, Q, Q]), np.tile(pid, (2, 1)), 1)
    with pytest.raises(ValueError):
        api.simulate_histories_models(z, Q, pid, 1, observe=[1, 2])


def test_ppp_on_hand_computed_numbers():
    # 2 of 5 above, 1 tie: 2/5 + 1/10
    assert posterior.ppp(3.0, [1.0, 2.0, 3.0, 4.0, 5.0]) == 0.5
    assert posterior.ppp(3.0, [1.0, 3.0, 3.0, 3.0, 5.0, 6.0, 7.0, 0.0]) == 3 / 8 + 0.5 * 3 / 8
    assert posterior.ppp(10.0, [1, 2, 3]) == 0.0 and posterior.ppp(0.0, [1, 2, 3]) == 1.0
    assert posterior.ppp(2, [2, 2, 2, 2]) == 0.5                               # all ties
    assert posterior.ppp(1.5, np.array([[1.0, 2.0], [2.0, 1.0]])) == 0.5       # any shape of replicates
    with pytest.raises(ValueError):
        posterior.ppp(1.0, [])


def test_predictive_row_selection_with_a_stubbed_device_call(monkeypatch):
    model = ratemodel.ard(2)
    rows, chains, p = 7, 3, model.p
    theta = 1.0 + np.arange(rows * chains * p, dtype=np.float64).reshape(rows, chains, p)
    result = dict(theta=theta, model=model)
    z = {"edge": np.zeros((4, 2), dtype=np.int32), "edge.length": np.ones(4), "Nnode": 2}
    seen = {}

    def stub(z_, Qs, pid, R, observe=None, **opt):
        seen.update(Qs=np.array(Qs), pid=pid, R=R, observe=observe, opt=opt)
        K = Qs.shape[0]
        tips = np.arange(K * 3, dtype=np.int32).reshape(K, 1, 3)
        stats = np.arange(K * 7, dtype=np.float64).reshape(K, 1, 7)
        return tips, stats

    monkeypatch.setattr(api, "simulate_histories_models", stub)
    # burn, then every chain of every kept row, row-major: row 2 chain 0, row 2 chain 1, ...
    r = posterior.predictive(result, z, [0.5, 0.5], burn=2, observe=[1, 2], seed=9, replica_offset=5)
    want = theta[2:].reshape(-1, p)
    assert r["theta"].shape == (15, p) and np.array_equal(r["theta"], want)
    assert np.array_equal(r["theta"][1], theta[2, 1]) and np.array_equal(r["theta"][3], theta[3, 0])
    assert seen["R"] == 1 and seen["observe"] == [1, 2] and seen["opt"] == dict(seed=9, replica_offset=5)
    assert np.array_equal(seen["Qs"], posterior.rate_matrices(model, want))
    assert r["tips"].shape == (15, 3) and np.array_equal(r["tips"][4], [12, 13, 14])
    assert r["stats"].shape == (15, 7) and r["stats"][2, 0] == 14.0
    # thinning: M of N rows, evenly, rows (j N) // M
    r = posterior.predictive(result, z, [0.5, 0.5], burn=2, draws=4)
    assert np.array_equal(r["theta"], want[[0, 3, 7, 11]])
    r = posterior.predictive(result, z, [0.5, 0.5], burn=0, draws=21)
    assert np.array_equal(r["theta"], theta.reshape(-1, p))                    # every row: no thinning left
    r = posterior.predictive(result, z, [0.5, 0.5], burn=6, draws=1)
    assert np.array_equal(r["theta"], theta[6, :1])
    assert np.array_equal(posterior.predictive_rows(result, 2, 4), want[[0, 3, 7, 11]])
    # a per-site result [rows, S, chains, p] flattens the same way
    ps = dict(theta=theta.reshape(rows, 1, chains, p), model=model)
    assert np.array_equal(posterior.predictive(ps, z, [0.5, 0.5], burn=2)["theta"], want)
    for kw in (dict(burn=7), dict(draws=0), dict(burn=2, draws=16)):
        with pytest.raises(ValueError):
            posterior.predictive(result, z, [0.5, 0.5], **kw)
    failed = dict(theta=theta.copy(), model=model)
    failed["theta"][4:, 1] = np.nan
    with pytest.raises(ValueError):
        posterior.predictive(failed, z, [0.5, 0.5])
