"""The exact sampler of histories over many rate matrices at 9..64 states without a device (phm_sample_histories_models_wide,
DESIGN.md section 24): where the symbol is declared and bound, every refusal of the entry point before its first device call, the
Python twin (tests/samplemodelsref.py) above 8 states against the exact conditional expectations, and the place where its
jump-count series first divides by 2^512.  No GPU needed.

|z| < 5 is a condition, not a measurement (tests/test_sample_models_cpu.py): the seeds are fixed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import exactref
import samplecases as sc
import samplemodelsref as ref
from phylomap_amd import _lib, api, synth
from test_sample_models_cpu import z_columns, z_nodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = "phm_sample_histories_models_wide"
NARROW = "phm_sample_histories_models"


@pytest.fixture(scope="module", autouse=True)
def one_blas_thread():
    try:
        import threadpoolctl
    except ImportError:
        yield
        return
    with threadpoolctl.threadpool_limits(limits=1):
        yield


def test_symbol_is_declared_apart_and_bound_like_the_narrow_one():
    L = _lib.load()
    assert hasattr(L, WIDE)
    assert _lib.EXT_EXPORTS == [WIDE] and WIDE not in _lib.EXPORTS
    assert L.phm_version() == 300
    assert list(getattr(L, WIDE).argtypes) == list(getattr(L, NARROW).argtypes)
    ext = open(os.path.join(ROOT, "include", "phylomap_hip_ext.h")).read()
    assert re.findall(r"\b(phm_[A-Za-z0-9_]+)\s*\(", ext) == [WIDE] and '#include "phylomap_hip.h"' in ext
    hdr = open(os.path.join(ROOT, "include", "phylomap_hip.h")).read()
    assert WIDE not in hdr
    assert "2..64 states" in api.sample_histories.__doc__


def _raw(z, Qs, pid, draws=2, n=None, S=2, observe=None, som=None, tree=True, q=True, prior=True, stats=True, ll=True,
         map_off="none", map_cap=0, fill=False, only=None):
    """one call of the wide entry point with 1-state-per-tip sites tiled S times -> (status, message)"""
    Qs = np.asarray(Qs, dtype=np.float64)
    K, nq = Qs.shape[0], Qs.shape[1]
    n = nq if n is None else n
    Qf = np.ascontiguousarray(Qs.transpose(0, 2, 1))
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    pt = _lib.PlainTree(z, np.tile(z["states"], (S, 1)))
    obs = None if observe is None else np.ascontiguousarray(observe, dtype=np.int32)
    so = None if som is None else np.ascontiguousarray(som, dtype=np.int32)
    o = _lib.make_options(n_replicas=S, tips_per_replica=True)
    H = K * S * max(draws, 1)
    res = np.zeros(H * nq * nq) if stats else None
    lik = np.zeros(K * S) if ll else None
    off = None if isinstance(map_off, str) else np.ascontiguousarray(map_off, dtype=np.int64)
    dw = np.zeros(max(map_cap, 1)) if fill and only != "state" else None
    ms = np.zeros(max(map_cap, 1), dtype=np.int32) if fill and only != "dwell" else None
    L = _lib.load()
    status = getattr(L, WIDE)(C.byref(pt.c) if tree else None, n, K, _lib._p(Qf if q else None, C.c_double),
                              _lib._p(pid if prior else None, C.c_double), pid.size // nq, _lib._p(obs, C.c_int32),
                              _lib._p(so, C.c_int32), draws, C.byref(o), _lib._p(res, C.c_double), _lib._p(lik, C.c_double), None,
                              _lib._p(off, C.c_int64), map_cap, _lib._p(dw, C.c_double), _lib._p(ms, C.c_int32))
    return status, L.phm_last_error().decode()


def test_refusals_need_no_device():
    L = _lib.load()
    z4, _, _, _ = synth.config_problem(2, n_tips=16)
    z = dict(z4, states=np.ones(16, dtype=np.int32))
    E = 30
    n = 9
    Q = sc.random_Q(n, 1)
    Qs = np.stack([Q, 2 * Q, 3 * Q])
    pid = np.full(n, 1 / n)
    for missing in ("tree", "q", "prior", "stats", "ll"):
        st, msg = _raw(z, Qs, pid, **{missing: False})
        assert st == 1 and msg.startswith(WIDE + ": NULL argument"), (missing, st, msg)
    for draws in (0, -3):
        st, msg = _raw(z, Qs, pid, draws=draws)
        assert st == 1 and msg.startswith(WIDE) and "draws" in msg
    Q8 = sc.random_Q(8, 1)
    st, msg = _raw(z, Q8[None], np.full(8, 1 / 8))
    assert st == 2 and msg.startswith(WIDE) and msg.endswith("go to " + NARROW)
    Q65 = sc.random_Q(65, 1)
    st, msg = _raw(z, Q65[None], np.full(65, 1 / 65))
    assert st == 1 and msg.startswith(WIDE)
    assert _raw(z, Qs, pid, n=1)[0] == 1
    bad = Qs.copy()
    bad[2, 0, 3], bad[2, 0, 1] = -0.05, bad[2, 0, 1] + 0.05                  # a negative rate in model 2
    st, msg = _raw(z, bad, pid)
    assert st == 1 and msg.startswith("model 2")
    assert _raw(z, Qs, pid, som=[0, 1, 2])[0] == 1                            # S = 2
    assert _raw(z, Qs, pid, observe=[1, 2, 1, 2, 1, 2, 1, 2, 10])[0] == 1
    zl = dict(z, **{"edge.length": z["edge.length"] * (40000.0 / (z["edge.length"].max() * np.max(-np.diag(Qs[1]))))})
    st, msg = _raw(zl, Qs, pid)                                               # model 0 stays below the limit, model 1 does not
    assert st == 2 and "model 1" in msg and "32768" in msg
    # the map arguments: phm_maps::validate's messages, under this entry point's name
    R = 3 * 2 * 2
    good = np.arange(R * E + 1, dtype=np.int64)
    cap = int(good[-1])
    st, msg = _raw(z, Qs, pid, map_off=np.r_[1, good[1:]], map_cap=cap, fill=True)
    assert st == 1 and msg.startswith(WIDE + ":") and "map_off[0]" in msg
    dec = good.copy()
    dec[5] = 3
    st, msg = _raw(z, Qs, pid, map_off=dec, map_cap=cap, fill=True)
    assert st == 1 and msg.startswith(WIDE + ":") and "row 4" in msg
    st, msg = _raw(z, Qs, pid, map_off=good, map_cap=cap - 1, fill=True)
    assert st == 1 and msg.startswith(WIDE + ":") and "map_cap" in msg
    st, msg = _raw(z, Qs, pid, map_off="none", map_cap=5, fill=True)          # segment arrays without offsets
    assert st == 1 and msg.startswith(WIDE + ":") and "map_off is NULL" in msg
    for only in ("dwell", "state"):
        st, msg = _raw(z, Qs, pid, map_off=good, map_cap=cap, fill=True, only=only)
        assert st == 1 and msg.startswith(WIDE + ":") and "both map_dwell and map_state" in msg
    if L.phm_device_count() == 0:                                              # a valid call gets as far as the device
        assert _raw(z, Qs, pid)[0] == 3
        assert _raw(z, Qs, pid, map_off=np.zeros(R * E + 1, dtype=np.int64))[0] == 3
        Q64 = sc.random_Q(64, 1)
        assert _raw(z, Q64[None], np.full(64, 1 / 64))[0] == 3


@pytest.mark.parametrize("n,D", [(9, 4096), (17, 2048)])
def test_twin_above_8_states_against_the_exact_expectations(n, D):
    edge, lens = sc.tree()
    Q = sc.random_Q(n, 1) * 4.0 / n
    pid = np.full(n, 1.0 / n)
    tips = sc.tips_for(edge, lens, Q, 5, None, 0.1)
    assert np.sum(tips == 0) == 2 and lens.min() == 0.0 and lens.max() == 6.0
    r = ref.sample_evaluation(edge, lens, Q, pid, tips, None, eval_id=0, D=D, seed=7 + n)
    want, ll, post = exactref.expected(edge, lens, Q, pid, tips[None], nodes=True)
    assert abs(r["loglik"] - ll[0]) < 1e-12 * abs(ll[0])
    zc = z_columns(r["stats"], want[0])
    zn = z_nodes(r["nodes"], post[0])
    print(f"n={n}: max |z| columns {zc.max():.2f}, nodes {zn.max():.2f}")
    assert zc.max() < 5.0
    assert zn.max() < 5.0


def test_rescaling_boundary_of_the_jump_count_series():
    # the device's long-branch case (mu t = 400) crosses the division by 2^512; mu t = 300 does not reach it
    Q = sc.random_Q(9, 1) * 4.0 / 9
    for x, R_want in ((300.0, 0), (400.0, 1)):
        M = ref.stop_index(x)
        _, _, beta = ref.model_table(Q, M)
        S, M_got, R = ref.jump_count_series(x, beta[:, [0, 3], [0, 5]])
        assert M_got == M and R == R_want, (x, M, M_got, R)
        assert np.all(S > 0.0) and np.all(np.isfinite(S))
