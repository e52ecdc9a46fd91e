"""ctypes front end to the device-block harness (tests/native/device_blocks.hip -> build/tests/libphm_device_blocks.so).
TEST INFRASTRUCTURE ONLY.  Lazy: importing this module loads nothing; the library (and with it the HIP runtime) is opened by
the first call, so collecting the tests leaves the GPU untouched."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO_PATH = os.path.join(_ROOT, "build", "tests", "libphm_device_blocks.so")

_u32p, _i32p, _f64p, _u64p, _u8p = (C.POINTER(t) for t in (C.c_uint32, C.c_int32, C.c_double, C.c_uint64, C.c_uint8))
_int, _u32, _f64 = C.c_int, C.c_uint32, C.c_double

# every entry the harness exports, with its argument types (all return the hipError_t as an int; -1 = refused arguments)
ENTRIES = {
    "phmtb_philox": [_u32p, _u32p, _u32p, _int],
    "phmtb_u01": [_u32p, _f64p, _int],
    "phmtb_stream": [_u32, _u32, _u32p, _u32p, _u32p, _u32p, _int, _u32p, _f64p, _u32p, _f64p, _int],
    "phmtb_neglog": [_u32p, _f64p, _f64p, _int],
    "phmtb_log": [_f64p, _f64p, _int],
    "phmtb_exp": [_f64p, _f64p, _int],
    "phmtb_matvec_u": [_int, _f64p, _f64p, _f64p, _int],
    "phmtb_sample_cat": [_int, _f64p, _f64p, _i32p, _u32p, _int],
    "phmtb_matvec": [_int, _int, _int, _f64p, _i32p, _f64p, _int, _f64p, _f64p, _f64p, _f64p, _int],
    "phmtb_shift": [_u64p, _u64p, _u64p, _int],
    "phmtb_readlane": [_u64p, _int, _u64p, _int],
    "phmtb_coop_sum": [_f64p, _int, _f64p, _int],
    "phmtb_coop_sample": [_int, _int, _f64p, _f64p, _i32p, _u32p, _int],
    "phmtb_wave_max": [_int, _i32p, _i32p, _int],
    "phmtb_statlanes": [_int, _int, _int, _int, _i32p, _f64p, _i32p, _i32p, _u8p, _int, _f64, _f64, _u64p, _u32p, _f64p, _int],
    "phmtb_ll_rescale": [_int, _f64p, _f64p, _i32p, _int],
    "phmtb_model": [_int, _f64p, _f64p, _f64p, _int],
}

_PTR_DTYPE = {_u32p: np.uint32, _i32p: np.int32, _f64p: np.float64, _u64p: np.uint64, _u8p: np.uint8}
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(SO_PATH)
        for name, argtypes in ENTRIES.items():
            fn = getattr(L, name)
            fn.restype = C.c_int
            fn.argtypes = argtypes
        _lib = L
    return _lib


def _call(name, *args):
    """Arrays must already be C-contiguous and of the entry's dtype (outputs are written in place)."""
    conv = []
    for a, t in zip(args, ENTRIES[name]):
        if t in _PTR_DTYPE:
            assert isinstance(a, np.ndarray) and a.dtype == _PTR_DTYPE[t] and a.flags.c_contiguous, (name, t)
            conv.append(a.ctypes.data_as(t))
        else:
            conv.append(a)
    assert len(conv) == len(ENTRIES[name])
    rc = getattr(lib(), name)(*conv)
    if rc != 0:
        raise RuntimeError(f"{name} returned {rc}")


def _in(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def philox(ctr, key):
    ctr, key = _in(ctr, np.uint32).reshape(-1, 4), _in(key, np.uint32).reshape(-1, 2)
    out = np.zeros_like(ctr)
    _call("phmtb_philox", ctr, key, out, len(ctr))
    return out


def u01(x):
    x = _in(x, np.uint32)
    out = np.zeros(x.size)
    _call("phmtb_u01", x, out, x.size)
    return out


def stream(seed_lo, seed_hi, rep, it, ent, dseq):
    """-> (draw_word, draw, stream_word, stream_u), each [lane, position in dseq]"""
    rep, it, ent, dseq = (_in(a, np.uint32) for a in (rep, it, ent, dseq))
    N, nd = rep.size, dseq.size
    wk, wf = np.zeros((N, nd), np.uint32), np.zeros((N, nd), np.uint32)
    uk, uf = np.zeros((N, nd)), np.zeros((N, nd))
    _call("phmtb_stream", seed_lo, seed_hi, rep, it, ent, dseq, nd, wk, uk, wf, uf, N)
    return wk, uk, wf, uf


def neglog(k):
    """-> (table in LDS, table in global memory)"""
    k = _in(k, np.uint32)
    a, b = np.zeros(k.size), np.zeros(k.size)
    _call("phmtb_neglog", k, a, b, k.size)
    return a, b


def log(x):
    x = _in(x, np.float64)
    out = np.zeros(x.size)
    _call("phmtb_log", x, out, x.size)
    return out


def exp(x):
    x = _in(x, np.float64)
    out = np.zeros(x.size)
    _call("phmtb_exp", x, out, x.size)
    return out


def matvec_u(M, v):
    M, v = _in(M, np.float64), _in(v, np.float64)
    N, ns = v.shape
    assert M.shape == (N, ns, ns)
    out = np.zeros_like(v)
    _call("phmtb_matvec_u", ns, M, v, out, N)
    return out


def sample_cat(p, u):
    p, u = _in(p, np.float64), _in(u, np.float64)
    N, ns = p.shape
    idx, err = np.zeros(N, np.int32), np.zeros(N, np.uint32)
    _call("phmtb_sample_cat", ns, p, u, idx, err, N)
    return idx, err


FORMS = {"coop_matvec": 0, "coop_matvec_lds": 1, "coop_matvec_regs": 2, "coop_matvec_ell": 3, "coop_matvec_band1": 4,
         "coop_matvec_band2": 5}


def matvec(form, n, vin, M=None, ldn=0, ecol=None, eval_=None, coef=None):
    """-> (f(v), f(f(v))), each [wave, lane]; M is [n, ldn] (forms 0-2), ecol / eval_ [n, w] (form 3), coef [64, 5] (bands)"""
    vin = _in(vin, np.float64)
    nw = vin.shape[0]
    assert vin.shape == (nw, 64)
    M = _in(M if M is not None else np.zeros(1), np.float64)
    ecol = _in(ecol if ecol is not None else np.zeros((1, 1)), np.int32)
    eval_ = _in(eval_ if eval_ is not None else np.zeros((1, 1)), np.float64)
    coef = _in(coef if coef is not None else np.zeros((64, 5)), np.float64)
    assert coef.shape == (64, 5) and ecol.shape == eval_.shape
    if FORMS[form] <= 2:
        assert M.shape == (n, ldn)
    if FORMS[form] == 3:
        assert ecol.shape[0] == n
    o1, o2 = np.zeros((nw, 64)), np.zeros((nw, 64))
    _call("phmtb_matvec", FORMS[form], n, ldn, M, ecol, eval_, ecol.shape[1], coef, vin, o1, o2, nw)
    return o1, o2


def shift(bits):
    """-> (wave_from_below, wave_from_above) of [wave, lane] uint64 bit patterns"""
    bits = _in(bits, np.uint64)
    nw = bits.shape[0]
    assert bits.shape == (nw, 64)
    lo, hi = np.zeros_like(bits), np.zeros_like(bits)
    _call("phmtb_shift", bits, lo, hi, nw)
    return lo, hi


def readlane(bits, n):
    """-> [wave, l, lane]: what each lane received from readlane_f64(v, l), l < n"""
    bits = _in(bits, np.uint64)
    nw = bits.shape[0]
    assert bits.shape == (nw, 64)
    out = np.zeros((nw, n, 64), np.uint64)
    _call("phmtb_readlane", bits, n, out, nw)
    return out


def coop_sum(x, n):
    x = _in(x, np.float64)
    nw = x.shape[0]
    assert x.shape == (nw, 64)
    out = np.zeros((nw, 64))
    _call("phmtb_coop_sum", x, n, out, nw)
    return out


def coop_sample(which, n, p, u):
    """which: 'coop_sample' | 'coop_sample_lds' -> (index, error bits), each [wave, lane]"""
    p, u = _in(p, np.float64), _in(u, np.float64)
    nw = p.shape[0]
    assert p.shape == (nw, 64) and u.shape == (nw,)
    idx, err = np.zeros((nw, 64), np.int32), np.zeros((nw, 64), np.uint32)
    _call("phmtb_coop_sample", {"coop_sample": 0, "coop_sample_lds": 1}[which], n, p, u, idx, err, nw)
    return idx, err


def wave_max(which, v):
    """which: 'count' | 'w' | 'min_idiom'"""
    v = _in(v, np.int32)
    nw = v.shape[0]
    assert v.shape == (nw, 64)
    out = np.zeros((nw, 64), np.int32)
    _call("phmtb_wave_max", {"count": 0, "w": 1, "min_idiom": 2}[which], v, out, nw)
    return out


def statlanes(ns, n, ncount, dcol, dx, ccol, cell, live, ncell, fx_scale, fx_inv, dw_init, ct_init):
    """-> (dwell cells [n, ncell] uint64, count cells [ncount, ncell] uint32, stat_cell_value [n + ncount, ncell])"""
    dcol, ccol, cell = (_in(a, np.int32) for a in (dcol, ccol, cell))
    dx, live = _in(dx, np.float64), _in(live, np.uint8)
    N, nseg = dcol.shape
    assert dx.shape == ccol.shape == (N, nseg) and cell.shape == live.shape == (N,)
    dw, ct = np.array(dw_init, dtype=np.uint64, order="C"), np.array(ct_init, dtype=np.uint32, order="C")
    assert dw.shape == (n, ncell) and ct.shape == (ncount, ncell)
    vals = np.zeros((n + ncount, ncell))
    _call("phmtb_statlanes", ns, n, ncount, nseg, dcol, dx, ccol, cell, live, ncell, float(fx_scale), float(fx_inv), dw, ct, vals, N)
    return dw, ct, vals


def ll_rescale(V):
    """V [vector, n], n = 2 .. 8 -> (rescaled vectors, exponents): ll_rescale<n> reached through ll_with_states"""
    V = _in(V, np.float64)
    cnt, n = V.shape
    out, e = np.zeros_like(V), np.zeros(cnt, np.int32)
    _call("phmtb_ll_rescale", n, V, out, e, cnt)
    return out, e


def model(Qs):
    """Qs [K, n, n] -> (mu [K], B [K, n, n]): model_mu and model_b on the model-fastest layout of the lane kernels"""
    Qs = _in(Qs, np.float64)
    K, n, _ = Qs.shape
    q = np.ascontiguousarray(Qs.reshape(K, n * n).T)
    mu, B = np.zeros(K), np.zeros_like(q)
    _call("phmtb_model", n, q, mu, B, K)
    return mu, np.ascontiguousarray(B.T).reshape(K, n, n)
