"""References for the device building blocks (tests/test_gpu_device_blocks.py), transcribed from DESIGN.md section 2 and not from
the device headers.  Plain Python on IEEE doubles (Python floats) and integers; the one vectorised twin, fused_chain_np, exists
because 64 vectors at 64 states are half a million fused multiply-adds, and tests/test_device_blocks_cpu.py holds it to the
plain definition on every product the GPU cases use."""
from __future__ import annotations

import ctypes as C
import ctypes.util
import math
from fractions import Fraction

import numpy as np

DERR_ZERO_PROB = 1
ENT_NODE, ENT_BSTATE, ENT_BEXP, ENT_BUNIF = 0, 1 << 30, 2 << 30, 3 << 30


# ---- fused multiply-add --------------------------------------------------------------------------------------------------
def fma(a: float, b: float, c: float) -> float:
    """a * b + c with ONE rounding: exact rational arithmetic, then the correctly rounded int / int division of float().
    An exact zero takes IEEE's sign: -0 only when the product and c are both -0 (round to nearest)."""
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        prod_neg = (math.copysign(1.0, a) * math.copysign(1.0, b)) < 0
        exact_zero_product = a == 0 or b == 0
        if exact_zero_product and prod_neg and c == 0 and math.copysign(1.0, c) < 0:
            return -0.0
        return 0.0
    return float(r)


_libm = None


def libm_fma(a: float, b: float, c: float) -> float:
    global _libm
    if _libm is None:
        _libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.fma.restype = C.c_double
        _libm.fma.argtypes = [C.c_double] * 3
    return _libm.fma(a, b, c)


def fused_chain(row, v, order=None, fma_fn=fma) -> float:
    """acc = +0; for j ascending: acc = fma(M[c][j], v[j], acc)  (mat-vec of the MCMC chains, n > 4)"""
    acc = 0.0
    for j in (range(len(row)) if order is None else order):
        acc = fma_fn(float(row[j]), float(v[j]), acc)
    return acc


def unfused_chain(row, v) -> float:
    """((M_i0 x_0 + M_i1 x_1) + M_i2 x_2) + ...: left to right, every product and every sum rounded"""
    acc = float(row[0]) * float(v[0])
    for j in range(1, len(row)):
        acc = acc + float(row[j]) * float(v[j])
    return acc


def matvec_unfused(M, v):
    return [unfused_chain(M[i], v) for i in range(len(v))]


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    t = 134217729.0 * a
    hi = t - (t - a)
    return hi, a - hi


def fma_np(a, b, c):
    """Vectorised fma on float64 arrays from basic operations only (Boldo and Melquiond 2008, 'Emulation of a FMA and
    correctly-rounded sums: proved algorithms using rounding to odd'): the exact product as a pair (Dekker), the exact sum of c and
    its high part, the remaining two terms rounded TO ODD, one final rounding to nearest.  Valid while nothing over- or underflows
    (|a b| well inside the normal range), which the block inputs keep; checked against fma() on every product they use."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    uh = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    ul = ((ah * bh - uh) + ah * bl + al * bh) + al * bl
    th, tl = _two_sum(c, uh)
    s, e = _two_sum(tl, ul)
    bits = np.ascontiguousarray(s).view(np.int64).copy()
    need = (e != 0) & ((bits & 1) == 0)
    away = (e > 0) == (s > 0)
    bits += np.where(need, np.where(away, 1, -1), 0).astype(np.int64)
    return th + bits.view(np.float64)


def fused_matvec_np(M, V, descending=False):
    """rows of M (n x n) against the vectors V (k x n): out[k, c] = the fused ascending chain of row c on vector k"""
    M, V = np.asarray(M, np.float64), np.asarray(V, np.float64)
    n = M.shape[0]
    acc = np.zeros((V.shape[0], n))
    for j in (range(n - 1, -1, -1) if descending else range(n)):
        acc = fma_np(M[None, :, j], V[:, j, None], acc)
    return acc


def unfused_matvec_np(M, V):
    M, V = np.asarray(M, np.float64), np.asarray(V, np.float64)
    acc = M[None, :, 0] * V[:, 0, None]
    for j in range(1, M.shape[0]):
        acc = acc + M[None, :, j] * V[:, j, None]
    return acc


# ---- normalisation sum and categorical draw ------------------------------------------------------------------------------
def coop_sum(x) -> float:
    """n > 4: four interleaved partial sums t_g = x_g + x_{g+4} + ... (from +0, ascending), combined as (t0 + t1) + (t2 + t3)"""
    t = [0.0, 0.0, 0.0, 0.0]
    for j, xj in enumerate(x):
        t[j & 3] = t[j & 3] + float(xj)
    return (t[0] + t[1]) + (t[2] + t[3])


def draw(p, u: float, strict: bool = False):
    """first j with u * sum(p) <= p_0 + .. + p_j, the sums formed left to right; n - 1 comparisons decide it (the last one is
    always true for a proper vector since u < 1), so a threshold no partial sum reaches -- a NaN total -- gives n - 1.
    -> (index, error bits): DERR_ZERO_PROB for a total that is zero, negative, infinite or NaN."""
    n = len(p)
    total = float(p[0])
    for j in range(1, n):
        total = total + float(p[j])
    err = DERR_ZERO_PROB if (not (total > 0.0)) or math.isinf(total) else 0
    thr = u * total
    cum = float(p[0])
    for j in range(n - 1):
        if j:
            cum = cum + float(p[j])
        if (thr < cum) if strict else (thr <= cum):
            return j, err
    return n - 1, err


# ---- StatLanes: fixed-point dwell sums ------------------------------------------------------------------------------------------
MASK64 = (1 << 64) - 1


def to_fixed(x: float, fx_scale: float) -> int:
    """round half to even of the double x * fx_scale, as a 64-bit two's-complement pattern"""
    return round(x * fx_scale) & MASK64          # Python's round(float) is round-half-even and exact


def from_fixed(cell: int, fx_inv: float) -> float:
    v = cell - (1 << 64) if cell >= (1 << 63) else cell
    return float(v) * fx_inv                     # float(int) rounds to nearest even, like the signed 64-bit conversion


def statlanes(n, ncount, dcol, dx, ccol, cell, live, ncell, fx_scale, dw_init, ct_init):
    """-> (dwell cells [n][ncell] mod 2^64, count cells [ncount][ncell] mod 2^32) after every live lane added its segments"""
    dw = [[int(v) for v in row] for row in dw_init]
    ct = [[int(v) for v in row] for row in ct_init]
    for i in range(len(cell)):
        if not live[i]:
            continue
        for s in range(len(dcol[i])):
            if 0 <= dcol[i][s] < n:
                dw[dcol[i][s]][cell[i]] = (dw[dcol[i][s]][cell[i]] + to_fixed(float(dx[i][s]), fx_scale)) & MASK64
            if 0 <= ccol[i][s] < ncount:
                ct[ccol[i][s]][cell[i]] = (ct[ccol[i][s]][cell[i]] + 1) & 0xFFFFFFFF
    return dw, ct


# ---- phm_ll_device.h: the rescale rule, mu_k and B_k ---------------------------------------------------------------------------------
def ll_rescale(v):
    """-> (v * 2^-e, e) with max(v) * 2^-e in [1/2, 1), by numpy's frexp / ldexp; e = 0 and v untouched when no entry is positive"""
    v = np.asarray(v, dtype=np.float64)
    mx = max(0.0, float(v.max()))
    if not mx > 0.0:
        return v.copy(), 0
    e = int(np.frexp(mx)[1])
    return np.ldexp(v, -e), e


def model_mu_b(Q):
    """-> (mu = max_i(-q_ii) from 0, B = I + Q / mu with the quotient and the sum rounded one after the other; B = I when mu = 0)"""
    Q = np.asarray(Q, dtype=np.float64)
    mu = max(0.0, float((-np.diag(Q)).max()))
    eye = np.eye(len(Q))
    return mu, (eye + Q / mu if mu > 0.0 else eye)


# ---- the oracle's exported scalar functions, elementwise ----------------------------------------------------------------------------
def _oracle():
    import oracle_lib as O
    L = O.lib()
    L.orc_neglog_u32.restype = C.c_double
    L.orc_neglog_u32.argtypes = [C.c_uint32]
    L.orc_stream_word.restype = C.c_uint32
    L.orc_stream_word.argtypes = [C.c_uint32] * 6
    return O, L


def orc_philox7(ctr, key):
    O, _ = _oracle()
    return np.array([O.philox([int(x) for x in c], [int(x) for x in k], 7) for c, k in zip(ctr, key)], dtype=np.uint32)


def orc_map(name, xs):
    _, L = _oracle()
    f = getattr(L, name)
    conv = int if name in ("orc_u01", "orc_neglog_u32") else float
    return np.array([f(conv(x)) for x in xs], dtype=np.float64)


def orc_stream(seed_lo, seed_hi, rep, it, ent, dseq):
    """-> (words, uniforms), each [lane, position]: draw d = word d & 3 of Philox block d >> 2 of counter (block, entity, iteration, replica)"""
    _, L = _oracle()
    w = np.array([[L.orc_stream_word(seed_lo, seed_hi, int(r), int(i), int(e), int(d)) for d in dseq] for r, i, e in zip(rep, it, ent)],
                 dtype=np.uint32)
    u = np.array([[L.orc_stream_u(seed_lo, seed_hi, int(r), int(i), int(e), int(d)) for d in dseq] for r, i, e in zip(rep, it, ent)])
    return w, u


def stream_word_from_blocks(seed_lo, seed_hi, rep, it, ent, d):
    """the stream addressing of DESIGN.md section 3 written out: counter (d >> 2, entity, iteration, replica), key = seed"""
    O, _ = _oracle()
    return O.philox([d >> 2, int(ent), int(it), int(rep)], [seed_lo, seed_hi], 7)[d & 3]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
