"""The inputs of the device-block tests, shared by tests/test_gpu_device_blocks.py (which runs them on the GPU) and
tests/test_device_blocks_cpu.py (which checks that they are sharp and measures the oracle on them).  Everything is generated
from fixed seeds; nothing here touches the GPU."""
from __future__ import annotations

import functools
import struct

import numpy as np

import blocksref as R

# either side of the batches of eight, the 16-lane DPP rows and the full wave
COOP_N = (5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64)
N_VEC = 64                    # vectors (= waves) per case: 16 workgroups of four waves
ELL_W = (1, 3, 7)
DENSE_FORMS = ("coop_matvec", "coop_matvec_lds", "coop_matvec_regs")


def _d(bits: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def _mixed(rs, shape, lo=-8, hi=8):
    """signed finite values of mixed magnitude: a 53-bit mantissa in [0.5, 1) times 2^[lo, hi]"""
    return np.ldexp(rs.uniform(0.5, 1.0, shape) * rs.choice([-1.0, 1.0], shape), rs.integers(lo, hi + 1, shape))


# ---- Philox, u01, streams ----------------------------------------------------------------------------------------------------
PHILOX7_KAT = (   # Random123's kat_vectors, philox4x32 with 7 rounds (the three of tests/test_oracle_cpu.py)
    ([0, 0, 0, 0], [0, 0], [0x5f6fb709, 0x0d893f64, 0x4f121f81, 0x4f730a48]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x5207ddc2, 0x45165e59, 0x4d8ee751, 0x8c52f662]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0x4dfccaba, 0x190a87f0, 0xc47362ba, 0xb6b5242a]),
)


@functools.lru_cache(None)
def philox_random():
    rs = np.random.default_rng(101)
    return rs.integers(0, 2 ** 32, (4096, 4), dtype=np.uint64).astype(np.uint32), rs.integers(0, 2 ** 32, (4096, 2), dtype=np.uint64).astype(np.uint32)


@functools.lru_cache(None)
def u01_words():
    rs = np.random.default_rng(102)
    return np.concatenate([np.array([0, 1, 0x7fffffff, 0x80000000, 0xffffffff], dtype=np.uint32),
                           rs.integers(0, 2 ** 32, 1019, dtype=np.uint64).astype(np.uint32)])


STREAM_SEED = (0x9E3779B9, 0x7F4A7C15)
STREAM_IN_ORDER = tuple(range(20))
STREAM_OUT_OF_ORDER = (5, 4, 7, 0, 9, 8, 1, 13, 12)      # the kept block changes 1, 1, 1, 0, 2, 2, 0, 3, 3


@functools.lru_cache(None)
def stream_lanes():
    """320 lanes (a partial last workgroup) that differ in replica, iteration and entity; the entities cycle through the ENT_* tags"""
    rs = np.random.default_rng(103)
    N = 320
    rep = rs.integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
    it = rs.integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
    it[::7] = 0xFFFFFFFF                                  # the forward simulator's iteration word
    tags = np.array([R.ENT_NODE, R.ENT_BSTATE, R.ENT_BEXP, R.ENT_BUNIF], dtype=np.uint32)
    ent = (tags[np.arange(N) % 4] | rs.integers(0, 2 ** 30, N, dtype=np.uint64).astype(np.uint32)).astype(np.uint32)
    rep[:3], it[:3], ent[:3] = 0, 0, tags[1:4]            # the smallest addresses of each branch tag
    return rep, it, ent


# ---- neglog_u32 ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def neglog_words():
    rs = np.random.default_rng(104)
    ks = [0, 1, 2, 2 ** 32 - 2, 2 ** 32 - 1]
    for m in range(33):
        ks += [k for k in (2 ** m, 2 ** m - 1) if 0 <= k < 2 ** 32]
    ks += list(range(0xFEFFFFFF, 0xFF000002))             # the `top` switch: f >= 1 - 2^-8 in the top binade
    for j in range(128):                                  # 2k + 1 = 2^e f crosses f = 0.5 + j / 256 between k0 - 1 and k0
        ks += [2 ** 31 + j * 2 ** 24 - 1, 2 ** 31 + j * 2 ** 24]          # e = 33, the top binade
        ks += [2 ** 15 + j * 2 ** 8 - 1, 2 ** 15 + j * 2 ** 8]            # e = 17
    return np.concatenate([np.array(ks, dtype=np.uint64), rs.integers(0, 2 ** 32, 65536, dtype=np.uint64)]).astype(np.uint32)


# ---- phm_log -----------------------------------------------------------------------------------------------------------------------
DBL_MIN, DBL_MAX = 2.2250738585072014e-308, 1.7976931348623157e308


@functools.lru_cache(None)
def log_inputs():
    rs = np.random.default_rng(105)
    xs = [1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)]
    xs += [float(np.ldexp(1.0, e)) for e in range(-1074, 1024)]
    xs += [DBL_MIN, float(np.nextafter(DBL_MIN, 0.0)), float(np.nextafter(DBL_MIN, 1.0))]
    xs += [_d(int(b)) for b in rs.integers(1, 2 ** 52, 64)]               # subnormals
    xs += [_d(3), _d(2 ** 52 - 1)]
    xs.append(DBL_MAX)
    for e in (-500, 0, 10):                               # (hx + 0x95f64) & 0x100000 switches between mantissa words 0x6a09b and 0x6a09c
        for hx, lo in ((0x6a09b, 0xffffffff), (0x6a09c, 0x00000000), (0x6a09b, 0x12345678), (0x6a09c, 0x9abcdef0)):
            xs.append(_d(((1023 + e) << 52) | (hx << 32) | lo))
        # either reduction is a valid logarithm and most mantissas round alike under both (about one in sixteen does not), so the
        # two mantissa words next to the switch are taken with 64 low words each
        for hx in (0x6a09b, 0x6a09c):
            xs += [_d(((1023 + e) << 52) | (hx << 32) | int(lo)) for lo in rs.integers(0, 2 ** 32, 64)]
    words = rs.integers(0, 2 ** 32, 4096, dtype=np.uint64)
    xs += list((words.astype(np.float64) + 0.5) / 2.0 ** 32)
    xs += list(np.exp2(rs.uniform(-1074.0, 1024.0, 4096)))
    return np.array(xs, dtype=np.float64)


# ---- phm_exp -----------------------------------------------------------------------------------------------------------------------
EXP_OVERFLOW, EXP_UNDERFLOW = 7.09782712893383973096e+02, -7.45133219101941108420e+02
HALF_LN2 = 0.34657359027997264


@functools.lru_cache(None)
def exp_inputs():
    rs = np.random.default_rng(106)
    xs = [float("nan"), 0.0, -0.0, 1e-300, -1e-300, _d(5), -_d(5)]
    for cut in (EXP_OVERFLOW, EXP_UNDERFLOW, HALF_LN2, -HALF_LN2):
        xs += [float(np.nextafter(cut, -np.inf)), cut, float(np.nextafter(cut, np.inf))]
    xs += list(np.linspace(-745.13, -708.4, 256))         # subnormal results
    xs += [k * 0.6931471805599453 / 2 for k in range(-2000, 2001)]       # the ties of k = round(x / ln 2)
    xs += list(rs.uniform(-745.0, 709.0, 8192))
    return np.array(xs, dtype=np.float64)


# ---- matvec_u, sample_cat (n <= 4) -----------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def matvec_u_case(ns):
    """256 matrix / vector pairs (four waves; the first 64 are the issue's), signed, mixed magnitude"""
    rs = np.random.default_rng(200 + ns)
    return _mixed(rs, (256, ns, ns)), _mixed(rs, (256, ns))


# ---- categorical draws -----------------------------------------------------------------------------------------------------------
U_LOW, U_HIGH = 2.0 ** -33, 1.0 - 2.0 ** -53


@functools.lru_cache(None)
def draw_case(n):
    """-> (P [k, n], u [k], kind [k]) for sample_cat (n <= 4) and the cooperative draws (n > 4).  kind: 'ok' (index and a clear
    error word), 'bad' (zero / inf / NaN total: index and DERR_ZERO_PROB), 'neg' (negative total: the error bit only -- 'first j'
    and the kernels' count of failed comparisons are different numbers once the partial sums decrease)."""
    rs = np.random.default_rng(300 + n)
    P, U, K = [], [], []

    def add(p, u, kind="ok"):
        P.append(np.asarray(p, dtype=np.float64)); U.append(float(u)); K.append(kind)

    def ru():
        return (float(rs.integers(0, 2 ** 32)) + 0.5) / 2.0 ** 32

    for _ in range(24):
        add(rs.uniform(0.0, 1.0, n) * np.exp2(rs.integers(-6, 1, n)), ru())
    for lead in (1, 2):
        if lead < n:
            p = rs.uniform(0.1, 1.0, n); p[:lead] = 0.0; add(p, ru()); add(p, U_LOW)
    if n > 2:
        p = rs.uniform(0.1, 1.0, n); p[n // 2] = 0.0; p[1] = 0.0; add(p, ru()); add(p, 0.5)
    for trail in (1, 2):
        if trail < n:
            p = rs.uniform(0.1, 1.0, n); p[n - trail:] = 0.0; add(p, ru()); add(p, U_HIGH)
    for hot in (0, n - 1):
        p = np.zeros(n); p[hot] = 0.75; add(p, ru()); add(p, U_LOW); add(p, U_HIGH)
    sub = rs.integers(1, 9, n).astype(np.float64) * 5e-324                 # subnormal entries, subnormal total
    add(sub, ru()); add(sub, 0.5); add(sub, U_HIGH)
    mixed = rs.uniform(0.1, 1.0, n); mixed[::2] = sub[::2]; add(mixed, ru())
    m = 1 << (n.bit_length() - 1)                                          # m equal powers of two: u * total = the (u m)-th partial sum exactly
    for u in (0.25, 0.5, 0.75):
        p = np.zeros(n); p[:m] = 0.125; add(p, u)
        p = np.zeros(n); p[n - m:] = 0.125; add(p, u)
    for _ in range(3):
        p = rs.uniform(0.0, 1.0, n); add(p, U_LOW); add(p, U_HIGH)
    add(np.zeros(n), ru(), "bad")
    for q in sorted({0, n // 2, n - 1}):
        p = rs.uniform(0.1, 1.0, n); p[q] = np.inf; add(p, ru(), "bad")
        p = rs.uniform(0.1, 1.0, n); p[q] = np.nan; add(p, ru(), "bad")
    add(-rs.uniform(0.1, 1.0, n), ru(), "neg")
    while len(P) % 4:                                                      # whole workgroups of four waves
        add(rs.uniform(0.0, 1.0, n), ru())
    return np.array(P), np.array(U), tuple(K)


# ---- the matrix-vector forms -----------------------------------------------------------------------------------------------------
def pad_lanes(V, n, fill):
    """[k, n] -> [k, 64]: lanes >= n hold `fill` ('nan', 'zero', or 'finite': values found in no live lane)"""
    V = np.asarray(V, dtype=np.float64)
    out = np.zeros((V.shape[0], 64))
    out[:, :n] = V
    if fill == "nan":
        out[:, n:] = np.nan
    elif fill == "finite":
        out[:, n:] = 1000.0 + np.arange(n, 64)[None, :] + np.arange(V.shape[0])[:, None] / 128.0
    return out


@functools.lru_cache(None)
def vectors(n):
    """64 vectors: signed finite entries of mixed magnitude, with exact zeros of both signs"""
    rs = np.random.default_rng(400 + n)
    V = _mixed(rs, (N_VEC, n))
    z = rs.uniform(0.0, 1.0, (N_VEC, n))
    V[z < 0.06] = 0.0
    V[(z >= 0.06) & (z < 0.12)] = -0.0
    V[0, 0], V[1, n - 1], V[2, 0], V[3, n - 1] = 0.0, 0.0, -0.0, -0.0
    return V


@functools.lru_cache(None)
def dense_matrix(n):
    return _mixed(np.random.default_rng(500 + n), (n, n), -4, 4)


def with_stride(M, ldn):
    """row stride ldn = n | 1 as in phm_wbranch.hip and phm_wide.hip; the padding column holds a value no product may meet"""
    n = M.shape[0]
    out = np.full((n, ldn), 7777.0)
    out[:, :n] = M
    return out


@functools.lru_cache(None)
def ell_matrix(n, w):
    """-> (dense [n, n], ecol [n, w], eval [n, w]): at most w non-zeros per row, columns ascending, the padding as the engine
    writes it (column = the row's own index, value 0); some rows are shorter than w and one has no entry at all"""
    rs = np.random.default_rng(600 + 8 * n + w)
    M = np.zeros((n, n))
    ecol, ev = np.zeros((n, w), np.int32), np.zeros((n, w))
    for i in range(n):
        cnt = w if rs.uniform() < 0.6 else int(rs.integers(max(1, w - 2), w + 1))
        if i == n // 2 and w > 1:
            cnt = 0
        cols = np.sort(rs.choice(n, size=min(cnt, n), replace=False))
        vals = _mixed(rs, len(cols), -4, 4)
        M[i, cols] = vals
        ecol[i, :] = i
        ecol[i, :len(cols)] = cols
        ev[i, :len(cols)] = vals
    return M, ecol, ev


@functools.lru_cache(None)
def band_matrix(n, hb):
    """-> (dense [n, n], coef [64, 5]): coef[lane][d] = M[c][c + d - hb] for c = min(lane, n - 1), 0 where the matrix has no entry"""
    rs = np.random.default_rng(700 + 8 * n + hb)
    M = np.zeros((n, n))
    for i in range(n):
        for j in range(max(0, i - hb), min(n, i + hb + 1)):
            M[i, j] = _mixed(rs, (), -4, 4)
    coef = np.zeros((64, 5))
    for lane in range(64):
        c = min(lane, n - 1)
        for d in range(2 * hb + 1):
            j = c + d - hb
            if 0 <= j < n:
                coef[lane, d] = M[c, j]
    return M, coef


def matvec_cases():
    """every (name, n, dense matrix) the product forms run on: 'dense', 'ell1', 'ell3', 'ell7', 'band1', 'band2'"""
    for n in COOP_N:
        yield "dense", n, dense_matrix(n)
        for w in ELL_W:
            yield f"ell{w}", n, ell_matrix(n, w)[0]
        for hb in (1, 2):
            yield f"band{hb}", n, band_matrix(n, hb)[0]


@functools.lru_cache(None)
def chain_reference(name, n):
    """-> (f(V), f(f(V))) [64, n] each: the fused ascending chain applied once and twice to vectors(n)"""
    M = dict((nm, M) for nm, nn, M in matvec_cases() if nn == n)[name]
    y1 = R.fused_matvec_np(M, vectors(n))
    y2 = R.fused_matvec_np(M, y1)
    y1.setflags(write=False); y2.setflags(write=False)
    return y1, y2


@functools.lru_cache(None)
def sum_vectors(n):
    rs = np.random.default_rng(800 + n)
    V = _mixed(rs, (N_VEC, n), -20, 20)
    V[:, 0][::9] = 0.0
    return V


# ---- wave maxima -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def wave_max_inputs():
    """68 waves: the maximum in lane 0 .. 63 in turn, then all equal, all zero, a maximum of 2^31 - 1 in lane 17 and in lane 63"""
    rs = np.random.default_rng(900)
    v = rs.integers(0, 1000, (68, 64)).astype(np.int32)
    for w in range(64):
        v[w, w] = 5000 + w
    v[64, :] = 37
    v[65, :] = 0
    v[66, 17] = 2 ** 31 - 1
    v[67, 63] = 2 ** 31 - 1
    return v


@functools.lru_cache(None)
def wave_min_inputs():
    """the 65535 - wave_max_count(65535 - k) idiom of phm_wtiles.hip on k in 0 .. 65535: the minimum in each lane in turn, then all equal"""
    rs = np.random.default_rng(901)
    v = rs.integers(200, 65536, (68, 64)).astype(np.int32)
    for w in range(64):
        v[w, w] = w
    v[64, :] = 65535
    v[65, :] = 0
    v[66, :] = 4242
    v[67, 31] = 1
    return v


# ---- StatLanes -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def stat_case(ns, fx_exp):
    """320 lanes of 40 segments.  fx_scale = 2^(61 - fx_exp).  Dwells: values below 2^(fx_exp - 7) (40 of them stay below the 2^61 of
    the engine's contract), tiny values that the scale leaves with a fraction, and exact .5 ties of both parities; lane 5 alone
    carries sums that wrap past 2^64.  Every fourth lane from lane 2 is not live."""
    rs = np.random.default_rng(1000 + 16 * ns + fx_exp)
    n, ncount = (ns, ns * ns) if ns else (7, 12)
    N, nseg = 320, 40
    scale, inv = float(np.ldexp(1.0, 61 - fx_exp)), float(np.ldexp(1.0, fx_exp - 61))
    dcol = rs.integers(0, n, (N, nseg)).astype(np.int32)
    ccol = rs.integers(-1, ncount, (N, nseg)).astype(np.int32)            # -1: a segment that ends in no counted jump
    dx = rs.uniform(0.0, 1.0, (N, nseg)) * np.ldexp(1.0, fx_exp - 7)
    small = rs.uniform(0.0, 1.0, (N, nseg)) < 0.3
    dx[small] = (rs.uniform(0.0, 4096.0, (N, nseg)) * inv)[small]
    ties = rs.uniform(0.0, 1.0, (N, nseg)) < 0.2
    m = rs.integers(0, 2 ** 20, (N, nseg)).astype(np.float64)
    dx[ties] = ((m + 0.5) * inv)[ties]                                       # x * fx_scale = m + 0.5 exactly, m even and odd
    dx[0, :4] = np.array([0.5, 1.5, 2.5, 3.5]) * inv
    dx[5, :] = np.ldexp(1.0, fx_exp + 1) * rs.uniform(0.6, 1.0, nseg)        # each below 2^62 in fixed point; 40 of them wrap
    dcol[5, :] = np.arange(nseg) % 2
    dcol[6, :], ccol[6, :] = 0, -1                                           # a lane whose other accumulators stay zero at the flush
    cell = rs.permutation(N).astype(np.int32)
    live = np.ones(N, np.uint8)
    live[2::4] = 0
    dw_init = rs.integers(0, 2 ** 40, (n, N)).astype(np.uint64)
    dw_init[:, ::3] = 0
    ct_init = rs.integers(0, 1000, (ncount, N)).astype(np.uint32)
    return dict(ns=ns, n=n, ncount=ncount, dcol=dcol, dx=dx, ccol=ccol, cell=cell, live=live, ncell=N, fx_scale=scale, fx_inv=inv,
                dw_init=dw_init, ct_init=ct_init)


def stat_reordered(case):
    """the same segments of every lane in another order"""
    rs = np.random.default_rng(77)
    perm = rs.permutation(case["dcol"].shape[1])
    out = dict(case)
    for k in ("dcol", "dx", "ccol"):
        out[k] = np.ascontiguousarray(case[k][:, perm])
    return out


# ---- phm_ll_device.h --------------------------------------------------------------------------------------------------------------------
LL_N = (2, 3, 4, 5, 6, 7, 8)
RESCALE_KINDS = ("all zero", "maximum exactly 1", "subnormal maximum", "2^1000", "maximum last", "random")


def rescale_vectors(n):
    """[kind, n] in the order of RESCALE_KINDS; every scaled entry stays a normal number or zero, so the scaling is exact"""
    rs = np.random.default_rng(7000 + n)
    one = rs.uniform(0.0, 1.0, n)
    one[rs.integers(n)] = 1.0                                          # frexp(1.0) = (0.5, 1): e = 1
    sub = np.array([_d(int(b)) for b in rs.integers(1, 1 << 40, n)])   # subnormals: the scaling by 2^-e goes UP
    big = rs.uniform(0.5, 1.0, n) * 2.0 ** rs.integers(960, 1000, n)
    big[0] = 2.0 ** 1000
    big[n - 1] = 0.0
    last = np.sort(rs.uniform(1e-3, 40.0, n))                          # the largest entry in the last position
    return np.stack([np.zeros(n), one, sub, big, last, np.abs(_mixed(rs, n))])


def model_matrices(n):
    """[3, n, n]: two non-symmetric generators (rows sum to zero; the second with one state that is never left) and the zero matrix"""
    rs = np.random.default_rng(7100 + n)
    Qs = rs.uniform(0.05, 3.0, (3, n, n))
    Qs[1, n - 1] = 0.0
    for Q in Qs:
        np.fill_diagonal(Q, 0.0)
        np.fill_diagonal(Q, -Q.sum(axis=1))
    Qs[2] = 0.0
    return Qs
