"""Keeps tests/test_gpu_device_blocks.py honest without a GPU: its references agree with libm's fma and with the oracle where the
oracle exports the same operation, its inputs are sharp (a wrong summation order, a dropped fusion or a `<` for a `<=` changes
results on them), the oracle functions it compares with are within their ulp bounds on exactly those inputs, and the harness
library exists and exports every entry the loader declares."""
import ctypes as C
import math
from fractions import Fraction
import os

import mpmath
import numpy as np
import pytest

import blockcases as Cs
import blocks_lib as B
import blocksref as R
import oracle_lib as O
import pyref

MATVEC_CASES = [(name, n) for name, n, _ in Cs.matvec_cases()]
MULTI_TERM = [(name, n) for name, n in MATVEC_CASES if name != "ell1"]       # a row of one term has one rounding under any rule


# ---- the fused reference ----------------------------------------------------------------------------------------------------------
def test_fraction_fma_basics():
    assert R.fma(3.0, 5.0, 7.0) == 22.0
    assert R.fma(1.0 + 2.0 ** -52, 1.0 + 2.0 ** -52, -1.0) == 2.0 ** -51 + 2.0 ** -104          # the product's low bits survive
    assert (1.0 + 2.0 ** -52) * (1.0 + 2.0 ** -52) - 1.0 == 2.0 ** -51
    for a, b, c in ((0.0, -3.0, 0.0), (0.0, 3.0, -0.0), (-0.0, 3.0, -0.0), (2.0, 3.0, -6.0), (0.0, -0.0, 1.5)):
        want = R.libm_fma(a, b, c)
        got = R.fma(a, b, c)
        assert got == want and math.copysign(1.0, got) == math.copysign(1.0, want), (a, b, c)


@pytest.mark.parametrize("name,n", MATVEC_CASES)
def test_fraction_fma_equals_libm_fma_on_every_product_the_gpu_cases_use(name, n):
    """Both applications of the chain, every term: the exact-rational fma, libm's fma and the vectorised twin give the same
    accumulator at every step.  Terms whose matrix entry is an exact zero leave the accumulator as it is under all three (the
    accumulator is never -0 here); they are checked for that instead of being put through the rationals."""
    M = dict((nm, m) for nm, nn, m in Cs.matvec_cases() if nn == n)[name]
    y1, y2 = Cs.chain_reference(name, n)
    for V, Y in ((Cs.vectors(n), y1), (np.asarray(y1), y2)):
        assert np.isfinite(V).all()
        for k in range(V.shape[0]):
            for c in range(n):
                acc = 0.0
                for j in range(n):
                    a, x = float(M[c, j]), float(V[k, j])
                    if a == 0.0:
                        same = R.libm_fma(a, x, acc)
                        assert same == acc and math.copysign(1.0, same) == math.copysign(1.0, acc), (name, n, k, c, j)
                        continue
                    nxt = R.fma(a, x, acc)
                    assert nxt == R.libm_fma(a, x, acc), (name, n, k, c, j)
                    acc = nxt
                assert acc == Y[k, c] and math.copysign(1.0, acc) == math.copysign(1.0, Y[k, c]), (name, n, k, c)


def test_references_agree_with_the_oracle_and_its_python_twin():
    rs = np.random.default_rng(5)
    for n in (5, 8, 17):
        M, v = rs.uniform(-1, 1, (n, n)), rs.uniform(-1, 1, n)
        want = pyref.matvec(M.tolist(), v.tolist())                          # the oracle's Python twin (mcmc_matvec, n > 4)
        got = [R.fused_chain(M[c], v) for c in range(n)]
        assert got == [float(x) for x in want]
        assert np.array_equal(R.fused_matvec_np(M, v[None, :])[0], np.array(got))
    for n in (2, 3, 4):
        M, v = rs.uniform(-1, 1, (n, n)), rs.uniform(-1, 1, n)
        assert R.matvec_unfused(M, v) == [float(x) for x in pyref.matvec_lr(M.tolist(), v.tolist())]
    for n in (2, 4, 9):
        for _ in range(200):
            p, u = rs.uniform(0, 1, n), float(rs.uniform(0, 1))
            assert R.draw(p, u) == (pyref.sample(p.tolist(), u), 0)          # the oracle's Python twin of its categorical draw
    for n in (5, 8, 9, 63):
        x = rs.uniform(-1, 1, n)
        assert R.coop_sum(x) == pyref.rowsum(x.tolist())
    x = Cs.u01_words()
    assert np.array_equal(R.orc_map("orc_u01", x), (x.astype(np.float64) + 0.5) / 2.0 ** 32)
    for ctr, key, want in Cs.PHILOX7_KAT:
        assert O.philox(ctr, key, 7) == want
    rep, it, ent = Cs.stream_lanes()
    assert {int(e) >> 30 for e in ent} == {0, 1, 2, 3}
    w, u = R.orc_stream(*Cs.STREAM_SEED, rep[:8], it[:8], ent[:8], Cs.STREAM_OUT_OF_ORDER)
    for lane in range(8):
        for q, d in enumerate(Cs.STREAM_OUT_OF_ORDER):
            assert int(w[lane, q]) == R.stream_word_from_blocks(*Cs.STREAM_SEED, rep[lane], it[lane], ent[lane], d)
            assert u[lane, q] == (int(w[lane, q]) + 0.5) / 2.0 ** 32
    blocks = [d >> 2 for d in Cs.STREAM_OUT_OF_ORDER]
    assert any(b1 < b0 for b0, b1 in zip(blocks, blocks[1:])) and any(b1 > b0 for b0, b1 in zip(blocks, blocks[1:]))


# ---- the inputs are sharp ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", MULTI_TERM)
def test_product_inputs_tell_fused_from_unfused_and_ascending_from_descending(name, n):
    M = dict((nm, m) for nm, nn, m in Cs.matvec_cases() if nn == n)[name]
    V = Cs.vectors(n)
    fused = R.bits(np.asarray(Cs.chain_reference(name, n)[0]))
    unfused = R.bits(R.unfused_matvec_np(M, V))
    descending = R.bits(R.fused_matvec_np(M, V, descending=True))
    k, c = 1, n - 2                                                          # the vectorised variants against the plain definitions
    assert R.unfused_matvec_np(M, V)[k, c] == R.unfused_chain(M[c], V[k])
    assert R.fused_matvec_np(M, V, descending=True)[k, c] == R.fused_chain(M[c], V[k], order=range(n - 1, -1, -1), fma_fn=R.libm_fma)
    assert int((fused != unfused).sum()) >= 8, (name, n)
    assert int((fused != descending).sum()) >= 8, (name, n)


@pytest.mark.parametrize("n", (2, 3, 4) + Cs.COOP_N)
def test_draw_inputs_tell_less_or_equal_from_less(n):
    P, U, kinds = Cs.draw_case(n)
    changed = [i for i in range(len(U)) if kinds[i] == "ok" and R.draw(P[i], U[i])[0] != R.draw(P[i], U[i], strict=True)[0]]
    assert changed, n
    assert len(U) % 4 == 0 and {"ok", "bad", "neg"} == set(kinds)
    for i, kind in enumerate(kinds):
        assert (R.draw(P[i], U[i])[1] != 0) == (kind != "ok")
        assert 0.0 < U[i] < 1.0


def test_statlanes_inputs_hold_ties_of_both_parities_and_a_wrap():
    for ns in (0, 2, 3, 4):
        for e in (1, 11):
            case = Cs.stat_case(ns, e)
            assert case["fx_scale"] == 2.0 ** (61 - e) and case["fx_scale"] * case["fx_inv"] == 1.0
            prod = case["dx"] * case["fx_scale"]
            tie = (prod - np.floor(prod)) == 0.5
            assert (tie & (np.floor(prod) % 2 == 0)).sum() > 100 and (tie & (np.floor(prod) % 2 == 1)).sum() > 100
            assert R.to_fixed(0.5 * case["fx_inv"], case["fx_scale"]) == 0 and R.to_fixed(1.5 * case["fx_inv"], case["fx_scale"]) == 2
            assert R.to_fixed(2.5 * case["fx_inv"], case["fx_scale"]) == 2 and R.to_fixed(3.5 * case["fx_inv"], case["fx_scale"]) == 4
            assert sum(R.to_fixed(float(x), case["fx_scale"]) for x in case["dx"][5, 0::2]) >= 1 << 64
            assert len(set(case["cell"].tolist())) == len(case["cell"])     # one cell per lane, as at the call sites
    assert R.from_fixed((1 << 64) - 3, 0.5) == -1.5


# ---- ulp errors of the oracle functions on exactly the GPU inputs ------------------------------------------------------------------------
def _ulp_of(want):
    """one unit in the last place of the double nearest `want` (an mpf), normal range"""
    return mpmath.ldexp(1, int(mpmath.floor(mpmath.log(abs(want), 2))) - 52)


def test_orc_log_within_its_bound_on_the_gpu_inputs():
    """tests/test_oracle_cpu.py asserts <= 2 ulp for orc_log; the same bound on every GPU input, subnormals and both ends of the range included"""
    mpmath.mp.dps = 50
    x = Cs.log_inputs()
    got = R.orc_map("orc_log", x)
    assert (x > 0).all() and np.isfinite(x).all() and (x < Cs.DBL_MIN).sum() >= 64 + 52
    worst = 0.0
    for xi, gi in zip(x, got):
        want = mpmath.log(mpmath.mpf(float(xi)))
        if want == 0:
            assert gi == 0.0
            continue
        worst = max(worst, float(abs(mpmath.mpf(float(gi)) - want) / _ulp_of(want)))
    print(f"orc_log: worst {worst:.3f} ulp on {len(x)} inputs")
    assert worst <= 2.0


SUBNORMAL_EXP_MEASURED = 0.65     # units of 2^-1074, measured on exp_inputs(); asserted with one unit of margin


def test_orc_exp_within_its_bound_on_the_gpu_inputs():
    """Normal results: the <= 2 ulp tests/test_oracle_cpu.py asserts for orc_exp.  Subnormal results have a fixed spacing of 2^-1074;
    the error is measured in that unit and asserted at the measured figure plus one unit."""
    mpmath.mp.dps = 50
    x = Cs.exp_inputs()
    got = R.orc_map("orc_exp", x)
    worst, worst_sub, n_sub = 0.0, 0.0, 0
    tiny = mpmath.ldexp(1, -1074)
    for xi, gi in zip(x, got):
        if math.isnan(xi):
            assert math.isnan(gi)
            continue
        if xi > Cs.EXP_OVERFLOW:
            assert gi == math.inf
            continue
        if xi < Cs.EXP_UNDERFLOW:
            assert gi == 0.0
            continue
        want = mpmath.exp(mpmath.mpf(float(xi)))
        if want < mpmath.mpf(Cs.DBL_MIN):
            n_sub += 1
            worst_sub = max(worst_sub, float(abs(mpmath.mpf(float(gi)) - want) / tiny))
        else:
            worst = max(worst, float(abs(mpmath.mpf(float(gi)) - want) / _ulp_of(want)))
    print(f"orc_exp: worst {worst:.3f} ulp on normal results, {worst_sub:.3f} units of 2^-1074 on {n_sub} subnormal results")
    assert n_sub >= 256
    assert worst <= 2.0
    assert worst_sub <= SUBNORMAL_EXP_MEASURED + 1.0
    assert worst_sub >= SUBNORMAL_EXP_MEASURED - 0.25, "the recorded figure is stale: measure again and update DESIGN.md"


def test_orc_neglog_u32_within_its_bound_on_the_gpu_inputs():
    """tests/test_oracle_cpu.py asserts a relative error below 1.5 * 2^-52 for orc_neglog_u32; the same bound on every GPU word"""
    mpmath.mp.dps = 50
    k = Cs.neglog_words()
    for must in (0, 1, 2, 2 ** 32 - 2, 2 ** 32 - 1, 0xFEFFFFFF, 0xFF000000, 0xFF000001, 2 ** 31 - 1, 2 ** 31):
        assert must in k
    got = R.orc_map("orc_neglog_u32", k)
    worst = 0.0
    two32 = mpmath.mpf(2) ** 32
    for ki, gi in zip(k.tolist(), got.tolist()):
        want = -mpmath.log((mpmath.mpf(ki) + 0.5) / two32)
        worst = max(worst, float(abs((mpmath.mpf(gi) - want) / want)))
    print(f"orc_neglog_u32: worst relative error {worst / 2.0 ** -52:.3f} * 2^-52 on {len(k)} words")
    assert worst < 1.5 * 2.0 ** -52


# ---- phm_ll_device.h ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", Cs.LL_N)
def test_rescale_inputs_hold_every_case_and_scale_exactly(n):
    V = Cs.rescale_vectors(n)
    assert len(V) == len(Cs.RESCALE_KINDS) and not V[0].any() and V[1].max() == 1.0 and V[3].max() == 2.0 ** 1000
    assert 0.0 < V[2].max() < 2.0 ** -1022 and V[4].argmax() == n - 1 and (V >= 0.0).all()
    for v in V:
        got, e = R.ll_rescale(v)
        assert [Fraction(float(x)) for x in got] == [Fraction(float(x)) / Fraction(2) ** e for x in v]     # nothing rounds
        assert not v.any() or 0.5 <= got.max() < 1.0


@pytest.mark.parametrize("n", [3, 8])
def test_model_inputs_and_their_reference(n):
    Qs = Cs.model_matrices(n)
    assert not Qs[2].any() and (np.abs(Qs[:2].sum(axis=2)) < 1e-12).all() and Qs[1, n - 1, n - 1] == 0.0
    for Q in Qs:
        mu, Bm = R.model_mu_b(Q)
        assert mu == max(0.0, max(-Q[i, i] for i in range(n)))
        want = [[(1.0 if i == j else 0.0) + (Q[i, j] / mu if mu > 0.0 else 0.0) for j in range(n)] for i in range(n)]
        assert Bm.tolist() == want
    assert np.array_equal(R.model_mu_b(Qs[2])[1], np.eye(n))


# ---- the built harness ------------------------------------------------------------------------------------------------------------------
def test_harness_library_exports_every_declared_entry():
    """`make` builds it next to the library; opening it with ctypes resolves symbols only (no HIP call)"""
    assert os.path.exists(B.SO_PATH), "build/tests/libphm_device_blocks.so is missing: run make"
    L = C.CDLL(B.SO_PATH)
    missing = [name for name in B.ENTRIES if not hasattr(L, name)]
    assert not missing, missing
