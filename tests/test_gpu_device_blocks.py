"""The device building blocks of phm_device.h, phm_coop.h, phm_history.h and phm_ll_device.h, each run on its own through the test-only harness
tests/native/device_blocks.hip (built with the library's flags, the headers unchanged) and compared BIT FOR BIT with the
references of tests/blocksref.py and with the oracle's exported functions.  The inputs (tests/blockcases.py) are the ones
tests/test_device_blocks_cpu.py proves sharp and measures the oracle on, so equality with the oracle here inherits the ulp
bounds asserted there.

Lane contracts of the cooperative blocks, as found at their call sites (phm_wide.hip, phm_wbranch.hip) and as supplied here:
  coop_matvec, coop_matvec_lds   the caller passes row c = min(lane, n - 1); lanes >= n hold a finite copy of that row's entry and
                                 are never read as vector entries -- supplied: finite values found in no live lane; returned: row n - 1.
  coop_matvec_regs               masks lanes >= n itself (brow is zero beyond n) -- supplied: NaN.
  coop_matvec_ell                columns < n only, padding (column = own row, value 0) -- lanes >= n finite, never gathered.
  coop_matvec_band<HB>           lanes >= n hold FINITE values and coefficients are 0 where the matrix has no entry: lane n - 1 multiplies
                                 lane n's value by that 0.  What lanes >= n return is finite and otherwise unspecified.
  coop_sum, readlane_f64         read lanes < n only -- lanes >= n finite, distinct.
  coop_sample                    lanes >= n carry p = 0 (every caller selects 0 there).
  coop_sample_lds                masks lanes >= n itself -- supplied: NaN.
  wave_max_count, wave_max_w     all 64 lanes active, non-negative counts."""
import numpy as np
import pytest

import blockcases as Cs
import blocks_lib as B
import blocksref as R

pytestmark = pytest.mark.gpu


def same_bits(got, want, what=""):
    got, want = R.bits(got), R.bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]:#018x} want {want[tuple(bad[0])]:#018x}"


def wave_uniform(a, what=""):
    """every lane of a wave reports the value lane 0 reports"""
    a = np.asarray(a)
    bad = np.argwhere(a != a[:, :1])
    assert bad.size == 0, f"{what}: not wave-uniform, first at (wave, lane) {tuple(bad[0])}"


# ---- Philox, u01, streams ------------------------------------------------------------------------------------------------------
def test_philox_known_answers_and_random_blocks():
    ctr = np.array([k[0] for k in Cs.PHILOX7_KAT], dtype=np.uint32)
    key = np.array([k[1] for k in Cs.PHILOX7_KAT], dtype=np.uint32)
    assert B.philox(ctr, key).tolist() == [k[2] for k in Cs.PHILOX7_KAT]
    ctr, key = Cs.philox_random()
    assert np.array_equal(B.philox(ctr, key), R.orc_philox7(ctr, key))


def test_u01_is_exact():
    x = Cs.u01_words()
    got = B.u01(x)
    same_bits(got, (x.astype(np.float64) + 0.5) / 2.0 ** 32, "u01")          # exact in a double: 33 significant bits
    same_bits(got, R.orc_map("orc_u01", x), "u01 against the oracle")
    assert got[0] == 2.0 ** -33 and got[4] == 1.0 - 2.0 ** -33


@pytest.mark.parametrize("order", ["in_order", "out_of_order"])
def test_stream_draws_in_any_order(order):
    """Stream keeps one Philox block; a draw from another block -- ahead or BEHIND -- must replace it, and a draw is addressed by
    (replica, iteration, entity, d) alone.  Every lane has another address; all four ENT_* tags occur."""
    dseq = Cs.STREAM_IN_ORDER if order == "in_order" else Cs.STREAM_OUT_OF_ORDER
    rep, it, ent = Cs.stream_lanes()
    wk, uk, wf, uf = B.stream(*Cs.STREAM_SEED, rep, it, ent, dseq)
    w, u = R.orc_stream(*Cs.STREAM_SEED, rep, it, ent, dseq)
    for name, got in (("Stream::draw_word", wk), ("stream_word", wf)):
        bad = np.argwhere(got != w)
        assert bad.size == 0, f"{name}: first difference at (lane, position) {tuple(bad[0])}, draw {dseq[bad[0][1]]}"
    same_bits(uk, u, "Stream::draw")
    same_bits(uf, u, "stream_u")
    for lane in (0, 1, 2, 3, 319):                        # the addressing written out: counter = (d >> 2, entity, iteration, replica)
        for q, d in enumerate(dseq):
            assert int(wk[lane, q]) == R.stream_word_from_blocks(*Cs.STREAM_SEED, rep[lane], it[lane], ent[lane], d)


# ---- neglog_u32, phm_log, phm_exp --------------------------------------------------------------------------------------------------
def test_neglog_u32_equals_the_oracle_from_lds_and_from_global_memory():
    k = Cs.neglog_words()
    from_lds, from_global = B.neglog(k)
    want = R.orc_map("orc_neglog_u32", k)
    same_bits(from_lds, want, "neglog_u32, table in LDS")
    same_bits(from_global, want, "neglog_u32, table in global memory")


def test_phm_log_equals_the_oracle():
    x = Cs.log_inputs()
    same_bits(B.log(x), R.orc_map("orc_log", x), "phm_log")


def test_phm_exp_equals_the_oracle():
    x = Cs.exp_inputs()
    got, want = B.exp(x), R.orc_map("orc_exp", x)
    nan = np.isnan(want)
    assert nan.sum() == 1 and np.array_equal(np.isnan(got), nan)
    same_bits(got[~nan], want[~nan], "phm_exp")


# ---- n <= 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [2, 3, 4])
def test_matvec_u_is_left_to_right_and_unfused(ns):
    M, v = Cs.matvec_u_case(ns)
    want = np.array([R.matvec_unfused(M[i], v[i]) for i in range(len(v))])
    same_bits(B.matvec_u(M, v), want, f"matvec_u<{ns}>")


def _draw_reference(P, U):
    ref = [R.draw(p, u) for p, u in zip(P, U)]
    return np.array([r[0] for r in ref]), np.array([r[1] for r in ref])


def _check_draw(what, idx, err, P, U, kinds):
    want_idx, want_err = _draw_reference(P, U)
    for i, kind in enumerate(kinds):
        where = f"{what}, vector {i} ({kind}), p = {P[i][:8]}.., u = {U[i]!r}"
        assert err[i] == want_err[i], where
        assert (want_err[i] != 0) == (kind != "ok"), where
        if kind != "neg":
            assert idx[i] == want_idx[i], where


@pytest.mark.parametrize("ns", [2, 3, 4])
def test_sample_cat(ns):
    P, U, kinds = Cs.draw_case(ns)
    idx, err = B.sample_cat(P, U)
    _check_draw(f"sample_cat<{ns}>", idx, err, P, U, kinds)


# ---- the matrix-vector forms ------------------------------------------------------------------------------------------------------
def _check_product(what, n, got, want, upper):
    """lanes < n against the reference; lanes >= n: 'row' = the value of row n - 1 (the caller's clamped row), 'finite' = finite"""
    for step, (g, w) in enumerate(zip(got, want), 1):
        same_bits(g[:, :n], w, f"{what}, n = {n}, application {step} [vector, lane]")
        if n < 64:
            if upper == "row":
                same_bits(g[:, n:], np.repeat(w[:, n - 1:n], 64 - n, axis=1), f"{what}, n = {n}, application {step}, lanes >= n")
            else:
                assert np.isfinite(g[:, n:]).all()


@pytest.mark.parametrize("n", Cs.COOP_N)
def test_dense_products_are_fused_ascending_chains(n):
    M = Cs.with_stride(Cs.dense_matrix(n), n | 1)
    want = Cs.chain_reference("dense", n)
    for form in Cs.DENSE_FORMS:
        vin = Cs.pad_lanes(Cs.vectors(n), n, "nan" if form == "coop_matvec_regs" else "finite")
        _check_product(form, n, B.matvec(form, n, vin, M=M, ldn=n | 1), want, "row")


@pytest.mark.parametrize("w", Cs.ELL_W)
@pytest.mark.parametrize("n", Cs.COOP_N)
def test_ellpack_product_equals_the_dense_forms(n, w):
    M, ecol, ev = Cs.ell_matrix(n, w)
    want = Cs.chain_reference(f"ell{w}", n)
    vin = Cs.pad_lanes(Cs.vectors(n), n, "finite")
    _check_product(f"coop_matvec_ell w = {w}", n, B.matvec("coop_matvec_ell", n, vin, ecol=ecol, eval_=ev), want, "row")
    dense = B.matvec("coop_matvec_regs", n, Cs.pad_lanes(Cs.vectors(n), n, "nan"), M=Cs.with_stride(M, n | 1), ldn=n | 1)
    _check_product(f"coop_matvec_regs on the ELLPACK matrix w = {w}", n, dense, want, "row")


@pytest.mark.parametrize("hb", [1, 2])
@pytest.mark.parametrize("n", Cs.COOP_N)
def test_band_product_equals_the_dense_forms(n, hb):
    M, coef = Cs.band_matrix(n, hb)
    want = Cs.chain_reference(f"band{hb}", n)
    vin = Cs.pad_lanes(Cs.vectors(n), n, "finite")
    _check_product(f"coop_matvec_band<{hb}>", n, B.matvec(f"coop_matvec_band{hb}", n, vin, coef=coef), want, "finite")
    dense = B.matvec("coop_matvec", n, vin, M=Cs.with_stride(M, n | 1), ldn=n | 1)
    _check_product(f"coop_matvec on the band matrix hb = {hb}", n, dense, want, "row")


# ---- wave shifts, readlane, sums ----------------------------------------------------------------------------------------------------
def test_wave_shifts_move_all_64_bits_across_row_boundaries():
    wave, lane = np.meshgrid(np.arange(8, dtype=np.uint64), np.arange(64, dtype=np.uint64), indexing="ij")
    x = ((np.uint64(0xA5000000) | (wave << np.uint64(8)) | lane) << np.uint64(32)) | (np.uint64(0x3C000000) | (lane << np.uint64(12)) | wave)
    x[1, :] = np.uint64(0x7FF8DEAD00000000) | (np.uint64(0xBEEF0000) + lane[1])            # quiet NaNs with payloads
    x[2, 15], x[2, 16], x[2, 47], x[2, 48] = (np.uint64(v) for v in (0x7FF0000000000001, 0xFFF8000000000002, 0x8000000000000000, 0x0000000000000001))
    below, above = B.shift(x)
    zero = np.zeros((8, 1), np.uint64)
    for name, got, want in (("wave_from_below", below, np.concatenate([zero, x[:, :-1]], axis=1)),
                            ("wave_from_above", above, np.concatenate([x[:, 1:], zero], axis=1))):
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{name}: first wrong (wave, lane) {tuple(bad[0])}: got {got[tuple(bad[0])]:#018x} want {want[tuple(bad[0])]:#018x}"


@pytest.mark.parametrize("n", Cs.COOP_N)
def test_readlane_f64_and_coop_sum(n):
    V = Cs.sum_vectors(n)
    vin = Cs.pad_lanes(V, n, "finite")
    got = B.readlane(R.bits(vin), n)                                         # [wave, l, lane]
    want = np.repeat(R.bits(vin)[:, :n, None], 64, axis=2)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"readlane_f64: first wrong (wave, source lane, lane) {tuple(bad[0])}"
    s = B.coop_sum(vin, n)
    wave_uniform(R.bits(s), f"coop_sum n = {n}")
    same_bits(s[:, 0], np.array([R.coop_sum(v) for v in V]), f"coop_sum n = {n}")


# ---- cooperative draws ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", Cs.COOP_N)
def test_cooperative_draws(n):
    P, U, kinds = Cs.draw_case(n)
    results = {}
    for which, fill in (("coop_sample", "zero"), ("coop_sample_lds", "nan")):
        idx, err = B.coop_sample(which, n, Cs.pad_lanes(P, n, fill), U)
        wave_uniform(idx, f"{which} n = {n} index")
        wave_uniform(err, f"{which} n = {n} error word")
        _check_draw(f"{which} n = {n}", idx[:, 0], err[:, 0], P, U, kinds)
        results[which] = (idx, err)
    assert np.array_equal(results["coop_sample"][0], results["coop_sample_lds"][0])
    assert np.array_equal(results["coop_sample"][1], results["coop_sample_lds"][1])


# ---- wave maxima ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["count", "w"])
def test_wave_maximum_from_every_lane(which):
    v = Cs.wave_max_inputs()
    got = B.wave_max(which, v)
    wave_uniform(got, f"wave_max_{which}")
    bad = np.argwhere(got[:, 0] != v.max(axis=1))
    assert bad.size == 0, f"wave_max_{which}: wrong in wave {bad[0][0]} (waves 0 .. 63 hold their maximum in the lane of that number)"


def test_wave_minimum_idiom():
    v = Cs.wave_min_inputs()
    got = B.wave_max("min_idiom", v)
    wave_uniform(got, "65535 - wave_max_count(65535 - k)")
    bad = np.argwhere(got[:, 0] != v.min(axis=1))
    assert bad.size == 0, f"minimum idiom: wrong in wave {bad[0][0]}"


# ---- StatLanes, stat_cell_value ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fx_exp", [1, 11])
@pytest.mark.parametrize("ns", [0, 2, 3, 4])
def test_statlanes_fixed_point_cells(ns, fx_exp):
    case = Cs.stat_case(ns, fx_exp)
    n, ncount, inv = case["n"], case["ncount"], case["fx_inv"]
    args = [case[k] for k in ("ns", "n", "ncount", "dcol", "dx", "ccol", "cell", "live", "ncell", "fx_scale", "fx_inv", "dw_init", "ct_init")]
    dw, ct, vals = B.statlanes(*args)
    want_dw, want_ct = R.statlanes(n, ncount, case["dcol"].tolist(), case["dx"].tolist(), case["ccol"].tolist(), case["cell"].tolist(),
                                   case["live"].tolist(), case["ncell"], case["fx_scale"], case["dw_init"].tolist(), case["ct_init"].tolist())
    bad = np.argwhere(dw != np.array(want_dw, dtype=np.uint64))
    assert bad.size == 0, f"dwell cells: first wrong (column, cell) {tuple(bad[0])}"
    bad = np.argwhere(ct != np.array(want_ct, dtype=np.uint32))
    assert bad.size == 0, f"count cells: first wrong (column, cell) {tuple(bad[0])}"
    dead = case["cell"][case["live"] == 0]                                   # a lane that is not live adds nothing
    assert np.array_equal(dw[:, dead], case["dw_init"][:, dead]) and np.array_equal(ct[:, dead], case["ct_init"][:, dead])
    want_vals = np.array([[R.from_fixed(c, inv) for c in row] for row in want_dw] + [[float(c) for c in row] for row in want_ct])
    same_bits(vals, want_vals, "stat_cell_value")
    re = Cs.stat_reordered(case)                                             # exact in any order
    dw2, ct2, vals2 = B.statlanes(*[re[k] for k in ("ns", "n", "ncount", "dcol", "dx", "ccol", "cell", "live", "ncell", "fx_scale", "fx_inv",
                                                    "dw_init", "ct_init")])
    assert np.array_equal(dw2, dw) and np.array_equal(ct2, ct)
    same_bits(vals2, vals, "stat_cell_value after reordering")


# ---- phm_ll_device.h: the rescale rule through the state-count dispatch, mu_k and B_k ------------------------------------------------
@pytest.mark.parametrize("n", Cs.LL_N)
def test_ll_rescale_through_ll_with_states(n):
    V = Cs.rescale_vectors(n)
    got, e = B.ll_rescale(V)
    want = [R.ll_rescale(v) for v in V]
    for i, kind in enumerate(Cs.RESCALE_KINDS):
        assert e[i] == want[i][1], f"ll_rescale<{n}> ({kind}): exponent {e[i]}, want {want[i][1]}"
        same_bits(got[i], want[i][0], f"ll_rescale<{n}> ({kind})")
    assert e[0] == 0 and e[1] == 1 and e[2] < -1021 and e[3] == 1001
    same_bits(got[0], V[0], "an all-zero vector is left as it is")
    assert 0.5 <= got[1:].max(axis=1).min() and got[1:].max() < 1.0 and got[4].argmax() == n - 1


@pytest.mark.parametrize("n", [3, 8])
def test_model_mu_and_b(n):
    Qs = Cs.model_matrices(n)
    mu, Bs = B.model(Qs)
    for k, Q in enumerate(Qs):
        want_mu, want_B = R.model_mu_b(Q)
        same_bits(mu[k], want_mu, f"model_mu, n = {n}, matrix {k}")
        same_bits(Bs[k], want_B, f"model_b, n = {n}, matrix {k}")
    assert mu[2] == 0.0 and np.array_equal(Bs[2], np.eye(n))
