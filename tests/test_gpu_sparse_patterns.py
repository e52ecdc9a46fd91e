"""The pattern-generated sparse pruning kernel (phm_rtc.cpp, chosen in upload_model) beyond the one symmetric matrix it had been
run on: the unstructured NON-symmetric patterns of tests/sparsepatterns.py -- odd n, padding rows, n = 5 and n = 32, a full row
next to rows of two, the fill and LDS-slot boundaries -- under every driver that can reach the kernel (BIGTREE, PLAIN, the SPARSE
threshold, parity-observed tips, the n + n^2 layout, per-replica tips, set_model).  Every case asserts which pruning kernel
served it (info().sparse_chains & 4), is compared with the CPU oracle (counts exact, dwell rtol 1e-10, the partial likelihoods
of a dumped replica bit for bit) and, every replica and sweep, with the matrix-core kernels (sparse_chains = 2) bit for bit.
24 tips (40 at n >= 31), 5 sweeps, 70 replicas = two tiles, the second holding 6 lanes."""
import numpy as np
import pytest

import sparsepatterns as sp
from phylomap_amd import _lib, api
from test_gpu_configs import WIDE_MAPPINGS, _check_dump, _check_ks_rows, _check_rows

pytestmark = pytest.mark.gpu

N, S = sp.N_SWEEPS, sp.S_REPLICAS
DUMP_KEYS = ("seg_count", "node_states", "PL", "seg_dwell")


def _engine(p, variant, S=S, **opt):
    ev, _, rescale = sp.VARIANTS[variant]
    return _lib.Engine(p.tree(variant), p.Q, p.pid, p.Omega, N, variant=ev, seed=p.seed, n_replicas=S, mapping="tiles", rescale=rescale, **opt)


def _run(p, variant, S=S, **opt):
    """(info().sparse_chains, stats [S, N, cols], the dump of every replica) after N sweeps"""
    eng = _engine(p, variant, S, **opt)
    eng.run(N); eng.sync()
    res = (eng.info().sparse_chains, eng.stats(0, N), [eng.dump(r) for r in range(S)])
    eng.close()
    return res


def _same_as(a, b):
    """every replica and sweep of two runs: statistics and chain state bit for bit"""
    np.testing.assert_array_equal(a[1], b[1])
    assert len(a[2]) == len(b[2])
    for da, db in zip(a[2], b[2]):
        for key in DUMP_KEYS:
            np.testing.assert_array_equal(da[key], db[key])


def _against_oracle(p, variant, run, replicas, sites=False):
    _, st, dumps = run
    for r in replicas:
        want, rc = sp.oracle_rows(p, variant, r, sites)
        assert rc == 0
        if variant in ("ks", "bf"):
            _check_ks_rows(st[r], want, p.n)
        else:
            _check_rows(st[r], want, p.n, False)
    np.testing.assert_allclose(st[:, :, :p.n].sum(2), p.length, rtol=1e-11)          # every replica, every sweep
    if not sites:
        r = replicas[-1]
        _, rc, dump = sp.oracle_dump(p, variant, r)
        assert rc == 0
        d = dumps[r]
        if variant == "ks":      # the tips are re-sampled inside the parity class: the engine's dump reports the observed class there
            d = dict(d, node_states=np.concatenate([dump.node_states[:p.tips], d["node_states"][p.tips:]]),
                     PL=np.concatenate([dump.PL[:p.tips], d["PL"][p.tips:]]))
        _check_dump(d, dump)


def _refused(p, variant, **opt):
    with pytest.raises(_lib.PhmError) as e:
        _engine(p, variant, **opt)
    assert e.value.status == 2


def _generated_kernel_case(p, variant, S=S, replicas=sp.REPLICAS):
    """sparse_chains = 1: the generated kernel ran (bit 2; bit 0 with it; no band draws on an unstructured B) -- against the
    oracle and against the matrix cores; the automatic choice takes the generated kernel too"""
    gen = _run(p, variant, S, sparse_chains=1)
    assert gen[0] == 5
    eng = _engine(p, variant, S)
    assert eng.info().sparse_chains & 4
    eng.close()
    _against_oracle(p, variant, gen, replicas)
    dense = _run(p, variant, S, sparse_chains=2)
    assert dense[0] == 0
    _same_as(gen, dense)


@pytest.mark.parametrize("variant", ["bigtree", "plain"])
@pytest.mark.parametrize("name", sp.GENERATED)
def test_generated_kernel_on_every_named_pattern(name, variant):
    _generated_kernel_case(sp.problem(name), variant)


@pytest.mark.parametrize("name,variant", [r for r in sp.SPARSE_DRIVER_RUNS if r[1] != "bigtree"])
def test_sparse_driver_thresholded_chain_matrix(name, variant):
    """the SPARSE driver (chain matrix thresholded at 1e-7, dense forward rows), rescaled and -- on tiny10 -- as the reference
    has it.  tiny10's B is dense and only its thresholded Bc is sparse: the kernel is generated for Bc."""
    p = sp.problem(name)
    assert (np.count_nonzero(p.Bc) < np.count_nonzero(p.B)) == (name == "tiny10")
    _generated_kernel_case(p, variant)


def test_dense_chain_matrix_of_the_thresholded_case_goes_to_the_matrix_cores():
    """BIGTREE on tiny10's Q: no thresholding, Bc = B is full -- matrix cores, and sparse_chains = 1 is refused"""
    p = sp.problem("tiny10")
    run = _run(p, "bigtree")
    assert run[0] == 0
    _against_oracle(p, "bigtree", run, sp.REPLICAS)
    _refused(p, "bigtree", sparse_chains=1)


def test_fill_boundary_and_state_count_limit():
    """512 of 1 024 non-zeros get the generated kernel (test_generated_kernel_on_every_named_pattern[top32_half]); 513 do not and
    still match the oracle; requiring the kernel there, or for 33 states, is refused with status 2"""
    eng = _engine(sp.problem("top32_half"), "bigtree")
    assert eng.info().sparse_chains == 5
    eng.close()
    p = sp.problem("top32_over")
    run = _run(p, "bigtree")
    assert run[0] & 4 == 0 and run[0] == 0
    _against_oracle(p, "bigtree", run, sp.REPLICAS)
    _refused(p, "bigtree", sparse_chains=1)
    n = sp.RTC_SPARSE_NMAX + 1
    p33 = sp.Problem("n33", sp.pattern_Q(n, 3 * n, 0x5A33), 0x5EED1033, 33)
    assert sp.accepted(p33.Q)
    _refused(p33, "bigtree", sparse_chains=1)
    eng = _engine(p33, "bigtree")
    assert eng.info().sparse_chains == 0
    eng.close()


@pytest.mark.parametrize("name,variant", sp.LAYOUT_RUNS)
def test_parity_tips_and_the_n_plus_n2_layout(name, variant):
    """ks: only the parity of a tip state is observed (tip_masks: the tip rows of the generated kernel come from the mask
    table), tips re-sampled; bf: observed tips; both count n x n pairs, self pairs included, so the LDS slots of the branch kernel
    number count_nonzero(B) -- 44 <= 96 on even12_parity (slots on), 120 on slots24_96 (off there, on in the n (n-1) layout).
    The one-shot calls against the oracle; an engine with the same arguments says which kernel served them."""
    p = sp.problem(name)
    n = p.n
    fn = api.sumstatMCMCks_sweep if variant == "ks" else api.sumstatMCMCbf_sweep
    got = fn(p.tree(variant), p.Q, p.pid, p.Omega, N, seed=p.seed, n_replicas=S, mapping="tiles", sparse_chains=1)
    assert got.shape == (S, N, n + n * n + (2 + 3 * (n // 2 - 1) + 1 if variant == "ks" else 3))
    gen = _run(p, variant, sparse_chains=1)
    assert gen[0] == 5
    np.testing.assert_array_equal(gen[1], got)
    eng = _engine(p, variant)
    assert eng.info().sparse_chains & 4
    eng.close()
    _against_oracle(p, variant, gen, sp.REPLICAS)
    cnt = got[:, :, n:n + n * n].reshape(S, N, n, n)
    assert np.all(cnt[:, :, p.B == 0] == 0) and cnt[:, :, np.eye(n, dtype=bool)].sum() > 0      # self pairs are counted, impossible pairs never
    dense = _run(p, variant, sparse_chains=2)
    assert dense[0] == 0
    _same_as(gen, dense)


@pytest.mark.parametrize("name", sp.SITE_CASES)
def test_per_replica_tips(name):
    """tips_per_replica: every lane prunes from its own tip rows -- replicas 0, 63, 69 against the oracle, each on its own tips;
    the reduced output is the sum of the per-replica rows"""
    p = sp.problem(name)
    n = p.n
    sites = np.array(sp.site_tips(name))
    runs = {}
    for sc in (1, 2):
        runs[sc] = _run(p, "bigtree", sparse_chains=sc, tips_per_replica=True, states=sites)
        assert runs[sc][0] == (5 if sc == 1 else 0)
    _against_oracle(p, "bigtree", runs[1], sp.REPLICAS, sites=True)
    _same_as(runs[1], runs[2])
    st = runs[1][1]
    eng = _engine(p, "bigtree", sparse_chains=1, tips_per_replica=True, states=sites, reduce=True)
    eng.run(N); eng.sync()
    assert eng.info().sparse_chains == 5
    red = eng.stats(0, N)
    eng.close()
    np.testing.assert_array_equal(red[:, n:], st.sum(0)[:, n:])
    np.testing.assert_allclose(red[:, :n], st.sum(0)[:, :n], rtol=1e-12)


def test_set_model_changes_the_pattern():
    """one engine through pad9's pattern -> another 9-state pattern (a new kernel) -> a Q without a zero (matrix cores) -> the first
    pattern again (the cached kernel, fresh coefficients); 2 + 1 + 1 + 2 sweeps, the phases of two as two run(1) calls.  The
    automatic choice reports 5, 5, 0, 5; statistics and the final chain state of every replica equal those of an engine held on
    the matrix cores through the same calls.  (sparsepatterns.set_model_cycle says why the added entries carry tiny rates.)"""
    p = sp.problem("pad9")
    Q1, Q2, Q3 = sp.set_model_cycle()
    assert Q1 is p.Q and not np.array_equal(Q1 != 0, Q2 != 0)
    res = {}
    for sc in (0, 2):
        eng = _lib.Engine(p.z, Q1, p.pid, p.Omega, 6, variant=_lib.PHM_MCMC_BIGTREE, seed=p.seed, n_replicas=S, mapping="tiles", sparse_chains=sc)
        seen = []
        for Q, sweeps in ((None, 2), (Q2, 1), (Q3, 1), (Q1, 2)):
            if Q is not None:
                eng.set_model(Q)
            for _ in range(sweeps):
                eng.run(1)
            eng.sync()
            seen.append(eng.info().sparse_chains)
        assert seen == ([5, 5, 0, 5] if sc == 0 else [0, 0, 0, 0])
        res[sc] = (seen, eng.stats(0, 6), [eng.dump(r) for r in range(S)])
        eng.close()
    _same_as(res[0], res[2])
    st = res[0][1]
    np.testing.assert_allclose(st[:, :, :9].sum(2), p.length, rtol=1e-11)
    assert st[:, :, 9:].sum((0, 2)).min() > 0
    for r in sp.REPLICAS:                                                    # the two sweeps before the first update are the oracle's
        want, rc = sp.oracle_rows(p, "bigtree", r)
        assert rc == 0
        _check_rows(st[r][:2], want[:2], 9, False)
        assert not np.array_equal(st[r][2:, 9:], want[2:, 9:])              # ... and the later ones saw other rates


def test_set_model_keeps_the_pattern():
    """tri8, Q -> 0.9 Q: the kernel of the pattern with new coefficients"""
    p = sp.problem("tri8")
    res = {}
    for sc in (1, 2):
        eng = _engine(p, "bigtree", sparse_chains=sc)
        eng.run(2); eng.sync()
        assert eng.info().sparse_chains == (5 if sc == 1 else 0)
        eng.set_model(p.Q * 0.9)
        eng.run(N - 2); eng.sync()
        assert eng.info().sparse_chains == (5 if sc == 1 else 0)
        res[sc] = (None, eng.stats(0, N), [eng.dump(r) for r in range(S)])
        eng.close()
    _same_as(res[1], res[2])
    for r in sp.REPLICAS:
        want, rc = sp.oracle_rows(p, "bigtree", r)
        assert rc == 0
        _check_rows(res[1][1][r][:2], want[:2], p.n, False)
        assert not np.array_equal(res[1][1][r][2:, p.n:], want[2:, p.n:])              # the new rates took effect


# the oracle's verdict on the inputs decides which random cases run (tests/test_sparse_patterns_cpu.py: at most 2 are left out)
RANDOM_KS = [k for k in range(sp.N_RANDOM)
             if all(sp.oracle_rows(sp.random_case(k)[0], sp.random_case(k)[1], r)[1] == 0 for r in sp.replicas_of(sp.random_case(k)[2]))]


@pytest.mark.parametrize("k", RANDOM_KS)
def test_seeded_random_patterns(k):
    p, variant, S_k, _ = sp.random_case(k)
    _generated_kernel_case(p, variant, S_k, sp.replicas_of(S_k))


@pytest.mark.parametrize("mapping", [m for m in WIDE_MAPPINGS if m != "tiles"])
@pytest.mark.parametrize("name", ["ring5", "tri8", "odd21"])
def test_other_mappings_on_asymmetric_unstructured_patterns(name, mapping):
    """"replicas" and "branches" do not use the generated kernel; an asymmetric unstructured Q goes through them once"""
    p = sp.problem(name)
    got = api.sumstatMCMC_bigtree(p.z, p.Q, p.pid, p.Omega, N, seed=p.seed, n_replicas=S, mapping=mapping)
    for r in sp.REPLICAS:
        want, rc = sp.oracle_rows(p, "bigtree", r)
        assert rc == 0
        _check_rows(got[r], want, p.n, False)
    np.testing.assert_allclose(got[:, :, :p.n].sum(2), p.length, rtol=1e-11)
