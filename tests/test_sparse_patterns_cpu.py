"""The pattern-generated sparse pruning kernel (phm_rtc.cpp) on the patterns of tests/sparsepatterns.py, without a GPU: the
generated text against the matrix it was generated for (rows, not columns; coefficient indices in CSR order; N / NP), a
cross-compile per state count, and the input conditions of every run tests/test_gpu_sparse_patterns.py compares with the oracle
-- so a bad input never shows up on the GPU first."""
import os
import re
import shutil
import subprocess
import tempfile
import time

import numpy as np
import pytest

import oracle_lib as O
import sparsepatterns as sp
from phylomap_amd import _lib, synth

NAMES = list(sp.CASES)


def check_source(src, M):
    """the generated kernel text belongs to the matrix M: one fused multiply-add per non-zero; row i's line reads x[] at the
    ascending non-zero columns of ROW i and C[] at row_ptr[i] .. row_ptr[i+1]-1 in order; N and NP"""
    n = M.shape[0]
    assert src.count("__builtin_fma(") == np.count_nonzero(M)
    assert re.findall(r"#define N (\d+)\n#define NP (\d+)\n", src) == [(str(n), str((n + 3) // 4 * 4))]
    lines = src.splitlines()
    k0 = 0
    for i in range(n):
        line, = [ln for ln in lines if f" y[{i}] = a; }}" in ln]
        terms = [(int(c), int(x)) for c, x in re.findall(r"a = __builtin_fma\(C\[(\d+)\], x\[(\d+)\], a\);", line)]
        assert line.count("__builtin_fma(") == len(terms)
        cols = np.nonzero(M[i])[0].tolist()
        assert [x for _, x in terms] == cols, (i, terms)
        assert [c for c, _ in terms] == list(range(k0, k0 + len(cols))), (i, terms)
        k0 += len(cols)
    assert k0 == np.count_nonzero(M)
    assert len([ln for ln in lines if re.search(r" y\[\d+\] = a; }", ln)]) == n


@pytest.mark.parametrize("name", NAMES)
def test_cases_stay_in_their_class(name):
    """the predicates sparsepatterns.py asserts at import, repeated: no case drifts to the band kernels, over half fill (one
    case: exactly one non-zero over), to a pattern with fewer than n one-way entries, or to symmetric values"""
    Q = sp.case_Q(name)
    n = Q.shape[0]
    B, Bc = sp.chain_matrices(Q)
    i, j = np.nonzero(Bc)
    hb = int(np.abs(i - j).max())
    assert hb > sp.WT_BAND_MAX or 2 * hb + 1 >= n
    if name == "top32_over":
        assert np.count_nonzero(Bc) == 513 > sp.RTC_SPARSE_MAX_FILL * n * n
    else:
        assert np.count_nonzero(Bc) <= sp.RTC_SPARSE_MAX_FILL * n * n
    assert np.count_nonzero((Bc != 0) & (Bc.T == 0)) >= n
    assert not np.array_equal(B, B.T) and not np.array_equal(Bc, Bc.T)
    assert 5 <= n <= sp.RTC_SPARSE_NMAX
    assert sp.omega_of(Q) == 1.25 * np.abs(np.diag(Q)).max() and np.allclose(Q.sum(1), 0, atol=1e-15)
    off = Q[~np.eye(n, dtype=bool)]
    big = off[off > 1e-6]
    assert big.min() >= 0.02 and big.max() <= 0.3
    if name != "tiny10":
        assert np.array_equal(B, Bc)
    sp.check_case(name)


@pytest.mark.parametrize("name", NAMES)
def test_generated_text_belongs_to_the_matrix(name):
    Bc = sp.chain_matrices(sp.case_Q(name))[1]
    check_source(_lib.sparse_kernel_source(Bc), Bc)


@pytest.mark.parametrize("name", NAMES)
def test_text_check_rejects_the_kernel_of_the_transposed_pattern(name):
    """what the check above is for: the source generated for Bc^T (rows taken from columns) does not pass it for Bc -- on every
    pattern here.  On synth.neighbour_Q(20, 6), the one matrix the kernel had been run on, the two sources are the same text."""
    Bc = sp.chain_matrices(sp.case_Q(name))[1]
    with pytest.raises(AssertionError):
        check_source(_lib.sparse_kernel_source(Bc.T.copy()), Bc)
    Qn = synth.neighbour_Q(20, 6)
    Bn = np.eye(20) + Qn / sp.omega_of(Qn)
    assert _lib.sparse_kernel_source(Bn) == _lib.sparse_kernel_source(Bn.T.copy()) and np.array_equal(Bn, Bn.T)


_ONE_PER_N = {}
for _c in NAMES:
    _ONE_PER_N.setdefault(sp.CASES[_c]["n"], _c)


@pytest.mark.parametrize("n", sorted(_ONE_PER_N))
def test_generated_kernel_compiles_for_gfx950_at_every_state_count(n):
    """hipcc with hipRTC's options (phm_rtc.cpp) on the source of one pattern per distinct n; ~1 s each"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = _lib.sparse_kernel_source(sp.chain_matrices(sp.case_Q(_ONE_PER_N[n]))[1])
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "k.hip")
        with open(f, "w") as fh:
            fh.write(src)
        t0 = time.time()
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-c", f, "-o", os.path.join(d, "k.o")],
                           capture_output=True, text=True)
        print(f"n = {n}: hipcc {time.time() - t0:.2f} s")
        assert r.returncode == 0, r.stderr[-2000:]


def _good_input(p, variant, replicas, sites):
    for r in replicas:
        rows, rc = sp.oracle_rows(p, variant, r, sites)
        assert rc == 0, (p.name, variant, r, rc)
        assert sp.transitions(rows, p.n, variant).min() >= 1, (p.name, variant, r)
        np.testing.assert_allclose(rows[:, :p.n].sum(1), p.length, rtol=1e-11, atol=0)


def test_every_compared_run_is_a_good_input_on_the_oracle():
    """rc == 0 for each compared replica, at least one transition in every sweep, dwell sums = tree length to 1e-11"""
    runs = sp.compared_runs()
    assert len(runs) == 2 * len(sp.GENERATED) + len(sp.SPARSE_DRIVER_RUNS) + 1 + len(sp.LAYOUT_RUNS) + len(sp.SITE_CASES)
    for p, variant, replicas, sites in runs:
        _good_input(p, variant, replicas, sites)
    p = sp.problem("odd7")
    assert not np.array_equal(sp.oracle_rows(p, "bigtree", 0, True)[0], sp.oracle_rows(p, "bigtree", 0, False)[0])      # own tips


def test_set_model_cycle_keeps_the_chain_state_possible():
    """the Q1 -> Q2 -> Q3 -> Q1 cycle of the GPU test: three different patterns of B (sparse, sparse, full), and the oracle, carried
    through the same cycle from its own dumped paths (other random numbers than the engine's, the same distribution), never meets
    a zero probability vector.  With ordinary rates on the added entries it does: see sparsepatterns.set_model_cycle."""
    p = sp.problem("pad9")
    Q1, Q2, Q3 = sp.set_model_cycle()
    n = 9
    pats = [np.eye(n) + Q / p.Omega != 0 for Q in (Q1, Q2, Q3)]
    assert np.count_nonzero(pats[0]) < np.count_nonzero(pats[1]) <= sp.RTC_SPARSE_MAX_FILL * n * n and pats[2].all()
    assert np.all(pats[1][pats[0]]) and sp.one_way_entries(pats[1]) >= n
    for Q in (Q2, Q3):
        assert np.all(np.eye(n) + Q / p.Omega >= 0)
        added = np.where(Q1 == 0, Q, 0.0)
        assert 0 < added[added > 0].min() and added.max() <= 1e-9
        assert sp.S_REPLICAS * p.length * added.sum(1).max() < 1e-3 / 2         # expected jumps through added entries, one sweep of every chain
        assert np.all(Q[Q1 > 0] <= Q1[Q1 > 0]) and not np.any(Q[Q1 > 0] == Q1[Q1 > 0])

    def carry_on(z, Q, sweeps, r, seed):
        _, rc, d = O.maketreelistMCMC(z, Q, p.pid, np.eye(n) + Q / p.Omega, p.Omega, p.nen, p.nodelist, p.root, sweeps,
                                      variant=O.BIGTREE, seed=seed, replica=r, dump=True)
        assert rc == 0, (r, rc)
        m = d.seg_count
        return dict(z, maps=[d.seg_dwell[b, :m[b]].copy() for b in range(len(m))], mapnames=[d.seg_state[b, :m[b]].copy() for b in range(len(m))])

    for r in range(sp.S_REPLICAS):
        z = carry_on(p.z, Q1, 2, r, p.seed)
        for k, (Q, sweeps) in enumerate(((Q2, 1), (Q3, 1), (Q1, 2))):
            z = carry_on(z, Q, sweeps, r, p.seed + 1 + k)


def test_random_cases_are_in_the_class_and_at_most_two_are_left_out():
    """the twelve seeded random patterns: accepted by the predicates, deterministic (redraws included), every n of the list once,
    and the oracle refuses at most 2 of them (those the GPU test leaves out); the rest are good inputs"""
    left_out, ns = 0, []
    for k in range(sp.N_RANDOM):
        p, variant, S, redraws = sp.random_case(k)
        sp.random_case.cache_clear()
        p2, variant2, S2, redraws2 = sp.random_case(k)
        assert np.array_equal(p.Q, p2.Q) and (variant, S, redraws, p.seed) == (variant2, S2, redraws2, p2.seed)
        assert np.array_equal(p.z["edge"], p2.z["edge"])
        assert sp.accepted(p.Q) and np.array_equal(p.B, p.Bc)
        n = p.n
        assert 2 * n + 1 <= np.count_nonzero(p.Bc) <= sp.RTC_SPARSE_MAX_FILL * n * n
        assert variant in ("bigtree", "plain", "sparse_rescaled") and S in (3, 70, 130)
        ns.append(n)
        if any(sp.oracle_rows(p2, variant, r)[1] != 0 for r in sp.replicas_of(S)):
            left_out += 1
        else:
            _good_input(p2, variant, sp.replicas_of(S), False)
    assert sorted(ns) == sorted(sp.RANDOM_NS)
    assert left_out <= 2
