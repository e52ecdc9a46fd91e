"""The per-branch expectations under many rate matrices without a device (phm_expected_branch_stats_models, DESIGN.md section
27): where the symbol is declared and bound, every refusal of the entry point before its first device call by status and message,
the pure host pieces (edge selection, label weights, the limit on mu t_b, the chunk plan) in a stand-alone program under
AddressSanitizer and UBSan, the two documented orders of addition (``branchrowscases``) pinned against the twin, and the label
helpers of ``ratemodel``.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

import branchrowscases as bc
import exactref
from phylomap_amd import _lib, ancestral, api, ratemodel, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "phm_expected_branch_stats_models"


def test_symbol_is_declared_apart_and_bound_to_the_prototype():
    L = _lib.load()
    assert hasattr(L, NAME) and _lib.EXT4_EXPORTS == [NAME]
    assert NAME not in _lib.EXPORTS + _lib.EXT_EXPORTS + _lib.EXT2_EXPORTS + _lib.EXT3_EXPORTS
    assert _lib.EXT3_EXPORTS == ["phm_expected_stats_models_wide"] and _lib.EXT2_EXPORTS == ["phm_gibbs_rates_wide"]
    assert _lib.EXT_EXPORTS == ["phm_sample_histories_models_wide"]
    assert L.phm_version() == 300
    i32, pi, pd = C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double)
    totals = list(L.phm_expected_stats_models.argtypes)
    # the first nine arguments are phm_expected_stats_models', then n_edges, edges, n_labels, labels, branch, loglik
    assert list(getattr(L, NAME).argtypes) == totals[:9] + [i32, pi, i32, pd, pd, pd]
    inc = os.path.join(ROOT, "include")
    for name in ("phylomap_hip.h", "phylomap_hip_ext.h", "phylomap_hip_ext2.h", "phylomap_hip_ext3.h"):
        assert NAME not in open(os.path.join(inc, name)).read()
    ext4 = open(os.path.join(inc, "phylomap_hip_ext4.h")).read()
    assert re.findall(r"\b(phm_[A-Za-z0-9_]+)\s*\(", ext4) == [NAME] and '#include "phylomap_hip_ext3.h"' in ext4
    proto = re.search(NAME + r"\s*\(([^;]*)\)\s*;", ext4).group(1)
    kinds = [re.sub(r"\s*\w+$", "", a.strip().replace("const ", "")) for a in proto.split(",")]   # each argument's type
    assert kinds == ["phm_tree*", "int32_t", "int32_t", "double*", "double*", "int32_t", "int32_t*", "int32_t*", "phm_options*",
                     "int32_t", "int32_t*", "int32_t", "double*", "double*", "double*"]
    assert NAME in api.expected_branch_stats_models.__doc__
    mk = open(os.path.join(ROOT, "Makefile")).read()
    for f in ("phm_branch_rows.hip", "phm_branch_rows_wide.hip", "phm_branch_rows_api.cpp", "include/phylomap_hip_ext4.h"):
        assert f in mk


def _raw(z, Qs, pid, S=2, edges=None, n_edges=None, labels=None, n_labels=None, branch=True, ll=True, tree=True, q=True, p=True):
    """one call of the entry point with the tree's tips tiled S times -> (status, message)"""
    Qs = np.asarray(Qs, dtype=np.float64)
    K, n = Qs.shape[0], Qs.shape[1]
    E = np.asarray(z["edge"]).shape[0]
    Qf = np.ascontiguousarray(Qs.transpose(0, 2, 1))
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    pt = _lib.PlainTree(z, np.tile(z["states"], (S, 1)))
    o = _lib.make_options(n_replicas=S, tips_per_replica=True)
    sel = None if edges is None else np.ascontiguousarray(edges, dtype=np.int32)
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.float64)
    ne = (0 if sel is None else sel.size) if n_edges is None else n_edges
    nl = (0 if lab is None else lab.shape[0]) if n_labels is None else n_labels
    lik = np.zeros(K * S) if ll else None
    br = np.zeros(K * S * max(n * n, nl, 1) * max(E, ne, 1)) if branch else None
    L = _lib.load()
    status = getattr(L, NAME)(C.byref(pt.c) if tree else None, n, K, _lib._p(Qf, C.c_double) if q else None,
                              _lib._p(pid, C.c_double) if p else None, pid.size // n, None, None, C.byref(o), ne,
                              _lib._p(sel, C.c_int32), nl, _lib._p(lab, C.c_double), _lib._p(br, C.c_double), _lib._p(lik, C.c_double))
    return status, L.phm_last_error().decode()


def _random_Q(n, rs):
    Q = rs.uniform(0.05, 1.0, (n, n)) * 4.0 / n
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q


def test_refusals_need_no_device():
    L = _lib.load()
    T = 16
    edge, lens = synth.random_tree(T, 0.5, 3)
    z = {"edge": edge, "edge.length": lens, "Nnode": T - 1, "states": np.ones(T, dtype=np.int32)}
    E = edge.shape[0]
    rs = np.random.default_rng(3)
    for n in (4, 9):                                                           # both families share every check
        Qs = np.stack([_random_Q(n, rs) for _ in range(3)])
        pid = np.ones(n)
        lab = rs.uniform(-1.0, 1.0, (2, n, n))
        for missing in ("tree", "q", "p", "branch"):
            st, msg = _raw(z, Qs, pid, **{missing: False})
            assert st == 1 and msg.startswith(NAME + ": NULL argument"), (missing, st, msg)
        bad = Qs.copy()
        bad[2, 0, 3], bad[2, 0, 1] = -0.05, bad[2, 0, 1] + 0.05                # ll_validate's checks, under this name where it names one
        st, msg = _raw(z, bad, pid)
        assert st == 1 and msg.startswith("model 2")
        st, msg = _raw(z, Qs, np.ones(2 * n))                                  # n_pid = 2 with 3 models
        assert st == 1 and msg.startswith(NAME + ": n_pid")
        for e in (-1, E):                                                      # an edge row outside [0, E): the position is named
            st, msg = _raw(z, Qs, pid, edges=[0, 3, e, 1])
            assert st == 1 and msg.startswith(NAME + ": edges[2] = " + str(e)), msg
        st, msg = _raw(z, Qs, pid, edges=[0, 1], n_edges=0)
        assert st == 1 and msg.startswith(NAME + ": n_edges must be >= 1"), msg
        st, msg = _raw(z, Qs, pid, edges=[0, 1], n_edges=-3)
        assert st == 1 and msg.startswith(NAME + ": n_edges must be >= 1"), msg
        st, msg = _raw(z, Qs, pid, labels=lab, n_labels=0)
        assert st == 1 and msg.startswith(NAME + ": n_labels must be >= 1"), msg
        for v in (np.nan, np.inf, -np.inf):
            poisoned = lab.copy()
            poisoned[1, 2, 1] = v
            st, msg = _raw(z, Qs, pid, labels=poisoned)
            assert st == 1 and msg.startswith(NAME + ": label 1 has a non-finite weight"), msg
        fast = Qs.copy()
        fast[1] *= 1e7                                                         # mu t_b above 1e6 on the longer branches
        mu = float(np.max(-np.diag(fast[1])))
        over = mu * lens > 1e6
        first = int(np.argmax(over))
        assert over[first] and not np.all(over)
        st, msg = _raw(z, fast, pid)
        assert st == 2 and msg == NAME + f": model 1, edge row {first + 1}: max(-q_ii) * t_b above 1e6", msg
        order = [int(b) for b in np.flatnonzero(over)[::-1]]                   # the first SELECTED edge over the limit is named
        st, msg = _raw(z, fast, pid, edges=order)
        assert st == 2 and f"model 1, edge row {order[0] + 1}:" in msg, msg
        if L.phm_device_count() == 0:                                          # a valid call gets as far as the device
            assert _raw(z, Qs, pid)[0] == 3
            assert _raw(z, Qs, pid, ll=False)[0] == 3                          # loglik may be NULL
            assert _raw(z, Qs, pid, edges=[E - 1, 0, 0], labels=lab)[0] == 3
            under = [int(b) for b in np.flatnonzero(~over)]                    # edges that are not selected are not held to the limit
            assert _raw(z, fast, pid, edges=under)[0] == 3
    for n in (1, 65):
        st, msg = _raw(z, np.zeros((1, n, n)), np.ones(n))
        assert st == 1 and msg.startswith(NAME + ": ") and "2..64" in msg, msg


def test_host_pieces_under_sanitizers(tmp_path):
    """tests/native/branch_rows_host_check.cpp: the edge selection, the label weights, the limit on mu t_b and the chunk plan of
    phm_branch_rows_host.h, host code only, under AddressSanitizer and UBSan; it checks itself and prints what it planned"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    exe = str(tmp_path / "branch_rows_host_check")
    csrc = os.path.join(ROOT, "phylomap_amd", "csrc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "native", "branch_rows_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok"
    scratch = 256 << 20
    plans = [ln.split() for ln in lines if ln.startswith("plan ")]
    assert len(plans) >= 20
    for _, n, labels, unit, kc0, sc0, chunk, n_sel, kc, sc, ne in (tuple(p[:1]) + tuple(int(v) for v in p[1:]) for p in plans):
        cell = 8 * max(n * n, labels)
        assert 1 <= ne <= n_sel and unit <= kc <= max(kc0, unit) and 1 <= sc <= sc0 and kc % unit == 0
        if chunk > 0:
            assert ne <= chunk
        if kc > unit or sc > 1:                                                # one entry fits, unless a single unit and site cannot
            assert cell * kc * sc <= scratch
        if ne > 1:
            assert cell * kc * sc * ne <= scratch
        if cell * kc0 * sc0 * n_sel <= scratch and chunk == 0:                 # nothing to shrink: one launch takes the whole selection
            assert (kc, sc, ne) == (kc0, sc0, min(n_sel, 65535))


def test_sum_in_run_order_is_the_twins_total():
    """pins the helper itself: the rows of exactref.expected(per_branch=True) added in run order are its totals within the
    project's bar, on the 40-tip tree (ragged last run) and the 6-tip tree (one ragged run)"""
    for z, n in ((bc.tree40(), 4), (bc.tree6(), 3)):
        T = int(z["Nnode"]) + 1
        Qs, pid = bc.models(n, 1)
        tips = bc.sites(n, T)
        want, _, rows = exactref.expected(z["edge"], z["edge.length"], Qs[0], pid[0], tips, per_branch=True)
        got = bc.sum_in_run_order(rows)
        length = float(np.sum(z["edge.length"]))
        err = np.abs(got - want)
        allow = 1e-12 * np.abs(want) + 1e-14 * length
        print(f"E={rows.shape[1]}: run order against the twin's totals: error / allowance {np.max(err / allow):.3g}")
        assert got.shape == want.shape and np.all(err <= allow)
    rows = np.arange(2 * 35 * 3, dtype=np.float64).reshape(2, 35, 3) * 0.1     # the order itself, on rows whose sums round
    want = np.zeros((2, 3))
    for r0 in (0, 16, 32):
        acc = np.zeros((2, 3))
        for b in range(r0, min(35, r0 + 16)):
            acc = acc + rows[:, b]
        want = want + acc
    assert np.array_equal(bc.sum_in_run_order(rows), want)


def test_label_reduce_is_the_column_loop():
    n = 3
    rs = np.random.default_rng(5)
    rows = rs.uniform(0.0, 1.0, (4, n * n))
    labels = rs.uniform(-1.0, 1.0, (2, n, n))
    w = bc.weights(n, labels)
    assert w.shape == (2, 9)
    assert np.array_equal(w[:, :3], np.stack([np.diag(l) for l in labels]))
    assert np.array_equal(w[0, 3:], [labels[0, 0, 1], labels[0, 0, 2], labels[0, 1, 0], labels[0, 1, 2], labels[0, 2, 0], labels[0, 2, 1]])
    got = bc.label_reduce(rows, labels)
    for r in range(4):
        for l in range(2):
            acc = 0.0
            for col in range(9):
                acc = acc + float(w[l, col]) * float(rows[r, col])
            assert got[r, l] == acc


def test_label_helpers_at_four_states():
    observe = (1, 2, 1, 2)
    got = ratemodel.observed_change_labels(observe)
    want = np.array([[0.0, 1.0, 0.0, 1.0],
                     [1.0, 0.0, 1.0, 0.0],
                     [0.0, 1.0, 0.0, 1.0],
                     [1.0, 0.0, 1.0, 0.0]])
    assert got.dtype == np.float64 and np.array_equal(got, want)
    got = ratemodel.count_labels(4, [(0, 1), (3, 2), (2, 2)])
    want = np.array([[0.0, 1.0, 0.0, 0.0],
                     [0.0, 0.0, 0.0, 0.0],
                     [0.0, 0.0, 1.0, 0.0],
                     [0.0, 0.0, 1.0, 0.0]])
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(ratemodel.count_labels(4, []), np.zeros((4, 4)))
    try:
        ratemodel.count_labels(4, [(0, 4)])
    except ValueError:
        pass
    else:
        raise AssertionError("a state outside 0..n-1 must be refused")
    # hidden <-> hidden changes of the same observed class are what the label leaves out
    both = ratemodel.count_labels(4, [(i, j) for i in range(4) for j in range(4) if i != j])
    assert np.array_equal(both - ratemodel.observed_change_labels(observe), ratemodel.count_labels(4, [(0, 2), (2, 0), (1, 3), (3, 1)]))


def test_model_average_takes_per_branch_arrays():
    """ancestral.model_average over the model axis of a [K, S, n_sel, C] array: weighted, a NaN model of weight 0 left out"""
    rs = np.random.default_rng(7)
    branch = rs.uniform(0.0, 1.0, (3, 2, 5, 4))
    branch[1] = np.nan                                                         # an impossible model
    got = ancestral.model_average(branch, weights=[1.0, 0.0, 3.0])
    assert got.shape == (2, 5, 4)
    np.testing.assert_allclose(got, 0.25 * branch[0] + 0.75 * branch[2], rtol=1e-15)
    paired = rs.uniform(0.0, 1.0, (4, 5, 3))
    np.testing.assert_allclose(ancestral.model_average(paired), paired.mean(axis=0), rtol=1e-15)
    assert "expected_branch_stats_models" in ancestral.model_average.__doc__
