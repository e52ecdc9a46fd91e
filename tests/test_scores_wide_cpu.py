"""The expected statistics of many rate matrices at 9..64 states without a device (phm_expected_stats_models_wide, DESIGN.md
section 26): where the symbol is declared and bound, every refusal of the entry point before its first device call by status and
message, the host's decision between the two forms of the branch stage (phm_scores_wide_form.h, built into a small native
program) against a Python restatement of section 18's stopping rule, and a Python restatement of the short form's sum order
against ``exactref.expected``.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import exactref
from phylomap_amd import _lib, api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = "phm_expected_stats_models_wide"
NARROW = "phm_expected_stats_models"
SC_RUN = 16                                                                   # phm_scores.h


def terms(x, cap=1 << 21):
    """section 18's weights and stopping rule: r_0 = x, r_{m+1} = r_m x / (m + 2), S = 1 + sum r_m, both multiplied by 2^-512
    whenever r passes 2^512; the first m past the mode whose geometric tail bound is at most 2^-60 S, or cap + 1"""
    r, S = x, 1.0 + x
    for m in range(cap + 1):
        rn = r * (x / (m + 2))
        if x < m + 2 and rn <= 2.0 ** -60 * S * (1.0 - x / (m + 3)):
            return m
        r = rn
        S += r
        if r > 2.0 ** 512:
            r *= 2.0 ** -512
            S *= 2.0 ** -512
    return cap + 1


def _cap():
    src = open(os.path.join(ROOT, "phylomap_amd", "csrc", "phm_scores_wide_form.h")).read()
    return int(re.search(r"constexpr int SW_M_CAP = (\d+);", src).group(1))


def test_symbol_is_declared_apart_and_bound_like_the_narrow_one():
    L = _lib.load()
    assert hasattr(L, WIDE) and _lib.EXT3_EXPORTS == [WIDE]
    assert WIDE not in _lib.EXPORTS + _lib.EXT_EXPORTS + _lib.EXT2_EXPORTS
    assert _lib.EXT2_EXPORTS == ["phm_gibbs_rates_wide"] and _lib.EXT_EXPORTS == ["phm_sample_histories_models_wide"]
    assert L.phm_version() == 300
    assert list(getattr(L, WIDE).argtypes) == list(getattr(L, NARROW).argtypes)
    inc = os.path.join(ROOT, "include")
    for name in ("phylomap_hip.h", "phylomap_hip_ext.h", "phylomap_hip_ext2.h"):
        assert WIDE not in open(os.path.join(inc, name)).read()
    ext3 = open(os.path.join(inc, "phylomap_hip_ext3.h")).read()
    assert re.findall(r"\b(phm_[A-Za-z0-9_]+)\s*\(", ext3) == [WIDE] and '#include "phylomap_hip_ext2.h"' in ext3
    assert WIDE in api.expected_sumstat_models.__doc__ and WIDE in api.loglik_models.__doc__


def _random_Q(n, rs):
    Q = rs.uniform(0.05, 1.0, (n, n)) * 4.0 / n
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q


def _raw(z, Qs, pid, S=2, tree=True, q=True, p=True, stats=True, ll=True):
    """one call of the wide entry point with the tree's tips tiled S times -> (status, message)"""
    Qs = np.asarray(Qs, dtype=np.float64)
    K, n = Qs.shape[0], Qs.shape[1]
    Qf = np.ascontiguousarray(Qs.transpose(0, 2, 1))
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    pt = _lib.PlainTree(z, np.tile(z["states"], (S, 1)))
    o = _lib.make_options(n_replicas=S, tips_per_replica=True)
    lik = np.zeros(K * S) if ll else None
    st = np.zeros(K * S * n * n) if stats else None
    L = _lib.load()
    status = getattr(L, WIDE)(C.byref(pt.c) if tree else None, n, K, _lib._p(Qf, C.c_double) if q else None,
                              _lib._p(pid, C.c_double) if p else None, pid.size // n, None, None, C.byref(o),
                              _lib._p(st, C.c_double), _lib._p(lik, C.c_double))
    return status, L.phm_last_error().decode()


def test_refusals_need_no_device():
    L = _lib.load()
    n, T = 9, 16
    edge, lens = synth.random_tree(T, 0.5, 3)
    z = {"edge": edge, "edge.length": lens, "Nnode": T - 1, "states": np.ones(T, dtype=np.int32)}
    rs = np.random.default_rng(3)
    Qs = np.stack([_random_Q(n, rs) for _ in range(3)])
    pid = np.ones(n)
    for missing in ("tree", "q", "p", "ll"):
        st, msg = _raw(z, Qs, pid, **{missing: False})
        assert st == 1 and msg.startswith(WIDE + ": NULL argument"), (missing, st, msg)
    bad = Qs.copy()
    bad[2, 0, 3], bad[2, 0, 1] = -0.05, bad[2, 0, 1] + 0.05                   # ll_validate's checks come first
    st, msg = _raw(z, bad, pid)
    assert st == 1 and msg.startswith("model 2")
    for stats in (True, False):                                                # 8 states: the narrow entry point's
        st, msg = _raw(z, synth.dense_Q(8, 0.01, 0.04)[None], np.ones(8), stats=stats)
        assert st == 2 and msg.startswith(WIDE + ": ") and msg.endswith("go to " + NARROW), msg
    assert _raw(z, synth.dense_Q(2, 0.01, 0.04)[None], np.ones(2))[0] == 2
    st, msg = _raw(z, synth.dense_Q(65, 0.01, 0.04)[None], np.ones(65))
    assert st == 1 and "2..64" in msg
    fast = Qs.copy()
    fast[1] *= 1e7                                                             # mu t_b above 1e6 on the longer branches
    mu = float(np.max(-np.diag(fast[1])))
    first = int(np.argmax(mu * lens > 1e6))
    assert mu * lens[first] > 1e6
    st, msg = _raw(z, fast, pid)
    assert st == 2 and msg.startswith(WIDE + ": ") and f"model 1, edge row {first + 1}: max(-q_ii) * t_b above 1e6" in msg, msg
    if L.phm_device_count() == 0:                                              # a valid call gets as far as the device
        assert _raw(z, Qs, pid)[0] == 3
        assert _raw(z, Qs, pid, stats=False)[0] == 3                           # the log-likelihoods alone
        assert _raw(z, fast, pid, stats=False)[0] == 3                         # ... are not held to the branch stage's limit


def test_form_decision_of_the_host_against_the_restated_rule(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    exe = str(tmp_path / "scores_wide_form_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "phylomap_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "scores_wide_form_check.cpp"), "-o", exe])
    cap = _cap()
    assert cap == 63
    lo, hi = 1.0, 64.0                                                         # the two x where M steps from cap to cap + 1
    assert terms(lo) <= cap < terms(hi)
    while np.nextafter(lo, hi) < hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if terms(mid) <= cap else (lo, mid)
    assert terms(lo) == cap and terms(hi) == cap + 1
    xs = [0.0, 1e-6, 1.0, 16.0, 800.0, 2280.0, lo, hi]
    assert [terms(x) for x in xs[:6]] == [0, 1, 18, 61, 1060, 2710]
    for c in (0, 1 << 21):                                                     # the header's cap, and no cap in reach
        run = subprocess.run([exe, str(c)] + [float(x).hex() for x in xs], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
        lines = run.stdout.splitlines()
        use = cap if c == 0 else c
        assert lines[0] == f"cap {use}" and len(lines) == 1 + len(xs)
        for x, line in zip(xs, lines[1:]):
            hx, m = line.split()
            assert float.fromhex(hx) == x and int(m) == terms(x, use), (x, line)
    print(f"M steps from {cap} to {cap + 1} between mu t = {lo!r} and {hi!r}")


def _short_form_stats(edge, lens, Q, pid, tips, observe=None):
    """E[dwell], E[N] with the branch integral in the short form's order (phm_scores_wide.hip): v_0 .. v_M, then for l = 0 .. M
    g_l = sum_{r <= M - l} w_{l+r} v_r (r ascending), I += u_l g_l^T, u_{l+1} = B^T u_l; divided by S mu at the end; the edge rows
    added in runs of SC_RUN in edge order, the run totals in run order.  The passes are exactref's."""
    n, E = Q.shape[0], edge.shape[0]
    r = exactref.passes(edge, lens, Q, pid, tips, observe)
    S_ = r["loglik"].shape[0]
    mu = float(np.max(-np.diag(Q)))
    B = np.eye(n) + Q / mu
    pairs = exactref.columns(n)
    qcol = np.array([Q[i, j] for i, j in pairs])
    tot = np.zeros((S_, n * n))
    run = None
    for b in range(E):
        x = mu * float(lens[b])
        M = terms(x)
        w = [x]
        Ssum = 1.0 + x
        for m in range(M):
            w.append(w[-1] * (x / (m + 2)))
            Ssum += w[-1]
        c = int(edge[b, 1])
        V = [r["L"][c]]
        for _ in range(M):
            nv = np.zeros_like(V[-1])
            for j in range(n):
                nv = nv + B[:, j][None, :] * V[-1][:, j][:, None]
            V.append(nv)
        u = r["F"][b]
        I = np.zeros((S_, n, n))
        for l in range(M + 1):
            g = np.zeros_like(u)
            for rr in range(M - l + 1):
                g = g + w[l + rr] * V[rr]
            I = I + u[:, :, None] * g[:, None, :]
            if l < M:
                nu = np.zeros_like(u)
                for k in range(n):
                    nu = nu + B[k, :][None, :] * u[:, k][:, None]
                u = nu
        inv = 1.0 / (Ssum * mu)
        f = np.ldexp(1.0 / r["lam"], (r["sF"][b] + r["sL"][c] - r["sL"][r["root"]]).astype(np.int64))
        row = np.concatenate([np.einsum("sii->si", I) * inv * f[:, None],
                              qcol[None, :] * (np.stack([I[:, i, j] for i, j in pairs], axis=1) * inv) * f[:, None]], axis=1)
        run = 0.0 + row if b % SC_RUN == 0 else run + row
        if b % SC_RUN == SC_RUN - 1 or b == E - 1:
            tot = tot + run
    return tot, r["loglik"]


@pytest.mark.parametrize("n", [9, 17])
def test_short_form_order_does_not_spend_the_bar(n):
    T = 24
    rs = np.random.default_rng(0xC26 + n)
    edge, lens = synth.random_tree(T, 0.5, 0xC26 + n)
    lens = lens.copy()
    lens[3] = 0.0
    Q, pid = _random_Q(n, rs), rs.uniform(0.2, 1.0, n)
    tips = rs.integers(1, n + 1, (3, T)).astype(np.int32)
    tips[rs.random(tips.shape) < 0.1] = 0
    assert max(terms(float(np.max(-np.diag(Q))) * float(t)) for t in lens) <= _cap()
    want, ll_want = exactref.expected(edge, lens, Q, pid, tips)
    got, ll = _short_form_stats(edge, lens, Q, pid, tips)
    length = float(np.sum(lens))
    err = np.abs(got - want)
    allow = 1e-12 * np.abs(want) + 1e-14 * length                              # test_gpu_scores.py's _bar
    print(f"n={n}: the short form's order against exactref.expected: error / allowance {np.max(err / allow):.3g}")
    assert np.array_equal(ll, ll_want) and np.all(err <= allow)
    np.testing.assert_allclose(got[:, :n].sum(axis=1), length, rtol=1e-12)
