"""Expected statistics of many rate matrices at 9..64 states (phm_expected_stats_models_wide): device time
(phm_last_kernel_ms) and call time (host clock around the call) on the squamate tree, cross mode, at 20 states
(synth.neighbour_Q) and 61 states (synth.dense_Q), every rate of every model jittered on its own, K = 1 / 16 / 64 models, S = 1
and S = 64 sites: the new call, the call that asks for the log-likelihoods alone and, alternating with them in the same process,
the route there was before: the C-ABI phm_expected_stats_models (one model after the other through phm_expected_stats), timed
per model on min(K, 8) models.  Beside each case the share of its (model, edge) items that take the long form of the branch
stage, from the stopping rule restated here.  One process, warm-up first, medians of 3 (a call of more than 5 s is timed once per round).
python tools/probes/probe_scores_wide.py [--quick] [--only N]   (--quick: K up to 16; --only 20 or 61: that state count alone)
python tools/probes/probe_scores_wide.py --one N     (N = 20 or 61: ONE call, K = 16, S = 1, no warm-up -- the program to put
    behind `rocprofv3 --kernel-trace --stats --` for the split of the device time between the kernels, in a run of its own)"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from phylomap_amd import _lib, api, synth  # noqa: E402

L = _lib.load()
QUICK = "--quick" in sys.argv
SW_M_CAP = 63


def terms(x, cap=SW_M_CAP):
    """sw_form_terms of phm_scores_wide_form.h"""
    r, S = x, 1.0 + x
    for m in range(cap + 1):
        rn = r * (x / (m + 2))
        if x < m + 2 and rn <= 2.0 ** -60 * S * (1.0 - x / (m + 3)):
            return m
        r = rn
        S += r
    return cap + 1


def call(name, z, Qs, pid, tips, stats=True):
    n, a, shape, head = api._models_on_tips(z, Qs, pid, tips, None, None, {})
    ll = np.zeros(shape)
    st = np.zeros((n * n,) + shape) if stats else None
    _lib.check(getattr(L, name)(*head, C.byref(a.opt), _lib._p(st, C.c_double), _lib._p(ll, C.c_double)))
    return st, ll


def timed(fn, reps=3):
    """(median device ms, median call ms, the last result); a call of more than 5 s is timed once"""
    ks, ws, out = [], [], None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        ws.append((time.perf_counter() - t) * 1e3)
        ks.append(L.phm_last_kernel_ms())
        if ws[-1] > 5e3:
            break
    return float(np.median(ks)), float(np.median(ws)), out


def models(Q, K, rs):
    """K copies of Q, every rate of every model jittered on its own"""
    n = Q.shape[0]
    off = ~np.eye(n, dtype=bool)
    Qs = np.repeat(Q[None], K, axis=0)
    Qs[:, off] *= np.exp(rs.normal(0.0, 0.3, (K, n * n - n)))
    for Qk in Qs:
        np.fill_diagonal(Qk, 0.0)
        np.fill_diagonal(Qk, -Qk.sum(axis=1))
    return Qs


def case(label, z, Q, Ks):
    rs = np.random.default_rng(1)
    n = Q.shape[0]
    pid = np.full(n, 1.0 / n)
    tips64, _ = api.simulate_histories(z, Q, pid, 64, seed=7)
    lens = np.asarray(z["edge.length"], dtype=np.float64)
    for K in Ks:
        Qs = models(Q, K, rs)
        ms = [[terms(float(np.max(-np.diag(Qk))) * float(t)) for t in lens] for Qk in Qs]
        long_share = float(np.mean(np.array(ms) > SW_M_CAP))
        for S in (1, 64):
            tips = tips64[:S]
            new = lambda: call("phm_expected_stats_models_wide", z, Qs, pid, tips)             # noqa: E731
            call("phm_expected_stats_models_wide", z, Qs[:1], pid, tips)      # warm-up: code objects, first allocations
            call("phm_expected_stats_models", z, Qs[:1], pid, tips)
            nk, nw, _ = timed(new)
            bk, bw = [], []                                                    # the route of the parent commit, alternating
            for i in range(min(K, 8)):
                t = time.perf_counter()
                old = call("phm_expected_stats_models", z, Qs[i:i + 1], pid, tips)
                bw.append((time.perf_counter() - t) * 1e3)
                bk.append(L.phm_last_kernel_ms())
            nk2, nw2, got = timed(new)
            nk, nw = min(nk, nk2), min(nw, nw2)
            lk, lw, _ = timed(lambda: call("phm_expected_stats_models_wide", z, Qs, pid, tips, stats=False))
            same = bool(np.array_equal(got[1][min(K, 8) - 1], old[1][0]))      # the last baseline model: loglik bit for bit
            rel = float(np.nanmax(np.abs(got[0][:, min(K, 8) - 1] - old[0][:, 0]) / (1e-12 * np.abs(old[0][:, 0]) + 1e-14 * lens.sum())))
            b_call, b_kern = float(np.median(bw)), float(np.median(bk))
            print(f"{label:22s} K={K:3d} S={S:2d} cross | new: device {nk:10.3f} ms  call {nw:10.2f} ms  per model {nw / K:9.3f} ms | "
                  f"phm_expected_stats_models per model: device {b_kern:9.3f} ms  call {b_call:9.2f} ms | per-model speed-up, call "
                  f"time {b_call / (nw / K):7.1f}x, device time {b_kern / (nk / K):7.1f}x | loglik alone: device {lk:10.3f} ms  call "
                  f"{lw:10.2f} ms | long-form items {100 * long_share:.2f} %, largest M word {int(np.max(ms))} | against the baseline: "
                  f"loglik equal {same}, stats error / allowance {rel:.3g}", flush=True)


d = np.load(os.path.join(ROOT, "tests", "golden", "squamate", "seed101_tips.npz"))
T = len(d["states"])
zs = {"edge": d["edge"], "edge.length": d["edge_length"], "Nnode": T - 1, "states": d["states"]}
if "--one" in sys.argv:
    n1 = int(sys.argv[sys.argv.index("--one") + 1])
    Q1 = synth.neighbour_Q(20) if n1 == 20 else synth.dense_Q(n1)
    pid1 = np.full(n1, 1.0 / n1)
    tips1, _ = api.simulate_histories(zs, Q1, pid1, 1, seed=7)
    call("phm_expected_stats_models_wide", zs, models(Q1, 16, np.random.default_rng(1)), pid1, tips1)
    print(f"n={n1} K=16 S=1: device {L.phm_last_kernel_ms():.3f} ms")
    sys.exit(0)
KS = (1, 16) if QUICK else (1, 16, 64)
ONLY = int(sys.argv[sys.argv.index("--only") + 1]) if "--only" in sys.argv else 0
if ONLY in (0, 20):
    case("squamate neighbour(20)", zs, synth.neighbour_Q(20), KS)
if ONLY in (0, 61):
    case("squamate dense(61)", zs, synth.dense_Q(61), KS)
