"""Ancestral states under many rate matrices (phm_ancestral_models): device time (phm_last_kernel_ms) and call
time (host clock around the Python call) at K = 1 / 64 / 1 024 / 16 384 models on the squamate tree (ard(2), and the 4-state
hidden-rates model with parity tips), one site, cross mode, every node reported: the marginal call, the joint call and both, and,
alternating with them in the same process, the only route there was before for the marginals: one
api.expected_sumstat(nodes=True) call per model, timed on 32 calls.  With each case the joint part's share of the whole call and
the algorithmic bytes of the max-product up pass over the device time the joint part adds.  One process, warm-up first, medians
of 3.
python tools/probes/probe_ancestral.py [--quick]   (--quick: K up to 1 024)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from phylomap_amd import _lib, api, ratemodel  # noqa: E402

L = _lib.load()
HBM_PEAK = 8.0e12                                     # bytes / s, MI355X data sheet
QUICK = "--quick" in sys.argv


def timed(fn, reps=3):
    ks, ws = [], []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ws.append((time.perf_counter() - t) * 1e3)
        ks.append(L.phm_last_kernel_ms())
    return float(np.median(ks)), float(np.median(ws))


def up_bytes(z, n, evals, models):
    """what the max-product up pass and the traceback must move -- an algorithmic-bytes count, not a counter: P read once per
    model; per evaluation every M row (n values and an exponent) written and read once, every pointer word written and read once"""
    E = np.asarray(z["edge"]).shape[0]
    Nn = E // 2
    return 8.0 * E * n * n * models + evals * (2.0 * 8.0 * Nn * (n + 1) + 2.0 * 4.0 * E)


def case(label, z, model, theta0, pid, observe, Ks):
    rs = np.random.default_rng(1)
    n = model.n
    for K in Ks:
        thetas = np.asarray(theta0) * np.exp(rs.normal(0.0, 0.3, (K, model.p)))
        Qs = model.Qs(thetas)
        run = lambda **kw: api.ancestral_states_models(z, Qs, pid, observe=observe, **kw)    # noqa: E731
        api.ancestral_states_models(z, Qs[:min(K, 64)], pid, observe=observe)  # warm-up: code objects, first allocations
        api.expected_sumstat(z, Qs[0], pid, observe=observe, nodes=True)
        mk, mw = timed(lambda: run(joint=False))
        bk, bw = [], []                                                        # the route of the parent commit, alternating
        for i in range(32):
            t = time.perf_counter()
            api.expected_sumstat(z, Qs[i % K], pid, observe=observe, nodes=True)
            bw.append((time.perf_counter() - t) * 1e3)
            bk.append(L.phm_last_kernel_ms())
        mk2, mw2 = timed(lambda: run(joint=False))
        mk, mw = min(mk, mk2), min(mw, mw2)
        jk, jw = timed(lambda: run(marginal=False))
        lk, _ = timed(lambda: api.loglik_models(z, Qs, pid, observe=observe))
        ak, aw = timed(lambda: run())
        b_call, b_kern = float(np.median(bw)), float(np.median(bk))
        extra = max(jk - lk, 1e-6)                                             # device time of the joint part: the call minus section 17's
        rate = up_bytes(z, n, K, K) / (extra * 1e-3)
        print(f"{label:20s} K={K:6d} cross S=1, all nodes | marginal: device {mk:9.3f} ms  call {mw:9.2f} ms  per model "
              f"{1e3 * mw / K:9.2f} us | expected_sumstat(nodes=True) per call: device {b_kern:7.3f} ms  call {b_call:7.2f} ms | "
              f"per-model speed-up of the marginal call, call time {b_call / (mw / K):8.1f}x, device time {b_kern / (mk / K):8.1f}x | "
              f"joint: device {jk:9.3f} ms  call {jw:9.2f} ms (loglik_models alone: device {lk:8.3f} ms) | both: device {ak:9.3f} ms  "
              f"call {aw:9.2f} ms, the joint part's share of the device time {100 * (ak - mk) / ak:5.1f} % | max-product pass and "
              f"traceback: bytes / added device time {rate / 1e9:8.1f} GB/s ({100 * rate / HBM_PEAK:5.2f} % of the "
              f"{HBM_PEAK / 1e12:.0f} TB/s HBM peak)", flush=True)


d = np.load(os.path.join(ROOT, "tests", "golden", "squamate", "seed101_tips.npz"))
T = len(d["states"])
zs = {"edge": d["edge"], "edge.length": d["edge_length"], "Nnode": T - 1, "states": d["states"]}
KS = (1, 64, 1024) if QUICK else (1, 64, 1024, 16384)
case("squamate ard(2)", zs, ratemodel.ard(2), [0.001, 0.006], [.5, .5], None, KS)
case("squamate hidden(1)", zs, ratemodel.hidden_rates(1), [0.001, 0.006, 0.001, 0.03, 16.0], [.25] * 4, [1, 2, 1, 2], KS)
