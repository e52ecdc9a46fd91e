"""Batched log-likelihood over many rate matrices (phm_loglik_models): device time (phm_last_kernel_ms) and
call time (host clock around the Python call) at K = 1 / 64 / 1 024 / 16 384 models on the squamate tree (2 states, and the
4-state hidden-rates model with parity tips) and on C3 (10 000 tips, 4 states), one site, cross mode; K = 1 024 paired with
1 024 simulated sites; and, alternating with them in the same process, the only route there was before: one
api.expected_sumstat call per model (which also runs the down pass and the branch stage), timed on 32 calls and scaled.
Then api.fit_ml on the squamate fixture.  python tools/probes/probe_loglik_models.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from phylomap_amd import _lib, api, ratemodel, synth  # noqa: E402

L = _lib.load()
HBM_PEAK = 8.0e12                                     # bytes / s, MI355X data sheet


def timed(fn, reps):
    ks, ws = [], []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ws.append((time.perf_counter() - t) * 1e3)
        ks.append(L.phm_last_kernel_ms())
    return float(np.median(ks)), float(np.median(ws))


def up_bytes(z, n, evals, models):
    """what the up pass must move: every L row (n values and an exponent) written once and read once per evaluation, every P
    entry read once per model -- an algorithmic-bytes count, not a counter"""
    E = np.asarray(z["edge"]).shape[0]
    NT = E + 1
    return 8.0 * (2.0 * NT * (n + 1) * evals + E * n * n * models)


def case(label, z, model, theta0, pid, observe, Ks):
    rs = np.random.default_rng(1)
    n = model.n
    base = {}
    for K in Ks:
        thetas = np.asarray(theta0) * np.exp(rs.normal(0.0, 0.3, (K, model.p)))
        Qs = model.Qs(thetas)
        api.loglik_models(z, Qs[:min(K, 64)], pid, observe=observe)          # warm-up: code objects, first allocations
        api.expected_sumstat(z, Qs[0], pid, observe=observe)
        k_ms, w_ms = timed(lambda: api.loglik_models(z, Qs, pid, observe=observe), 3)
        # the route of the parent commit, alternating: up + down passes and the branch stage, one model per call
        bk, bw = [], []
        for i in range(32):
            t = time.perf_counter()
            api.expected_sumstat(z, Qs[i % K], pid, observe=observe)
            bw.append((time.perf_counter() - t) * 1e3)
            bk.append(L.phm_last_kernel_ms())
        k2, w2 = timed(lambda: api.loglik_models(z, Qs, pid, observe=observe), 3)
        k_ms, w_ms = min(k_ms, k2), min(w_ms, w2)
        b_call, b_kern = float(np.median(bw)), float(np.median(bk))
        rate = up_bytes(z, n, K, K) / (k_ms * 1e-3)
        print(f"{label:22s} K={K:6d} cross S=1: device {k_ms:9.3f} ms  call {w_ms:9.2f} ms  per model {1e3 * w_ms / K:10.2f} us | "
              f"expected_sumstat per call: device {b_kern:7.3f} ms  call {b_call:7.2f} ms | per-model speed-up, call time "
              f"{b_call / (w_ms / K):9.1f}x, device time {b_kern / (k_ms / K):9.1f}x | up-pass bytes / device time "
              f"{rate / 1e9:8.1f} GB/s ({100 * rate / HBM_PEAK:5.2f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak)", flush=True)
        base[K] = (k_ms, w_ms)
    return base


def paired(label, z, model, theta0, pid, observe, Qtrue, K=1024):
    rs = np.random.default_rng(2)
    tips, _ = api.simulate_histories(z, Qtrue, pid, K, observe=observe, seed=9)
    Qs = model.Qs(np.asarray(theta0) * np.exp(rs.normal(0.0, 0.3, (K, model.p))))
    som = np.arange(K)
    api.loglik_models(z, Qs, pid, sites=tips, observe=observe, site_of_model=som)
    k_ms, w_ms = timed(lambda: api.loglik_models(z, Qs, pid, sites=tips, observe=observe, site_of_model=som), 3)
    rate = up_bytes(z, model.n, K, K) / (k_ms * 1e-3)
    print(f"{label:22s} K={K:6d} paired, {K} sites: device {k_ms:9.3f} ms  call {w_ms:9.2f} ms  per model {1e3 * w_ms / K:10.2f} us | "
          f"up-pass bytes / device time {rate / 1e9:8.1f} GB/s", flush=True)


d = np.load(os.path.join(ROOT, "tests", "golden", "squamate", "seed101_tips.npz"))
T = len(d["states"])
zs = {"edge": d["edge"], "edge.length": d["edge_length"], "Nnode": T - 1, "states": d["states"]}
KS = (1, 64, 1024, 16384)
case("squamate ard(2)", zs, ratemodel.ard(2), [0.001, 0.006], [.5, .5], None, KS)
case("squamate hidden(1)", zs, ratemodel.hidden_rates(1), [0.001, 0.006, 0.001, 0.03, 16.0], [.25] * 4, [1, 2, 1, 2], KS)
z3, Q3, pid3, _ = synth.config_problem(3)
case("C3 hidden(1) n=4", z3, ratemodel.hidden_rates(1), [0.1, 0.1, 0.2, 0.2, 10.0], pid3, None, KS)
paired("squamate ard(2)", zs, ratemodel.ard(2), [0.001, 0.006], [.5, .5], None, np.array([[-0.001, 0.001], [0.006, -0.006]]))
paired("C3 hidden(1) n=4", z3, ratemodel.hidden_rates(1), [0.1, 0.1, 0.2, 0.2, 10.0], pid3, None, Q3)

api.fit_ml(zs, ratemodel.ard(2), [.5, .5], starts=8, seed=101)                 # warm-up
t = time.perf_counter()
r = api.fit_ml(zs, ratemodel.ard(2), [.5, .5], starts=8, seed=101)
print(f"fit_ml squamate ard(2), 8 starts: loglik {r['loglik']:.6f} theta {r['theta']} iterations {r['iterations']} "
      f"likelihood calls {r['calls']} wall {(time.perf_counter() - t) * 1e3:.1f} ms converged {bool(r['converged'])}", flush=True)
