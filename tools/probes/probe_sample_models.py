"""Exact sampler of histories over many rate matrices (phm_sample_histories_models): device time
(phm_last_kernel_ms) and call time (host clock around the Python call), medians of 3 after a warm-up.
  * C3 (10 000 tips, 4 states, fully observed tips), K = 1, D = 1 024, alternating in the same process with the only exact
    sampler there was before, api.sumstatEXP(N = 1 024, rescale_pruning on) on the same tree;
  * C3 with K = 16 x D = 64 and K = 1 024 x D = 1 (the same 1 024 histories, the models spread over a fit's uncertainty);
  * the squamate tree (3 951 tips) at mu = 10 (mu t_b up to about 2 280), 2 states, K = 1, D = 64: no baseline exists.
python tools/probes/probe_sample_models.py [--quick]     (--quick: no squamate case)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from phylomap_amd import _lib, api, synth  # noqa: E402

L = _lib.load()
QUICK = "--quick" in sys.argv


def timed(fn, reps=3):
    ks, ws = [], []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ws.append((time.perf_counter() - t) * 1e3)
        ks.append(L.phm_last_kernel_ms())
    return float(np.median(ks)), float(np.median(ws))


z3, Q3, pid3, _ = synth.config_problem(3)
n = Q3.shape[0]
E3 = np.asarray(z3["edge"]).shape[0]
mu3 = float(np.max(-np.diag(Q3)))
print(f"C3: {E3 // 2 + 1} tips, {n} states, max mu t_b = {mu3 * float(np.max(z3['edge.length'])):.2f}, "
      f"mean mu t_b = {mu3 * float(np.mean(z3['edge.length'])):.3f}", flush=True)
api.sample_histories(z3, Q3, pid3, 64, seed=1)                                 # warm-up: code objects, first allocations
api.sumstatEXP(z3, Q3, pid3, 64, seed=1, rescale=True)
rows = []
for rnd in range(3):                                                            # alternating
    t = time.perf_counter()
    st, ll = api.sample_histories(z3, Q3, pid3, 1024, seed=2 + rnd)
    w_new, k_new = (time.perf_counter() - t) * 1e3, L.phm_last_kernel_ms()
    t = time.perf_counter()
    old = api.sumstatEXP(z3, Q3, pid3, 1024, seed=2 + rnd, rescale=True)
    w_old, k_old = (time.perf_counter() - t) * 1e3, L.phm_last_kernel_ms()
    rows.append((k_new, w_new, k_old, w_old))
    print(f"  round {rnd}: sample_histories device {k_new:8.3f} ms call {w_new:8.2f} ms | sumstatEXP device {k_old:8.3f} ms call "
          f"{w_old:8.2f} ms | mean dwell sum {st[0, 0, :, :n].sum(axis=1).mean():.6f} / {old[:, :n].sum(axis=1).mean():.6f}, mean jumps "
          f"{st[0, 0, :, n:].sum(axis=1).mean():.2f} / {old[:, n:].sum(axis=1).mean():.2f}", flush=True)
k_new, w_new, k_old, w_old = (float(np.median(c)) for c in zip(*rows))
print(f"C3 K=1 D=1024: sample_histories device {k_new:.3f} ms, call {w_new:.2f} ms | sumstatEXP N=1024 device {k_old:.3f} ms, call "
      f"{w_old:.2f} ms | ratio device {k_new / k_old:.2f}x, call {w_new / w_old:.2f}x", flush=True)
k, w = timed(lambda: api.sample_histories(z3, Q3, pid3, 1024, maps=True, seed=5))
print(f"C3 K=1 D=1024 with maps (sizing + filling): device (filling call) {k:.3f} ms, call {w:.2f} ms", flush=True)

rs = np.random.default_rng(1)
for K, D in ((16, 64), (1024, 1)):
    Qs = Q3[None] * np.exp(rs.normal(0.0, 0.1, (K, 1, 1)))
    k, w = timed(lambda: api.sample_histories(z3, Qs, pid3, D, seed=3))
    print(f"C3 K={K} D={D}: device {k:.3f} ms, call {w:.2f} ms, per history {1e3 * k / (K * D):.2f} us of device time", flush=True)

if not QUICK:
    d = np.load(os.path.join(ROOT, "tests", "golden", "squamate", "seed101_tips.npz"))
    T = len(d["states"])
    zs = {"edge": d["edge"], "edge.length": d["edge_length"], "Nnode": T - 1, "states": d["states"]}
    Qs = np.array([[-10.0, 10.0], [6.0, -6.0]])
    x = 10.0 * np.asarray(zs["edge.length"], dtype=np.float64)
    api.sample_histories(zs, Qs, [.5, .5], 64, seed=1)
    t = time.perf_counter()
    st, ll = api.sample_histories(zs, Qs, [.5, .5], 64, seed=4)
    w = (time.perf_counter() - t) * 1e3
    print(f"squamate mu=10 ({T} tips, max mu t_b {x.max():.0f}, sum mu t_b {x.sum():.0f}) K=1 D=64: device "
          f"{L.phm_last_kernel_ms():.3f} ms, call {w:.2f} ms, loglik {ll[0, 0]:.3f}, mean jumps per history "
          f"{st[0, 0, :, 2:].sum(axis=1).mean():.0f}, dwell sum - tree length {np.max(np.abs(st[0, 0, :, :2].sum(axis=1) - x.sum() / 10.0)):.3g}",
          flush=True)
