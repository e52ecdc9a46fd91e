"""Exact conditional expectations (phm_expected_stats): HIP-event time of the passes + branch stage and whole-call time, C3
(10 000 tips, 4 states) at 1 / 64 / 1 024 sites, the 500-tip C4 tree with a 61-state dense_Q at 128 sites, and the squamate tree
(3 951 tips, 2 states, max(-q_ii) t_b up to 2 280) at 64 sites.  python tools/probes/probe_expected.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from phylomap_amd import _lib, api, synth  # noqa: E402

L = _lib.load()


def run(label, z, Q, pid, S, reps=3):
    tips, _ = api.simulate_histories(z, Q, pid, S, seed=7)
    api.expected_sumstat(z, Q, pid, sites=tips)                      # warm-up: code objects, first allocations
    ks, ws = [], []
    for _ in range(reps):
        t = time.perf_counter()
        api.expected_sumstat(z, Q, pid, sites=tips)
        ws.append((time.perf_counter() - t) * 1e3)
        ks.append(L.phm_last_kernel_ms())
    mu = float(np.max(-np.diag(Q)))
    steps = float(np.sum(mu * np.asarray(z["edge.length"])))
    print(f"{label:16s} S={S:5d}: kernel {np.median(ks):9.3f} ms (min {min(ks):8.3f})  whole call {np.median(ws):9.1f} ms   "
          f"sum_b mu t_b = {steps:9.0f}", flush=True)


z3, Q3, pid3, _ = synth.config_problem(3)
for S in (1, 64, 1024):
    run("C3 n=4", z3, Q3, pid3, S)
z4, _, _, _ = synth.config_problem(4)
run("C4 tree n=61", z4, synth.dense_Q(61), np.ones(61), 128)
d = np.load(os.path.join(ROOT, "tests", "golden", "squamate", "seed101_tips.npz"))
T = len(d["states"])
zs = {"edge": d["edge"], "edge.length": d["edge_length"], "Nnode": T - 1, "states": d["states"]}
run("squamate n=2", zs, np.array([[-10.0, 10.0], [6.0, -6.0]]), np.ones(2), 64)
