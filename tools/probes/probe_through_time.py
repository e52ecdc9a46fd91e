"""Exact expectations through time (phm_expected_through_time): HIP-event time split into passes (P(t_b) included), along-branch
vectors (P(s), P(t_b - s) and the vectors), branch stage and reductions (phase_timing), and whole-call time, next to
phm_expected_stats on the same sites.  C3 (10 000 tips, 4 states) at 1 / 64 / 1 024 sites with 100 equal bins over the depth, a
density grid of 10 points per branch at one site, and the 500-tip C4 tree with a 61-state dense_Q at 128 sites and 20 bins.
python tools/probes/probe_through_time.py"""
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from phylomap_amd import _lib, api, synth  # noqa: E402
from phylomap_amd.maps import node_depths  # noqa: E402

L = _lib.load()


def phases(fn):
    """fn() with fd 2 caught: (its device-time phases [passes, along, branch, reductions] ms, summed over shards)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode()
    rows = re.findall(r"passes ([\d.]+) ms, along-branch vectors ([\d.]+) ms, branch stage ([\d.]+) ms, reductions ([\d.]+) ms", text)
    return np.array(rows[-1], dtype=float)


def timed(fn, reps):
    ks, ws = [], []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ws.append((time.perf_counter() - t) * 1e3)
        ks.append(L.phm_last_kernel_ms())
    return float(np.median(ks)), float(np.median(ws))


def run(label, z, Q, pid, S, bounds=None, points=None, reps=3):
    tips, _ = api.simulate_histories(z, Q, pid, S, seed=7)
    call = lambda **o: api.expected_through_time(z, Q, pid, bounds=bounds, points=points, sites=tips, **o)  # noqa: E731
    call()                                                                 # warm-up: code objects, first allocations
    api.expected_sumstat(z, Q, pid, sites=tips)
    k_ex, w_ex = timed(lambda: api.expected_sumstat(z, Q, pid, sites=tips), reps)
    k, w = timed(call, reps)
    ph = phases(lambda: call(phase_timing=1))
    print(f"{label:24s} S={S:5d}: kernel {k:9.3f} ms  whole call {w:9.1f} ms  | phases: passes {ph[0]:8.3f}  along {ph[1]:8.3f}  "
          f"branch {ph[2]:8.3f}  reductions {ph[3]:8.3f} ms | phm_expected_stats kernel {k_ex:8.3f} ms, call {w_ex:8.1f} ms "
          f"-> call x{w / w_ex:5.2f}, kernel x{k / k_ex:5.2f}", flush=True)


print("# tools/probes/probe_through_time.py on one MI355X (HIP-event kernel time = phm_last_kernel_ms; phases from phase_timing = 1; "
      "whole call = host clock around the Python call incl. planning, P, allocation and copies home; medians of 3)", flush=True)
z3, Q3, pid3, _ = synth.config_problem(3)
d3 = node_depths(z3)
b3 = np.linspace(0.0, d3.max(), 101)
for S in (1, 64, 1024):
    run("C3 n=4, 100 bins", z3, Q3, pid3, S, bounds=b3)
el3 = np.asarray(z3["edge.length"])
E3 = el3.size
grid = (np.repeat(np.arange(E3), 10), (np.tile(np.arange(10), E3) + 0.5) / 10.0 * np.repeat(el3, 10))
run("C3 n=4, 10 pts/branch", z3, Q3, pid3, 1, points=grid)
z4, _, _, _ = synth.config_problem(4)
d4 = node_depths(z4)
run("C4 tree n=61, 20 bins", z4, synth.dense_Q(61), np.ones(61), 128, bounds=np.linspace(0.0, d4.max(), 21))
