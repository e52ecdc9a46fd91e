"""Forward simulation (phm_simulate_histories): HIP-event kernel time and whole-call time, C3 (10 000 tips, 4 states) at 1 / 64 /
1 024 / 16 384 replicas and a 61-state model on the 500-tip C4 tree at 128 replicas; then, for scale, one MCMC sweep of C3 at
16 384 chains on the resident engine (the workload of bench.py).  python tools/probes/probe_simulate.py [--no-sweep]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

from phylomap_amd import _lib, api, synth  # noqa: E402

L = _lib.load()


def run(label, z, Q, pid, R, reps=3):
    api.simulate_histories(z, Q, pid, R, seed=1)                     # warm-up: code objects, first allocations
    ks, ws = [], []
    for i in range(reps):
        t = time.perf_counter()
        tips, stats = api.simulate_histories(z, Q, pid, R, seed=2 + i)
        ws.append((time.perf_counter() - t) * 1e3)
        ks.append(L.phm_last_kernel_ms())
    jumps = stats[:, Q.shape[0]:Q.shape[0] * (Q.shape[0] + 1)].sum(axis=1).mean()
    E = z["edge"].shape[0]
    print(f"{label:14s} R={R:6d}: kernel {np.median(ks):9.3f} ms (min {min(ks):8.3f})  whole call {np.median(ws):9.1f} ms   "
          f"{E * R / (np.median(ks) / 1e3) / 1e9:7.3f} G branch-replicas/s   {jumps:8.1f} jumps / replica", flush=True)


z3, Q3, pid3, Om3 = synth.config_problem(3)
for R in (1, 64, 1024, 16384):
    run("C3 n=4", z3, Q3, pid3, R)
z4, Q4, pid4, _ = synth.config_problem(4)
run("C4 n=61", z4, Q4, pid4, 128)

if "--no-sweep" not in sys.argv:
    e = _lib.Engine(z3, Q3, pid3, Om3, 24, variant=_lib.PHM_MCMC_BIGTREE, n_replicas=16384, reduce=True)
    e.run(4)
    e.sync()
    t = time.perf_counter()
    e.run(20)
    e.sync()
    print(f"C3 MCMC sweep, 16384 chains (resident engine, reduce): {(time.perf_counter() - t) * 1e3 / 20:8.3f} ms / sweep "
          f"(HIP events of the last run: {e.info().last_run_ms / 20:8.3f} ms / sweep)", flush=True)
    e.close()
