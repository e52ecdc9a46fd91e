"""Expectations through time under many rate matrices at 9..64 states: the batched call
(phm_expected_through_time_models_wide, ``api.expected_through_time_models(batched=True)``) against the parent's route (the default
``api.expected_through_time_models``: one phm_expected_through_time call per model), in one process on the same inputs, a warm-up
first, medians of 3.  Device time is phm_last_kernel_ms (phase_timing = 1 prints the phases of every call on stderr: one line a
call for the batched route, one line a model for the parent's), call time the host clock around the Python call.
  * n = 20 and 61 states, K = 16 copies of one random Q with every rate jittered log-normally (sigma = 0.3), one site and 8
    sites simulated under the first model, 50 equal bins over the depth (51 bounds: occupancy and bins);
  * the 40-tip tree, and a ladder of larger random trees (160, 640, 2 560 tips): the ladder stops after the first tree on which
    one call of the parent's route takes more than LIMIT seconds, so the last tree reported is the largest on which that route
    finishes within a minute.
python tools/probes/probe_time_models_wide.py [--quick]    (--quick: the 40-tip tree alone)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from phylomap_amd import _lib, api, synth  # noqa: E402
from phylomap_amd.maps import node_depths  # noqa: E402

L = _lib.load()
QUICK = "--quick" in sys.argv
K = 16
LIMIT = 15.0                                                                  # a parent call above this: the next tree (4 x the tips) would pass a minute


def models(n, rs):
    Q = rs.uniform(0.05, 1.0, (n, n)) * min(1.0, 4.0 / n)
    off = ~np.eye(n, dtype=bool)
    Qs = np.repeat(Q[None], K, axis=0)
    Qs[:, off] *= np.exp(rs.normal(0.0, 0.3, (K, n * n - n)))
    for Qk in Qs:
        np.fill_diagonal(Qk, 0.0)
        np.fill_diagonal(Qk, -Qk.sum(axis=1))
    return Qs


def timed(fn, runs):
    kernel, wall, out = [], [], None
    for _ in range(runs):
        t = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t) * 1e3)
        kernel.append(L.phm_last_kernel_ms())
    return float(np.median(kernel)), float(np.median(wall)), out


def case(T, n, S):
    """-> call ms of the parent's route"""
    edge, lens = synth.random_tree(T, 0.5, 0xB27)
    z = {"edge": edge, "edge.length": lens, "Nnode": T - 1, "states": np.ones(T, dtype=np.int32)}
    Qs = models(n, np.random.default_rng(29 + n))
    pid = np.full(n, 1.0 / n)
    tips, _ = api.simulate_histories(z, Qs[0], pid, S, seed=0xC3)
    bounds = np.linspace(0.0, float(node_depths(z).max()), 51)
    length = float(np.sum(lens))
    new = lambda q: api.expected_through_time_models(z, q, pid, sites=tips, bounds=bounds, batched=True, phase_timing=1)   # noqa: E731
    old = lambda q: api.expected_through_time_models(z, q, pid, sites=tips, bounds=bounds, phase_timing=1)                 # noqa: E731
    label = f"T={T} n={n} K={K} S={S} bins=50"
    print(f"--- {label}: warm-up", file=sys.stderr, flush=True)
    new(Qs[:1])
    t = time.perf_counter()
    old(Qs[:1])
    one = time.perf_counter() - t
    print(f"--- {label}: batched", file=sys.stderr, flush=True)
    nk, nw, got = timed(lambda: new(Qs), 3)
    runs = 3 if one * K < 5.0 else 1                                           # a slow parent call is timed once
    print(f"--- {label}: model by model, {runs} run(s)", file=sys.stderr, flush=True)
    ok, ow, ref = timed(lambda: old(Qs), runs)
    # phm_last_kernel_ms of the parent's route is the sum over its K single-model calls
    occ =float(np.nanmax(np.abs(got.occupancy - ref.occupancy)))
    rel = float(np.nanmax(np.abs(got.bins - ref.bins) / (1e-12 * np.abs(ref.bins) + 1e-14 * length)))
    same = bool(np.array_equal(got.loglik, ref.loglik))
    print(f"{label:34s} E={edge.shape[0]:5d} | batched: device {nk:10.3f} ms  call {nw:10.2f} ms | model by model ({runs} run(s)): "
          f"device {ok:10.2f} ms  call {ow:10.2f} ms | batched over model by model: call {nw / ow:.4f}, device {nk / ok:.4f} | "
          f"loglik equal {same}, occupancy difference {occ:.3g}, bins difference / allowance {rel:.3g}", flush=True)
    return ow


for T in (40,) if QUICK else (40, 160, 640, 2560):
    worst = 0.0
    for n in (20, 61):
        for S in (1, 8):
            worst = max(worst, case(T, n, S))
    if worst > LIMIT * 1e3:
        break
