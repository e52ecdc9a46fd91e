"""Expectations through time under many rate matrices (phm_expected_through_time_models): device time
(phm_last_kernel_ms) by phase (phase_timing = 1 prints the phases of every call on stderr) and call time (host clock around the
Python call), one process, a warm-up first, medians of 3.
  * C3's tree (10 000 tips, 4 states), 100 equal bins over the depth (101 bounds: occupancy and bins), one site, K = 64 and 1 024
    copies of C3's Q with every rate jittered log-normally (sigma = 0.3);
  * a 40-tip tree with the same bins, K = 1 024.
The baseline is the only route there was before: a Python loop of K api.expected_through_time calls.  It is run in full at
K = 64; at K = 1 024 it is K times the median of 16 calls on different models, run in the same process next to the new call.
python tools/probes/probe_time_models.py [--quick]    (--quick: K = 64 only)"""
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


def jitter(Q, K, rs):
    """K copies of Q, every rate of every model jittered on its own"""
    n = Q.shape[0]
    off = ~np.eye(n, dtype=bool)
    Qs = np.repeat(Q[None], K, axis=0)
    Qs[:, off] *= np.exp(rs.normal(0.0, 0.3, (K, n * n - n)))
    for Qk in Qs:
        np.fill_diagonal(Qk, 0.0)
        np.fill_diagonal(Qk, -Qk.sum(axis=1))
    return Qs


def case(label, z, Q, pid, Ks):
    tips, _ = api.simulate_histories(z, Q, pid, 1, seed=0xC3)
    bounds = np.linspace(0.0, float(node_depths(z).max()), 101)
    length = float(np.sum(z["edge.length"]))
    new = lambda Qs: api.expected_through_time_models(z, Qs, pid, sites=tips, bounds=bounds, phase_timing=1)      # noqa: E731
    old = lambda Qk: api.expected_through_time(z, Qk, pid, bounds=bounds, sites=tips, phase_timing=1)             # noqa: E731
    for K in Ks:
        Qs = jitter(Q, K, np.random.default_rng(28))
        print(f"--- {label}, K = {K}: warm-up", file=sys.stderr, flush=True)
        new(Qs[:1])
        old(Qs[0])
        nk, nw, got = [], [], None
        for r in range(3):
            print(f"--- {label}, K = {K}: new call, run {r}", file=sys.stderr, flush=True)
            t = time.perf_counter()
            got = new(Qs)
            nw.append((time.perf_counter() - t) * 1e3)
            nk.append(L.phm_last_kernel_ms())
        loop = min(K, 64 if K <= 64 else 16)
        print(f"--- {label}, K = {K}: baseline, {loop} calls", file=sys.stderr, flush=True)
        bk, bw, ref = [], [], None
        for k in range(loop):
            t = time.perf_counter()
            ref = old(Qs[k])
            bw.append((time.perf_counter() - t) * 1e3)
            bk.append(L.phm_last_kernel_ms())
        k = loop - 1
        same = bool(np.array_equal(got.loglik[k], ref["loglik"]))
        occ = float(np.max(np.abs(got.occupancy[k] - ref["occupancy"])))
        rel = float(np.max(np.abs(got.bins[k] - ref["bins"]) / (1e-12 * np.abs(ref["bins"]) + 1e-14 * length)))
        nk, nw = float(np.median(nk)), float(np.median(nw))
        if loop == K:
            loop_k, loop_w, how = float(np.sum(bk)), float(np.sum(bw)), "the whole loop"
        else:
            loop_k, loop_w, how = K * float(np.median(bk)), K * float(np.median(bw)), f"K x the median of {loop} calls"
        print(f"{label:10s} K={K:5d} E={np.asarray(z['edge']).shape[0]} bins=100 S=1 | new: device {nk:10.3f} ms  call {nw:10.2f} ms | "
              f"loop of K expected_through_time calls ({how}): device {loop_k:10.2f} ms  call {loop_w:10.2f} ms "
              f"(one call: device {float(np.median(bk)):.3f} ms, call {float(np.median(bw)):.3f} ms) | new over loop: call "
              f"{nw / loop_w:.4f}, device {nk / loop_k:.4f} | model {k} against its own call: loglik equal {same}, occupancy error "
              f"{occ:.3g}, bins error / allowance {rel:.3g}", flush=True)


z3, Q3, pid3, _ = synth.config_problem(3)
case("C3", z3, Q3, pid3, (64,) if QUICK else (64, 1024))
if not QUICK:
    edge, lens = synth.random_tree(40, 0.5, 0xB27)
    z40 = {"edge": edge, "edge.length": lens, "Nnode": 39, "states": np.ones(40, dtype=np.int32)}
    case("40 tips", z40, Q3, pid3, (1024,))
