"""Exact sampler of histories over many rate matrices at 9..64 states (phm_sample_histories_models_wide):
device time (phm_last_kernel_ms) and call time (host clock around the Python call) on the squamate tree (3 951 tips), one site,
cross mode, D = 64 draws per model, at 20 states (synth.neighbour_Q) and 61 states (synth.dense_Q), K = 1 and 16 models, without
and with maps (with maps: the sizing and the filling call together; the device time is the filling call's).  After each case one
more call under phm_debug_options.phase_timing, which prints the split of the device time into the Pade launches, the table, the
tree passes and the sampling launches to stderr.  For scale only: the narrow entry point at 8 states (a dense Q with the 61-state
model's largest leaving rate) on the same tree and shape.  The parent commit has no route to an exact sample above 8 states, so
there is no ratio.  One process, warm-up first, medians of 5.
python tools/probes/probe_sample_wide.py [--quick]   (--quick: K = 1 only)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from phylomap_amd import _lib, api, synth  # noqa: E402

L = _lib.load()
QUICK = "--quick" in sys.argv
D = 64


def timed(fn, reps=5):
    ks, ws = [], []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ws.append((time.perf_counter() - t) * 1e3)
        ks.append(L.phm_last_kernel_ms())
    return float(np.median(ks)), float(np.median(ws))


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
    tips, _ = api.simulate_histories(z, Q, pid, 1, seed=7)
    t_max = float(np.max(z["edge.length"]))
    for K in Ks:
        Qs = models(Q, K, rs)
        mu = float(np.max(-Qs[:, np.arange(n), np.arange(n)]))
        api.sample_histories(z, Qs[:1], pid, D, sites=tips, seed=1)             # warm-up: code objects, first allocations
        k0, w0 = timed(lambda: api.sample_histories(z, Qs, pid, D, sites=tips, seed=2))
        k1, w1 = timed(lambda: api.sample_histories(z, Qs, pid, D, sites=tips, maps=True, seed=2))
        st, ll = api.sample_histories(z, Qs, pid, D, sites=tips, seed=2)
        print(f"{label:24s} K={K:3d} D={D} | max mu t_b {mu * t_max:7.1f} | no maps: device {k0:9.3f} ms  call {w0:9.2f} ms | maps: "
              f"device (filling call) {k1:9.3f} ms  call (both calls) {w1:9.2f} ms | mean jumps per history "
              f"{st[..., n:].sum(axis=-1).mean():9.1f}", flush=True)
        if n > 8:
            sys.stderr.flush()
            api.sample_histories(z, Qs, pid, D, sites=tips, seed=2, phase_timing=1)
            sys.stderr.flush()
            _lib.set_debug_options()


d = np.load(os.path.join(ROOT, "tests", "golden", "squamate", "seed101_tips.npz"))
T = len(d["states"])
zs = {"edge": d["edge"], "edge.length": d["edge_length"], "Nnode": T - 1, "states": d["states"]}
Ks = (1,) if QUICK else (1, 16)
print(f"squamate tree: {T} tips, tree length {float(np.sum(zs['edge.length'])):.1f}, longest branch {float(np.max(zs['edge.length'])):.1f}",
      flush=True)
Q61 = synth.dense_Q(61)
case("neighbour_Q(20)", zs, synth.neighbour_Q(20), Ks)
case("dense_Q(61)", zs, Q61, Ks)
Q8 = synth.dense_Q(8)
Q8 *= float(np.max(-np.diag(Q61))) / float(np.max(-np.diag(Q8)))
case("narrow, dense 8 states", zs, Q8, Ks)
