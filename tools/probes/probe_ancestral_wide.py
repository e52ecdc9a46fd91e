"""Ancestral states under many rate matrices at 9..64 states (phm_ancestral_models_wide): device time
(phm_last_kernel_ms) and call time (host clock around the Python call) on the squamate tree, one site, cross mode, at 20 states
(synth.neighbour_Q) and 61 states (synth.dense_Q), K = 1 / 16 / 64 models, with eight clade ancestors selected and with every
node reported: the marginal call, the joint call and both, and, alternating with them in the same process, the only route there
was before for the marginals: one api.expected_sumstat(nodes=True) call per model, timed on min(K, 32) calls.  Beside the joint
call the device time of api.loglik_models on the same inputs.  One process, warm-up first, medians of 3.
python tools/probes/probe_ancestral_wide.py [--quick]   (--quick: K up to 16)
python tools/probes/probe_ancestral_wide.py --one N     (N = 20 or 61: ONE call, K = 16, eight nodes, both parts, no warm-up -- the
    program to put behind `rocprofv3 --kernel-trace --stats --` for the split of the device time between the Pade launches and the
    passes, in a run of its own)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from phylomap_amd import _lib, ancestral, api, synth  # noqa: E402

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


def case(label, z, Q, Ks, clades):
    rs = np.random.default_rng(1)
    n = Q.shape[0]
    pid = np.full(n, 1.0 / n)
    tips, _ = api.simulate_histories(z, Q, pid, 1, seed=7)
    for K in Ks:
        Qs = models(Q, K, rs)
        for what, nodes in (("8 clade ancestors", clades), ("all nodes", None)):
            run = lambda **kw: api.ancestral_states_models(z, Qs, pid, sites=tips, nodes=nodes, **kw)    # noqa: E731
            api.ancestral_states_models(z, Qs[:1], pid, sites=tips, nodes=nodes)   # warm-up: code objects, first allocations
            api.expected_sumstat(z, Qs[0], pid, sites=tips, nodes=True)
            mk, mw = timed(lambda: run(joint=False))
            bk, bw = [], []                                                    # the route of the parent commit, alternating
            for i in range(min(K, 32)):
                t = time.perf_counter()
                api.expected_sumstat(z, Qs[i % K], pid, sites=tips, nodes=True)
                bw.append((time.perf_counter() - t) * 1e3)
                bk.append(L.phm_last_kernel_ms())
            mk2, mw2 = timed(lambda: run(joint=False))
            mk, mw = min(mk, mk2), min(mw, mw2)
            jk, jw = timed(lambda: run(marginal=False))
            lk, lw = timed(lambda: api.loglik_models(z, Qs, pid, sites=tips))
            ak, aw = timed(lambda: run())
            b_call, b_kern = float(np.median(bw)), float(np.median(bk))
            print(f"{label:22s} K={K:3d} cross S=1, {what:17s} | marginal: device {mk:9.3f} ms  call {mw:9.2f} ms  per model "
                  f"{mw / K:9.3f} ms | expected_sumstat(nodes=True) per call: device {b_kern:8.3f} ms  call {b_call:8.2f} ms | "
                  f"per-model speed-up of the marginal call, call time {b_call / (mw / K):7.1f}x, device time "
                  f"{b_kern / (mk / K):7.1f}x | joint: device {jk:9.3f} ms  call {jw:9.2f} ms (loglik_models: device {lk:9.3f} ms  "
                  f"call {lw:9.2f} ms) | both: device {ak:9.3f} ms  call {aw:9.2f} ms", flush=True)


d = np.load(os.path.join(ROOT, "tests", "golden", "squamate", "seed101_tips.npz"))
T = len(d["states"])
zs = {"edge": d["edge"], "edge.length": d["edge_length"], "Nnode": T - 1, "states": d["states"]}
CLADES = [ancestral.mrca(zs, [i * T // 8 + 1, (i + 1) * T // 8]) for i in range(8)]
if "--one" in sys.argv:
    n1 = int(sys.argv[sys.argv.index("--one") + 1])
    Q1 = synth.neighbour_Q(20) if n1 == 20 else synth.dense_Q(n1)
    pid1 = np.full(n1, 1.0 / n1)
    tips1, _ = api.simulate_histories(zs, Q1, pid1, 1, seed=7)
    api.ancestral_states_models(zs, models(Q1, 16, np.random.default_rng(1)), pid1, sites=tips1, nodes=CLADES)
    print(f"n={n1} K=16, 8 clade ancestors, both parts: device {L.phm_last_kernel_ms():.3f} ms")
    sys.exit(0)
KS = (1, 16) if QUICK else (1, 16, 64)
case("squamate neighbour(20)", zs, synth.neighbour_Q(20), KS, CLADES)
case("squamate dense(61)", zs, synth.dense_Q(61), KS, CLADES)
