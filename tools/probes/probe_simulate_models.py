"""Forward simulation under many rate matrices (phm_simulate_histories_models): device time
(phm_last_kernel_ms) and call time (host clock around the Python call) at K = 64 / 1 024 / 16 384 models, R = 1, on a 200-tip tree
(2 states), the squamate tree (4 states, hidden rates) and C3 (10 000 tips, hidden rates), against the route of the parent commit:
one api.simulate_histories call per model (the median of 32 calls, alternated with the new call in the same run, scaled by K).
Then K = 1 at R = 64 and 16 384 on C3 against simulate_histories at the same R, and the launches per call of each tree.
One process, warm-up first, medians of 3.  python tools/probes/probe_simulate_models.py [--small]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from phylomap_amd import _lib, api, ratemodel, synth  # noqa: E402

L = _lib.load()
SMALL = "--small" in sys.argv


def timed(fn, reps=3):
    ks, ws = [], []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ws.append((time.perf_counter() - t) * 1e3)
        ks.append(L.phm_last_kernel_ms())
    return float(np.median(ks)), float(np.median(ws))


def levels(z):
    """depth levels of the tree: the level launches of one chunk"""
    edge = np.asarray(z["edge"])
    depth = {}
    children = set(int(c) for c in edge[:, 1])
    root = next(int(p) for p in edge[:, 0] if int(p) not in children)
    kids = {}
    for p, c in edge:
        kids.setdefault(int(p), []).append(int(c))
    depth[root] = 0
    stack, deepest = [root], 0
    while stack:
        v = stack.pop()
        for c in kids.get(v, ()):
            depth[c] = depth[v] + 1
            deepest = max(deepest, depth[c])
            stack.append(c)
    return deepest


def case(label, z, model, theta0, pid, observe, Ks):
    rs = np.random.default_rng(1)
    lv = levels(z)
    print(f"{label}: {np.asarray(z['edge']).shape[0]} edges, {lv} depth levels -> {lv + 2} launches per chunk of histories "
          f"(root, levels, finish) + 1 transpose", flush=True)
    for K in Ks:
        Qs = model.Qs(np.asarray(theta0) * np.exp(rs.normal(0.0, 0.3, (K, model.p))))
        api.simulate_histories_models(z, Qs[:64], pid, 1, observe=observe, seed=1)          # warm-up: code objects, first allocations
        api.simulate_histories(z, Qs[0], pid, 1, observe=observe, seed=1)
        k_ms, w_ms = timed(lambda: api.simulate_histories_models(z, Qs, pid, 1, observe=observe, seed=2))
        bk, bw, loop_tips = [], [], []
        for i in range(32):                                                              # the parent commit's only route
            t = time.perf_counter()
            tp, _ = api.simulate_histories(z, Qs[i % K], pid, 1, observe=observe, seed=2, replica_offset=i % K)
            bw.append((time.perf_counter() - t) * 1e3)
            bk.append(L.phm_last_kernel_ms())
            loop_tips.append(tp[0])
        k2, w2 = timed(lambda: api.simulate_histories_models(z, Qs, pid, 1, observe=observe, seed=2))
        tips, stats = api.simulate_histories_models(z, Qs, pid, 1, observe=observe, seed=2)
        same = all(np.array_equal(tips[i % K, 0], loop_tips[i]) for i in range(32))
        k_ms, w_ms = min(k_ms, k2), min(w_ms, w2)
        b_call, b_kern = float(np.median(bw)), float(np.median(bk))
        n = model.n
        jumps = stats[:, 0, n:n + n * n].sum(axis=1).mean()
        print(f"{label:22s} K={K:6d} R=1: device {k_ms:9.3f} ms  call {w_ms:9.2f} ms  per model {1e3 * w_ms / K:10.2f} us | "
              f"simulate_histories per call: device {b_kern:7.3f} ms  call {b_call:7.2f} ms | per-model speed-up, call time "
              f"{b_call / (w_ms / K):9.1f}x, device time {b_kern / (k_ms / K):9.1f}x | {jumps:9.1f} jumps / history | "
              f"tips equal to the loop's: {same}", flush=True)


def one_model(z, Q, pid, R):
    api.simulate_histories_models(z, Q[None], pid, R, seed=1)
    api.simulate_histories(z, Q, pid, R, seed=1)
    a1 = timed(lambda: api.simulate_histories_models(z, Q[None], pid, R, seed=3))
    b1 = timed(lambda: api.simulate_histories(z, Q, pid, R, seed=3))
    a2 = timed(lambda: api.simulate_histories_models(z, Q[None], pid, R, seed=3))
    b2 = timed(lambda: api.simulate_histories(z, Q, pid, R, seed=3))
    a, b = (min(a1[0], a2[0]), min(a1[1], a2[1])), (min(b1[0], b2[0]), min(b1[1], b2[1]))
    print(f"C3 n=4 K=1 R={R:6d}: simulate_histories_models device {a[0]:9.3f} ms  call {a[1]:9.2f} ms | simulate_histories device "
          f"{b[0]:9.3f} ms  call {b[1]:9.2f} ms", flush=True)


KS = (64, 256) if SMALL else (64, 1024, 16384)
edge, lens = synth.random_tree(200, 1.0, 0x200)
z200 = {"edge": edge, "edge.length": lens, "Nnode": 199}
case("200 tips ard(2)", z200, ratemodel.ard(2), [0.6, 0.9], [.5, .5], None, KS)
d = np.load(os.path.join(ROOT, "tests", "golden", "squamate", "seed101_tips.npz"))
T = len(d["states"])
zs = {"edge": d["edge"], "edge.length": d["edge_length"], "Nnode": T - 1}
case("squamate hidden(1)", zs, ratemodel.hidden_rates(1), [0.001, 0.006, 0.001, 0.03, 16.0], [.25] * 4, [1, 2, 1, 2], KS)
z3, Q3, pid3, _ = synth.config_problem(3)
case("C3 hidden(1) n=4", z3, ratemodel.hidden_rates(1), [0.1, 0.1, 0.2, 0.2, 10.0], pid3, None, KS)
for R in ((64,) if SMALL else (64, 16384)):
    one_model(z3, Q3, pid3, R)
