"""Per-branch expected statistics under many rate matrices (phm_expected_branch_stats_models): device time
(phm_last_kernel_ms) and call time (host clock around the Python call), medians of 3 after a warm-up, one process.
  * the squamate tree with ard(2) and with hidden_rates(1) (tips seen up to parity), K = 1 / 64 / 1 024 draws of the rates, full
    rows, one site.  The baseline is the only route there was before: one api.expected_sumstat(per_branch=True) call per model,
    the median of 32 calls (min(K, 32) different models, cycled), run alternately with the new call in the same run.
  * one 20-state model (synth.neighbour_Q) and one 61-state model (synth.dense_Q) on a 200-tip tree, K = 64, three labels against
    the full rows of the same call: the label path's saving in copied bytes.
python tools/probes/probe_branch_models.py [--quick]    (--quick: K up to 64)
python tools/probes/probe_branch_models.py --one CASE   (CASE = ard2, hrm1, n20, n61, n20labels or n61labels: ONE call at the
    case's largest K, no warm-up -- the program to put behind `rocprofv3 --kernel-trace --stats --` for the split of the device
    time between the kernels, in a run of its own)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from phylomap_amd import _lib, api, ratemodel, synth  # noqa: E402

L = _lib.load()
QUICK = "--quick" in sys.argv


def timed(fn, reps=3):
    """(median device ms, median call ms, the last result)"""
    ks, ws, out = [], [], None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        ws.append((time.perf_counter() - t) * 1e3)
        ks.append(L.phm_last_kernel_ms())
    return float(np.median(ks)), float(np.median(ws)), out


def squamate():
    d = np.load(os.path.join(ROOT, "tests", "golden", "squamate", "seed101_tips.npz"))
    T = len(d["states"])
    return {"edge": d["edge"], "edge.length": d["edge_length"], "Nnode": T - 1, "states": d["states"]}


def draws(model, K, z, seed):
    """K draws of the rates around tips / tree length, spread log-normally"""
    rs = np.random.default_rng(seed)
    rate0 = (int(z["Nnode"]) + 1) / float(np.sum(z["edge.length"]))
    return model.Qs(rate0 * np.exp(rs.normal(0.0, 0.5, (K, model.p))))


def squamate_case(label, model, observe, Ks):
    z = squamate()
    n = model.n
    pid = np.full(n, 1.0 / n)
    E = np.asarray(z["edge"]).shape[0]
    length = float(np.sum(z["edge.length"]))
    for K in Ks:
        Qs = draws(model, K, z, 11)
        new = lambda: api.expected_branch_stats_models(z, Qs, pid, observe=observe)                # noqa: E731
        old = lambda k: api.expected_sumstat(z, Qs[k], pid, observe=observe, per_branch=True)      # noqa: E731
        api.expected_branch_stats_models(z, Qs[:1], pid, observe=observe)     # warm-up: code objects, first allocations
        old(0)
        nk, nw, bk, bw = [], [], [], []
        got = ref = None
        for r in range(4):                                                    # 4 rounds of (the new call, 8 baseline calls)
            a, b, got = timed(new, reps=1)
            if r > 0:                                                         # medians of 3: the first round is a warm-up at this K
                nk.append(a)
                nw.append(b)
            for i in range(8):
                k = (8 * r + i) % min(K, 32)
                t = time.perf_counter()
                ref = (k, old(k))
                bw.append((time.perf_counter() - t) * 1e3)
                bk.append(L.phm_last_kernel_ms())
        bw_all = bw
        nk, nw, bk, bw = (float(np.median(v)) for v in (nk, nw, bk, bw))
        k, (_, ll_one, br_one) = ref
        same = bool(np.array_equal(got[1][k], ll_one))
        rel = float(np.max(np.abs(got[0][k] - br_one) / (1e-12 * np.abs(br_one) + 1e-14 * length)))
        ratio = (nw / K) / bw
        print(f"{label:22s} K={K:5d} E={E} full rows | new: device {nk:10.3f} ms  call {nw:10.2f} ms  per model {nw / K:9.4f} ms | "
              f"expected_sumstat(per_branch=True) per model (median of {len(bw_all)}): device {bk:8.3f} ms  call {bw:8.3f} ms | per-model "
              f"cost over the baseline's, call time {ratio:8.5f} (bar at K = 1 024: at most 0.125), device time {(nk / K) / bk:8.5f} | "
              f"output {got[0].nbytes / 1e6:.2f} MB | against the baseline: loglik equal {same}, rows error / allowance {rel:.3g}", flush=True)


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


def wide_inputs(n, K=64):
    T = 200
    edge, lens = synth.random_tree(T, 0.1, 0xB27)
    z = {"edge": edge, "edge.length": lens, "Nnode": T - 1, "states": np.ones(T, dtype=np.int32)}
    Q = synth.neighbour_Q(20) if n == 20 else synth.dense_Q(n)
    pid = np.full(n, 1.0 / n)
    tips, _ = api.simulate_histories(z, Q, pid, 1, seed=7)
    Qs = jitter(Q, K, np.random.default_rng(1))
    rs = np.random.default_rng(2)
    lab = np.stack([ratemodel.observed_change_labels(np.arange(n) % 2 + 1), ratemodel.count_labels(n, [(0, 1), (1, 0)]),
                    rs.uniform(-1.0, 1.0, (n, n))])
    return z, Qs, pid, tips, lab


def wide_case(n):
    z, Qs, pid, tips, lab = wide_inputs(n)
    K, E = len(Qs), np.asarray(z["edge"]).shape[0]
    full = lambda: api.expected_branch_stats_models(z, Qs, pid, sites=tips)                       # noqa: E731
    labelled = lambda: api.expected_branch_stats_models(z, Qs, pid, sites=tips, labels=lab)       # noqa: E731
    api.expected_branch_stats_models(z, Qs[:1], pid, sites=tips)
    api.expected_branch_stats_models(z, Qs[:1], pid, sites=tips, labels=lab)
    fk, fw, f = timed(full)
    lk, lw, g = timed(labelled)
    fk2, fw2, _ = timed(full)
    lk2, lw2, _ = timed(labelled)
    fk, fw, lk, lw = min(fk, fk2), min(fw, fw2), min(lk, lk2), min(lw, lw2)
    print(f"200 tips, n={n:2d} K={K} E={E} | full rows: device {fk:10.3f} ms  call {fw:10.2f} ms  copied {f[0].nbytes / 1e6:9.2f} MB | "
          f"3 labels: device {lk:10.3f} ms  call {lw:10.2f} ms  copied {g[0].nbytes / 1e6:7.3f} MB | labels over full rows: call time "
          f"{lw / fw:.3f}, device time {lk / fk:.3f}, bytes {g[0].nbytes / f[0].nbytes:.5f}", flush=True)


if "--one" in sys.argv:
    which = sys.argv[sys.argv.index("--one") + 1]
    if which in ("ard2", "hrm1"):
        m = ratemodel.ard(2) if which == "ard2" else ratemodel.hidden_rates(1)
        zs = squamate()
        K1 = 64 if QUICK else 1024
        api.expected_branch_stats_models(zs, draws(m, K1, zs, 11), np.full(m.n, 1.0 / m.n), observe=None if which == "ard2" else (1, 2, 1, 2))
    else:
        z1, Qs1, pid1, tips1, lab1 = wide_inputs(20 if which.startswith("n20") else 61)
        api.expected_branch_stats_models(z1, Qs1, pid1, sites=tips1, labels=lab1 if which.endswith("labels") else None)
    print(f"{which}: device {L.phm_last_kernel_ms():.3f} ms")
    sys.exit(0)
KS = (1, 64) if QUICK else (1, 64, 1024)
squamate_case("squamate ard(2)", ratemodel.ard(2), None, KS)
squamate_case("squamate hidden_rates(1)", ratemodel.hidden_rates(1), (1, 2, 1, 2), KS)
wide_case(20)
wide_case(61)
