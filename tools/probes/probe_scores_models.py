"""Expected statistics of many rate matrices (phm_expected_stats_models): device time (phm_last_kernel_ms) and
call time (host clock around the Python call) at K = 1 / 64 / 1 024 / 16 384 models on the squamate tree (2 states, and the
4-state hidden-rates model with parity tips) and on C3 (10 000 tips, 4 states), one site, cross mode, and, alternating with them
in the same process, the only route there was before: one api.expected_sumstat call per model, timed on 32 calls.  With each case
the algorithmic bytes of the passes over the device time.  Then api.fit_ml with gradient="fd" against gradient="exact" at p = 2 and p = 12.
python tools/probes/probe_scores_models.py [--quick | --lockstep]   (--quick: K up to 1 024, no fits; --lockstep: the lock-step loss
of the branch stage (a wave runs to its lanes' largest M) for the same models at K = 1 024, alone and on the host: it needs no device)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from phylomap_amd import _lib, api, ratemodel, synth  # noqa: E402

L = _lib.load()
HBM_PEAK = 8.0e12                                     # bytes / s, MI355X data sheet
QUICK = "--quick" in sys.argv
LOCKSTEP = "--lockstep" in sys.argv


def timed(fn, reps):
    ks, ws = [], []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ws.append((time.perf_counter() - t) * 1e3)
        ks.append(L.phm_last_kernel_ms())
    return float(np.median(ks)), float(np.median(ws))


def pass_bytes(z, n, evals, models):
    """what the passes must move per call -- an algorithmic-bytes count, not a counter.  Per evaluation: every L, O and F row (n
    values and an exponent) written once; L read by the up step, by the sibling's down step and by the branch stage, O by the down
    step, F by the branch stage.  Per model: every P entry written once and read by the up step and twice by the down steps."""
    E = np.asarray(z["edge"]).shape[0]
    NT = E + 1
    rows = NT * (1 + 3) + NT * (1 + 1) + E * (1 + 1)
    return 8.0 * (rows * (n + 1) * evals + 4.0 * E * n * n * models)


def lockstep(z, Qs):
    """steps of the lanes' weight rule per (branch, model), and what a wave of 64 consecutive models runs: its largest"""
    t = np.asarray(z["edge.length"], dtype=np.float64)[:, None]
    mu = np.max(-np.diagonal(Qs, axis1=1, axis2=2), axis=1)[None, :]
    x = mu * t
    r, S = x.copy(), 1.0 + x
    M = np.zeros(x.shape, dtype=np.int64)
    live = np.ones(x.shape, dtype=bool)
    m = 0
    while np.any(live):
        rn = r * (x / (m + 2))
        with np.errstate(over="ignore", invalid="ignore"):
            stop = (x < m + 2) & (rn <= 2.0 ** -60 * S * (1.0 - x / (m + 3)))
        live &= ~stop
        r = np.where(live, rn, r)
        S = np.where(live, S + r, S)
        big = live & (r > 2.0 ** 512)
        r, S = np.where(big, r * 2.0 ** -512, r), np.where(big, S * 2.0 ** -512, S)
        M += live
        m += 1
    K = Qs.shape[0]
    pad = (-K) % 64
    Mw = np.concatenate([M, np.zeros((M.shape[0], pad), dtype=np.int64)], axis=1).reshape(M.shape[0], -1, 64)
    run = Mw.max(axis=2) + 1                                                    # a wave's steps, the first term included
    own = (M + 1).sum()
    return float(own) / float(run.sum() * 64), float(own) / float(run.sum() * min(K, 64)) if K < 64 else None, int(M.max())


def case(label, z, model, theta0, pid, observe, Ks):
    rs = np.random.default_rng(1)
    n = model.n
    for K in Ks:
        thetas = np.asarray(theta0) * np.exp(rs.normal(0.0, 0.3, (K, model.p)))
        Qs = model.Qs(thetas)
        if LOCKSTEP:
            if K == 1024:
                eff, _, m_max = lockstep(z, Qs)
                print(f"{label:22s} K={K:6d} branch-stage steps: largest M {m_max}, lanes' own steps / steps their waves run "
                      f"{100 * eff:.1f} %", flush=True)
            continue
        api.expected_sumstat_models(z, Qs[:min(K, 64)], pid, observe=observe)  # warm-up: code objects, first allocations
        api.expected_sumstat(z, Qs[0], pid, observe=observe)
        k_ms, w_ms = timed(lambda: api.expected_sumstat_models(z, Qs, pid, observe=observe), 3)
        bk, bw = [], []                                                        # the route of the parent commit, alternating
        for i in range(32):
            t = time.perf_counter()
            api.expected_sumstat(z, Qs[i % K], pid, observe=observe)
            bw.append((time.perf_counter() - t) * 1e3)
            bk.append(L.phm_last_kernel_ms())
        k2, w2 = timed(lambda: api.expected_sumstat_models(z, Qs, pid, observe=observe), 3)
        k_ms, w_ms = min(k_ms, k2), min(w_ms, w2)
        b_call, b_kern = float(np.median(bw)), float(np.median(bk))
        rate = pass_bytes(z, n, K, K) / (k_ms * 1e-3)
        print(f"{label:22s} K={K:6d} cross S=1: device {k_ms:9.3f} ms  call {w_ms:9.2f} ms  per model {1e3 * w_ms / K:10.2f} us | "
              f"expected_sumstat per call: device {b_kern:7.3f} ms  call {b_call:7.2f} ms | per-model speed-up, call time "
              f"{b_call / (w_ms / K):9.1f}x, device time {b_kern / (k_ms / K):9.1f}x | pass bytes / device time "
              f"{rate / 1e9:8.1f} GB/s ({100 * rate / HBM_PEAK:5.2f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak)", flush=True)


def fits(label, z, model, pid, sites=None, observe=None, starts=8, seed=101):
    out = {}
    for mode in ("fd", "exact"):
        api.fit_ml(z, model, pid, sites=sites, observe=observe, starts=starts, seed=seed, gradient=mode, max_iter=3)   # warm-up
        ws = []
        for _ in range(3):
            t = time.perf_counter()
            r = api.fit_ml(z, model, pid, sites=sites, observe=observe, starts=starts, seed=seed, gradient=mode, max_iter=500)
            ws.append((time.perf_counter() - t) * 1e3)
        out[mode] = r
        print(f"fit_ml {label} p={model.p} {starts} starts gradient={mode:5s}: wall {np.median(ws):9.1f} ms  calls {r['calls']:4d}  "
              f"evaluations {r['evals']:7d}  iterations {r['iterations']:4d}  loglik {r['loglik']:.6f}  converged "
              f"{bool(r['converged'])}  max |grad| {np.max(np.abs(r['grad'])):.3g}", flush=True)
    print(f"fit_ml {label}: loglik exact - fd {out['exact']['loglik'] - out['fd']['loglik']:.3g}, max relative theta difference "
          f"{np.max(np.abs(out['exact']['theta'] - out['fd']['theta']) / out['fd']['theta']):.3g}", flush=True)


d = np.load(os.path.join(ROOT, "tests", "golden", "squamate", "seed101_tips.npz"))
T = len(d["states"])
zs = {"edge": d["edge"], "edge.length": d["edge_length"], "Nnode": T - 1, "states": d["states"]}
KS = (1, 64, 1024) if QUICK else (1, 64, 1024, 16384)
case("squamate ard(2)", zs, ratemodel.ard(2), [0.001, 0.006], [.5, .5], None, KS)
case("squamate hidden(1)", zs, ratemodel.hidden_rates(1), [0.001, 0.006, 0.001, 0.03, 16.0], [.25] * 4, [1, 2, 1, 2], KS)
z3, Q3, pid3, _ = synth.config_problem(3)
case("C3 hidden(1) n=4", z3, ratemodel.hidden_rates(1), [0.1, 0.1, 0.2, 0.2, 10.0], pid3, None, KS)

if not QUICK and not LOCKSTEP:
    fits("squamate ard(2)", zs, ratemodel.ard(2), [.5, .5])
    m4 = ratemodel.ard(4)                                                       # p = 12: 1 000 tips simulated under a known ard(4)
    edge, lens = synth.random_tree(1000, 0.4, 31)
    z4 = {"edge": edge, "edge.length": lens, "Nnode": 999, "states": np.ones(1000, dtype=np.int32)}
    truth = m4.Q(np.array([.3, .1, .2, .2, .4, .1, .15, .25, .3, .1, .2, .35]))
    tips4, _ = api.simulate_histories(z4, truth, [.25] * 4, 1, seed=31)
    fits("1000 tips ard(4)", dict(z4, states=tips4[0]), m4, [.25] * 4, seed=3)
