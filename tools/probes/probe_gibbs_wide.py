"""Posterior sampling of rates at 9..64 states (phm_gibbs_rates_wide / api.posterior_rates): wall and device
time per iteration of the driver against the only route there was before it -- a Python loop over
``api.sample_histories(draws=1, replica_offset=i)`` (one lane in 64 filled, every site's full statistics row downloaded) with a
host update -- alternating in one process after a warm-up, medians of 3 (12 iterations a run of the driver, 3 of the loop).
The loop's host update is numpy's vectorised Gamma generator on the summed rows: cheaper than the driver's own (one Philox stream
per chain and parameter), so the comparison favours the loop.
  * sym(20) and er(61) on a 200-tip tree and on the squamate fixture tree (3 951 tips), tips simulated under the model;
  * C = 4 and 64 chains, S = 64 and 512 sites, joint; one paired case (4 chains on each of 16 sites).
With q_timing the driver prints the split of an iteration (upload, launches + device + download with the Pade share, host update)
and its launch count to stderr.
python tools/probes/probe_gibbs_wide.py [--full]   (without --full: the 200-tip cases but er(61) at C = 64, S = 512, and of the
squamate tree C = 4, S = 64 alone; what is left out is printed as not measured)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from phylomap_amd import _lib, api, posterior, ratemodel, synth  # noqa: E402

L = _lib.load()
FULL = "--full" in sys.argv
ITERS_D, ITERS_L = 12, 3                             # iterations of a timed run: driver, loop


def loop_route(z, model, pid, prior, th0, iters, theta_max, sites, som, seed):
    """the parent's only route: one sample_histories call per iteration, every site's row to the host, summed and updated there"""
    n, p = model.n, model.p
    idx = np.asarray(model.index)
    A = np.zeros((n * (n - 1), p))                       # counts -> N_c
    W = np.zeros((n, p))                                 # dwell -> W_c (dwell_i once per entry of c in row i)
    for i in range(n):
        for j in range(n):
            if i != j and idx[i, j] > 0:
                A[i * (n - 1) + (j - 1 if j > i else j), idx[i, j] - 1] = 1.0
                W[i, idx[i, j] - 1] += 1.0
    th = th0.copy()
    rng = np.random.default_rng(seed)
    dev = 0.0
    for i in range(iters):
        st, ll = api.sample_histories(z, posterior.rate_matrices(model, th), pid, 1, sites=sites, site_of_model=som, seed=seed,
                                      replica_offset=i)
        dev += L.phm_last_kernel_ms()
        st = st[..., 0, :].reshape(th.shape[0], -1, st.shape[-1]).sum(axis=1)
        fresh = rng.gamma(prior[None, :, 0] + st[:, n:] @ A, 1.0 / (prior[None, :, 1] + st[:, :n] @ W))
        th = np.where(fresh <= theta_max, fresh, th)
    return dev, th


def case(name, edge, lens, model, Cn, S, paired=False):
    n = model.n
    pid = np.full(n, 1.0 / n)
    T = edge.shape[0] // 2 + 1
    rate0 = T / float(lens.sum()) / (n - 1)              # a state's total rate about tips / tree length
    theta_max = min(100.0 * rate0, 0.9 * 32768.0 / ((n - 1) * float(lens.max())))
    Q = model.Q(np.full(model.p, rate0))
    sites = np.stack([synth.simulate_tips(edge, lens, Q, pid, 100 + s) for s in range(min(S, 8))]).astype(np.int32)
    sites = sites[np.arange(S) % sites.shape[0]]         # S sites from 8 simulated ones: the work per site is what is timed
    z = {"edge": edge, "edge.length": lens, "Nnode": edge.shape[0] // 2, "states": sites[0]}
    prior = np.ones((model.p, 2))
    per = Cn // S if paired else Cn
    som = np.repeat(np.arange(S, dtype=np.int32), per) if paired else None
    th0 = np.random.default_rng(Cn).uniform(0.5, 1.5, (Cn, model.p)) * min(rate0, 0.5 * theta_max)

    def driver(iters, q_timing=False):
        kw = {"q_timing": 1} if q_timing else {}
        t = time.perf_counter()
        r = api.posterior_rates(z, model, pid, prior, iters, chains=per, sites=sites, per_site=paired, theta0=th0, theta_max=theta_max,
                                seed=5, **kw)
        return (time.perf_counter() - t) * 1e3, L.phm_last_kernel_ms(), r

    def loop(iters):
        t = time.perf_counter()
        dev, _ = loop_route(z, model, pid, prior, th0, iters, theta_max, sites, som, 5)
        return (time.perf_counter() - t) * 1e3, dev

    driver(1)
    loop(1)                                              # warm-up of both
    rows = []
    for _ in range(3):                                   # alternating
        wd, kd, r = driver(ITERS_D)
        wl, kl = loop(ITERS_L)
        rows.append((wd / ITERS_D, kd / ITERS_D, wl / ITERS_L, kl / ITERS_L))
    wd, kd, wl, kl = (float(np.median(c)) for c in zip(*rows))
    mode = f"paired, {per} chains on each of {S} sites" if paired else f"C={Cn:3d} S={S:4d}"
    print(f"  {name:9s} {model.n:2d} states p={model.p:4d} {mode}: driver wall {wd:10.3f} ms/iter, device {kd:10.3f} | loop wall "
          f"{wl:10.3f} ms/iter, device {kl:10.3f} | loop / driver: wall {wl / wd:7.2f}x, device {kl / kd:7.2f}x | rejected "
          f"{int(r['rejected'].sum())}, failed chains {int(r['status'].sum())}", flush=True)
    sys.stderr.flush()
    driver(ITERS_D, q_timing=True)                       # the split, to stderr
    sys.stderr.flush()


def skipped(text):
    print(f"  not measured: {text}", flush=True)


sym20, er61 = ratemodel.sym(20), ratemodel.er(61)
edge, lens = synth.random_tree(200, 0.3, 17)
print(f"200-tip tree, longest branch {lens.max():.3g}; medians of 3 alternating runs of {ITERS_D} (driver) and {ITERS_L} (loop) iterations",
      flush=True)
for model in (sym20, er61):
    for Cn in (4, 64):
        for S in (64, 512):
            if not FULL and model is er61 and Cn == 64 and S == 512:
                skipped("200-tip er(61) C=64 S=512 (--full)")
                continue
            case("200-tip", edge, lens, model, Cn, S)
case("200-tip", edge, lens, sym20, 64, 16, paired=True)

d = np.load(os.path.join(ROOT, "tests", "golden", "squamate", "seed101_tips.npz"))
se, sl = np.asarray(d["edge"]), np.asarray(d["edge_length"], dtype=np.float64)
print(f"squamate tree, {se.shape[0] // 2 + 1} tips, longest branch {sl.max():.3g}", flush=True)
case("squamate", se, sl, sym20, 4, 64)
case("squamate", se, sl, er61, 4, 64)
if FULL:
    for model, Cn, S in ((sym20, 64, 64), (sym20, 4, 512), (er61, 64, 64), (er61, 4, 512), (sym20, 64, 512), (er61, 64, 512)):
        case("squamate", se, sl, model, Cn, S)
else:
    skipped("the squamate tree beyond C=4 S=64 (--full)")
