"""Batched posterior sampling of rates (phm_gibbs_rates / api.posterior_rates): wall and device time per
iteration of the driver against the only route there was before it -- a Python loop over
``api.sample_histories(draws=1, replica_offset=i)`` with a host update -- alternating in one process after a warm-up, medians of 3.
The loop's host update is numpy's vectorised Gamma generator on the same shapes and rates: cheaper than the driver's own
(one Philox stream per chain and parameter), so the comparison favours the loop.
  * 2 states (ard) on a 200-tip tree, 4 states (a hidden-rates pattern seen through parity) on the squamate fixture (3 951 tips);
  * C = 64, 1 024 and 16 384 chains on the one site.
With q_timing the driver prints the split of an iteration (upload, launches + device + download, host update) and its launch count.
python tools/probes/probe_gibbs.py [--quick]     (--quick: no 16 384-chain squamate case)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from phylomap_amd import _lib, api, posterior, ratemodel, synth  # noqa: E402

L = _lib.load()
QUICK = "--quick" in sys.argv
HIDDEN_INDEX = [[0, 1, 2, 0], [3, 0, 0, 2], [4, 0, 0, 1], [0, 4, 3, 0]]


def loop_route(z, model, pid, prior, th0, iters, theta_max, obs, seed):
    """the parent's only route: one sample_histories call per iteration (one lane in 64 filled), update on the host"""
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
    som = np.zeros(th.shape[0], dtype=np.int32)
    dev = 0.0
    for i in range(iters):
        st, ll = api.sample_histories(z, posterior.rate_matrices(model, th), pid, 1, observe=obs, site_of_model=som, seed=seed,
                                      replica_offset=i)
        dev += L.phm_last_kernel_ms()
        st = st[:, 0, :]
        fresh = rng.gamma(prior[None, :, 0] + st[:, n:] @ A, 1.0 / (prior[None, :, 1] + st[:, :n] @ W))
        th = np.where(fresh <= theta_max, fresh, th)
    return dev, th


def case(name, z, model, pid, obs, Cs, iters_of):
    lens = np.asarray(z["edge.length"], dtype=np.float64)
    T = len(z["states"])
    rate0 = T / float(lens.sum())
    row_max = int(np.max(np.sum(np.asarray(model.index) > 0, axis=1)))
    theta_max = min(100.0 * rate0, 0.9 * 32768.0 / (row_max * float(lens.max())))
    prior = np.ones((model.p, 2))
    print(f"{name}: {T} tips, {model.n} states, {model.p} rates, theta_max {theta_max:.3g}, longest branch {lens.max():.3g}", flush=True)
    for Cn in Cs:
        iters = iters_of(Cn)
        th0 = np.random.default_rng(Cn).uniform(0.5, 1.5, (Cn, model.p)) * min(rate0, 0.5 * theta_max)

        def driver(q_timing=False):
            kw = {"q_timing": 1} if q_timing else {}
            t = time.perf_counter()
            r = api.posterior_rates(z, model, pid, prior, iters, chains=Cn, observe=obs, per_site=True, theta0=th0,
                                    theta_max=theta_max, seed=5, **kw)
            return (time.perf_counter() - t) * 1e3, L.phm_last_kernel_ms(), r

        def loop():
            t = time.perf_counter()
            dev, _ = loop_route(z, model, pid, prior, th0, iters, theta_max, obs, 5)
            return (time.perf_counter() - t) * 1e3, dev

        api.posterior_rates(z, model, pid, prior, 2, chains=Cn, observe=obs, per_site=True, theta0=th0, theta_max=theta_max, seed=5)
        loop_route(z, model, pid, prior, th0, 2, theta_max, obs, 5)                              # warm-up of both
        rows = []
        for _ in range(3):                                                                        # alternating
            wd, kd, r = driver()
            wl, kl = loop()
            rows.append((wd / iters, kd / iters, wl / iters, kl / iters))
        wd, kd, wl, kl = (float(np.median(c)) for c in zip(*rows))
        print(f"  C={Cn:6d} ({iters} iterations): driver wall {wd:9.3f} ms/iter, device {kd:9.3f} | loop wall {wl:9.3f} ms/iter, device "
              f"{kl:9.3f} | loop / driver: wall {wl / wd:6.2f}x, device {kl / kd:6.2f}x | rejected {int(r['rejected'].sum())}, "
              f"failed chains {int(r['status'].sum())}", flush=True)
        sys.stderr.flush()
        driver(q_timing=True)                                                                     # the split, to stderr
        sys.stderr.flush()


m2 = ratemodel.ard(2)
edge, lens = synth.random_tree(200, 0.3, 17)
tips = synth.simulate_tips(edge, lens, m2.Q([0.3, 0.6]), np.array([.5, .5]), 3).astype(np.int32)
z2 = {"edge": edge, "edge.length": lens, "Nnode": edge.shape[0] // 2, "states": tips}
case("200-tip tree", z2, m2, np.array([.5, .5]), None, (64, 1024, 16384), lambda c: 20 if c <= 1024 else 6)

d = np.load(os.path.join(ROOT, "tests", "golden", "squamate", "seed101_tips.npz"))
Ts = len(d["states"])
zs = {"edge": d["edge"], "edge.length": d["edge_length"], "Nnode": Ts - 1, "states": d["states"]}
case("squamate", zs, ratemodel.index_model(HIDDEN_INDEX), np.full(4, .25), (1, 2, 1, 2), (64, 1024) if QUICK else (64, 1024, 16384),
     lambda c: 6 if c <= 1024 else 3)
