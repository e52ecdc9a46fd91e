"""The AIC companion of run_dic.py: maximum-likelihood fits of the 2-state model and of the 4-state hidden-rates model to the
seed-101 tip data on the 3 951-tip squamate tree (tests/golden/squamate/seed101_tips.npz), by ``api.fit_ml`` over the batched
likelihood.  The reference gets this half of its model-selection study from corHMM
(get_corHMM_AIC_result, R/sourceme.R:694-757: rate.cat = 1 against rate.cat = 2).

  python tools/squamate_dic/run_aic.py            # needs an MI355X

The models are this project's: ``ratemodel.ard(2)`` (2 parameters) and ``ratemodel.hidden_rates(1)`` = synth.make2sQ
(5 parameters, tips observed up to parity) -- not corHMM's 8-parameter rate.cat = 2 matrix -- so the outcome is recorded, not
pinned against the published table.  TEST TOOLING; prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def load_tree(path=os.path.join(ROOT, "tests", "golden", "squamate", "seed101_tips.npz")):
    d = np.load(path)
    T = len(d["states"])
    return {"edge": d["edge"], "Nnode": T - 1, "edge.length": d["edge_length"], "states": d["states"]}


def run(starts=8, seed=101, max_iter=200, **opt):
    """{"ard2": fit, "hidden_rates1": fit, "seconds": ..}: the two ``api.fit_ml`` results on the squamate fixture"""
    from phylomap_amd import api, ratemodel
    z = load_tree()
    t0 = time.time()
    two = api.fit_ml(z, ratemodel.ard(2), [.5, .5], starts=starts, seed=seed, max_iter=max_iter, **opt)
    four = api.fit_ml(z, ratemodel.hidden_rates(1), [.25] * 4, observe=[1, 2, 1, 2], starts=starts, seed=seed, max_iter=max_iter,
                      **opt)
    return {"ard2": two, "hidden_rates1": four, "seconds": time.time() - t0, "tree": z}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--starts", type=int, default=8)
    ap.add_argument("--seed", type=int, default=101)
    a = ap.parse_args()
    r = run(a.starts, a.seed)
    out = {"starts": a.starts, "seed": a.seed, "seconds": round(r["seconds"], 2)}
    for name in ("ard2", "hidden_rates1"):
        f = r[name]
        out[name] = {"loglik": round(float(f["loglik"]), 6), "aic": round(float(f["aic"]), 6), "theta": [float(t) for t in f["theta"]],
                     "converged": bool(f["converged"]), "at_bound": [bool(b) for b in f["at_bound"]],
                     "iterations": int(f["iterations"]), "likelihood_calls": int(f["calls"]),
                     "max_abs_fd_gradient": float(np.max(np.abs(f["grad"])))}
    out["delta_aic_4_minus_2"] = round(out["hidden_rates1"]["aic"] - out["ard2"]["aic"], 6)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
