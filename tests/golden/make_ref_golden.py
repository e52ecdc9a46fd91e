"""Generates tests/golden/ref/*.npz: for a fixed subset of the grid of tests/refcases.py, the inputs and the output matrix that
the REFERENCE's own src/phylomap.cpp wrote when run on them (built on the stand-in headers, oracle/ref_build.sh).  Data only.
Needs oracle/_ref/libphm_ref.so, i.e. a machine with the reference tree.  Run from the repo root:
    python tests/golden/make_ref_golden.py
tests/test_reference_pin_cpu.py::test_recorded_fixtures_match_a_live_reference_run fails when these files and the reference
disagree, so they cannot drift."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import refcases as RC  # noqa: E402

OUT = os.path.join(HERE, "ref")


def recorded():
    """name -> dict of arrays, for every recorded case, from a live run of the reference."""
    out = {}
    for c in RC.cases():
        if c["record"]:
            ref_out, ref_rc = RC.run_reference(c)
            out[c["name"]] = RC.pack_case(c, ref_out, ref_rc)
    return out


def sampler_inputs():
    """Inputs of the per-function fixture: weight vectors (NaN-padded rows) with uniforms for sampleOnce -- among them uniforms
    that EQUAL a cumulative sum, where its strict `<` decides, and vectors on which it runs off the end -- and probability
    vectors with seeds for sample(), ties included."""
    rs = np.random.default_rng(2024)
    W = np.full((40, 8), np.nan)
    U = np.zeros(40)
    hand = [([1.0, 1.0], 0.5), ([0.25, 0.75], 0.25), ([0.5, 0.25, 0.25], 0.75), ([1.0, 1.0, 2.0], 0.25), ([0.25, 0.5], 1.0), ([1.0], 1.0),
            ([0.0, 0.0], 0.5), ([2.0, 2.0, 2.0, 2.0], 0.5), ([0.0, 1.0, 0.0], 0.0), ([1.0, 3.0], 0.2499999999999999)]
    for i in range(40):
        w, u = hand[i] if i < len(hand) else (rs.random(int(rs.integers(1, 9))), float(rs.random()))
        W[i, :len(w)] = w
        U[i] = u
    P = np.full((40, 16), np.nan)
    seeds = np.arange(1, 41, dtype=np.int64)
    for i in range(40):
        n = int(rs.integers(1, 17))
        p = rs.random(n) * (rs.random(n) > 0.25)
        if i % 3 == 0:
            p = np.round(p * 4) / 4                      # exact ties (and exact zeros)
        if not p.any():
            p[0] = 1.0
        P[i, :n] = p
    return W, U, P, seeds


def recorded_functions():
    """The per-function fixture from a live run of the reference: sampleOnce's index per (weights, uniform) and sample()'s per
    (probabilities, seed)."""
    import ref_lib as R
    W, U, P, seeds = sampler_inputs()
    once, drawn = [], []
    for w, u in zip(W, U):
        i, rc = R.sampleOnce(w[~np.isnan(w)], float(u))
        assert rc == R.OK
        once.append(i)
    for p, seed in zip(P, seeds):
        i, rc = R.sample(p[~np.isnan(p)], int(seed))
        assert rc == R.OK
        drawn.append(i)
    return {"W": W, "U": U, "sampleonce_ref": np.array(once, dtype=np.int32), "P": P, "seeds": seeds,
            "sample_ref": np.array(drawn, dtype=np.int32)}


def main():
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "fn_samplers.npz"), **recorded_functions())
    print("fn_samplers", os.path.getsize(os.path.join(OUT, "fn_samplers.npz")), "bytes")
    for name, d in recorded().items():
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **d)
        print(name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
