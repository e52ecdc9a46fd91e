"""Stochastic maps (phm_simulate_histories_maps, phm_maketreelistEXP_maps): the sizing call and the filling call against the
plain call, HIP-event kernel time (sampler + offsets scan) and whole-call time.  The simulator on C3 (10 000 tips, 4 states) at
1 024 and 16 384 histories and on the 500-tip C4 tree with 61 states at 128; sumstatEXP at N = 1 000 on C3 (rescaled pruning).
python tools/probes/probe_maps.py"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

from phylomap_amd import _lib, api, synth  # noqa: E402

L = _lib.load()


def timed(fn):
    t = time.perf_counter()
    _lib.check(fn())
    return L.phm_last_kernel_ms(), (time.perf_counter() - t) * 1e3


def probe(label, plain, maps_fn, args, R, E, reps):
    off = np.zeros(R * E + 1, dtype=np.int64)
    plain(*args)                                                      # warm-up: code objects, first allocations
    rows = {"plain": [], "sizing": [], "filling": []}
    for _ in range(reps):
        rows["plain"].append(timed(lambda: plain(*args)))
        rows["sizing"].append(timed(lambda: maps_fn(*args, _lib._p(off, C.c_int64), 0, None, None)))
        total = int(off[-1])
        dwell, state = np.empty(total), np.empty(total, dtype=np.int32)
        dwell[::4096] = 0.0                                          # first touch of the pages outside the timed region
        state[::4096] = 0
        rows["filling"].append(timed(lambda: maps_fn(*args, _lib._p(off, C.c_int64), total, _lib._p(dwell, C.c_double),
                                                     _lib._p(state, C.c_int32))))
        del dwell, state
    k0 = np.median([k for k, _ in rows["plain"]])
    w0 = np.median([w for _, w in rows["plain"]])
    print(f"{label}: {total} segments ({total / R:.0f} per history), {12 * total / 2**30 + 8 * (R * E + 1) / 2**30:.2f} GiB", flush=True)
    for name in ("plain", "sizing", "filling"):
        k = np.median([x for x, _ in rows[name]])
        w = np.median([x for _, x in rows[name]])
        print(f"  {name:8s} kernel {k:9.2f} ms ({k / k0:5.2f}x)   whole call {w:9.1f} ms ({w / w0:5.2f}x)", flush=True)


def sim_args(z, Q, pid, R):
    Q = np.asfortranarray(Q, dtype=np.float64)
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    ft = _lib.FlatTree(z)
    o = _lib.make_options(n_replicas=R, seed=0x3A)
    n = Q.shape[0]
    tips = np.zeros((R, ft.T), dtype=np.int32)
    stats = np.zeros((R, n * (n + 1) + 1), order="F")
    keep.append((Q, pid, ft, o, tips, stats))
    return (C.byref(ft.c), n, _lib._p(Q, C.c_double), _lib._p(pid, C.c_double), None, C.byref(o), _lib._p(tips, C.c_int32), None,
            _lib._p(stats, C.c_double))


def exp_args(z, Q, pid, N):
    Q = np.asfortranarray(Q, dtype=np.float64)
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    n = Q.shape[0]
    nen, nodelist, root = _lib.tree_orders(z)
    lefts, rights, d = (np.asfortranarray(a) for a in api.eigen_decompose(Q))
    ft = _lib.FlatTree(z)
    o = _lib.make_options(seed=0x3B, rescale=True)
    out = np.zeros((N, n + n * (n - 1)), order="F")
    keep.append((Q, pid, nen, nodelist, lefts, rights, d, ft, o, out))
    return (C.byref(ft.c), n, _lib._p(Q, C.c_double), _lib._p(pid, C.c_double), _lib._p(nen, C.c_int32), _lib._p(nodelist, C.c_int32),
            int(root), N, _lib._p(lefts, C.c_double), _lib._p(rights, C.c_double), _lib._p(d, C.c_double), C.byref(o),
            _lib._p(out, C.c_double))


keep = []
z3, Q3, pid3, _ = synth.config_problem(3)
E3 = z3["edge"].shape[0]
probe("simulator C3 n=4 R=1024", L.phm_simulate_histories, L.phm_simulate_histories_maps, sim_args(z3, Q3, pid3, 1024), 1024, E3, 3)
probe("simulator C3 n=4 R=16384", L.phm_simulate_histories, L.phm_simulate_histories_maps, sim_args(z3, Q3, pid3, 16384), 16384, E3, 1)
probe("sumstatEXP C3 n=4 N=1000", L.phm_maketreelistEXP, L.phm_maketreelistEXP_maps, exp_args(z3, Q3, pid3, 1000), 1000, E3, 3)
z4, Q4, pid4, _ = synth.config_problem(4)
probe("simulator C4 n=61 R=128", L.phm_simulate_histories, L.phm_simulate_histories_maps, sim_args(z4, Q4, pid4, 128), 128,
      z4["edge"].shape[0], 3)
