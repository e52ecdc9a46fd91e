"""Stochastic maps of the MCMC samplers (phm_maketreelistMCMC_maps): what a recorded sweep costs.  Plain: a resident engine on
the same (tile, branch) kernels runs the N sweeps (HIP-event span of the sweeps) and the plain one-shot driver gives the whole-call
time.  Maps: the sizing and the filling call, whose phm_last_kernel_ms is the same span with the replays in it.  A recorded sweep
costs plain + (maps - plain) / J of sweep time.  Plain and maps calls alternate in one process after a warm-up; medians.
C3 (10 000 tips, 4 states, _bigtree) at 1 024 chains with J = 1 and 10 of N = 100 and at 16 384 with J = 1; C4's 500-tip tree at 61 states with
128 chains; C5 (5 000 tips, 20 states tridiagonal, SPARSE with the rescaled pruning pass) at 1 024 chains.
At 16 384 chains J = 1 only: J = 10 would be ~9.8e9 segments, 118 GB of maps.
python tools/probes/probe_mcmc_maps.py [reps]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

from phylomap_amd import _lib, api, synth  # noqa: E402

L = _lib.load()
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
FN = {_lib.PHM_MCMC_BIGTREE: "sumstatMCMC_bigtree", _lib.PHM_MCMC: "sumstatMCMC", _lib.PHM_MCMC_SPARSE: "SPARSEsumstatMCMC"}


def probe(label, cfg, variant, S, N, J, reps=REPS, **extra):
    z, Q, pid, Om = synth.config_problem(cfg)
    E = z["edge"].shape[0]
    n = Q.shape[0]
    its = np.ascontiguousarray(np.linspace(0, N - 1, J).round().astype(np.int32))
    opt = dict(seed=0x3C, n_replicas=S, reduce=True, mapping="tiles", **extra)
    Qf = np.asfortranarray(Q, dtype=np.float64)
    B = np.asfortranarray(np.eye(n) + Q / Om)
    pidc = np.ascontiguousarray(pid, dtype=np.float64)
    nen, nodelist, root = _lib.tree_orders(z)
    ft = _lib.FlatTree(z)
    o = _lib.make_options(**opt)
    out = np.zeros((N, n + n * (n - 1)), order="F")
    args = (int(variant), C.byref(ft.c), n, _lib._p(Qf, C.c_double), _lib._p(pidc, C.c_double), _lib._p(B, C.c_double), float(Om),
            _lib._p(nen, C.c_int32), _lib._p(nodelist, C.c_int32), int(root), int(N), _lib._p(its, C.c_int32), int(J), C.byref(o),
            _lib._p(out, C.c_double))
    off = np.zeros(S * J * E + 1, dtype=np.int64)

    def plain_kernel():
        eng = _lib.Engine(z, Q, pid, Om, N, variant=variant, **opt)
        eng.run(N)
        eng.sync()
        ms = eng.info().last_run_ms
        eng.close()
        return ms

    def plain_call():
        t = time.perf_counter()
        getattr(api, FN[variant])(z, Q, pid, Om, N, **opt)
        return (time.perf_counter() - t) * 1e3

    def maps_call(fill):
        if fill:
            total = int(off[-1])
            dwell, state = np.empty(max(total, 1)), np.empty(max(total, 1), dtype=np.int32)
            dwell[::4096] = 0.0                                          # first touch of the pages outside the timed region
            state[::4096] = 0
            tail = (_lib._p(off, C.c_int64), total, _lib._p(dwell, C.c_double), _lib._p(state, C.c_int32))
        else:
            tail = (_lib._p(off, C.c_int64), 0, None, None)
        t = time.perf_counter()
        _lib.check(L.phm_maketreelistMCMC_maps(*args, *tail))
        return L.phm_last_kernel_ms(), (time.perf_counter() - t) * 1e3

    plain_kernel(); plain_call(); maps_call(False); maps_call(True)          # warm-up: code objects, first allocations
    rows = {"plain": [], "sizing": [], "filling": []}
    for _ in range(reps):
        rows["plain"].append((plain_kernel(), plain_call()))
        rows["sizing"].append(maps_call(False))
        rows["filling"].append(maps_call(True))
    k0 = np.median([k for k, _ in rows["plain"]])
    w0 = np.median([w for _, w in rows["plain"]])
    total = int(off[-1])
    print(f"{label}: N={N} J={J}, {total} segments ({total / (S * J):.0f} per history), "
          f"{12 * total / 2**30 + 8 * (S * J * E + 1) / 2**30:.2f} GiB; plain sweep {k0 / N:.3f} ms", flush=True)
    for name in ("plain", "sizing", "filling"):
        k = np.median([x for x, _ in rows[name]])
        w = np.median([x for _, x in rows[name]])
        rec = (k0 / N + (k - k0) / J) / (k0 / N)
        print(f"  {name:8s} sweeps {k:9.2f} ms   recorded sweep {rec:5.2f}x plain   whole call {w:9.1f} ms ({w / w0:5.2f}x)", flush=True)


probe("C3 bigtree S=1024", 3, _lib.PHM_MCMC_BIGTREE, 1024, 100, 1)
probe("C3 bigtree S=1024", 3, _lib.PHM_MCMC_BIGTREE, 1024, 100, 10)
probe("C3 bigtree S=16384", 3, _lib.PHM_MCMC_BIGTREE, 16384, 100, 1, reps=1)
# (16 384 chains with J = 10 would be 163 840 histories: ~9.8e9 segments, 118 GB of maps -- beyond the host memory of a filling call)
probe("C4 61 states bigtree S=128", 4, _lib.PHM_MCMC_BIGTREE, 128, 100, 10)
probe("C5 20 states SPARSE (rescaled pruning) S=1024", 5, _lib.PHM_MCMC_SPARSE, 1024, 100, 10, rescale=True)
