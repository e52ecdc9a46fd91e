"""The small problems of tests/test_gpu_sweep_parts.py, shared with tests/golden/sweep_parts/make_golden.py (which records what the
commit BEFORE the sweep parts computed for them: that build knows no phm_debug_options.sweep_parts, so nothing here names it)."""
import numpy as np

from phylomap_amd import _lib, synth

RUNS = (2, 4)      # six sweeps as run(2) + run(4): the fork / join happens twice and the `it & 1` dwell buffers alternate across calls


def problem(name):
    """(z, Q, pid, Omega, variant): random trees of about 40 tips at 4 and 2 states, the hidden-rates (KS) sweep at 4 states, and
    the 1 000-tip C2 tree, on which 66 tiles make a wave of the branch kernel walk TWO branches: only there does the branch kernel
    write a segment row per group (with one branch per wave the reduction walks the segment counts itself)."""
    if name == "c2":
        return synth.config_problem(2) + (_lib.PHM_MCMC_BIGTREE,)
    if name == "n4":
        Q = synth.config_Q(2)
    elif name == "n2":
        Q = synth.config_Q(1)
    elif name == "ks":
        Q = synth.make2sQ(.1, .1, .2, .2, 10)
    else:
        raise KeyError(name)
    n = Q.shape[0]
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    pid = np.full(n, 1.0 / n)
    tips, seed = {"n4": (41, 23), "n2": (39, 29), "ks": (43, 31)}[name]
    variant = _lib.PHM_MCMC_KS if name == "ks" else _lib.PHM_MCMC_BIGTREE
    return synth.make_tree(tips, Q, Omega, seed, pid), Q, pid, Omega, variant


def sweep(name, S, reduce, level_groups=1, omega_scale=1.0, **debug):
    """run(2) + run(4) of `name` at S replicas on the (tile, branch) mapping.  Returns (statistics of the six sweeps, seg_read after
    each run, recoveries, launches of each run).  level_groups = 1: one launch per tree level -- on trees this small the automatic
    choice is the cluster kernels, which never run in parts."""
    z, Q, pid, Omega, variant = problem(name)
    Omega = omega_scale * Omega
    N = sum(RUNS)
    eng = _lib.Engine(z, Q, pid, Omega, N, variant=variant, seed=0xC0FFEE, n_replicas=S, mapping="tiles", reduce=reduce,
                      level_groups=level_groups, **debug)
    seg, launches = [], []
    for k in RUNS:
        eng.run(k); eng.sync()
        info = eng.info()
        seg.append(int(info.seg_read)); launches.append(int(info.last_run_launches))
    stats = np.array(eng.stats(0, N))
    rec = int(eng.info().recoveries)
    eng.close()
    return stats, np.array(seg, dtype=np.int64), rec, launches


# what the fixture holds: (problem, replicas, level_groups, reduce) -- per-replica rows for two cases only (the file stays small)
GOLDEN_CASES = [("n4", 320, 1, True), ("n4", 300, 1, True), ("n4", 300, 1, False), ("n2", 300, 1, True), ("ks", 300, 1, True),
                ("ks", 300, 1, False), ("n4", 300, 2, True), ("ks", 300, 2, True), ("c2", 4224, 1, True)]


def golden_key(name, S, lg, reduce):
    return f"{name}_S{S}_lg{lg}_{'red' if reduce else 'rep'}"
