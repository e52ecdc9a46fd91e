"""Inputs shared by the CPU and GPU tests of the MCMC stochastic maps at every class of the 5 to 64 state sweep (the replay
mcmc_maps_wtiles_kernel of phm_mcmc_maps.hip against the ten draws of wt_branch_kernel): the cases of
tests/wtilesclasses.py by reference, four new ones (a SPARSE chain whose pruning matrix is banded and whose draw matrix is not, the
same beyond 32 states, and a branch beyond 64 segments at 17 and at 40 states), the branch kernel each engine run of a case is
listed for, and the oracle's maps: the path a sweep leaves, virtual jumps included, with equal neighbours merged (computed once
per session, shared, never written).  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import wtilesclasses as W
from phylomap_amd import synth

LADDER_CLASSES = ((12, 2), (32, 1))
SPARSE_NS = (12, 36)
LONG_NS = (17, 40)
LONG_SEGMENTS, LONG_JUMPS = 100, 90.0


def map_iters(N):
    """the recorded iterations of the device tests: the first sweep (from the initial paths), one inside, the last"""
    return [0, 2, N - 1]


def branch_kernel(ks, small, b2l, band):
    return W.kname("wt_branch_kernel", ks, small, b2l, band)


class MapCase:
    """A wtilesclasses.Case with the engine option sets the maps are asked for under (the case's runs without ``reduce``: the maps
    are per chain) and, per option set, the wt_branch_kernel instantiation the case is listed for -- written down per family
    below, not taken from wtilesclasses.dispatch"""

    def __init__(self, case, family, listed, runs=None, long_branch=False):
        self.case, self.family, self.name, self.long_branch = case, family, case.name, long_branch
        sets = []
        for r in (case.runs if runs is None else runs):
            r = {k: v for k, v in r.items() if k != "reduce"}
            if r not in sets:
                sets.append(r)
        self.runs = tuple(sets)
        self.listed = tuple(listed(r) for r in self.runs) if callable(listed) else (listed,) * len(self.runs)
        # the Python twin where it is affordable: about 2 s a chain at 17 states on 11 to 14 tips (not on the 300-tip ladders)
        self.twin = case.n <= 17 and family != "ladder"

    def __getattr__(self, k):
        return getattr(self.case, k)


@functools.lru_cache(maxsize=None)
def sparse_case(n):
    """SPARSE with one rate below the driver's threshold in the far corner: the chain matrix of the pruning pass is tridiagonal,
    the matrix the branch kernel draws from is not"""
    Q = W.banded_Q(n, 1, seed=n)
    Q[0, n - 1] = 2e-8 * W._omega(Q)
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(1))
    pid = W.skew_pid(n, 100 * n + 1)
    z = synth.make_tree(12, Q, W._omega(Q), 800 + n + 1, pid, states=W.spread_tips(12, n, n + 1), init_segments=n)
    return W.Case(f"sparse_mixed_n{n}", f"SPARSE, n = {n}: chain matrix of half-bandwidth 1, draw matrix with B[0, {n - 1}] = 2e-8", Q, pid,
                  z, "sparse", 6, 70, 61, W.REPLICAS_2_TILES, ({},))


@functools.lru_cache(maxsize=None)
def long_case(n):
    """dense_case(n)'s model and tree with edge row 0 stretched to 90 / Omega in 100 initial segments: more than 64 segments on
    that branch sweep after sweep (the problem of tests/test_gpu_mcmc_maps.py's long branch, at 17 and 40 states)"""
    Q = synth.dense_Q(n, 0.02, 0.08, seed=n)
    pid = np.full(n, 1.0 / n)
    Omega = W._omega(Q)
    z = synth.make_tree(11, Q, Omega, 700 + n, pid, init_segments=3)
    z["edge.length"] = np.array(z["edge.length"], dtype=np.float64)
    z["edge.length"][0] = LONG_JUMPS / Omega
    end = int(z["mapnames"][0][-1])
    z["maps"][0], z["mapnames"][0] = synth.initial_path(z["edge.length"][0], end, LONG_SEGMENTS)
    return W.Case(f"long_n{n}", f"dense n = {n}: edge row 0 beyond 64 segments in every sweep", Q, pid, z, "bigtree", 6, 70, 83,
                  W.REPLICAS_2_TILES, ({},))


def new_cases():
    return [MapCase(sparse_case(12), "sparse", branch_kernel(False, True, True, 0)),
            MapCase(sparse_case(36), "sparse", branch_kernel(False, False, False, 0)),
            MapCase(long_case(17), "long", branch_kernel(False, True, True, 0), long_branch=True),
            MapCase(long_case(40), "long", branch_kernel(False, False, False, 0), long_branch=True)]


B2L_GROUPS = (1, 4, 64)                                 # 26 edges: 4 leaves a short last group, 64 puts the tree in one wave


def _band_of(name):
    return int(name.split("_")[0][len("band"):])


def class_cases():
    """the cases of wtilesclasses the maps are asked of, each with the branch kernel it is listed for"""
    out = []
    for c in W.dense_cases():
        out.append(MapCase(c, "dense", branch_kernel(False, c.n <= 32, c.n <= 32, 0)))
    for c in W.band_cases():
        hb = _band_of(c.name)
        if c.name.endswith("random"):
            out.append(MapCase(c, "band", branch_kernel(False, True, True, hb)))
        elif (4 * W.ceil_div(c.n, 4), hb) in LADDER_CLASSES:
            out.append(MapCase(c, "ladder", branch_kernel(False, True, True, hb)))
    for c in W.b2l_cases():
        ks = c.variant == "ks"
        out.append(MapCase(c, "b2l", lambda r, ks=ks: branch_kernel(ks, False, r["branch_group"] >= 4, 0),
                           runs=tuple({"branch_group": g} for g in B2L_GROUPS)))
    for c, (_, hb) in zip(W.slot_cases(), W.SLOT_CASES):
        out.append(MapCase(c, "slots", branch_kernel(False, True, True, hb)))
    for c, band in zip(W.ks_small_cases(), (2, 1, 0)):
        out.append(MapCase(c, "ks_small", branch_kernel(True, True, True, band)))
    for c in W.ks_form_cases():
        out.append(MapCase(c, "ks_forms", branch_kernel(True, c.n <= 32, c.n <= 32, 0)))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(class_cases() + new_cases())


def by_name(name):
    return next(c for c in all_cases() if c.name == name)


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle's maps
# ---------------------------------------------------------------------------------------------------------------------------
def merged_dump(dump):
    """(off int64 [E + 1], dwell, state 0-based) of an oracle dump's paths with equal neighbours merged: within a run of equal
    states the dwells are added left to right, one addition per step as a scalar loop would make them"""
    count = np.asarray(dump.seg_count, dtype=np.int64)
    E, cap = count.size, int(count.max())
    live = np.arange(cap)[None, :] < count[:, None]
    d, s = np.asarray(dump.seg_dwell)[:, :cap][live], np.asarray(dump.seg_state)[:, :cap][live]
    row = np.repeat(np.arange(E), count)
    first = np.ones(d.size, dtype=bool)
    first[1:] = (row[1:] != row[:-1]) | (s[1:] != s[:-1])
    start = np.nonzero(first)[0]
    run = np.diff(np.append(start, d.size))
    dwell = d[start].copy()
    for j in range(1, int(run.max())):
        sel = run > j
        dwell[sel] = dwell[sel] + d[start[sel] + j]
    off = np.concatenate([[0], np.cumsum(np.bincount(row[start], minlength=E))]).astype(np.int64)
    return off, dwell, s[start].astype(np.int32)


@functools.lru_cache(maxsize=None)
def oracle_maps(case, replica):
    """For every iteration 0 .. N - 1: (off int64 [E + 1], dwell, state 0-based, raw segment counts [E]) -- the path sweep ``it``
    left on every edge row is the chain state after ``it + 1`` sweeps, virtual jumps included; merged, it is the map of ``it``.
    ``case`` is a wtilesclasses.Case."""
    out = []
    for it in range(case.N):
        _, rc, dump = case.oracle(replica, dump=True, N=it + 1)
        assert rc == 0, (case.name, replica, it, rc)
        arrs = merged_dump(dump) + (np.array(dump.seg_count, dtype=np.int64),)
        for a in arrs:
            a.setflags(write=False)
        out.append(arrs)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def twin_rows(case, replica):
    """rows[(it, b)] = [(dwell, state 0-based), ...] of the Python twin (tests/mcmcmapsref.py), every iteration recorded"""
    import mcmcmapsref
    _, rows = mcmcmapsref.sumstatMCMC(case.z, case.Q.tolist(), case.pid.tolist(), case.Omega, case.N, [int(v) for v in case.nen],
                                      [int(v) for v in case.nodelist], int(case.root), case.seed, replica, variant=case.variant)
    return rows


def longest_branch(case):
    """L of the dwell bar: the case's longest branch on the oracle, in segments, over the compared replicas and every sweep"""
    return max(W.oracle_walk(case, r)[0] for r in case.replicas)


def dwell_bar(case):
    """Both sides add at most L positive numbers left to right (the device the old path's dwells into a merged segment, the oracle
    the pieces the virtual jumps cut it into); each sum is within (L - 1) 2^-53 relative of the exact one, so the two differ by at
    most 2 L 2^-53 relative.  The bar allows twice that."""
    return 4.0 * longest_branch(case) * 2.0 ** -53


def interior(off, state):
    """the states of the segments that are neither the first nor the last of their row"""
    idx = np.arange(state.size)
    row = np.repeat(np.arange(off.size - 1), np.diff(off))
    return state[(idx != off[row]) & (idx != off[row + 1] - 1)]
