"""Inputs shared by the CPU and GPU tests of the rate-updating drivers beyond six states (sumstatMCMCks, sumstatMCMCksDICt,
sumstatMCMCksmt; DESIGN.md section 10, "Dispatch classes under a changing model"): hidden-rates models whose state counts are
chosen by the branch of upload_model (phm_engine.cpp) they take, the trees they run on, the oracle's runs (computed once per
session, shared, never written) and the dispatch rules of the host, restated.  TEST INFRASTRUCTURE ONLY.

A hidden-rates Q (synth.make2sQ) has half-bandwidth 2, four non-zeros in every row of B = I + Q/Omega but the four outer ones,
and 4n - 4 possible transitions counting self pairs; with every regime-switching rate zero it has half-bandwidth 1, two non-zeros
per row and 2n transitions, and the first accepted update of a kappa widens it."""
import functools

import numpy as np

import oracle_lib as O
from phylomap_amd import synth, treeorder

# the engine's constants (phm_wtiles.h, phm_wbranch.h, phm_wide.h)
WT_BAND_MAX, WT_BAND_NMAX, WT_MAX_SLOTS, WB_ELL_MAX, WIDE_SEG_CAP = 2, 32, 96, 16, 128

PRIOR = (1.0, 10.0, 2.0, 10.0, 20.0, 2.0)          # vignettes/phylomap_tutorial.Rnw:248-256
PRIOR_MT = (1.0, 10.0, 1.5, 11.0, 2.0, 10.0, 20.0, 2.0)
N_ITERS, SEED = 12, 7
MAPPINGS = ("replicas", "branches", "tiles")

# name -> (n, band-widening start, tips, tree seed).  What each n is there for:
#   8   band kernels, LDS slots (28), dense rows on the branch mapping (3 * 4 > 8)
#   12  ELLPACK switches on (3 * 4 <= 12)
#   24  92 slots: the last n with LDS slots
#   26  100 slots > 96: band kernels without slots
#   32  the last n with band kernels
#   34  matrix cores, no band, the n > 32 counting
#   62  the size C4 names;  64  k = 31, the largest a hidden-rates model takes
#   widen8 / widen12: rk = lk = 0 at the start; ELLPACK width 2 -> 4, which at n = 8 switches it off
CASES = {
    "n8": (8, False, 30, 16), "n12": (12, False, 30, 16), "n24": (24, False, 30, 16), "n26": (26, False, 30, 16),
    "n32": (32, False, 30, 16), "n34": (34, False, 30, 16), "n62": (62, False, 30, 16), "n64": (64, False, 30, 16),
    "widen8": (8, True, 30, 16), "widen12": (12, True, 30, 16),
}
# the classes the cases were chosen for, at the start and once every kappa is positive: (band, LDS slots, ELLPACK width)
EXPECTED = {
    "n8": ((2, 28, 0),) * 2, "n12": ((2, 44, 4),) * 2, "n24": ((2, 92, 4),) * 2, "n26": ((2, 0, 4),) * 2, "n32": ((2, 0, 4),) * 2,
    "n34": ((0, 0, 4),) * 2, "n62": ((0, 0, 4),) * 2, "n64": ((0, 0, 4),) * 2,
    "widen8": ((1, 16, 2), (2, 28, 0)), "widen12": ((1, 24, 2), (2, 44, 4)),
}
MULTI_NS = ("n8", "n26", "n34")                    # the multi-site runs
MULTI_S = (3, 70)                                  # a partly filled tile; two tiles, the second with 6 lanes
RECOVERY = ("n8", "n34")
LIST_NS = (12, 34)                                 # sumstatMCMCksmt
DIC_NS = ("n8", "n34")


def hidden_rates_Q(n, widen=False):
    """make2sQ(0.05, 0.08, rk, lk, gam) with the rk / lk / gam of tests/test_gpu_configs.py::_hidden_rates_62, cut to k = n/2 - 1"""
    k = n // 2 - 1
    rk = 0.02 + 0.01 * (np.arange(k) % 5)
    lk = 0.03 + 0.01 * (np.arange(k) % 3)
    gam = 0.5 + 0.25 * (np.arange(k) % 7)
    if widen:
        rk, lk = np.zeros(k), np.zeros(k)
    return synth.make2sQ(0.05, 0.08, rk, lk, gam)


def orders(z):
    return treeorder.pruningwiseedgeorder(z), treeorder.makenodelist(z), treeorder.myreorder(z)


def parity_tips(z):
    """only the parity of a tip state is observed, in the tip vector and at the end of the initial paths"""
    T = len(z["states"])
    z = dict(z, states=((z["states"] - 1) % 2 + 1).astype(np.int32), mapnames=[m.copy() for m in z["mapnames"]])
    for b, (_, c) in enumerate(z["edge"]):
        if c <= T:
            z["mapnames"][b][-1] = z["states"][c - 1]
    return z


class Problem:
    def __init__(self, name):
        self.name = name
        self.n, self.widen, self.tips, tree_seed = CASES[name]
        self.k = self.n // 2 - 1
        self.Q = hidden_rates_Q(self.n, self.widen)
        self.Q.setflags(write=False)
        self.Omega = 4.0 * float(np.max(np.abs(np.diag(self.Q))))     # room for the rates the updates draw
        self.pid = np.full(self.n, 1.0 / self.n)
        self.z = parity_tips(synth.make_tree(self.tips, self.Q, self.Omega / 3, tree_seed, self.pid))
        self.nen, self.nodelist, self.root = orders(self.z)
        self.length = float(self.z["edge.length"].sum())
        self.ncnt = self.n * self.n
        self.cols = self.n + self.ncnt + 2 + 3 * self.k + 1

    @property
    def B(self):
        return np.eye(self.n) + self.Q / self.Omega


@functools.lru_cache(maxsize=None)
def problem(name):
    return Problem(name)


# ---------------------------------------------------------------------------------------------------------------------------
# the host's dispatch rules (upload_model, phm_engine.cpp), restated; tests/test_rate_updates_cpu.py pins the cases to them
# ---------------------------------------------------------------------------------------------------------------------------
def half_bandwidth(M):
    i, j = np.nonzero(M)
    return int(np.max(np.abs(i - j)))


def band_class(B):
    """tiles mapping: the half-bandwidth the band kernels run with, 0 where they do not (usable(hb))"""
    n, hb = B.shape[0], half_bandwidth(B)
    return hb if (n <= WT_BAND_NMAX and 1 <= hb <= WT_BAND_MAX and 2 * hb + 1 < n) else 0


def slot_class(B):
    """tiles mapping, ks layout: the number of LDS transition slots (self pairs counted), 0 where the kernel counts in registers"""
    n, cnt = B.shape[0], int(np.count_nonzero(B))
    return cnt if (n <= 32 and cnt <= WT_MAX_SLOTS) else 0


def ell_class(B):
    """branches mapping: the ELLPACK width, 0 for dense rows"""
    n, w = B.shape[0], int(np.count_nonzero(B, axis=1).max())
    return w if (1 <= w <= WB_ELL_MAX and 3 * w <= n) else 0


def classes(Q, Omega):
    B = np.eye(Q.shape[0]) + np.asarray(Q) / Omega
    return band_class(B), slot_class(B), ell_class(B)


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle's runs
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_run(name, dic=False):
    """(rows [N_ITERS, cols], rc) of the updating driver, one chain"""
    p = problem(name)
    rows, rc = O.maketreelistMCMC(p.z, p.Q, p.pid, p.B, p.Omega, p.nen, p.nodelist, p.root, N_ITERS, variant=O.KS, seed=SEED,
                                  prior=PRIOR, dic=dic)
    rows.setflags(write=False)
    return rows, rc


RECOVERY_OMEGA_FACTOR = 2.0        # twice the virtual jumps: with cap_tail = 0.9 a branch slot holds about its expected count, no more


@functools.lru_cache(maxsize=None)
def recovery_oracle(name):
    """(rows, rc, Omega) of the updating driver at RECOVERY_OMEGA_FACTOR times the case's Omega"""
    p = problem(name)
    Om = RECOVERY_OMEGA_FACTOR * p.Omega
    rows, rc = O.maketreelistMCMC(p.z, p.Q, p.pid, np.eye(p.n) + p.Q / Om, Om, p.nen, p.nodelist, p.root, N_ITERS, variant=O.KS,
                                  seed=SEED, prior=PRIOR)
    rows.setflags(write=False)
    return rows, rc, Om


def schedule_from_rows(variant, Q0, Omega, prior, rows, seed):
    """[N, n, n]: Q_0 and, for every further iteration, what orc_qupdate_apply makes of (Q_i, row i, seed, i)"""
    Qs = [np.array(Q0, dtype=np.float64)]
    for i in range(len(rows) - 1):
        Qn, rc = O.qupdate_apply(variant, Qs[-1], Omega, prior, rows[i], seed, i)
        assert rc == 0
        Qs.append(Qn)
    return np.stack(Qs)


@functools.lru_cache(maxsize=None)
def oracle_schedule(name):
    """the Qs the oracle's run of the case went through"""
    p = problem(name)
    Qs = schedule_from_rows(O.KS, p.Q, p.Omega, PRIOR, oracle_run(name)[0], SEED)
    Qs.setflags(write=False)
    return Qs


def param_columns(Q):
    """recordQks (src/phylomap.cpp:1789-1798) of one Q"""
    k = Q.shape[0] // 2 - 1
    i = np.arange(k)
    return np.concatenate([[Q[0, 1], Q[1, 0]], Q[2 * i, 2 * i + 2], Q[2 * i + 2, 2 * i], Q[2 * i + 2, 2 * i + 3] / Q[0, 1]])


@functools.lru_cache(maxsize=None)
def longest_branch(name):
    """the largest segment count any branch of the oracle's chain holds after any of its sweeps (the dump shows the chain after the
    last sweep: one run under the first i Qs for every i)"""
    p, Qs = problem(name), oracle_schedule(name)
    longest = 0
    for i in range(1, N_ITERS + 1):
        _, rc, dump = O.maketreelistMCMC_schedule(p.z, Qs[:i], p.pid, p.Omega, p.nen, p.nodelist, p.root, seed=SEED, dump=True)
        assert rc == 0
        longest = max(longest, int(dump.seg_count.max()))
    return longest


_SUMS = {}


def summed_schedule_rows(name, Qs, S):
    """The inductive reference of the multi-site runs: the oracle's schedule entry under ``Qs`` for every replica r < S, the rows
    summed over r (dwell sums, counts, root state; the parameter columns are one replica's).  Kept per schedule: the mappings
    that add the dwell times alike share it."""
    key = (name, S, np.ascontiguousarray(Qs).tobytes())
    if key not in _SUMS:
        p = problem(name)
        total = None
        for r in range(S):
            rows, rc = O.maketreelistMCMC_schedule(p.z, Qs, p.pid, p.Omega, p.nen, p.nodelist, p.root, seed=SEED, replica=r)
            assert rc == 0
            if total is None:
                total = rows.copy()
            else:
                total[:, :p.n + p.ncnt] += rows[:, :p.n + p.ncnt]
                total[:, -1] += rows[:, -1]
        total.setflags(write=False)
        _SUMS[key] = total
    return _SUMS[key]


# ---------------------------------------------------------------------------------------------------------------------------
# lists of trees (sumstatMCMCksmt) and the trees of the DIC pass
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def list_problem(n):
    """(trees, Q, pid, Omega, nen_m, nodelist_m, roots) of 5 trees of 14 tips"""
    Q = hidden_rates_Q(n)
    Omega = 4.0 * float(np.max(np.abs(np.diag(Q))))
    pid = np.full(n, 1.0 / n)
    trees = [parity_tips(z) for z in synth.make_treelist(5, 14, Q, Omega / 3, 2024, pid)]
    od = [orders(z) for z in trees]
    return trees, Q, pid, Omega, np.stack([o[0] for o in od]), np.stack([o[1] for o in od]), [o[2] for o in od]


@functools.lru_cache(maxsize=None)
def list_oracle(n, seed):
    trees, Q, pid, Omega, nen_m, nodelist_m, roots = list_problem(n)
    rows, rc = O.maketreelistMCMCmt(trees, Q, pid, np.eye(n) + Q / Omega, Omega, nen_m, nodelist_m, roots, N_ITERS, PRIOR_MT,
                                    variant=O.KSMT, seed=seed)
    rows.setflags(write=False)
    return rows, rc


def tree_from_edges(edge, lens, states):
    """a phylomap tree object on a given topology: two half-length pieces per branch, state 1 and then the tip's state"""
    edge = np.asarray(edge, dtype=np.int32)
    T = edge.shape[0] // 2 + 1
    states = np.asarray(states, dtype=np.int32)
    maps, mapnames = [], []
    for r in range(edge.shape[0]):
        child = int(edge[r, 1])
        m, mn = synth.initial_path(float(lens[r]), int(states[child - 1]) if child <= T else 1, 2)
        maps.append(m)
        mapnames.append(mn)
    return {"edge": edge, "Nnode": T - 1, "edge.length": np.asarray(lens, dtype=np.float64), "states": states, "maps": maps,
            "mapnames": mapnames}


def ladder_edges(T, seed):
    """the caterpillar of T tips in cladewise order: T - 1 internal nodes on one path, every one with a tip; T - 1 height levels"""
    edges = []
    for i in range(T - 1):
        node = T + 1 + i
        edges.append((node, i + 1))
        edges.append((node, node + 1) if i < T - 2 else (node, T))
    # cladewise rows list a node's first child's whole clade before the second child: the tip first keeps that order
    lens = np.random.default_rng(seed).uniform(0.05, 0.6, len(edges))
    return np.asarray(edges, dtype=np.int32), lens


def height_level_sizes(edge):
    """internal nodes by height (1 + the larger height of the two children, tips 0), the lowest level first: the levels
    launch_exp_pl_loglik (phm_exp.hip) walks -- a level of more than EXP_RUN_BLOCK nodes gets a launch of its own, narrower ones
    share a run kernel, EXP_RUN_LEVELS at the most per launch"""
    edge = np.asarray(edge)
    T = edge.shape[0] // 2 + 1
    height = np.zeros(2 * T, dtype=np.int64)
    for p, c in edge[::-1]:                              # cladewise rows: a node's children come after it
        height[p] = max(height[p], height[c] + 1)
    return np.bincount(height[T + 1:2 * T])[1:].tolist()


EXP_RUN_BLOCK, EXP_RUN_LEVELS = 1024, 63                 # phm_exp.hip
DIC_SHAPES = ("complete4096", "ladder200")          # a height level of 2 048 nodes; 199 height levels


@functools.lru_cache(maxsize=None)
def dic_shape_problem(shape, n):
    """(z, Q, pid, Omega, prior, oracle variant) of the two tree shapes of the DIC pass, n = 2 (bf) or 4 (ks)"""
    import wavegroups
    if shape == "complete4096":
        edge, lens = wavegroups.complete_tree(12, seed=4096)
        lens = np.where(lens == 0.0, 0.3, lens)          # complete_tree zeroes one length for the simulation's sake
    else:
        edge, lens = ladder_edges(200, 200)
    if n == 2:
        Q, prior, variant = np.array([[-.1, .1], [.1, -.1]]), (.55, 1, .56, 1.01), O.BF
    else:
        Q, prior, variant = synth.make2sQ(.1, .1, .2, .2, 10), PRIOR, O.KS
    pid = np.full(n, 1.0 / n)
    # tips simulated at eight times the rates: neighbours differ often enough that log p(y | Q) of 4 096 tips lies far below
    # log(DBL_MIN), where a pass without scale factors has long underflowed
    states = synth.simulate_tips(edge, lens, 8.0 * Q, pid, 0xD1C + n)
    z = tree_from_edges(edge, lens, (states - 1) % 2 + 1)
    return z, Q, pid, 25.0, prior, variant


DIC_SHAPE_ITERS, DIC_SHAPE_SEED = 4, 5


@functools.lru_cache(maxsize=None)
def dic_shape_oracle(shape, n):
    z, Q, pid, Omega, prior, variant = dic_shape_problem(shape, n)
    nen, nodelist, root = orders(z)
    rows, rc = O.maketreelistMCMC(z, Q, pid, np.eye(n) + Q / Omega, Omega, nen, nodelist, root, DIC_SHAPE_ITERS, variant=variant,
                                  seed=DIC_SHAPE_SEED, prior=prior, dic=True)
    rows.setflags(write=False)
    return rows, rc


def scaled_loglik(z, Q, pid, masks):
    """log p(y | Q) by a Felsenstein pass with scipy's expm, every internal row divided by its sum and the logs of the sums added up
    (an unscaled pass underflows on thousands of tips); ``masks``: only the parity of the tip state is observed"""
    from scipy.linalg import expm
    Q = np.asarray(Q, dtype=np.float64)
    n, E = Q.shape[0], np.asarray(z["edge"])
    T = len(z["states"])
    nen, root = treeorder.pruningwiseedgeorder(z), treeorder.myreorder(z)
    PL = np.zeros((2 * T - 1, n))
    for i, s in enumerate(z["states"]):
        if masks:
            PL[i, (0 if s % 2 == 1 else 1)::2] = 1
        else:
            PL[i, s - 1] = 1
    P = expm(np.asarray(z["edge.length"])[:, None, None] * Q)          # one call for every branch
    S = 0.0
    for i in range(T - 1):
        ea, eb = nen[2 * i] - 1, nen[2 * i + 1] - 1
        row = (P[ea] @ PL[E[ea, 1] - 1]) * (P[eb] @ PL[E[eb, 1] - 1])
        S += np.log(row.sum())
        PL[E[ea, 0] - 1] = row / row.sum()
    return float(np.log(PL[root - 1] @ pid) + S)
