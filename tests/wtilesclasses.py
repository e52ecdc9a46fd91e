"""Inputs shared by the CPU and GPU tests of the state-count classes of the lane-per-replica sweep kernels for 5 to 64 states
(phm_wtiles.hip; DESIGN.md section 4c, "State-count classes"): the host's choice of kernel instantiation restated, the list of every
instantiation its launchers hold, and small problems chosen by the class they land in, with the oracle's runs of them (computed once
per session, shared, never written).  TEST INFRASTRUCTURE ONLY."""
import functools
import re

import numpy as np

import oracle_lib as O
import rateupdatecases as RC
from phylomap_amd import synth, treeorder

# the engine's constants (phm_wtiles.h, phm_rtc.h, wtiles_setup)
WT_FEW_TILES, RTC_SPARSE_NMAX, RTC_SPARSE_MAX_FILL, GROUP_WAVES, GROUP_MAX = 112, 32, 0.5, 65536, 8
MSPLIT_TILES = {2: 64, 3: 192, 4: 256}
VARIANTS = {"plain": O.PLAIN, "bigtree": O.BIGTREE, "sparse": O.SPARSE, "ks": O.KS}


def ceil_div(a, b):
    return -(-a // b)


def kname(kernel, *targs):
    """the name a kernel trace prints, without return type, namespace and arguments"""
    if not targs:
        return kernel
    return kernel + "<" + ", ".join(("true" if a else "false") if isinstance(a, bool) else str(a) for a in targs) + ">"


def plain_slot_class(B):
    """tiles mapping, n + n(n - 1) layout: the number of LDS transition slots (pairs a != c with B[a][c] != 0), 0 where the kernel
    counts in global memory (upload_model; RC.slot_class is the ks layout's count, self pairs included)"""
    n = B.shape[0]
    cnt = int(np.count_nonzero(B)) - int(np.count_nonzero(np.diag(B)))
    return cnt if (n <= 32 and cnt <= RC.WT_MAX_SLOTS) else 0


def slot_count(B, variant):
    return RC.slot_class(B) if variant == "ks" else plain_slot_class(B)


def chain_matrix(B, variant):
    """the matrix of the pruning pass: B, thresholded at 1e-7 by the SPARSE driver (build_model, matTospmat)"""
    return np.where(B > 1e-7, B, 0.0) if variant == "sparse" else B


def branch_group(tiles, n_edge, forced=0):
    """branches per wave of the branch kernel (wtiles_setup)"""
    return min(64, forced) if forced > 0 else max(1, min(GROUP_MAX, tiles * n_edge // GROUP_WAVES))


def dispatch(n, B, variant="bigtree", tiles=1, pruning_form=0, level_groups=0, deep=False, branch_group_opt=0, reduce=False,
             n_edge=0, sparse_chains=0):
    """The kernel instantiations one sweep of the tiles mapping launches at 5 to 64 states: launch_wtiles_sweep, launch_wtiles_up,
    launch_up_levels and launch_up_band (phm_wtiles.hip) under the band, slot and cluster rules of upload_model and wtiles_setup
    (phm_engine.cpp).  ``reduce`` changes what the branch kernel does (branch_paths) and not which kernel runs."""
    assert 5 <= n <= 64 and B.shape == (n, n)
    B = np.asarray(B)
    Bc = chain_matrix(B, variant)
    usable = lambda M: RC.band_class(M) if sparse_chains != 2 else 0
    band_up, band_draw = usable(Bc), usable(B)
    clusters = n <= 32 and (level_groups >= 2 or (level_groups == 0 and deep))
    mt, npad, out = ceil_div(n, 16), 4 * ceil_div(n, 4), set()
    # pruning pass
    generated = (not band_up and sparse_chains != 2 and n <= RTC_SPARSE_NMAX and np.count_nonzero(Bc) <= RTC_SPARSE_MAX_FILL * n * n)
    if generated:
        out.add("phm_sparse_up")                        # the kernel generated for the pattern (phm_rtc.cpp), a launch per level
    elif band_up:
        out.add(kname("wt_up_band_cluster_kernel" if clusters else "wt_up_band_kernel", npad, band_up))
    else:
        form = pruning_form & 3
        split = form == 2 or (form == 0 and (tiles < MSPLIT_TILES[mt] if mt >= 2 else tiles < WT_FEW_TILES))
        if mt >= 2 and split:
            out.add(kname("wt_up_msplit_kernel", mt))
        elif split:
            out.add(kname("wt_up_blocks_kernel", mt))
        elif mt >= 2 and form != 1:
            out.add(kname("wt_up2_kernel", mt, ceil_div(n, 4)))
        else:
            out.add(kname("wt_up_kernel", mt))
    # root and node draws
    out.add("wt_root_kernel")
    if clusters:
        out.add(kname("wt_down1r_cluster_kernel", npad))
    elif mt >= 3:
        out.add(kname("wt_down1_kernel", mt))
    else:
        out.add(kname("wt_down1r_kernel", npad))
    # branch paths
    small = n <= 32
    b2l = small or branch_group(tiles, n_edge, branch_group_opt) >= 4
    out.add(kname("wt_branch_kernel", variant == "ks", small, b2l, band_draw if small else 0))
    out.add("wt_stats_kernel")
    return frozenset(out)


def branch_paths(n, B, variant, reduce):
    """(LDS slots, red_pc, red_dw) of the branch kernel: where it counts transitions and adds dwell times (branch_lds)"""
    slots = slot_count(B, variant)
    return slots, bool(reduce) and slots == 0, bool(reduce) and n > 32


# ---------------------------------------------------------------------------------------------------------------------------
# Every instantiation the launchers of phm_wtiles.hip hold, written out by hand from the kernel file and not derived from
# ``dispatch``: (kernel, template arguments, smallest n, largest n)
# ---------------------------------------------------------------------------------------------------------------------------
_T, _F = True, False
_TABLE = (
    ("wt_root_kernel", (), 5, 64), ("wt_stats_kernel", (), 5, 64),
    # the matrix in registers: pruning_form 1; <1> also pruning_form 3 and from WT_FEW_TILES tiles on
    ("wt_up_kernel", (1,), 5, 16), ("wt_up_kernel", (2,), 17, 32), ("wt_up_kernel", (3,), 33, 48),
    ("wt_up_kernel", (4,), 49, 64),
    # few tiles: a wave per 16-replica block (n <= 16), a workgroup of MT waves per block (n >= 17)
    ("wt_up_blocks_kernel", (1,), 5, 16), ("wt_up_msplit_kernel", (2,), 17, 32),
    ("wt_up_msplit_kernel", (3,), 33, 48), ("wt_up_msplit_kernel", (4,), 49, 64),
    # the matrix in LDS, <MT, KSU = ceil(n / 4)>: twelve schedules of MT * KSU fragments in chunks of eight
    ("wt_up2_kernel", (2, 5), 17, 20), ("wt_up2_kernel", (2, 6), 21, 24), ("wt_up2_kernel", (2, 7), 25, 28),
    ("wt_up2_kernel", (2, 8), 29, 32), ("wt_up2_kernel", (3, 9), 33, 36), ("wt_up2_kernel", (3, 10), 37, 40),
    ("wt_up2_kernel", (3, 11), 41, 44), ("wt_up2_kernel", (3, 12), 45, 48), ("wt_up2_kernel", (4, 13), 49, 52),
    ("wt_up2_kernel", (4, 14), 53, 56), ("wt_up2_kernel", (4, 15), 57, 60), ("wt_up2_kernel", (4, 16), 61, 64),
    # banded chain matrix <NP, HB>, a launch per level; the host wants 2 HB + 1 < n
    ("wt_up_band_kernel", (8, 1), 5, 8), ("wt_up_band_kernel", (8, 2), 6, 8),
    ("wt_up_band_kernel", (12, 1), 9, 12), ("wt_up_band_kernel", (12, 2), 9, 12),
    ("wt_up_band_kernel", (16, 1), 13, 16), ("wt_up_band_kernel", (16, 2), 13, 16),
    ("wt_up_band_kernel", (20, 1), 17, 20), ("wt_up_band_kernel", (20, 2), 17, 20),
    ("wt_up_band_kernel", (24, 1), 21, 24), ("wt_up_band_kernel", (24, 2), 21, 24),
    ("wt_up_band_kernel", (28, 1), 25, 28), ("wt_up_band_kernel", (28, 2), 25, 28),
    ("wt_up_band_kernel", (32, 1), 29, 32), ("wt_up_band_kernel", (32, 2), 29, 32),
    # the same over subtree clusters (a deep tree, or level_groups >= 2)
    ("wt_up_band_cluster_kernel", (8, 1), 5, 8), ("wt_up_band_cluster_kernel", (8, 2), 6, 8),
    ("wt_up_band_cluster_kernel", (12, 1), 9, 12), ("wt_up_band_cluster_kernel", (12, 2), 9, 12),
    ("wt_up_band_cluster_kernel", (16, 1), 13, 16), ("wt_up_band_cluster_kernel", (16, 2), 13, 16),
    ("wt_up_band_cluster_kernel", (20, 1), 17, 20), ("wt_up_band_cluster_kernel", (20, 2), 17, 20),
    ("wt_up_band_cluster_kernel", (24, 1), 21, 24), ("wt_up_band_cluster_kernel", (24, 2), 21, 24),
    ("wt_up_band_cluster_kernel", (28, 1), 25, 28), ("wt_up_band_cluster_kernel", (28, 2), 25, 28),
    ("wt_up_band_cluster_kernel", (32, 1), 29, 32), ("wt_up_band_cluster_kernel", (32, 2), 29, 32),
    # node draws <NP> per level and over clusters (n <= 32), <MT> in one pass beyond
    ("wt_down1r_kernel", (8,), 5, 8), ("wt_down1r_kernel", (12,), 9, 12), ("wt_down1r_kernel", (16,), 13, 16),
    ("wt_down1r_kernel", (20,), 17, 20), ("wt_down1r_kernel", (24,), 21, 24), ("wt_down1r_kernel", (28,), 25, 28),
    ("wt_down1r_kernel", (32,), 29, 32),
    ("wt_down1r_cluster_kernel", (8,), 5, 8), ("wt_down1r_cluster_kernel", (12,), 9, 12),
    ("wt_down1r_cluster_kernel", (16,), 13, 16), ("wt_down1r_cluster_kernel", (20,), 17, 20),
    ("wt_down1r_cluster_kernel", (24,), 21, 24), ("wt_down1r_cluster_kernel", (28,), 25, 28),
    ("wt_down1r_cluster_kernel", (32,), 29, 32),
    ("wt_down1_kernel", (3,), 33, 48), ("wt_down1_kernel", (4,), 49, 64),
    # branch paths <KS, SMALL, B2L, BAND>
    ("wt_branch_kernel", (_F, _T, _T, 0), 5, 32), ("wt_branch_kernel", (_F, _T, _T, 1), 5, 32),
    ("wt_branch_kernel", (_F, _T, _T, 2), 6, 32), ("wt_branch_kernel", (_F, _F, _F, 0), 33, 64),
    ("wt_branch_kernel", (_F, _F, _T, 0), 33, 64),
    ("wt_branch_kernel", (_T, _T, _T, 0), 5, 32), ("wt_branch_kernel", (_T, _T, _T, 1), 5, 32),
    ("wt_branch_kernel", (_T, _T, _T, 2), 6, 32), ("wt_branch_kernel", (_T, _F, _F, 0), 33, 64),
    ("wt_branch_kernel", (_T, _F, _T, 0), 33, 64),
)
ALL_CLASSES = {kname(k, *targs): range(lo, hi + 1) for k, targs, lo, hi in _TABLE}
assert len(ALL_CLASSES) == len(_TABLE)
REACHABLE = frozenset(ALL_CLASSES)                                              # the launchers name no kernel they cannot launch

_TRACE_NAME = re.compile(r"\b(wt_[a-z0-9_]+_kernel)\s*(<[^>]*>)?")


def trace_names(text):
    """the kernels of phm_wtiles.hip named in a kernel trace's statistics, in ``kname``'s spelling"""
    out = set()
    for k, targs in _TRACE_NAME.findall(text):
        out.add(k + ("<" + ", ".join(a.strip() for a in targs[1:-1].split(",")) + ">" if targs else ""))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
DENSE_NS = tuple(n for k in range(2, 17) for n in (4 * k - 3, 4 * k))          # bottom and top of every class of ceil(n / 4)
DENSE_PLAIN_NS = (9, 25, 41, 49, 53, 57)                                       # bottoms that also run without normalisation
BAND_CLASSES = tuple((npad, hb) for npad in range(8, 33, 4) for hb in (1, 2))
B2L_CASES = (("bigtree", 33), ("bigtree", 49), ("bigtree", 64), ("ks", 34), ("ks", 64))
SLOT_CASES = ((10, 0), (11, 0), (25, 2), (26, 2))                              # (n, band): 90 | 110 and 94 | 98 pairs around 96
REPLICAS_3_TILES = (0, 15, 16, 63, 64, 129, 149)
REPLICAS_2_TILES = (0, 63, 64, 69)


def dense_forms(n):
    return (0, 1, 2, 3) if n >= 17 else (0, 1, 2)


def band_ns(npad, hb):
    """the smallest and the largest n of the class that the host rule accepts (2 hb + 1 < n)"""
    return max(npad - 3, 2 * hb + 2), npad


def banded_Q(n, hb, seed, lo=0.02, hi=0.3, hole=False):
    Q = synth.dense_Q(n, lo, hi, seed=seed)
    idx = np.arange(n)
    Q[np.abs(idx[:, None] - idx[None, :]) > hb] = 0.0
    if hole:
        Q[3, 4] = 0.0                                   # a zero inside the band: the band kernels multiply by it, the slots skip it
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(1))
    return Q


def skew_pid(n, seed):
    pid = np.random.default_rng(seed).dirichlet(np.full(n, 4.0))
    return pid / pid.sum()


def spread_tips(T, n, seed):
    """tip states (1-based) that hold both ends of the state space: every third tip in state 1, every third in state n, the others
    uniform -- under a banded B a path between the ends passes the states between them, so no state is left unvisited"""
    s = np.random.default_rng(seed).integers(1, n + 1, T)
    s[0::3], s[1::3] = 1, n
    return s.astype(np.int32)


def orders(z):
    return treeorder.pruningwiseedgeorder(z), treeorder.makenodelist(z), treeorder.myreorder(z)


def ladder_tree(T, mean_len, states, init_segments):
    """the caterpillar of tests/test_gpu_level_groups.py: internal node k hangs tip k and node k + 1, exponential lengths"""
    rs = np.random.default_rng(5)
    edges = []
    for k in range(T - 1):
        node = T + 1 + k
        edges.append((node, k + 1))
        edges.append((node, node + 1) if k < T - 2 else (node, T))
    edge = np.asarray(edges, dtype=np.int32)
    lens = rs.exponential(mean_len, size=edge.shape[0])
    maps, mapnames = [], []
    for r in range(edge.shape[0]):
        child = int(edge[r, 1])
        m, mn = synth.initial_path(lens[r], int(states[child - 1]) if child <= T else 1, init_segments)
        maps.append(m)
        mapnames.append(mn)
    return {"edge": edge, "Nnode": T - 1, "edge.length": lens, "states": states, "maps": maps, "mapnames": mapnames}


class Case:
    """One problem: model, tree, run lengths, the replicas compared with the oracle, what it is there for, and the dispatch
    inputs of each engine run the GPU test makes of it (``runs``: keyword sets for wtilesclasses.dispatch / _lib.Engine)"""

    def __init__(self, name, purpose, Q, pid, z, variant, N, S, seed, replicas, runs, deep=False):
        self.name, self.purpose, self.Q, self.pid, self.z, self.variant = name, purpose, Q, pid, z, variant
        self.N, self.S, self.seed, self.replicas, self.runs, self.deep = N, S, seed, replicas, runs, deep
        self.n = Q.shape[0]
        self.Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
        self.B = np.eye(self.n) + Q / self.Omega
        self.nen, self.nodelist, self.root = orders(z)
        self.tiles, self.n_edge = ceil_div(S, 64), len(z["edge"])
        self.length = float(np.sum(z["edge.length"]))
        self.ks = variant == "ks"
        self.ncnt = self.n * self.n if self.ks else self.n * (self.n - 1)
        for a in (self.Q, self.pid, self.B):
            a.setflags(write=False)

    def kernels(self, run):
        """the restated dispatch's answer for one of the case's engine runs"""
        return dispatch(self.n, self.B, self.variant, self.tiles, run.get("pruning_form", 0), run.get("level_groups", 0), self.deep,
                        run.get("branch_group", 0), run.get("reduce", False), self.n_edge, run.get("sparse_chains", 0))

    def oracle(self, replica, dump=False, N=None):
        return O.maketreelistMCMC(self.z, self.Q, self.pid, self.B, self.Omega, self.nen, self.nodelist, self.root,
                                  self.N if N is None else N, variant=VARIANTS[self.variant], seed=self.seed, replica=replica, dump=dump)


def _omega(Q):
    return 1.25 * float(np.max(np.abs(np.diag(Q))))


@functools.lru_cache(maxsize=None)
def dense_case(n, variant="bigtree"):
    Q = synth.dense_Q(n, 0.02, 0.08, seed=n)
    pid = np.full(n, 1.0 / n)
    z = synth.make_tree(11, Q, _omega(Q), 700 + n, pid, init_segments=3)
    runs = tuple({"pruning_form": f} for f in (dense_forms(n) if variant == "bigtree" else (0,)))
    return Case(f"dense{n}{'' if variant == 'bigtree' else '_plain'}", f"dense n = {n}: ceil(n / 4) = {ceil_div(n, 4)}, n mod 4 = {n % 4}",
                Q, pid, z, variant, 6, 150, 77, REPLICAS_3_TILES, runs)


@functools.lru_cache(maxsize=None)
def band_case(n, hb, tree):
    """``tree``: "random" (12 tips, a launch per level) or "ladder" (300 tips: subtree clusters forced, chosen and switched off)"""
    Q = banded_Q(n, hb, seed=n, hole=hb == 1)
    pid = skew_pid(n, 100 * n + hb)
    if tree == "random":
        z = synth.make_tree(12, Q, _omega(Q), 800 + n + hb, pid, states=spread_tips(12, n, n + hb), init_segments=n)
        return Case(f"band{hb}_n{n}_random", f"NP = {4 * ceil_div(n, 4)}, HB = {hb}, a launch per level", Q, pid, z, "bigtree", 6, 70, 55,
                    REPLICAS_2_TILES, ({"level_groups": 1},))
    z = ladder_tree(LADDER_TIPS, 2.0 / _omega(Q), spread_tips(LADDER_TIPS, n, n + hb), init_segments=n)
    return Case(f"band{hb}_n{n}_ladder", f"NP = {4 * ceil_div(n, 4)}, HB = {hb}, subtree clusters", Q, pid, z, "bigtree", 4, 70, 19,
                REPLICAS_2_TILES, ({"level_groups": 1}, {"level_groups": 2}, {"level_groups": 0}), deep=True)


LADDER_TIPS = 300

_GROUP_RUNS = tuple({"branch_group": g, "reduce": r} for g in (1, 4) for r in (False, True))


@functools.lru_cache(maxsize=None)
def b2l_case(variant, n):
    pid = np.full(n, 1.0 / n)
    if variant == "ks":
        Q = RC.hidden_rates_Q(n)
        z = RC.parity_tips(synth.make_tree(14, Q, _omega(Q), 900 + n, pid))
    else:
        Q = synth.dense_Q(n, 0.02, 0.08, seed=n)
        z = synth.make_tree(14, Q, _omega(Q), 900 + n, pid, init_segments=3)
    return Case(f"b2l_{variant}{n}", f"n = {n} > 32, {variant}: rows of B in LDS (four branches per wave) against one branch per wave",
                Q, pid, z, variant, 6, 70, 41, REPLICAS_2_TILES, _GROUP_RUNS)


@functools.lru_cache(maxsize=None)
def slot_case(n, hb):
    if hb:
        Q = banded_Q(n, hb, seed=n)
        pid = skew_pid(n, 100 * n + hb)
        z = synth.make_tree(12, Q, _omega(Q), 800 + n + hb, pid, states=spread_tips(12, n, n + hb), init_segments=n)
    else:
        Q = synth.dense_Q(n, 0.02, 0.08, seed=n)
        pid = np.full(n, 1.0 / n)
        z = synth.make_tree(12, Q, _omega(Q), 800 + n, pid, init_segments=3)
    return Case(f"slots_n{n}_hb{hb}", f"n = {n}, band {hb}: either side of {RC.WT_MAX_SLOTS} LDS counting slots", Q, pid, z, "bigtree", 6, 70,
                23, REPLICAS_2_TILES, ({"reduce": False}, {"reduce": True}))


KS_SMALL_CASES = (("band2", 12), ("band1", 8), ("dense", 12))


@functools.lru_cache(maxsize=None)
def ks_small_case(kind, n):
    """The fixed-Q ks sweep at n <= 32, the three branch kernels no other case of this file reaches: a hidden-rates Q (band 2), one
    with every regime-switching rate zero (band 1), and the first with the band kernels switched off (sparse_chains = 2)"""
    Q = RC.hidden_rates_Q(n, widen=kind == "band1")
    pid = np.full(n, 1.0 / n)
    z = RC.parity_tips(synth.make_tree(14, Q, _omega(Q), 900 + n, pid))
    runs = tuple({"reduce": r, **({"sparse_chains": 2} if kind == "dense" else {})} for r in (False, True))
    return Case(f"ks_{kind}_n{n}", f"ks sweep at n = {n} <= 32, {kind}: self pairs counted, tips re-drawn", Q, pid, z, "ks", 6, 70, 37,
                REPLICAS_2_TILES, runs)


def ks_small_cases():
    return [ks_small_case(k, n) for k, n in KS_SMALL_CASES]


KS_FORM_NS = (12, 34)


@functools.lru_cache(maxsize=None)
def ks_form_case(n):
    """The ks sweep's tip rows (the parity-mask rows of the chain table) under every pruning form: the problems of
    ks_small_case("dense", 12) and b2l_case("ks", 34), the smallest n that reach a one-row-block and a three-row-block kernel of each
    form with mask tips"""
    Q = RC.hidden_rates_Q(n)
    pid = np.full(n, 1.0 / n)
    z = RC.parity_tips(synth.make_tree(14, Q, _omega(Q), 900 + n, pid))
    dense = {"sparse_chains": 2} if n <= 32 else {}
    runs = tuple({"pruning_form": f, **dense} for f in dense_forms(n))
    return Case(f"ks_forms_n{n}", f"ks sweep at n = {n}: mask tip rows in every pruning form", Q, pid, z, "ks", 6, 70, 37 if n <= 32 else 41,
                REPLICAS_2_TILES, runs)


def ks_form_cases():
    return [ks_form_case(n) for n in KS_FORM_NS]


def dense_cases():
    return [dense_case(n) for n in DENSE_NS] + [dense_case(n, "plain") for n in DENSE_PLAIN_NS]


def band_cases():
    return [band_case(n, hb, tree) for npad, hb in BAND_CLASSES for n in band_ns(npad, hb) for tree in ("random", "ladder")]


def b2l_cases():
    return [b2l_case(v, n) for v, n in B2L_CASES]


def slot_cases():
    return [slot_case(n, hb) for n, hb in SLOT_CASES]


def all_cases():
    return dense_cases() + band_cases() + b2l_cases() + slot_cases() + ks_small_cases() + ks_form_cases()


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle's runs
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_rows(case, replica):
    """(rows [N, cols], rc) of one replica"""
    rows, rc = case.oracle(replica)
    rows.setflags(write=False)
    return rows, rc


@functools.lru_cache(maxsize=None)
def oracle_dump(case, replica):
    """(rc, dump) after the last sweep"""
    _, rc, dump = case.oracle(replica, dump=True)
    return rc, dump


@functools.lru_cache(maxsize=None)
def oracle_walk(case, replica):
    """(largest segment count of a branch, the set of 0-based states a forward draw of a branch started from) over the chain
    states after each of the case's sweeps: the dump shows the state after the last sweep, so one run of i sweeps for every i.
    A segment that is not the last of its branch is the previous state of the draw that made the next one."""
    longest, parents = 0, set()
    for i in range(1, case.N + 1):
        _, rc, dump = case.oracle(replica, dump=True, N=i)
        assert rc == 0
        longest = max(longest, int(dump.seg_count.max()))
        for b, m in enumerate(dump.seg_count):
            parents.update(dump.seg_state[b, :m - 1].tolist())          # 0-based in the dump
    return longest, frozenset(parents)
