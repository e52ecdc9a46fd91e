"""Inputs shared by the CPU and GPU tests of the two other mappings of the 5 to 64 state sweep: "replicas" (phm_wide.hip: one wave
per tile, the replicas of the tile taking turns at the n-vector work) and "branches" (phm_wbranch.hip: one wave per (replica,
branch), level launches or transition maps for the tree passes).  The host's decisions for the two restated from phm_engine.cpp
and the launchers, the constants read from the headers, and small problems chosen by the path they reach, with the oracle's runs
of them (computed once per session, shared, never written).  DESIGN.md section 4c, "Classes of the replica and branch mappings".
TEST INFRASTRUCTURE ONLY."""
import functools
import os
import re

import numpy as np

import mcmcmapsclasses as M
import oracle_lib as O
import rateupdatecases as RC
import sparsepatterns as SP
import wtilesclasses as W
from phylomap_amd import _lib, synth

_CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")


def _source(name):
    with open(os.path.join(_CSRC, name)) as f:
        return f.read()


def _found(name, pattern, text):
    """the integer a source line holds: only code tokens are matched (any spacing, no comments); a miss names the constant"""
    m = re.search(pattern, text)
    if m is None:
        raise RuntimeError(f"widemapclasses: the source no longer holds {name} in the form /{pattern}/; restate the rule here")
    return int(m.group(1))


_WIDE_H, _WIDE_HIP, _WB_H, _WB_HIP, _ENGINE = (_source(f) for f in ("phm_wide.h", "phm_wide.hip", "phm_wbranch.h", "phm_wbranch.hip", "phm_engine.cpp"))
WIDE_BLOCK, WIDE_MAXSEG, WIDE_MAXSEG_BIG_N = (_found(k, rf"constexpr\s+int\s+{k}\s*=\s*(\d+)\s*;", _WIDE_H) for k in ("WIDE_BLOCK", "WIDE_MAXSEG", "WIDE_MAXSEG_BIG_N"))
WB_ELL_MAX, WB_BLOCK = (_found(k, rf"constexpr\s+int\s+{k}\s*=\s*(\d+)\s*;", _WB_H) for k in ("WB_ELL_MAX", "WB_BLOCK"))
WB_MERGED_LDS = _found("WB_MERGED_LDS", r"constexpr\s+int\s+WB_MERGED_LDS\s*=\s*(\d+)\s*;", _WB_HIP)
WB_FLUSH = _found("the notes per flush", r"\+\+n_tr\s*==\s*(\d+)\s*\)\s*flush_transitions\(\)", _WB_HIP)
WB_VARIATES = _found("the variates per refill", r"edraw\s*-\s*gen_base\s*>=\s*(\d+)u", _WB_HIP)
WB_B2_LDS_WAVES = _found("the S * E up to which B2 is staged", r"S\s*\*\s*p\.n_edge\s*<=\s*(\d+)\s*\)", _WB_HIP)
WB_WALK_LDS_NODES = _found("the nodes of the walk's LDS copy", r"use_lds\s*=\s*p\.n_node\s*<=\s*(\d+)\s*\*\s*1024\s*;", _WB_HIP) * 1024
WB_DMAP_BYTES = _found("the transition-map limit", r"S\s*\*\s*E\s*\*\s*n\s*<=\s*\(\s*(\d+)u\s*<<\s*20\s*\)", _ENGINE) << 20
WIDE_TARGET_TILES = _found("the tile target of rep_stride", r"\(\s*rpt\s*/\s*2\s*\)\s*<=\s*(\d+)\s*\)\s*rpt\s*/=\s*2\s*;", _ENGINE)
WIDE_LDS_DEFAULT = _found("the LDS default of launch_mcmc_wide", r"if\s*\(\s*lds\s*>\s*(\d+)\s*\*\s*1024\s*\)", _WIDE_HIP) * 1024
WB_LDS_DEFAULT = _found("the LDS default of launch_wbranch_sweep", r"if\s*\(\s*lds\s*>\s*(\d+)\s*\*\s*1024\s*\)", _WB_HIP) * 1024
SPARSE_THRESHOLD = SP.SPARSE_THRESHOLD
_STATUS = {name: code for code, name in _lib.STATUS.items()}
ST_UNSUPPORTED, ST_CAPACITY = _STATUS["PHM_ERR_UNSUPPORTED"], _STATUS["PHM_ERR_CAPACITY"]

ceil_div = W.ceil_div


# ---------------------------------------------------------------------------------------------------------------------------
# the host's decisions, restated
# ---------------------------------------------------------------------------------------------------------------------------
def rep_stride(S):
    """replicas per tile of the replica mapping, one tree (replicas_setup): halved while the tiles stay at or below 8 192; the
    step back up when the padded layout would not fit a quarter of the free memory is left out"""
    rpt = 64
    while rpt > 1 and ceil_div(S, rpt // 2) <= WIDE_TARGET_TILES:
        rpt //= 2
    return rpt


def wide_maxseg(n):
    return WIDE_MAXSEG_BIG_N if n > 40 else WIDE_MAXSEG


def model_lds_bytes(n, sparse):
    return 8 * ((2 if sparse else 1) * n * (n | 1) + n)


def wide_lds_bytes(n, sparse):
    return model_lds_bytes(n, sparse) + (WIDE_BLOCK // 64) * wide_maxseg(n) * 64


def wbranch_lds_bytes(n, sparse):
    return model_lds_bytes(n, sparse)


def ell_width(Mx):
    """ELLPACK width of a matrix on the branch mapping (upload_model), 0 for dense rows"""
    n, w = Mx.shape[0], int(np.count_nonzero(Mx, axis=1).max())
    return w if (1 <= w <= WB_ELL_MAX and 3 * w <= n) else 0


def chain_matrix(B, sparse):
    return np.where(B > SPARSE_THRESHOLD, B, 0.0) if sparse else B


def band_hb(Bc, sparse_chains=0):
    """half-bandwidth the pruning kernels of the branch mapping shift over, 0 where they walk ELLPACK or dense rows"""
    hb = RC.half_bandwidth(Bc)
    return hb if (ell_width(Bc) > 0 and 1 <= hb <= 2 and sparse_chains != 2) else 0


def branch_classes(B, sparse, sparse_chains=0):
    """(ell_w, ell2_w, band_hb) of a model on the branch mapping"""
    Bc = chain_matrix(B, sparse)
    return ell_width(Bc), ell_width(B), band_hb(Bc, sparse_chains)


def b2_in_lds(S, E, ell2_w):
    return ell2_w == 0 and S * E <= WB_B2_LDS_WAVES


def uses_dmap(S, E, n):
    """transition maps and one walk per chain; otherwise wb_root_kernel and a wb_down_kernel launch per depth level"""
    return S * E * n <= WB_DMAP_BYTES


def walk_uses_lds(n_internal):
    return n_internal <= WB_WALK_LDS_NODES


def height_level_sizes(z):
    """internal nodes per height level (phm_sched.cpp, height_levels): a node is one above its higher child, tips at 0"""
    edge = np.asarray(z["edge"])
    T = len(z["states"])
    kids = {}
    for p, c in edge:
        kids.setdefault(int(p), []).append(int(c))
    height = {}
    stack = [T + 1]
    while stack:
        v = stack[-1]
        todo = [c for c in kids[v] if c > T and c not in height]
        if todo:
            stack.extend(todo)
            continue
        stack.pop()
        height[v] = 1 + max((height[c] if c > T else 0) for c in kids[v])
    return np.bincount(np.array(list(height.values())))[1:]


def pruning_launches(sizes, dense):
    """launch_wbranch_sweep: [(first level, end level, "run" | "level")] -- at least two consecutive levels of at most four nodes
    (dense rows: 512 lanes, two waves a node) or eight (ELLPACK: 1 024 lanes) go into one wb_up_run_kernel launch"""
    lim = (512 if dense else 1024) // 128
    out, l, L = [], 0, len(sizes)
    while l < L:
        if sizes[l] <= lim and l + 1 < L and sizes[l + 1] <= lim:
            l1 = l
            while l1 < L and sizes[l1] <= lim:
                l1 += 1
            out.append((l, l1, "run"))
            l = l1
        else:
            out.append((l, l + 1, "level"))
            l += 1
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
_ENGINE_VARIANT = {"plain": _lib.PHM_MCMC, "bigtree": _lib.PHM_MCMC_BIGTREE, "sparse": _lib.PHM_MCMC_SPARSE, "ks": _lib.PHM_MCMC_KS}


class Case(W.Case):
    """A wtilesclasses.Case on one of the two mappings: ``opts`` are engine options that change the arithmetic (rescale) and the
    oracle follows them"""

    def __init__(self, name, purpose, Q, pid, z, variant, N, S, seed, replicas, mapping, rescale=False):
        super().__init__(name, purpose, Q, pid, z, variant, N, S, seed, tuple(sorted(set(replicas))), ())
        self.mapping, self.rescale = mapping, rescale
        self.sparse = variant == "sparse"
        self.E, self.T = self.n_edge, len(z["states"])
        self.cols = _lib.stat_cols(self.n, "ks" if self.ks else "plain")

    def classes(self, sparse_chains=0):
        return branch_classes(self.B, self.sparse, sparse_chains)

    def engine(self, S=None, mapping=None, **opt):
        if self.rescale:
            opt["rescale"] = True
        return _lib.Engine(self.z, self.Q, self.pid, self.Omega, self.N, variant=_ENGINE_VARIANT[self.variant], seed=self.seed,
                           n_replicas=self.S if S is None else S, mapping=self.mapping if mapping is None else mapping, **opt)

    def oracle(self, replica, dump=False, N=None, states=None):
        z = self.z if states is None else dict(self.z, states=states)
        v = W.VARIANTS[self.variant] | (O.FORCE_NORMALISE if self.rescale else 0)
        return O.maketreelistMCMC(z, self.Q, self.pid, self.B, self.Omega, self.nen, self.nodelist, self.root, self.N if N is None else N,
                                  variant=v, seed=self.seed, replica=replica, dump=dump)


oracle_rows, oracle_dump = W.oracle_rows, W.oracle_dump


@functools.lru_cache(maxsize=None)
def oracle_rows_on(case, replica, states_key):
    """(rows, rc) of one replica on tip states of its own (``states_key``: the bytes of an int32 vector)"""
    rows, rc = case.oracle(replica, states=np.frombuffer(states_key, dtype=np.int32))
    rows.setflags(write=False)
    return rows, rc


def _uniform(n):
    return np.full(n, 1.0 / n)


# ---- A. several replicas in a wave of the replica mapping -------------------------------------------------------------
MULTI_NS = (5, 20)
MULTI_S = (8193, 16385, 131073, 262145)                     # stride 2 (last tile holds one), 4, 32, 64 (last tile holds one)
MULTI_S_EXTRA = (8193, 262145)                              # per-site tips, reduced output, ks layout, chain dump
MULTI_STRIDE = {8192: 1, 8193: 2, 16385: 4, 131073: 32, 262145: 64}
MULTI_TIPS, MULTI_SWEEPS = 8, 3


def middle_replica(S):
    """a replica in the middle of the run that is not lane 0 of its tile"""
    st = rep_stride(S)
    return (S // 2 // st) * st + max(1, st * 37 // 64)


def multi_replicas(S):
    st = rep_stride(S)
    return tuple(sorted({0, 1, st - 1, st, middle_replica(S), S - 2, S - 1}))


@functools.lru_cache(maxsize=None)
def _multi_model(n, ks):
    if ks:
        Q = RC.hidden_rates_Q(n)
        z = RC.parity_tips(synth.make_tree(MULTI_TIPS, Q, W._omega(Q), 600 + n, _uniform(n)))
    else:
        Q = synth.dense_Q(n, 0.02, 0.08, seed=n)
        z = synth.make_tree(MULTI_TIPS, Q, W._omega(Q), 600 + n, _uniform(n), init_segments=3)
    return Q, z


@functools.lru_cache(maxsize=None)
def multi_case(n, S, ks=False):
    Q, z = _multi_model(n, ks)
    st = rep_stride(S)
    return Case(f"multi_{'ks' if ks else 'n'}{n}_S{S}", f"n = {n}, {S} replicas: {st} replicas take turns in a wave, the last tile holds "
                f"{S - (ceil_div(S, st) - 1) * st}", Q, _uniform(n), z, "ks" if ks else "bigtree", MULTI_SWEEPS, S, 91, multi_replicas(S), "replicas")


def multi_sites(case):
    """[S, tips] tip states of the per-site runs: replica r's tips are a function of r alone"""
    r = np.arange(case.S, dtype=np.int64)[:, None]
    t = np.arange(case.T, dtype=np.int64)[None, :]
    return ((r * 7 + t * 3 + (r // 5) * t) % case.n + 1).astype(np.int32)


LIST_N, LIST_TREES, LIST_S, LIST_SWEEPS = 12, 3, 5, 4


@functools.lru_cache(maxsize=None)
def list_problem():
    """three 10-tip trees under one dense 12-state model, five replicas a tree: the list engine's tiles (stride 64)"""
    Q = synth.dense_Q(LIST_N, 0.02, 0.08, seed=LIST_N)
    Omega = W._omega(Q)
    return Q, _uniform(LIST_N), Omega, synth.make_treelist(LIST_TREES, 10, Q, Omega, 612, _uniform(LIST_N), init_segments=3)


# ---- B. state-count and LDS edges, both mappings --------------------------------------------------------------------
EDGE_DENSE_NS = (5, 44, 45, 63, 64)
EDGE_SPARSE_NS = (31, 32, 55, 56, 64)
EDGE_S = {"branches": 3, "replicas": 70}


@functools.lru_cache(maxsize=None)
def _edge_tree(n):
    """the first 11-tip tree of the seeds 700 + n, 1700 + n, ... with five cherries: its lowest level is too wide for a run, so
    the pruning pass of the branch mapping launches both wb_up_kernel and wb_up_run_kernel<512, true>"""
    Q = synth.dense_Q(n, 0.02, 0.08, seed=n)
    for k in range(400):
        z = synth.make_tree(11, Q, W._omega(Q), 700 + n + 1000 * k, _uniform(n), init_segments=3)
        if {kind for _, _, kind in pruning_launches(height_level_sizes(z), dense=True)} == {"run", "level"}:
            return Q, z
    raise AssertionError(n)


@functools.lru_cache(maxsize=None)
def edge_case(n, variant, mapping):
    Q, z = _edge_tree(n)
    S = EDGE_S[mapping]
    return Case(f"edge_{variant}{n}_{mapping}", f"n = {n}, {variant}, dense rows: {64 - n} clamped lanes, "
                f"{wide_lds_bytes(n, variant == 'sparse') if mapping == 'replicas' else wbranch_lds_bytes(n, variant == 'sparse')} bytes of LDS",
                Q, _uniform(n), z, variant, 6, S, 77, (0, S - 1), mapping)


def edge_cases():
    return [edge_case(n, v, m) for m in ("branches", "replicas") for v, ns in (("bigtree", EDGE_DENSE_NS), ("sparse", EDGE_SPARSE_NS))
            for n in ns]


# ---- C. the ELLPACK rule, and chain matrices the threshold changes ---------------------------------------------------
ELL_PAIRS = ((6, 2), (5, 2), (12, 4), (11, 4), (48, 16), (47, 16), (64, 16), (64, 17))     # (n, w): ELLPACK | dense, pair by pair


def scattered_Q(n, w, seed, tiny=0, lo=0.02, hi=0.3):
    """Unbanded and asymmetric: per row the diagonal, the ring edge to the next state of a random relabelling and w - 2 further
    columns drawn at random -- w non-zeros in every row of B but one, which is left one short (from w = 3 on: at w = 2 the short
    row would be an absorbing state).  ``tiny``: that many more columns per row with rates U(1e-10, 1e-9) Omega-free, below the
    SPARSE driver's threshold."""
    rs = np.random.default_rng(seed)
    perm = rs.permutation(n)
    nxt = np.empty(n, dtype=np.int64)
    nxt[perm] = np.roll(perm, -1)
    Q = np.zeros((n, n))
    short = int(perm[n // 2]) if w >= 3 else -1
    for i in range(n):
        others = np.array([j for j in range(n) if j != i and j != nxt[i]])
        extra = rs.permutation(others)
        k = w - 2 - (1 if i == short else 0)
        cols = [int(nxt[i])] + [int(j) for j in extra[:k]]
        Q[i, cols] = rs.uniform(lo, hi, len(cols))
        if tiny:
            Q[i, extra[k:k + tiny]] = rs.uniform(1e-10, 1e-9, tiny)
    np.fill_diagonal(Q, -Q.sum(1))
    return Q


C_S, C_SWEEPS = 3, 8


def _c_tree(Q, seed, tips=11):
    n = Q.shape[0]
    return synth.make_tree(tips, Q, W._omega(Q), seed, _uniform(n), init_segments=n)


@functools.lru_cache(maxsize=None)
def ell_case(n, w, mapping="branches"):
    Q = scattered_Q(n, w, 1000 * n + w)
    return Case(f"ell_n{n}_w{w}_{mapping}", f"n = {n}, {w} non-zeros a row, unbanded: {'ELLPACK' if ell_width(np.eye(n) + Q) else 'dense'} rows",
                Q, _uniform(n), _c_tree(Q, 1100 + n + w), "bigtree", C_SWEEPS, C_S, 29, range(C_S), mapping)


@functools.lru_cache(maxsize=None)
def band16_case():
    Q = W.banded_Q(16, 2, seed=16)
    pid = W.skew_pid(16, 1602)
    z = synth.make_tree(12, Q, W._omega(Q), 818, pid, states=W.spread_tips(12, 16, 18), init_segments=16)
    return Case("band2_n16_branches", "half-bandwidth 2 at 16 states: wave shifts, and ELLPACK rows under sparse_chains = 2", Q, pid, z, "bigtree",
                C_SWEEPS, C_S, 55, range(C_S), "branches")


def _under_Q(n, seed):
    """tridiagonal rates over a floor of 2e-8 Omega everywhere else: B2 dense, Bc of half-bandwidth 1"""
    Q = W.banded_Q(n, 1, seed=seed)
    om = W._omega(Q)
    off = ~np.eye(n, dtype=bool) & (Q == 0.0)
    Q = Q.copy()
    Q[off] = 2e-8 * om
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(1))
    return Q


THRESHOLD_MODELS = ("corner12", "corner36", "under12", "under36", "tiny10", "ell6over4")


@functools.lru_cache(maxsize=None)
def threshold_case(model, rescale, mapping="branches"):
    """SPARSE with a chain matrix the threshold really changes.  corner: mcmcmapsclasses.sparse_case (tridiagonal Bc, B2 with the
    far corner); under: tridiagonal Bc under a dense B2; tiny10: sparsepatterns' dense B over a scattered Bc; ell6over4: B2 of
    ELLPACK width 6 over a Bc of width 4 at 24 states"""
    if model.startswith("corner"):
        c = M.sparse_case(int(model[6:]))
        Q, pid, z = c.Q, c.pid, c.z
    elif model.startswith("under"):
        n = int(model[5:])
        Q = _under_Q(n, n)
        pid = W.skew_pid(n, 100 * n + 1)
        # 36 states: tips simulated under Q, a few states apart.  With tips at both ends of the state space a branch that has
        # lost segments can be crossed by one of B2's 2e-8 entries alone, a path Bc does not know: oracle and engine then both
        # report a zero probability vector in a later sweep
        z = synth.make_tree(12, Q, W._omega(Q), 800 + n + 1, pid, states=W.spread_tips(12, n, n + 1) if n <= 12 else None, init_segments=n)
    elif model == "tiny10":
        p = SP.problem("tiny10")
        assert p.Omega == W._omega(p.Q)
        Q, pid, z = p.Q, p.pid, p.z
    else:
        Q = scattered_Q(24, 4, 24064, tiny=2)
        pid, z = _uniform(24), _c_tree(Q, 1164)
    return Case(f"thr_{model}_{'rescaled' if rescale else 'plain'}_{mapping}", f"SPARSE, {model}: Bc != B2", np.array(Q), np.array(pid), z, "sparse",
                C_SWEEPS, C_S, 61, range(C_S), mapping, rescale=rescale)


# ---- D. the windows of wb_branch_kernel -------------------------------------------------------------------------------
WINDOW_CASES = (("bigtree", 6), ("bigtree", 20), ("bigtree", 64), ("ks", 8))
WINDOW_JUMPS, WINDOW_SEGMENTS = 330.0, 400                  # Omega t of the long branches; initial segments of the third
WINDOW_S, WINDOW_SWEEPS, WINDOW_BIG_S = 2, 4, 1490


@functools.lru_cache(maxsize=None)
def window_case(variant, n, S=WINDOW_S):
    """a 12-tip tree whose edge rows 0, 1 and 2 are stretched to 330 / Omega, with exactly WB_MERGED_LDS + 1, WB_MERGED_LDS and 400
    initial segments: hundreds of segments on each in every sweep, and on the third more than WB_MERGED_LDS merged ones from the
    first sweep on (a sweep keeps 60 to 75 % of the segments it reads as merged ones and adds about 100 virtual jumps)"""
    ks = variant == "ks"
    Q = RC.hidden_rates_Q(n) if ks else synth.dense_Q(n, 0.02, 0.08, seed=n)
    Omega = W._omega(Q)
    z = synth.make_tree(12, Q, Omega, 1200 + n, _uniform(n), init_segments=3)
    z["edge.length"] = np.array(z["edge.length"], dtype=np.float64)
    for b, segs in ((0, WB_MERGED_LDS + 1), (1, WB_MERGED_LDS), (2, WINDOW_SEGMENTS)):
        z["edge.length"][b] = WINDOW_JUMPS / Omega
        z["maps"][b], z["mapnames"][b] = synth.initial_path(z["edge.length"][b], int(z["mapnames"][b][-1]), segs)
    if ks:
        z = RC.parity_tips(z)
    reps = range(S) if S <= 4 else (0, 63, S - 1)
    return Case(f"window_{variant}{n}_S{S}", f"n = {n}, {variant}: branches beyond {WB_MERGED_LDS} merged segments, {WB_FLUSH} noted transitions "
                f"and {WB_VARIATES} variates", Q, _uniform(n), z, variant, WINDOW_SWEEPS, S, 83, reps, "branches")


def window_cases():
    return [window_case(v, n) for v, n in WINDOW_CASES]


@functools.lru_cache(maxsize=None)
def oracle_windows(case, replica):
    """per sweep: (most merged segments of a branch, most transitions a branch notes, most exponential draws of a branch) from the
    oracle's chain state after each sweep.  The runs of equal states of a path are the merged segments of the sweep that left
    it; the branch kernel notes one transition per run boundary (one per consecutive pair of the segments it read in the
    n x n layout) and draws one variate per piece it writes (every dwell here is positive), i.e. per segment it leaves."""
    out = []
    m_in = np.array([len(m) for m in case.z["maps"]])        # segments the sweep reads
    for i in range(1, case.N + 1):
        _, rc, dump = case.oracle(replica, dump=True, N=i)
        assert rc == 0
        assert int(dump.seg_count.max()) <= dump.seg_state.shape[1]
        merged = notes = draws = 0
        for b, m in enumerate(dump.seg_count):
            s = dump.seg_state[b, :m]
            assert np.all(dump.seg_dwell[b, :m] > 0.0)
            runs = 1 + int(np.count_nonzero(s[1:] != s[:-1]))
            merged = max(merged, runs)
            notes = max(notes, int(m_in[b]) - 1 if case.ks else runs - 1)
            draws = max(draws, int(m))
        m_in = np.array(dump.seg_count)
        out.append((merged, notes, draws))
    return tuple(out)


# ---- E. the tree-pass fallbacks of the branch mapping ---------------------------------------------------------------
LEVELS_N, LEVELS_TIPS, LEVELS_S, LEVELS_SWEEPS = 64, 600, 3502, 2
WALK_N, WALK_TIPS, WALK_SWEEPS = 5, 61442, 2            # 61 441 internal nodes: the first count beyond the LDS copy


@functools.lru_cache(maxsize=None)
def levels_case():
    Q = synth.dense_Q(LEVELS_N, 0.02, 0.08, seed=LEVELS_N)
    z = synth.make_tree(LEVELS_TIPS, Q, W._omega(Q), 1300, _uniform(LEVELS_N), init_segments=2)
    return Case("levels_n64", "S E n just above 2^28: no transition maps, wb_root_kernel and wb_down_kernel per depth level", Q, _uniform(LEVELS_N),
                z, "bigtree", LEVELS_SWEEPS, LEVELS_S, 47, (0, LEVELS_S - 1), "branches")


@functools.lru_cache(maxsize=None)
def walk_case():
    Q = synth.dense_Q(WALK_N, 0.02, 0.08, seed=WALK_N)
    z = synth.make_tree(WALK_TIPS, Q, W._omega(Q), 1400, _uniform(WALK_N), init_segments=2)
    return Case("walk_n5", "61 441 internal nodes: the walk reads node states from global memory", Q, _uniform(WALK_N), z, "bigtree", WALK_SWEEPS,
                1, 53, (0,), "branches")


# ---- F. the segment limit of the replica mapping ----------------------------------------------------------------------
LIMIT_NS = (6, 41)


@functools.lru_cache(maxsize=None)
def limit_case(n, extra):
    """edge row 0 of a 10-tip tree with wide_maxseg(n) + extra initial segments on a branch of two expected jumps"""
    Q = synth.dense_Q(n, 0.02, 0.08, seed=n)
    Omega = W._omega(Q)
    z = synth.make_tree(10, Q, Omega, 1500 + n, _uniform(n), init_segments=3)
    z["edge.length"] = np.array(z["edge.length"], dtype=np.float64)
    z["edge.length"][0] = 2.0 / Omega
    z["maps"][0], z["mapnames"][0] = synth.initial_path(z["edge.length"][0], int(z["mapnames"][0][-1]), wide_maxseg(n) + extra)
    return Case(f"limit_n{n}_{extra:+d}", f"n = {n}: {wide_maxseg(n) + extra} initial segments on one branch", Q, _uniform(n), z, "bigtree", 1, 3, 67,
                range(3), "replicas")


OUTGROW_JUMPS, OUTGROW_SEGMENTS = 300.0, 120


@functools.lru_cache(maxsize=None)
def outgrow_case(n):
    """the same tree with edge row 0 stretched to 300 / Omega in 120 initial segments: accepted, and beyond the limit after the first
    sweep's virtual jumps"""
    Q = synth.dense_Q(n, 0.02, 0.08, seed=n)
    Omega = W._omega(Q)
    z = synth.make_tree(10, Q, Omega, 1500 + n, _uniform(n), init_segments=3)
    z["edge.length"] = np.array(z["edge.length"], dtype=np.float64)
    z["edge.length"][0] = OUTGROW_JUMPS / Omega
    z["maps"][0], z["mapnames"][0] = synth.initial_path(z["edge.length"][0], int(z["mapnames"][0][-1]), OUTGROW_SEGMENTS)
    return Case(f"outgrow_n{n}", f"n = {n}: a branch of 300 expected jumps", Q, _uniform(n), z, "bigtree", 3, 3, 67, range(3), "replicas")
