"""Inputs shared by the CPU and GPU tests of the classes of the one-chain branch mapping for 2 to 4 states (phm_narrow.h, phm_narrow.hip;
narrow_setup and fill_narrow_params of phm_engine.cpp; build_cluster_plan of phm_sched.cpp; DESIGN.md, "Classes of the one-chain
branch mapping"): the host's and the kernels' rules restated from their comments and formulas, functions that read off the oracle's
chain state which class every (wave, branch) of a sweep was in, and small problems chosen by the class they land in, with the oracle's
runs of them (computed once per session, shared, never written).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import functools

import numpy as np

import oracle_lib as O
import rateupdatecases as RC
import tilesclasses as T
from phylomap_amd import synth, treeorder

# the constants (phm_narrow.h, phm_narrow.hip)
WIDE_SEGMENTS, LONG = 96, 128                 # NARROW_WIDE_SEGMENTS, NARROW_LONG
LANES = 8                                     # lanes per branch, branches per wave of the eight-lane walk
MAP_WINDOW, EXP_WINDOW = 192, 256             # NARROW_MAP_WINDOW, NARROW_EXP_WINDOW
EXP_AHEAD = 8                                 # a branch's first allotment: m + 8 variates
OUT_STAGE = 32                                # NARROW_OUT_STAGE
BLOCK = 64                                    # NARROW_BLOCK: old segments and variates per block of the wave-wide walk
CLUSTER_NODES, CLUSTER_PASS, CLUSTER_STRIDE = 256, 64, 16      # NARROW_CLUSTER_NODES, NARROW_CLUSTER_BLOCK / 8, NARROW_CLUSTER_STRIDE
BAND = 8                                      # build_band_plan(s, 8): heights per tier of the (tile, branch) mapping's plan
WALK_BLOCK, WALK_RING, WALK_AHEAD, LDS_NODES = 1024, 4, 9, 61440
STATS_RIDING, STATS_OWN = 512, 256            # threads that add a statistics column: in the next sweep's first launch / a launch of its own

ORACLE_VARIANT = {"plain": O.PLAIN, "bigtree": O.BIGTREE, "ks": O.KS}
ceil_div = T.ceil_div
expected_segments = T.expected_segments       # 1 + Omega t_b, or the caller's path where that is longer
slot_caps = T.slot_caps                       # plan_slots


# ---------------------------------------------------------------------------------------------------------------------------
# the host's rules
# ---------------------------------------------------------------------------------------------------------------------------
def n_expected_wide(z, Omega):
    return sum(1 for x in expected_segments(z, Omega) if x >= WIDE_SEGMENTS)


def n_wide(z, Omega):
    """branches that get a wave each: every one expected to hold 96 segments, at least min(E / 16, 128) of them; at most all"""
    E = len(z["maps"])
    return min(E, max(n_expected_wide(z, Omega), min(E // 16, LONG)))


def dependency_driven(z, Omega, pruning_form=0):
    """the cluster kernel without level barriers: pruning_form 2 always, 1 never, 0 iff some branch is expected to hold 96 segments"""
    return pruning_form == 2 or (pruning_form == 0 and n_expected_wide(z, Omega) > 0)


def branch_order(caps):
    """largest slot first, stable"""
    return [int(b) for b in np.argsort(-np.asarray(caps), kind="stable")]


def n_waves(E, n_long):
    return n_long + ceil_div(E - n_long, LANES)


def wave_positions(E, n_long):
    """per eight-lane wave k: the sorted positions n_long + g n_waves8 + k of its groups g = 0 .. 7 (those below E)"""
    n8 = ceil_div(E - n_long, LANES)
    return [[n_long + g * n8 + k for g in range(LANES) if n_long + g * n8 + k < E] for k in range(n8)]


def windows(ms):
    """per group of one wave (segment counts ms, groups without a branch count as m = 1): (wb, pre, eb, epre) -- where its share
    of the map window and of the variate window starts and how much of it there is"""
    ms = list(ms) + [1] * (LANES - len(ms))
    out, wb, eb = [], 0, 0
    for m in ms:
        wb1, eb1 = min(wb + m - 1, MAP_WINDOW), min(eb + m + EXP_AHEAD, EXP_WINDOW)
        out.append((wb, wb1 - wb, eb, eb1 - eb))
        wb, eb = wb1, eb1
    return out


def stat_cols(n, ks):
    """columns the statistics kernels add: dwell sums, counts, and one more for the segment counter"""
    return n + (n * n if ks else n * (n - 1)) + 1


# ---------------------------------------------------------------------------------------------------------------------------
# tree shapes (the same constructions as tests/native/cluster_plan_check.cpp) and the cluster plans restated on them
# ---------------------------------------------------------------------------------------------------------------------------
class Shape:
    """a rooted binary tree: node 0 is the root, kid0[v] = -1 for a tip"""

    def __init__(self):
        self.kid0, self.kid1 = [-1], [-1]

    def split(self, v):
        self.kid0[v], self.kid1[v] = len(self.kid0), len(self.kid0) + 1
        self.kid0 += [-1, -1]; self.kid1 += [-1, -1]

    def edges(self):
        """edge table as R's ape writes it: tips 1 .. T, root T + 1, rows in cladewise order"""
        n = len(self.kid0)
        tips = (n + 1) // 2
        ids, parent = [0] * n, [-1] * n
        next_tip, next_int, stack, order = 1, tips + 1, [0], []
        while stack:
            v = stack.pop()
            order.append(v)
            if self.kid0[v] < 0:
                ids[v] = next_tip; next_tip += 1
            else:
                ids[v] = next_int; next_int += 1
                parent[self.kid0[v]] = parent[self.kid1[v]] = v
                stack += [self.kid1[v], self.kid0[v]]
        return np.array([(ids[parent[v]], ids[v]) for v in order if parent[v] >= 0], dtype=np.int32)

    def heights(self):
        h = [0] * len(self.kid0)
        for v in range(len(self.kid0) - 1, -1, -1):            # children carry larger numbers than their parents
            if self.kid0[v] >= 0:
                h[v] = 1 + max(h[self.kid0[v]], h[self.kid1[v]])
        return h                                               # tips 0, cherries 1: the engine's height + 1 on internal nodes


def ladder(tips):
    t, v = Shape(), 0
    for _ in range(tips - 1):
        t.split(v); v = t.kid1[v]
    return t


def _grow(t, v, tips, leaves):
    stack = [(v, tips)]
    while stack:
        v, k = stack.pop()
        if k == 1:
            leaves.append(v)
            continue
        t.split(v)
        stack += [(t.kid1[v], k // 2), (t.kid0[v], (k + 1) // 2)]


def balanced(tips):
    t = Shape()
    _grow(t, 0, tips, [])
    return t


def cherries(top, k):
    """a balanced top of ``top`` leaves, the first k of them (left to right) made cherries: top + k tips"""
    t, leaves = Shape(), []
    _grow(t, 0, top, leaves)
    for v in leaves[:k]:
        t.split(v)
    return t


def random_shape(tips):
    t, open_, x = Shape(), [0], 0x9e3779b97f4a7c15
    while len(open_) < tips:
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        i = (x >> 33) % len(open_)
        v = open_[i]
        t.split(v)
        open_[i] = t.kid0[v]; open_.append(t.kid1[v])
    return t


def cluster_tiers(t, max_nodes=CLUSTER_NODES):
    """build_cluster_plan: per tier the cluster sizes, largest first -- a tier takes every maximal subtree of at most ``max_nodes``
    internal nodes not taken by an earlier tier"""
    n = len(t.kid0)
    internal = [v for v in range(n) if t.kid0[v] >= 0]
    parent = [-1] * n
    for v in internal:
        parent[t.kid0[v]] = parent[t.kid1[v]] = v
    taken, tiers = [False] * n, []
    while not all(taken[v] for v in internal):
        left = [0] * n
        for v in reversed(internal):
            if not taken[v]:
                left[v] = 1 + left[t.kid0[v]] + left[t.kid1[v]]
        now = [False] * n
        sizes = []
        for v in internal:                                     # parents before children: a root, or below one
            if taken[v]:
                continue
            if left[v] <= max_nodes and (parent[v] < 0 or left[parent[v]] > max_nodes):
                sizes.append(left[v]); now[v] = True
            elif parent[v] >= 0 and now[parent[v]]:
                now[v] = True
        tiers.append(sorted(sizes, reverse=True))
        taken = [a or b for a, b in zip(taken, now)]
    return tiers


def band_tiers(t, band=BAND):
    """build_band_plan: tier k holds the heights [k band, (k + 1) band), a cluster is a maximal subtree inside its tier"""
    h = t.heights()
    internal = [v for v in range(len(t.kid0)) if t.kid0[v] >= 0]
    parent = {}
    for v in internal:
        parent[t.kid0[v]] = parent[t.kid1[v]] = v
    tier = {v: (h[v] - 1) // band for v in internal}
    root_of, size = {}, {}
    for v in internal:                                         # parents before children
        p = parent.get(v)
        root_of[v] = root_of[p] if p is not None and tier[p] == tier[v] else v
        size[root_of[v]] = size.get(root_of[v], 0) + 1
    return [sorted((s for r, s in size.items() if tier[r] == k), reverse=True) for k in range(max(tier.values()) + 1)]


# the trees tests/native/cluster_plan_check.cpp builds, by the names it prints
PLAN_TREES = ([("ladder 2", lambda: ladder(2))] + [(f"ladder {k}", functools.partial(ladder, k)) for k in (257, 258, 700)] +
              [(f"balanced {k}", functools.partial(balanced, k)) for k in (256, 257, 258, 1024)] + [("random 1000", lambda: random_shape(1000))] +
              [(f"cherries {a} {b}", functools.partial(cherries, a, b))
               for a, b in ((64, 63), (64, 64), (65, 65), (128, 65), (128, 128), (1024, 1024), (2048, 1025))])


def level_sizes(z):
    """(nodes per height level, edges to internal nodes per depth level) of the tree z"""
    edge, Tn = np.asarray(z["edge"]), len(z["states"])
    kids, depth = {}, {Tn + 1: 0}
    for p, c in edge:                                          # cladewise rows: parents first
        kids.setdefault(int(p), []).append(int(c))
        depth[int(c)] = depth[int(p)] + 1
    height = {}
    for p, c in edge[::-1]:
        height[int(p)] = max(height.get(int(p), 0), height.get(int(c), -1) + 1)
    up = np.bincount([h for h in height.values()])
    down = np.bincount([depth[int(p)] for p, c in edge if c > Tn], minlength=1) if np.any(edge[:, 1] > Tn) else np.zeros(0, dtype=int)
    return [int(v) for v in up], [int(v) for v in down]


# ---------------------------------------------------------------------------------------------------------------------------
# models, trees with paths
# ---------------------------------------------------------------------------------------------------------------------------
Q_SLOW = np.array([[-0.1, 0.1], [0.1, -0.1]])                  # with Omega = 1: B = [[.9, .1], [.1, .9]], nine virtual jumps per real one
Q_SLOWER = np.array([[-0.01, 0.01], [0.01, -0.01]])            # with Omega = 1: merged segments of about 100 pieces
Q_ABSORBING = np.array([[-.2, .1, .1], [.1, -.2, .1], [0., 0., 0.]])


def _pid(n):
    return np.full(n, 1.0 / n)


def model(n, variant="plain"):
    """tilesclasses' models; the ks sweep at 2 states runs under the plain 2-state matrix"""
    return T.model(n, variant if n == 4 else "plain")


def tree_from_shape(shape, Q, pid, Omega, seed, mean_steps=1.0, segs=2, lens=None):
    """a phylomap tree object on a hand-made topology: exponential branch lengths of mean ``mean_steps`` / Omega (or ``lens``), tips
    simulated under Q, ``segs`` equal pieces per branch in state 1, the last piece of a tip branch in the tip's state"""
    edge = shape.edges()
    E, Tn = edge.shape[0], edge.shape[0] // 2 + 1
    lens = np.random.default_rng(seed).exponential(mean_steps / Omega, size=E) if lens is None else np.asarray(lens, dtype=np.float64)
    states = np.asarray(synth.simulate_tips(edge, lens, np.asarray(Q), pid, seed), dtype=np.int32)
    maps, names, node_states = [], [], np.ones((E, 2), dtype=np.int32)
    for r in range(E):
        child = int(edge[r, 1])
        end = int(states[child - 1]) if child <= Tn else 1
        m, mn = synth.initial_path(float(lens[r]), end, segs)
        maps.append(m); names.append(mn)
        node_states[r, 1] = end
    return {"edge": edge, "Nnode": Tn - 1, "edge.length": lens, "states": states, "maps": maps, "mapnames": names, "node.states": node_states}


def with_paths(z, counts=None, lengths=None, zero_at=None):
    """z with the initial path of branch b cut into counts[b] equal pieces of total length lengths[b] (dicts or sequences; as
    test_one_branch_of_3000_segments_the_wave_wide_walk sets them); zero_at = (b, i): piece i of branch b has length zero"""
    z = dict(z, maps=[np.array(m, dtype=np.float64) for m in z["maps"]], mapnames=[np.array(m, dtype=np.int32) for m in z["mapnames"]])
    E = len(z["maps"])
    counts = dict(enumerate(counts)) if isinstance(counts, (list, tuple)) else dict(counts or {})
    lengths = dict(enumerate(lengths)) if isinstance(lengths, (list, tuple, np.ndarray)) else dict(lengths or {})
    for b in range(E):
        if b in counts or b in lengths:
            m = int(counts.get(b, len(z["maps"][b])))
            t = float(lengths.get(b, np.sum(z["maps"][b])))
            z["maps"][b], z["mapnames"][b] = synth.initial_path(t, int(z["mapnames"][b][-1]), m)
    if zero_at is not None:
        z["maps"][zero_at[0]][zero_at[1]] = 0.0
    z["edge.length"] = np.array([float(np.sum(m)) for m in z["maps"]])
    return z


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
class Case:
    """One problem and the engine runs the GPU test makes of it.  ``forms``: the values of pruning_form it runs under (0: automatic);
    ``dump_at``: the sweeps after which the chain state is compared (the last one always is); ``chains``: replicas; ``sites``:
    per-replica tips; ``opt``: further engine options; ``wants``: what tests/test_narrow_classes_cpu.py asserts of it"""

    def __init__(self, name, purpose, Q, Omega, z, variant="bigtree", chains=1, N=1, seed=1, forms=(1, 2), dump_at=(), sites=None, opt=None,
                 seg_cap=512, wants=None):
        self.name, self.purpose, self.Q, self.Omega, self.z, self.variant = name, purpose, np.asarray(Q, dtype=np.float64), float(Omega), z, variant
        self.S, self.N, self.seed, self.forms, self.sites, self.opt, self.seg_cap = chains, N, seed, tuple(forms), sites, dict(opt or {}), seg_cap
        self.dump_at = tuple(sorted(set(dump_at) | {N}))
        self.wants = dict(wants or {})
        self.n = self.Q.shape[0]
        self.pid = _pid(self.n)
        self.B = np.eye(self.n) + self.Q / self.Omega
        self.nen, self.nodelist, self.root = treeorder.pruningwiseedgeorder(z), treeorder.makenodelist(z), treeorder.myreorder(z)
        self.E, self.tips = len(z["maps"]), len(z["states"])
        self.ks = variant == "ks"
        self.ncnt = self.n * self.n if self.ks else self.n * (self.n - 1)
        self.length = float(np.sum(z["edge.length"]))
        self.caps = slot_caps(z, self.Omega, self.S, self.N, self.opt.get("cap_tail", 0.0))
        self.order = branch_order(self.caps)
        self.n_long = n_wide(z, self.Omega)
        self.n_waves = n_waves(self.E, self.n_long)
        self.waves = [[self.order[p] for p in w] for w in wave_positions(self.E, self.n_long)]       # branches of every eight-lane wave
        self.wide = self.order[:self.n_long]
        for a in (self.Q, self.B):
            a.setflags(write=False)

    def dependency_driven(self, form=0):
        return dependency_driven(self.z, self.Omega, form)

    def __repr__(self):
        return self.name


class State:
    """the oracle's chain state after some sweeps"""

    def __init__(self, rows, rc, db):
        self.rows, self.rc, self.seg_count, self.node_states, self.PL, self.seg_dwell, self.seg_state = (
            rows, rc, db.seg_count, db.node_states, db.PL, db.seg_dwell, db.seg_state)
        for a in (rows, db.seg_count, db.node_states, db.PL, db.seg_dwell, db.seg_state):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def oracle_state(case, chain, k):
    """statistics rows [k, cols] and chain state of one chain after k sweeps (k = 0: the caller's paths), seg_cap as the case sets it"""
    z = case.z if case.sites is None else dict(case.z, states=np.asarray(case.sites[chain], dtype=np.int32))
    ft = O.FlatTree(z)
    n = case.n
    cols = n + n * n + 2 + 3 * (n // 2 - 1) + 1 if case.ks else n + n * (n - 1)
    out = np.zeros((k, cols), order="F")
    Qc, Bc = np.asfortranarray(case.Q), np.asfortranarray(case.B)
    pid = np.ascontiguousarray(case.pid)
    nen, nodelist = np.ascontiguousarray(case.nen, dtype=np.int32), np.ascontiguousarray(case.nodelist, dtype=np.int32)
    rng, _ = O.make_rng(case.seed, case.opt.get("replica_offset", 0) + chain)
    db = O.DumpBuf(ft, n, seg_cap=case.seg_cap)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    rc = O.lib().orc_maketreelistMCMC(C.byref(ft.c), n, p(Qc, C.c_double), p(pid, C.c_double), p(Bc, C.c_double), C.c_double(case.Omega),
                                      p(nen, C.c_int32), p(nodelist, C.c_int32), int(case.root), int(k), int(ORACLE_VARIANT[case.variant]), 0,
                                      C.byref(rng), p(out, C.c_double), C.byref(db.c))
    if k == 0:                                                 # no sweep: the caller's paths
        db.seg_count[:] = [len(m) for m in z["maps"]]
    return State(out, rc, db)


# ---------------------------------------------------------------------------------------------------------------------------
# reach: which class every (wave, branch) of every sweep was in, from the oracle's state before and after the sweep
# ---------------------------------------------------------------------------------------------------------------------------
def longest_run(states):
    """pieces of the longest merged segment: the longest run of equal states"""
    s = np.asarray(states)
    if s.size == 0:
        return 0
    cut = np.flatnonzero(np.diff(s) != 0)
    return int(np.max(np.diff(np.concatenate([[-1], cut, [s.size - 1]]))))


@functools.lru_cache(maxsize=None)
def reach(case):
    """one record per (chain, sweep, branch): sweep k = 1 .. N reads the counts ``m`` left by sweep k - 1 and leaves ``new`` pieces --
    the variates the branch consumed, every variate emitting exactly one piece unless the walk is stuck on a non-positive segment
    (``stuck``: some piece of the old path is not positive).  Eight-lane branches carry their wave, group and window shares (wb,
    pre, eb, epre); ``beyond``: old segments past the map window; ``flushes``: full output stages written out on the way; wave-wide
    branches (``wide``) the 64-blocks of old segments (m - 1 change points) and of variates; ``run``: the longest merged segment in
    pieces.  A state change at the first or last lane of a block cannot be seen from here."""
    assert max(int(np.max(oracle_state(case, c, k).seg_count)) for c in range(case.S) for k in range(case.N + 1)) <= case.seg_cap
    out = []
    for c in range(case.S):
        for k in range(1, case.N + 1):
            old, new = oracle_state(case, c, k - 1), oracle_state(case, c, k)
            for b in case.wide:
                m, mn = int(old.seg_count[b]), int(new.seg_count[b])
                out.append(dict(chain=c, sweep=k, branch=b, wide=True, m=m, new=mn, old_blocks=ceil_div(m - 1, BLOCK),
                                var_blocks=ceil_div(mn, BLOCK), run=longest_run(new.seg_state[b, :mn]), stuck=_stuck(case, old, k, b)))
            for w, branches in enumerate(case.waves):
                win = windows([int(old.seg_count[b]) for b in branches])
                for g, b in enumerate(branches):
                    m, mn = int(old.seg_count[b]), int(new.seg_count[b])
                    wb, pre, eb, epre = win[g]
                    out.append(dict(chain=c, sweep=k, branch=b, wide=False, wave=w, group=g, m=m, new=mn, wb=wb, pre=pre, eb=eb, epre=epre,
                                    beyond=m - 1 - pre, flushes=mn // OUT_STAGE, run=longest_run(new.seg_state[b, :mn]),
                                    stuck=_stuck(case, old, k, b)))
    return tuple(out)


def _stuck(case, old, k, b):
    path = case.z["maps"][b] if k == 1 else old.seg_dwell[b, :int(old.seg_count[b])]
    return bool(np.any(np.asarray(path) <= 0.0))


def reached(case, **eq):
    """the records of reach(case) whose fields equal the keywords (a callable keyword is a predicate on the record)"""
    return [r for r in reach(case) if all((v(r) if callable(v) else r.get(k) == v) for k, v in eq.items())]


def _five(Q, Omega, seed, steps, counts=1, n_tips=5, **kw):
    """the smallest tree with one full eight-lane wave (5 tips: E = 8) or any other small size: a random topology, Omega t_b and the
    initial segment count per branch as given (scalars, or sequences that list the tip edges first: two sister tips in different
    states cannot both hang on one-segment paths)"""
    n = np.asarray(Q).shape[0]
    z = synth.make_tree(n_tips, Q, Omega, seed, _pid(n))
    E = len(z["maps"])
    steps = [steps] * E if np.isscalar(steps) else list(steps)
    counts = [counts] * E if np.isscalar(counts) else list(counts)
    assert len(steps) == E and len(counts) == E
    tip_rows = [b for b in range(E) if z["edge"][b][1] <= n_tips] + [b for b in range(E) if z["edge"][b][1] > n_tips]
    counts, steps = dict(zip(tip_rows, counts)), dict(zip(tip_rows, steps))      # sequences: the tip edges first, then the edges to internal nodes
    return with_paths(z, counts, {b: s / Omega for b, s in steps.items()}, **kw)


# -- tree passes: every case under pruning_form 1 and 2 -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_shape(name, kind, a, b=0, n=4, variant="bigtree", N=2, segs=2):
    """a tree of a given shape with short branches"""
    Q = model(n, variant)
    Omega = T.omega_of(Q)
    shape = {"ladder": ladder, "balanced": balanced}[kind](a) if kind != "cherries" else cherries(a, b)
    z = tree_from_shape(shape, Q, _pid(n), Omega, 7000 + a + b, mean_steps=1.0, segs=segs)
    if variant == "ks":
        z = RC.parity_tips(z)
    c = Case(name, f"{kind} {a} {b or ''}".strip(), Q, Omega, z, variant, chains=1, N=N, seed=600 + a, dump_at=range(1, N + 1), seg_cap=64)
    c.shape = shape
    return c


def cases_tree():
    c = [case_shape("P_tips2", "ladder", 2, n=2), case_shape("P_tips3", "ladder", 3, n=3, variant="plain"),
         case_shape("P_level64", "cherries", 64, 64, n=4), case_shape("P_level65", "cherries", 65, 65, n=3, variant="plain"),
         case_shape("P_level128", "cherries", 128, 128, n=2),
         case_shape("P_bushy256", "balanced", 257, n=4), case_shape("P_bushy257", "balanced", 258, n=2),
         case_shape("P_ladder256", "ladder", 257, n=2), case_shape("P_ladder257", "ladder", 258, n=4),
         case_shape("P_ks2", "balanced", 12, n=2, variant="ks", N=3), case_shape("P_ks4", "balanced", 12, n=4, variant="ks", N=3)]
    return c + [case_chain(s) for s in CHAIN_SEGMENTS] + [case_sites()]


CHAIN_SEGMENTS = (16, 17, 18, 32, 33, 34)      # chains of 15, 16, 17, 31, 32, 33 steps: either side of one and of two strides of 16


@functools.lru_cache(maxsize=None)
def case_chain(segs):
    Q = T.model(4)
    Omega = T.omega_of(Q)
    z = tree_from_shape(balanced(6), Q, _pid(4), Omega, 7100, segs=segs)
    return Case(f"P_chain{segs - 1}", f"{segs} initial segments per branch: chains of {segs - 1} steps on the edges to internal nodes", Q, Omega, z,
                "plain", N=1, seed=71)


@functools.lru_cache(maxsize=None)
def case_sites():
    Q = T.model(4)
    Omega = T.omega_of(Q)
    z = tree_from_shape(balanced(11), Q, _pid(4), Omega, 7200)
    sites = np.random.default_rng(72).integers(1, 5, size=(3, 11)).astype(np.int32)
    return Case("P_sites", "three chains whose tips differ (tips_per_replica)", Q, Omega, z, "bigtree", chains=3, N=2, seed=72, sites=sites)


# -- walk ---------------------------------------------------------------------------------------------------------------------------
LADDER_TIPS = tuple(range(2, 16))              # 0 .. 13 walk levels


def cases_walk():
    c = [case_shape(f"W_ladder{t}", "ladder", t, n=4 if t % 2 else 2, N=3) for t in LADDER_TIPS]
    c += [case_shape("W_level63", "cherries", 64, 63, n=2), case_shape("W_level64", "cherries", 64, 64, n=4),
          case_shape("W_level65", "cherries", 128, 65, n=2),
          case_shape("W_level1024", "cherries", 1024, 1024, n=2), case_shape("W_level1025", "cherries", 2048, 1025, n=2)]
    return c


# -- the eight-lane walk --------------------------------------------------------------------------------------------------------------
def _wave_case(name, purpose, counts, n=2, variant="plain", N=2, seed=81, steps=2.0, tips=5, wants=None, **kw):
    """one eight-lane wave (5 tips) whose branches start from the given segment counts, all of Omega t_b = ``steps``: the slots then
    sort by count, so group g of the wave holds the g-th largest count"""
    Q = model(n, variant)
    Omega = T.omega_of(Q)
    z = _five(Q, Omega, 8000 + sum(counts), steps, list(counts), n_tips=tips)
    if variant == "ks":
        z = RC.parity_tips(z)
    return Case(name, purpose, Q, Omega, z, variant, N=N, seed=seed, dump_at=(1,), wants=wants, **kw)


@functools.lru_cache(maxsize=None)
def case_map_window(total):
    """sum of (m - 1) over the wave: seven branches of 25 segments and one of total - 167"""
    return _wave_case(f"L_map{total}", f"map window: {total} change points in the wave", [25] * 7 + [total - 168 + 1], n=4, variant="bigtree",
                      wants={"map_sum": total})


@functools.lru_cache(maxsize=None)
def case_straddle(by):
    """seven branches of 27 segments (182 change points) and a last one of 11 + by: ``by`` old segments past the window end"""
    return _wave_case(f"L_straddle{by}", f"a branch {by} old segments past the end of the map window", [27] * 7 + [11 + by], n=3,
                      wants={"beyond": by})


@functools.lru_cache(maxsize=None)
def case_beyond():
    """95 + 95 + 11 segments fill the window (94 + 94 + 4 of 10); a branch of 6 lies wholly beyond it (wb = 192), one of 2 and three of one segment (the edges to internal nodes) follow"""
    return _wave_case("L_beyond", "a branch wholly beyond the map window, with m = 1 branches in the same wave", [95, 95, 11, 6, 2, 1, 1, 1], n=2,
                      wants={"wholly_beyond": True})


@functools.lru_cache(maxsize=None)
def case_exp_window(total):
    """sum of (m + 8) over the wave: seven branches of 24 segments and one of total - 64 - 168"""
    return _wave_case(f"L_exp{total}", f"variate window: {total} first variates in the wave", [24] * 7 + [total - 64 - 168], n=2,
                      wants={"exp_sum": total})


@functools.lru_cache(maxsize=None)
def case_allot(seed=None, steps=None):
    """one-segment paths under the slow chain: what a branch consumes against its first allotment m + 8"""
    z = _five(Q_SLOW, 1.0, ALLOT_SEED, ALLOT_STEPS if steps is None else steps, [2] * 5 + [1] * 3)
    return Case("L_allot", "branches that consume exactly m + 8, m + 9, m + 16 and m + 17 variates, and 31 .. 33, 64, 65 pieces", Q_SLOW, 1.0, z,
                "plain", chains=2, N=ALLOT_N, seed=ALLOT_RUN_SEED if seed is None else seed, dump_at=range(1, ALLOT_N + 1),
                wants={"over_allotment": (0, 1, 8, 9), "pieces": (31, 32, 33, 64, 65)})


ALLOT_SEED, ALLOT_RUN_SEED, ALLOT_N = 8100, 15, 6               # the run seed: the first of 0, 1, .. whose oracle runs reach all nine classes
ALLOT_STEPS = (12.0, 20.0, 66.0, 70.0, 74.0, 30.0, 34.0, 36.0)    # the tip edges (two segments), then the edges to internal nodes (one)


@functools.lru_cache(maxsize=None)
def case_ragged(tips, long_branch):
    """E - n_long mod 8: 5 tips 0; 9 tips (E = 16, one wave-wide branch by the E / 16 rule) 7; 6 tips with one branch of 96 segments 1;
    8 tips (E = 14) no wave-wide branch"""
    Q = T.model(4)
    Omega = T.omega_of(Q)
    z = synth.make_tree(tips, Q, Omega, 8200 + tips, _pid(4))
    if long_branch:
        z = with_paths(z, {int(np.argmax(z["edge.length"])): 96})
    return Case(f"L_ragged{tips}", f"{tips} tips", Q, Omega, z, "bigtree", chains=2, N=3, seed=82, forms=(0,))


@functools.lru_cache(maxsize=None)
def case_expected(value, through):
    """one branch expected to hold 95 or 96 segments -- through Omega t_b (Omega = 0.125, t_b = 8 (value - 1): exact) or through the
    caller's path -- on a 5-tip tree: 96 makes it the wave-wide branch and turns the automatic pruning form"""
    Q = T.model(2)
    Omega = T.omega_of(Q)
    assert Omega == 0.125
    z = _five(Q, Omega, 8300, 2.0, 2)
    b = 3
    z = with_paths(z, {b: 1}, {b: 8.0 * (value - 1)}) if through == "length" else with_paths(z, {b: value})
    return Case(f"L_expected{value}_{through}", f"a branch expected to hold {value} segments through its {through}", Q, Omega, z, "plain", chains=2,
                N=3, seed=83, forms=(0, 1, 2))


@functools.lru_cache(maxsize=None)
def case_cut():
    """seven branches of 30 segments and one of 10 under the slow chain at Omega t_b = 40: the seventh's share of the variate window is
    cut to 28 of 38 and the eighth's to none, and both consume more than that -- they refill from where their share ends"""
    z = _five(Q_SLOW, 1.0, 8150, 40.0, [30] * 7 + [10])
    return Case("L_cut", "a branch whose share of the variate window was cut and that refills from there", Q_SLOW, 1.0, z, "plain", N=2, seed=84,
                dump_at=(1,), wants={"cut_share": True})


def cases_lanes():
    return ([case_map_window(t) for t in (191, 192, 193)] + [case_straddle(b) for b in (1, 8, 9)] + [case_beyond()] +
            [case_exp_window(t) for t in (255, 256, 257)] + [case_allot(), case_cut()] +
            [case_ragged(5, False), case_ragged(9, False), case_ragged(6, True), case_ragged(8, False)] +
            [case_shape("L_wide127", "balanced", 1024, n=2), case_shape("L_wide128", "balanced", 1025, n=2)] +       # min(E / 16, 128)
            [case_expected(v, t) for v in (95, 96) for t in ("length", "path")])


# -- the wave-wide walk ---------------------------------------------------------------------------------------------------------------
WIDE_PATHS = (1, 2, 64, 65, 66, 129, 130)
WIDE_SWEEPS = (("plain", 2), ("plain", 3), ("plain", 4), ("ks", 2), ("ks", 4))


@functools.lru_cache(maxsize=None)
def case_wide(m0, variant, n, zero=False):
    """9 tips (E = 16): the branch with the largest slot is walked wave-wide by the E / 16 rule; it is made the longest by far
    (Omega t_b = 60) and starts from m0 segments.  Which lane of a block sees a state change is not asserted: the reach functions
    cannot see a change at the first or last lane of a block."""
    Q = model(n, variant)
    Omega = T.omega_of(Q)
    z = synth.make_tree(9, Q, Omega, 9000 + n, _pid(n))
    b = int(np.argmax(z["edge.length"]))
    z = with_paths(z, {b: m0}, {b: 60.0 / Omega}, zero_at=(b, 70) if zero else None)
    if variant == "ks":
        z = RC.parity_tips(z)
    c = Case(f"X_m{m0}_{variant}{n}" + ("_zero" if zero else ""), f"a wave-wide branch that starts from {m0} segments", Q, Omega, z, variant, chains=2,
             N=4, seed=91, forms=(0,), dump_at=(1, 2, 3))
    c.long_branch = b
    return c


@functools.lru_cache(maxsize=None)
def case_wide_consume(seed=None, l0=140.0, l1=70.0):
    """what the wave-wide branch consumes in a sweep: 63, 64, 65 and 129 variates, under the slow chain"""
    z = synth.make_tree(9, Q_SLOW, 1.0, 9100, _pid(2))
    order = np.argsort(-np.asarray(z["edge.length"]), kind="stable")
    z = with_paths(z, {int(order[0]): 100, int(order[1]): 100}, {int(order[0]): l0, int(order[1]): l1})
    return Case("X_consume", "wave-wide branches that consume 63, 64, 65 and 129 variates in a sweep", Q_SLOW, 1.0, z, "plain", chains=2,
                N=CONSUME_N, seed=CONSUME_RUN_SEED if seed is None else seed, forms=(0,), dump_at=range(1, CONSUME_N + 1), wants={"wide_consumes": (63, 64, 65, 129)})


CONSUME_RUN_SEED, CONSUME_N = 82, 8                          # the first seed whose oracle runs reach all four


@functools.lru_cache(maxsize=None)
def case_wide_run():
    """a merged segment cut into more than 64 pieces: a long branch, a slow 2-state chain, Omega a hundred times its rate"""
    z = synth.make_tree(9, Q_SLOWER, 1.0, 9200, _pid(2))
    b = int(np.argmax(z["edge.length"]))
    z = with_paths(z, {b: 3}, {b: 300.0})
    return Case("X_run", "a merged segment of more than 64 pieces on a wave-wide branch", Q_SLOWER, 1.0, z, "plain", chains=2, N=4, seed=92,
                forms=(0,), dump_at=(1, 2, 3), seg_cap=1024, wants={"wide_run_over": 64})


def cases_wide():
    c = [case_wide(m0, v, n) for m0 in WIDE_PATHS for v, n in WIDE_SWEEPS]
    return c + [case_wide(130, "plain", 2, zero=True), case_wide(130, "ks", 4, zero=True), case_wide_consume(), case_wide_run()]


# -- flags ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_absorbing():
    """state 3 absorbs: B[3, :] = (0, 0, 1), so a transition map's entry for the previous state 3 has all probabilities zero wherever the
    branch does not end in 3 -- in the down maps, in both walks and through compose_maps -- and that previous state never materialises"""
    Omega = 0.25
    z = synth.make_tree(9, Q_ABSORBING, Omega, 9300, _pid(3), states=np.array([1, 2, 1, 2, 3, 1, 2, 3, 1], dtype=np.int32), init_segments=3)
    b = int(np.argmax(z["edge.length"]))
    z = with_paths(z, {b: 130})
    return Case("F_absorbing", "an absorbing state: flagged map entries that never materialise", Q_ABSORBING, Omega, z, "plain", chains=2, N=4, seed=93,
                forms=(0, 1), dump_at=(1, 2))


@functools.lru_cache(maxsize=None)
def case_impossible():
    """tips in both transient states below a root that can only be in the absorbing one: pid = (0, 0, 1)"""
    c = case_absorbing()
    z = dict(c.z, states=np.where(np.asarray(c.z["states"]) == 3, 1, c.z["states"]).astype(np.int32))
    z = synth.with_tip_states(z, z["states"])
    bad = Case("F_impossible", "tips that are impossible under Q", Q_ABSORBING, 0.25, z, "plain", N=1, seed=94, forms=(0,))
    bad.pid = np.array([0.0, 0.0, 1.0])
    return bad


# -- capacity -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_capacity(kind, seed=90):
    """cap_tail = 0.9 under the slow chain: slots far too small on purpose.  "lanes": 5 tips, every branch in the eight-lane walk;
    "wide": 9 tips, the longest branch wave-wide"""
    if kind == "lanes":
        z = _five(Q_SLOW, 1.0, 9400, (50.0, 60.0, 70.0, 80.0, 40.0, 45.0, 55.0, 65.0), 2)
    else:
        z = synth.make_tree(9, Q_SLOW, 1.0, 9401, _pid(2))
        z = with_paths(z, None, {int(np.argmax(z["edge.length"])): 90.0})
    return Case(f"C_{kind}", f"a slot that overflows in {'an eight-lane' if kind == 'lanes' else 'the wave-wide'} branch", Q_SLOW, 1.0, z, "plain",
                chains=2, N=CAPACITY_N, seed=seed, forms=(0,), opt={"cap_tail": 0.9}, wants={"overflow": kind})


CAPACITY_N = 6


# -- statistics -----------------------------------------------------------------------------------------------------------------------
STAT_TIPS = (40, 1200, 2300)                   # wave rows per chain: 14, 412, 687


@functools.lru_cache(maxsize=None)
def case_stats(tips):
    Q = T.model(4)
    Omega = T.omega_of(Q)
    z = synth.make_tree(tips, Q, Omega, 9500 + tips, _pid(4))
    z = T.scaled(z, 0.25)                                                  # short branches: Omega t_b = 1 on average
    return Case(f"S_rows{tips}", f"{tips} tips, one chain: the statistics row of every sweep", Q, Omega, z, "bigtree", N=5, seed=96, forms=(0,), seg_cap=64)


REDUCE_CHAINS = (64, 65, 130)


@functools.lru_cache(maxsize=None)
def case_reduce(chains, variant):
    n = 4
    Q = model(n, variant)
    Omega = T.omega_of(Q)
    z = synth.make_tree(12, Q, Omega, 9600, _pid(n))
    if variant == "ks":
        z = RC.parity_tips(z)
    return Case(f"S_reduce{chains}_{variant}", f"{chains} chains summed per tile of 64", Q, Omega, z, variant, chains=chains, N=3, seed=97, forms=(0,),
                opt={"reduce": True})


def all_cases():
    return (cases_tree() + cases_walk() + cases_lanes() + cases_wide() + [case_absorbing(), case_capacity("lanes"), case_capacity("wide")] +
            [case_stats(t) for t in STAT_TIPS] + [case_reduce(c, v) for c in REDUCE_CHAINS for v in ("bigtree", "ks")])
