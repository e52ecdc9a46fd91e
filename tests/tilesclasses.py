"""Inputs shared by the CPU and GPU tests of the classes of the (tile, branch) sweep for 2 to 4 states (phm_tiles.hip; tiles_setup,
fill_tile_params and tiles_sweep_parts of phm_engine.cpp; DESIGN.md, "Classes of the 2 to 4 state tiles sweep"): the host's rules
restated from their comments and formulas, the list of every instantiation of the branch kernel and of the cluster pruning kernel,
and small problems chosen by the class they land in, with the oracle's runs of them (computed once per session, shared, never
written).  phm_debug_options.branch_group puts a 12-tip tree in the class of a 10 000-tip one.  TEST INFRASTRUCTURE ONLY."""
import functools
import math

import numpy as np

import oracle_lib as O
import rateupdatecases as RC
from phylomap_amd import synth, treeorder

# the engine's constants (phm_tiles.h, phm_engine.cpp)
GROUP_WAVES, GROUP_MAX, GROUP_FORCED_MAX = 65536, 16, 64      # tiles_branch_group, tiles_group
CHUNK = 64                                                    # TILES_CHUNK: group partials per second-stage sum
KTAB = 24                                                     # TILES_KTAB: chain-table rows the branch kernel keeps in LDS
LONG_SEGMENTS = 48.0                                          # PHM_TILES_LONG_SEGMENTS
CL_MAX_WORK = 65536                                           # TILES_CL_MAX_WORK
PART_MIN_WAVES, AUTO_PARTS, MAX_PARTS = 4 * 8 * 1024, 2, 4    # TILES_PART_MIN_ROUNDS x TILES_RESIDENT_WAVES, TILES_AUTO_PARTS
GIB = 1 << 30
BYTES_CAP = 8 * GIB                                           # what a case of natural size may ask of the device

ORACLE_VARIANT = {"plain": O.PLAIN, "bigtree": O.BIGTREE, "bf": O.BF, "ks": O.KS}


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------
# the host's rules
# ---------------------------------------------------------------------------------------------------------------------------
def group(tiles, E, forced=0):
    """branches per wave of the branch kernel: one while waves are scarce, up to 16 once there are 65 536 of them anyway;
    phm_debug_options.branch_group > 0 replaces it, clamped to 64"""
    if forced > 0:
        return min(GROUP_FORCED_MAX, forced)
    return max(1, min(GROUP_MAX, tiles * E // GROUP_WAVES))


def n_groups(E, g):
    return ceil_div(E, g)


def n_chunks(E, g):
    return ceil_div(n_groups(E, g), CHUNK)


def cnt_copies(tiles):
    """copies of a tile's transition counters: enough that 512 counter sets exist however few the tiles, at most 64"""
    c = 1
    while c < 64 and c * tiles < 512:
        c *= 2
    return c


def expected_segments(z, Omega):
    """per branch: what the host expects it to hold -- 1 + Omega t_b in stationarity, or the caller's path where that is longer"""
    return [max(1.0 + Omega * float(sum(m)), float(len(m))) for m in z["maps"]]


def long_form(z, Omega):
    """the branch kernel without its limit of 64 merged segments per branch and lane: some branch expected to hold more than 48"""
    return max(expected_segments(z, Omega)) > LONG_SEGMENTS


def clusters(tiles, Nn, deep=False, level_groups=0):
    """the tree passes over clusters of levels (one launch per tier) instead of one launch per level"""
    return level_groups >= 2 or (level_groups == 0 and (deep or tiles * Nn <= CL_MAX_WORK))


def parts(tiles, E, g, forced=0, clustered=False, recorded=False):
    """sweep parts on streams of their own: only the launch-per-level form without a recorded map iteration takes them; automatic:
    a part must still fill the chip four times over in the branch kernel"""
    if clustered or recorded:
        return 1
    p = forced if forced > 0 else min(AUTO_PARTS, tiles * n_groups(E, g) // PART_MIN_WAVES)
    return max(1, min(p, MAX_PARTS, tiles))


def poisson_capacity(lam, tail):
    """phm::poisson_capacity: the smallest slot that a 1 + Poisson(lam) count exceeds with probability below ``tail``"""
    if not lam > 0.0:
        return 1
    ltail = math.log(tail if tail > 0.0 else 1e-16)
    c = int(math.ceil(lam)) + 1
    while True:
        lp = -lam + c * math.log(lam) - math.lgamma(c + 1.0)
        ratio = lam / (c + 1.0)
        if ratio < 1.0 and lp - math.log1p(-ratio) < ltail:
            break
        if c > int(lam * 4 + 4096):
            break
        c += 1
    return min(c + 1, 60000)


def default_slot_tail(S, E, max_iters):
    return max(1e-16, min(1e-9, 0.05 / (float(max(S, 1)) * max(E, 1) * max(max_iters, 1))))


def slot_caps(z, Omega, S, max_iters, cap_tail=0.0):
    """plan_slots: rows of every branch's slot"""
    tail = cap_tail if cap_tail > 0.0 else default_slot_tail(S, len(z["maps"]), max_iters)
    caps = []
    for m in z["maps"]:
        tb = 0.0
        for v in m:
            tb += float(v)
        q = poisson_capacity(Omega * tb, tail)
        caps.append(max(q, len(m) + q - 1) + 2)
    return caps


def device_bytes(z, Omega, n, S, max_iters, ks_layout, extra_cols, g, cap_tail=0.0, reduce=False):
    """phm_info.device_bytes of the (tile, branch) engine for 2 to 4 states, as tiles_setup adds it up"""
    E, Nn = len(z["maps"]), int(z["Nnode"])
    tiles = ceil_div(S, 64)
    caps = slot_caps(z, Omega, S, max_iters, cap_tail)
    rows, klong = sum(caps), max(caps) + 1
    dcols = n + (n * n if ks_layout else n * (n - 1)) + extra_cols
    dw = 8 * tiles * rows * 64
    ms = tiles * rows * 64 if long_form(z, Omega) else 0
    pdw = 8 * tiles * E * n * 64
    gseg = 4 * tiles * ceil_div(E, g) * 64 if g > 1 else 0
    pl = 8 * tiles * Nn * n * 64
    stats = 8 * max_iters * (tiles * dcols if reduce else dcols * tiles * 64)
    red = 8 * max_iters * dcols if reduce else 0
    mcount = 2 * tiles * E * 64
    pchunk = 8 * tiles * ceil_div(E, CHUNK) * n * 64
    return 2 * dw + ms + pdw + gseg + pl + stats + red + mcount + pchunk + 8 * 3 * klong * n * n


# ---------------------------------------------------------------------------------------------------------------------------
# Every instantiation the launcher of phm_tiles.hip holds of the two kernels whose template arguments the host's classes choose,
# written out by hand from launch_tiles_sweep: tiles_branch_kernel<NS, KS, LONG> and tiles_up_cluster_kernel<NS, ASYNC>
# ---------------------------------------------------------------------------------------------------------------------------
BRANCH_KERNELS = tuple((ns, ks, lng) for ns in (2, 3, 4) for ks in (False, True) for lng in (False, True))
UP_CLUSTER_KERNELS = tuple((ns, asy) for ns in (2, 3, 4) for asy in (False, True))
assert len(BRANCH_KERNELS) == 12 and len(UP_CLUSTER_KERNELS) == 6


# ---------------------------------------------------------------------------------------------------------------------------
# models and trees
# ---------------------------------------------------------------------------------------------------------------------------
Q3 = np.array([[-.3, .2, .1], [.05, -.15, .1], [.2, .2, -.4]])             # the matrix of test_gpu_parity._problem


def model(n, variant="plain"):
    if variant == "ks":
        assert n == 4
        return synth.make2sQ(.1, .1, .2, .2, 10)
    return {2: synth.config_Q(1), 3: Q3.copy(), 4: synth.config_Q(2)}[n]


def omega_of(Q):
    return 1.25 * float(np.max(np.abs(np.diag(Q))))


def orders(z):
    return treeorder.pruningwiseedgeorder(z), treeorder.makenodelist(z), treeorder.myreorder(z)


def scaled(z, f):
    """every branch (maps, edge.length) by one common factor"""
    return dict(z, maps=[np.asarray(m, dtype=np.float64) * f for m in z["maps"]],
                **{"edge.length": np.asarray(z["edge.length"], dtype=np.float64) * f})


class Case:
    """One problem and the engine runs the GPU test makes of it.  ``groups``: the values of branch_group it runs under (0: automatic);
    ``base``: engine options common to its runs; ``runs``: the sweeps of each run() call; ``sites``: per-replica tips"""

    def __init__(self, name, purpose, Q, pid, z, variant, S, seed, groups=(1, 3, 64), runs=(1, 3), replicas=None, base=None, Omega=None,
                 sites=None):
        self.name, self.purpose, self.Q, self.pid, self.z, self.variant = name, purpose, np.asarray(Q, dtype=np.float64), pid, z, variant
        self.S, self.seed, self.groups, self.runs, self.base, self.sites = S, seed, tuple(groups), tuple(runs), dict(base or {}), sites
        self.N = sum(runs)
        self.n = self.Q.shape[0]
        self.Omega = omega_of(self.Q) if Omega is None else Omega
        self.B = np.eye(self.n) + self.Q / self.Omega
        self.nen, self.nodelist, self.root = orders(z)
        self.tiles, self.E, self.Nn = ceil_div(S, 64), len(z["edge"]), int(z["Nnode"])
        self.replicas = tuple(sorted({0, 63, 64, S - 1} & set(range(S)))) if replicas is None else tuple(replicas)
        self.length = float(np.sum(z["edge.length"]))
        self.ks_layout = variant in ("bf", "ks")
        self.ncnt = self.n * self.n if self.ks_layout else self.n * (self.n - 1)
        self.extra_cols = {"bf": 3, "ks": 2 + 3 * (self.n // 2 - 1) + 1}.get(variant, 0)
        self.long = long_form(z, self.Omega)
        for a in (self.Q, self.B):
            a.setflags(write=False)

    def group(self, forced):
        return group(self.tiles, self.E, forced)

    def clusters(self, level_groups=None):
        return clusters(self.tiles, self.Nn, False, self.base.get("level_groups", 0) if level_groups is None else level_groups)

    def branch_kernel(self):
        return (self.n, self.ks_layout, self.long)

    def up_cluster_kernel(self, level_groups=None):
        return (self.n, self.long) if self.clusters(level_groups) else None

    def bytes(self, forced=0):
        return device_bytes(self.z, self.Omega, self.n, self.S, self.N, self.ks_layout, self.extra_cols, self.group(forced),
                            self.base.get("cap_tail", 0.0), self.base.get("reduce", False))

    def oracle(self, replica, dump=False, N=None):
        z = self.z if self.sites is None else dict(self.z, states=np.asarray(self.sites[replica], dtype=np.int32))
        return O.maketreelistMCMC(z, self.Q, self.pid, self.B, self.Omega, self.nen, self.nodelist, self.root, self.N if N is None else N,
                                  variant=ORACLE_VARIANT[self.variant], seed=self.seed, replica=self.base.get("replica_offset", 0) + replica,
                                  dump=dump)

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def oracle_rows(case, replica):
    """rows [N, cols] of one replica"""
    rows, rc = case.oracle(replica)
    assert rc == 0
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def oracle_longest(case, replica):
    """the largest segment count of a branch after sweep 1"""
    _, rc, dump = case.oracle(replica, dump=True, N=1)
    assert rc == 0
    return int(dump.seg_count.max())


def _tree(n_tips, Q, seed, pid, init_segments=2, variant="plain"):
    z = synth.make_tree(n_tips, Q, omega_of(Q), seed, pid, init_segments=init_segments)
    return RC.parity_tips(z) if variant == "ks" else z


def _pid(n):
    return np.full(n, 1.0 / n)


# A. instantiation x group: seven sweeps, short and long paths ---------------------------------------------------------------
SWEEPS_A = (("plain", 2), ("plain", 3), ("plain", 4), ("bf", 2), ("bf", 3), ("bf", 4), ("ks", 4))
KINDS_A = {"short": (24, 2), "long": (12, 300)}                            # tips, init_segments: E = 46 and 22, both 1 mod 3


@functools.lru_cache(maxsize=None)
def case_a(variant, n, kind):
    tips, segs = KINDS_A[kind]
    Q = model(n, variant)
    z = _tree(tips, Q, 4100 + 10 * n + len(variant), _pid(n), segs, variant)
    return Case(f"A_{variant}{n}_{kind}", f"tiles_branch_kernel<{n}, {variant in ('bf', 'ks')}, {kind == 'long'}> at group 1, 3 (last group of one) "
                f"and 64 (one wave walks the tree)", Q, _pid(n), z, variant, 70, 1700 + n)


def cases_a():
    return [case_a(v, n, k) for v, n in SWEEPS_A for k in KINDS_A]


# B. chunks of the dwell reduction ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_b():
    z, Q, pid, Omega = synth.config_problem(1)
    return Case("B_chunks", "C1 tree, E = 198: 66 groups of 3 = 2 chunks (64 + 2), 198 groups of 1 = 4 chunks (the last of 6)", Q, pid, z,
                "bigtree", 70, 61, groups=(1, 3), Omega=Omega)


# C. the form rule at 48 | 49 caller-supplied segments, the LDS | global edge of the chain table -------------------------------
SEGMENTS_C = (25, 48, 49, 64, 65)


@functools.lru_cache(maxsize=None)
def case_c(segs):
    Q = model(4)
    z = _tree(10, Q, 4300, _pid(4), segs)
    return Case(f"C_segs{segs}", f"{segs} initial segments per branch: chain rows up to {segs - 2} of a table with {KTAB} rows in LDS, "
                f"{'LONG' if segs > 48 else 'packed'} form", Q, _pid(4), z, "bigtree", 70, 43, groups=(1, 3))


def cases_c():
    return [case_c(s) for s in SEGMENTS_C]


# The same edge under a chain that has not mixed by row 24: B = [[.02, .98], [.98, .02]] (Omega = 1.02 max|q_ii|) has the eigenvalue
# -0.96, so rows 23 and 24 of the chain table differ by 0.38 in every entry and a draw from the neighbouring row changes the path at
# once.  (Under Omega = 1.25 max|q_ii| the rows agree to 2e-4 and a wrong row goes unseen on four replicas.)  In sweep 1, 25 segments
# reach row 23 at the most, 26 row 24, the first outside LDS, and only that one, 49 the LONG form's prefetched rows; neighbouring
# segments rarely merge under this chain, so the paths grow by the virtual jumps of every sweep and later sweeps read further rows
SEGMENTS_C_SLOW = (25, 26, 49)


@functools.lru_cache(maxsize=None)
def case_c_slow(segs):
    Q = np.array([[-1.0, 1.0], [1.0, -1.0]])
    z = synth.make_tree(10, Q, 1.02, 4350, _pid(2), init_segments=segs)
    return Case(f"C_slow_segs{segs}", f"{segs} initial segments under a nearly periodic chain: chain rows up to {segs - 2}", Q, _pid(2), z,
                "bigtree", 70, 44, groups=(1, 3), Omega=1.02)


def cases_c_slow():
    return [case_c_slow(s) for s in SEGMENTS_C_SLOW]


# D. the hand-over of the 16-bit counters inside a group ---------------------------------------------------------------------
D_SEGMENTS, D_REPLICAS = 30000, (0, 5, 63, 69)


@functools.lru_cache(maxsize=None)
def case_d():
    Q = np.array([[-0.02, 0.02], [1.0, -1.0]])
    pid = np.array([.5, .5])
    z = synth.make_tree(6, Q, 1.25, 8, pid, states=np.ones(6, dtype=np.int32), init_segments=2)
    for b in np.argsort(-np.asarray(z["edge.length"]), kind="stable")[:3]:
        z["maps"][b] = np.full(D_SEGMENTS, z["edge.length"][b] / D_SEGMENTS)
        z["mapnames"][b] = np.ones(D_SEGMENTS, dtype=np.int32)
    assert all(int(m[-1]) == 1 for m in z["mapnames"])
    return Case("D_handover", "three branches of 30 000 segments in the sticky state: one lane counts more than 65 535 self pairs in sweep 1",
                Q, pid, z, "bf", 70, 23, groups=(64, 1), runs=(1, 2), replicas=D_REPLICAS, Omega=1.25)


# E. counter copies ---------------------------------------------------------------------------------------------------------
# S: copies.  9 tiles still take 64 copies (32 x 9 < 512); 33 and 129 tiles are there for 16 and 4 copies, which no other test runs
# (the suite's 1, 2 and 5 tiles take 64, 16 tiles 32, 66 tiles 8 and 256 tiles 2)
REPLICAS_E = {5: 64, 573: 64, 2085: 16, 8250: 4, 32768: 1}


@functools.lru_cache(maxsize=None)
def case_e(S):
    Q = model(4, "ks")
    z = _tree(20, Q, 4500, _pid(4), 2, "ks")
    return Case(f"E_S{S}", f"{ceil_div(S, 64)} tiles: {REPLICAS_E[S]} copies of the 16 counters, groups spread over them by grp & (copies - 1)",
                Q, _pid(4), z, "ks", S, 45, groups=(1, 3))


def cases_e():
    return [case_e(S) for S in REPLICAS_E]


# F. sweep parts x groups on an uneven tile split -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_f(n):
    Q = model(n)
    z = _tree(40, Q, 4600 + n, _pid(n))
    return Case(f"F_n{n}", "5 tiles (the last with 54 live lanes) in 1, 2 (3 + 2) and 3 (2 + 2 + 1) parts, one launch per level", Q, _pid(n), z,
                "bigtree", 310, 47, groups=(1, 3), replicas=(0, 63, 64, 255, 256, 309), base={"level_groups": 1})


PARTS_F = (1, 2, 3)


# G. per-replica tips and replica offsets with groups ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_g_sites():
    Q = model(4)
    z = synth.make_tree(30, Q, omega_of(Q), 17, _pid(4))                   # test_alignment_sites_through_the_r_level_api
    sites = np.random.default_rng(5).integers(1, 5, size=(130, 30)).astype(np.int32)
    return Case("G_sites", "130 alignment sites (tips per replica), three tiles, group 3", Q, _pid(4), z, "bigtree", 130, 9, groups=(1, 3),
                replicas=(0, 64, 129), sites=sites)


@functools.lru_cache(maxsize=None)
def case_g_offset():
    Q = model(2)
    z = _tree(24, Q, 4700, _pid(2))
    return Case("G_offset", "replica_offset = 1000: the random streams of replicas 1000 + r, group 3", Q, _pid(2), z, "bigtree", 70, 49,
                groups=(1, 3), base={"replica_offset": 1000})


# H. maps replay with groups -----------------------------------------------------------------------------------------------------
MAP_ITERS_H = (1, 3)


def cases_h():
    """the plain sweeps of family A: mcmc_maps_tiles_kernel walks the same groups over the same paths"""
    return [case_a("plain", n, k) for n in (2, 3, 4) for k in KINDS_A]


# I. capacity recovery with groups ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_i():
    Q = model(4)
    z = _tree(40, Q, 3, _pid(4))
    return Case("I_recovery", "slots provisioned far too small (cap_tail = 0.9 at six times the uniformization rate): the rebuilt engine "
                "replays in groups of 3", Q, _pid(4), z, "bigtree", 200, 51, groups=(1, 3), runs=(2, 4), base={"cap_tail": 0.9},
                Omega=6.0 * omega_of(Q))


# J. automatic classes at natural size -----------------------------------------------------------------------------------------
J_LAMBDA_MAX, J_CAP_TAIL = 0.1, 0.01


def _shrunk(z, Omega):
    """(tree, factor): every branch by the one factor that puts the longest at Omega t_b = J_LAMBDA_MAX.  With cap_tail = J_CAP_TAIL
    every branch then gets the smallest slot plan_slots gives a two-segment path of positive length (6 rows: poisson_capacity 3,
    the initial path on top, 2 spare), and a 1 + Poisson(0.1) count exceeds 6 once in 7e8 draws."""
    f = J_LAMBDA_MAX / (Omega * float(np.max(z["edge.length"])))
    return scaled(z, f), f


@functools.lru_cache(maxsize=None)
def case_j1(tips):
    """J1, the 1 | 2 edge of the automatic group: 64 tiles x 2 046 branches (1 024 tips) stay below 2 x 65 536 waves, 64 x 2 048 (1 025
    tips) reach them.  Factor 3.38e-3 (1 024 tips) and 2.61e-3 (1 025); 0.96 and 0.97 GiB."""
    Q = model(2)
    z, f = _shrunk(synth.make_tree(tips, Q, omega_of(Q), 4800 + tips, _pid(2)), omega_of(Q))
    c = Case(f"J1_tips{tips}", "4 096 replicas: automatic group " + ("1" if tips == 1024 else "2"), Q, _pid(2), z, "bigtree", 4096, 53,
             groups=(0,), replicas=(0, 63, 64, 4095), base={"cap_tail": J_CAP_TAIL})
    c.factor = f
    return c


@functools.lru_cache(maxsize=None)
def case_j2():
    """J2, the headline's class: 256 tiles (the last with 54 live lanes) x 4 198 branches -- group 16 with a last group of 6, 263 groups
    = 5 chunks (the last of 7), 2 counter copies, one launch per level, 2 parts automatically.  Factor 3.27e-3.  Every branch at the
    6-row floor of plan_slots the engine reports 9.41 GiB: lanes x branches = 2^26 at the least in this class (group 16 needs 2^20
    (tile, branch) pairs), each with 96 B of dwell rows, 32 B of partial sums, 16 B of partial likelihoods and 2 B of counts, so no
    factor or cap_tail brings this class under BYTES_CAP = 8 GiB; test_tiles_classes_cpu.py holds it to that floor instead."""
    z, Q, pid, Omega = synth.config_problem(3, n_tips=2100)
    z, f = _shrunk(z, Omega)
    c = Case("J2_headline", "16 374 replicas on 2 100 tips: group 16, 5 chunks, 2 copies, 2 parts", Q, pid, z, "bigtree", 16374, 57,
             groups=(0,), runs=(1, 2), replicas=(0, 63, 64, 16373), base={"cap_tail": J_CAP_TAIL}, Omega=Omega)
    c.factor = f
    return c


J_ROWS_FLOOR = 6                                                           # plan_slots: max(3, 2 + 3 - 1) + 2 rows, the least for m0 = 2


def all_cases():
    return (cases_a() + [case_b()] + cases_c() + cases_c_slow() + [case_d()] + cases_e() + [case_f(4), case_f(2)] + [case_g_sites(), case_g_offset()] +
            [case_i()] + [case_j1(1024), case_j1(1025), case_j2()])
