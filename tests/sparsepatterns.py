"""Inputs shared by the CPU and GPU tests of the pattern-generated sparse pruning kernel (phm_rtc.cpp; DESIGN.md section 4,
"Unstructured sparsity"): unstructured, NON-symmetric sparse rate matrices of 5 .. 32 states, the small trees they run
on, and the oracle's rows for them (computed once per session, shared, never written).  TEST INFRASTRUCTURE ONLY.

The one matrix the kernel had been run on, synth.neighbour_Q(20, 6), is symmetric in pattern and values, has 7 non-zeros in
every row and n = 20 = 5 * 4; everything here differs from its transpose, has rows of different lengths, and covers odd n, the
padding rows of NP = ceil(n/4)*4, n = 5 and n = 32, and the boundaries of the engine's own constants."""
import functools

import numpy as np

import oracle_lib as O
from phylomap_amd import _lib, synth, treeorder

# the engine's constants (phm_rtc.h, phm_wtiles.h)
RTC_SPARSE_MAX_FILL, RTC_SPARSE_NMAX, WT_MAX_SLOTS, WT_BAND_MAX = 0.5, 32, 96, 2
SPARSE_THRESHOLD = 1e-7                       # matTospmat (src/phylomap.cpp:811): the SPARSE driver's chain matrix keeps b > 1e-7

N_SWEEPS, S_REPLICAS = 5, 70                  # two tiles, the second holding 6 lanes: the smallest shape with a partial tile
REPLICAS = (0, 63, 69)                        # last lane of the full tile, first and last chain

# name -> (engine variant, oracle variant, rescaled pruning pass)
VARIANTS = {"bigtree": (_lib.PHM_MCMC_BIGTREE, O.BIGTREE, False), "plain": (_lib.PHM_MCMC, O.PLAIN, False),
            "sparse": (_lib.PHM_MCMC_SPARSE, O.SPARSE, False),
            "sparse_rescaled": (_lib.PHM_MCMC_SPARSE, O.SPARSE | O.FORCE_NORMALISE, True),
            "ks": (_lib.PHM_MCMC_KS, O.KS, False), "bf": (_lib.PHM_MCMC_BF, O.BF, False)}


def pattern_Q(n, nnz, seed, hub=False, thin=False, lone_column=False, upper=False, tiny=False):
    """A rate matrix whose B = I + Q/Omega has exactly ``nnz`` non-zeros (the n diagonal ones included).

    A directed ring over a random relabelling of the states (Q is irreducible; no ring edge has its reverse, the hub row's one
    aside), optionally a full "hub" row, a "thin" state whose row holds the diagonal and one rate, a state entered from one state
    only (``lone_column``), then random further off-diagonal entries -- never the reverse of a ring edge -- up to ``nnz``.  Rates
    U(0.02, 0.3), drawn per entry.  ``upper``: the ring is 0 -> 1 -> ... -> n-1 -> 0 and every further entry lies above the
    diagonal.  ``tiny``: every remaining off-diagonal rate is present too, U(1e-10, 1e-9), below the SPARSE driver's threshold."""
    rs = np.random.default_rng(seed)
    perm = np.arange(n) if upper else rs.permutation(n)
    M = np.zeros((n, n), dtype=bool)
    M[perm, np.roll(perm, -1)] = True
    ring = M.copy()
    closed_rows, closed_cols = [], []
    if thin:
        closed_rows.append(int(perm[1]))
    if lone_column:
        closed_cols.append(int(perm[n // 2]))
    if hub:
        h = int(perm[0])
        assert h not in closed_rows and not closed_cols
        M[h, :] = True
        M[h, h] = False
    cand = ~M & ~ring.T & ~np.eye(n, dtype=bool)
    cand[closed_rows, :] = False
    cand[:, closed_cols] = False
    if upper:
        cand &= np.triu(np.ones((n, n), dtype=bool), 1)
    need = nnz - n - int(M.sum())
    ci, cj = np.nonzero(cand)
    assert 0 <= need <= ci.size, (n, nnz, need, ci.size)
    pick = rs.permutation(ci.size)[:need]
    M[ci[pick], cj[pick]] = True
    Q = np.where(M, rs.uniform(0.02, 0.3, (n, n)), 0.0)
    if tiny:
        Q = np.where(M, Q, rs.uniform(1e-10, 1e-9, (n, n)))
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q


def omega_of(Q):
    return 1.25 * float(np.max(np.abs(np.diag(Q))))


def chain_matrices(Q, Omega=None):
    """(B, Bc): B = I + Q/Omega and the SPARSE driver's thresholded chain matrix (equal wherever no entry is 0 < b <= 1e-7)."""
    B = np.eye(Q.shape[0]) + Q / (omega_of(Q) if Omega is None else Omega)
    return B, np.where(B > SPARSE_THRESHOLD, B, 0.0)


def half_bandwidth(M):
    i, j = np.nonzero(M)
    return int(np.max(np.abs(i - j)))


def band_served(M):
    """the engine's usable(hb) rule (upload_model): the band kernels take the matrix"""
    hb, n = half_bandwidth(M), M.shape[0]
    return 1 <= hb <= WT_BAND_MAX and 2 * hb + 1 < n


def one_way_entries(M):
    """entries with M[i, j] != 0 and M[j, i] == 0: what a kernel built from the transposed pattern gets wrong"""
    return int(np.count_nonzero((M != 0) & (M.T == 0)))


def accepted(Q, over_fill=False):
    """The class every pattern here belongs to (on the thresholded chain matrix Bc): not served by the band kernels, at most
    half full (``over_fill``: one non-zero more than that), at least n one-way entries, non-symmetric values."""
    n = Q.shape[0]
    B, Bc = chain_matrices(Q)
    nz = np.count_nonzero(Bc)
    fill_ok = nz == int(RTC_SPARSE_MAX_FILL * n * n) + 1 if over_fill else nz <= RTC_SPARSE_MAX_FILL * n * n
    return (not band_served(Bc)) and fill_ok and one_way_entries(Bc) >= n and not np.array_equal(Bc, Bc.T) and \
        not np.array_equal(B, B.T) and bool(np.all(np.diag(Q) < 0))


# name -> pattern_Q arguments; the seeds are fixed, every class property below is asserted at import
CASES = {
    "ring5": dict(n=5, nnz=12, seed=0x5A01),                       # smallest n; 12 of 25 is the most that fits under half fill; NP = 8
    "odd7": dict(n=7, nnz=20, seed=0x5A02),                        # odd n: one padding row, the double2 tail of a tip row
    "pad9": dict(n=9, nnz=25, seed=0x5A03, hub=True),              # NP = 12, three padding rows; a row of 9 terms next to rows of 2
    "thin13": dict(n=13, nnz=46, seed=0x5A04, thin=True, lone_column=True),
    "odd21": dict(n=21, nnz=100, seed=0x5A05),                     # 79 possible transitions <= 96: LDS slots on, unstructured
    "slots24_96": dict(n=24, nnz=24 + 96, seed=0x5A06),            # the last pattern counted in LDS slots ...
    "slots24_97": dict(n=24, nnz=24 + 97, seed=0x5A06),            # ... and the first that is not
    "even12_parity": dict(n=12, nnz=44, seed=0x5B08),              # the ks / bf sweeps; Q[0, 1] present, Q[1, 0] not
    "top31": dict(n=31, nnz=480, seed=0x5A09, hub=True),           # odd n at the top, fill just under 0.5 (480 <= 480.5)
    "top32_half": dict(n=32, nnz=512, seed=0x5A0A, hub=True),      # exactly half full: the last pattern that gets the kernel
    "top32_over": dict(n=32, nnz=513, seed=0x5A0A, hub=True),      # one more: matrix cores
    "tri8": dict(n=8, nnz=30, seed=0x5A0B, upper=True),            # upper triangular + (n-1, 0): nearly every entry differs from the transpose
    "tiny10": dict(n=10, nnz=34, seed=0x5A0C, tiny=True),          # dense B, sparse thresholded Bc
}
GENERATED = tuple(c for c in CASES if c not in ("top32_over", "tiny10"))      # BIGTREE / PLAIN get the generated kernel


@functools.lru_cache(maxsize=None)
def case_Q(name):
    Q = pattern_Q(**CASES[name])
    Q.setflags(write=False)
    return Q


def n_tips_of(n):
    return 40 if n >= 31 else 24


def tree_for(Q, Omega, tips, seed, shuffle_seed=None):
    """(z, nen, nodelist, root): synth.make_tree with n initial segments per branch, so the ring connects state 1 to every tip
    state; ``shuffle_seed``: edge rows (and their paths) in a random order"""
    n = Q.shape[0]
    z = synth.make_tree(tips, Q, Omega, seed, np.full(n, 1.0 / n), init_segments=n)
    if shuffle_seed is not None:
        perm = np.random.default_rng(shuffle_seed).permutation(len(z["maps"]))
        z = dict(z, edge=z["edge"][perm], **{"edge.length": z["edge.length"][perm]}, maps=[z["maps"][i] for i in perm],
                 mapnames=[z["mapnames"][i] for i in perm])
    return z, treeorder.pruningwiseedgeorder(z), treeorder.makenodelist(z), treeorder.myreorder(z)


def parity_tips(z):
    """only the parity of a tip state is observed (the ks sweep), as tests/test_gpu_parity.py::test_ks_sweep_matches_oracle does"""
    T = len(z["states"])
    z = dict(z, states=((z["states"] - 1) % 2 + 1).astype(np.int32), mapnames=[m.copy() for m in z["mapnames"]])
    for b, (_, c) in enumerate(z["edge"]):
        if c <= T:
            z["mapnames"][b][-1] = z["states"][c - 1]
    return z


class Problem:
    """Q, pid, Omega, B, tree and orders of a case; ``seed``: the chains' seed"""

    def __init__(self, name, Q, tree_seed, seed, shuffle_seed=None, Omega=None):
        self.name, self.Q, self.n, self.seed = name, Q, Q.shape[0], seed
        self.Omega = omega_of(Q) if Omega is None else Omega
        self.pid = np.full(self.n, 1.0 / self.n)
        self.B, self.Bc = chain_matrices(Q, self.Omega)
        self.tips = n_tips_of(self.n)
        self.z, self.nen, self.nodelist, self.root = tree_for(Q, self.Omega, self.tips, tree_seed, shuffle_seed)
        self.zks = None
        self.length = float(self.z["edge.length"].sum())

    def tree(self, variant):
        if variant == "ks":
            if self.zks is None:
                self.zks = parity_tips(self.z)
            return self.zks
        return self.z


@functools.lru_cache(maxsize=None)
def problem(name):
    k = list(CASES).index(name)
    return Problem(name, case_Q(name), 0x5EED1000 + k, 7100 + k)


@functools.lru_cache(maxsize=None)
def site_tips(name):
    """[S_REPLICAS, tips] random per-replica tip states (the tips_per_replica runs)"""
    p = problem(name)
    a = np.random.default_rng(0x51E5 + p.n).integers(1, p.n + 1, (S_REPLICAS, p.tips)).astype(np.int32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _oracle(p, variant, replica, sites, dump):
    z = p.tree(variant)
    if sites:
        z = dict(z, states=site_tips(p.name)[replica])
    res = O.maketreelistMCMC(z, p.Q, p.pid, p.B, p.Omega, p.nen, p.nodelist, p.root, N_SWEEPS, variant=VARIANTS[variant][1],
                             seed=p.seed, replica=replica, dump=dump)
    res[0].setflags(write=False)
    return res


def oracle_rows(p, variant, replica, sites=False):
    """(rows [N_SWEEPS, cols], rc) of the CPU oracle; computed once per session"""
    return _oracle(p, variant, replica, sites, False)


def oracle_dump(p, variant, replica):
    """(rows, rc, dump) of the CPU oracle"""
    return _oracle(p, variant, replica, False, True)


def transitions(rows, n, variant):
    """per sweep: the number of real transitions (the n + n^2 layouts count self pairs too: left out)"""
    if variant in ("ks", "bf"):
        cnt = rows[:, n:n + n * n].reshape(-1, n, n)
        return cnt.sum((1, 2)) - np.trace(cnt, axis1=1, axis2=2)
    return rows[:, n:].sum(1)


@functools.lru_cache(maxsize=None)
def set_model_cycle():
    """(Q1, Q2, Q3): pad9's Q; a second 9-state pattern; a Q without a zero.  A chain state sampled under one pattern is in general
    IMPOSSIBLE under another (a branch of two segments cannot make a jump the new matrix lacks: oracle and engine both report a zero
    probability vector), and only a move to a superset of the pattern is always possible -- which no cycle can be.  So the entries
    that Q2 and Q3 add to Q1's pattern carry rates U(1e-10, 1e-9): B gets new non-zeros (another kernel for Q2, a full matrix for
    Q3) that change every partial likelihood in its low digits, while the expected number of jumps through them, over every chain
    and sweep of the test, stays below 1e-3 (asserted in tests/test_sparse_patterns_cpu.py), so the way back to Q1 stays open.  The
    rates on Q1's own pattern are redrawn (Q1 times U(0.5, 1) per entry), so Omega of Q1 serves all three."""
    Q1 = case_Q("pad9")
    n = Q1.shape[0]
    rs = np.random.default_rng(0x5A92)
    on, off = Q1 > 0, (Q1 == 0)
    extra = off & (rs.random((n, n)) < 0.15)

    def redrawn(tiny_at):
        Q = np.where(on, Q1 * rs.uniform(0.5, 1.0, (n, n)), np.where(tiny_at, rs.uniform(1e-10, 1e-9, (n, n)), 0.0))
        np.fill_diagonal(Q, 0.0)
        np.fill_diagonal(Q, -Q.sum(axis=1))
        Q.setflags(write=False)
        return Q
    Q2, Q3 = redrawn(extra), redrawn(off)
    assert 3 <= np.count_nonzero(extra) and np.count_nonzero(Q2) <= RTC_SPARSE_MAX_FILL * n * n and np.count_nonzero(Q3) == n * n
    assert not band_served(Q2) and omega_of(Q2) <= omega_of(Q1) and omega_of(Q3) <= omega_of(Q1)
    return Q1, Q2, Q3


# ---------------------------------------------------------------------------------------------------------------------------
# seeded random patterns
# ---------------------------------------------------------------------------------------------------------------------------
RANDOM_SEED = 0x5A5E
RANDOM_NS = (5, 6, 7, 9, 10, 11, 13, 17, 22, 27, 31, 32)
N_RANDOM = 12


@functools.lru_cache(maxsize=None)
def random_case(k):
    """(problem, variant, S, redraws) of random case ``k``: n drawn from RANDOM_NS without replacement over the twelve cases (every
    n once); fill uniform in [2/n + 1/n^2, 0.5], variant, replica count and edge order from the case's own generator; a pattern
    outside the class is drawn again (the count of redraws is part of the seed's determinism)"""
    n = int(np.random.default_rng(RANDOM_SEED).permutation(RANDOM_NS)[k])
    rs = np.random.default_rng([RANDOM_SEED, k])
    fill = float(rs.uniform(2.0 / n + 1.0 / (n * n), RTC_SPARSE_MAX_FILL))
    nnz = min(max(int(fill * n * n), 2 * n + 1), int(RTC_SPARSE_MAX_FILL * n * n))
    variant = ("bigtree", "plain", "sparse_rescaled")[int(rs.integers(3))]
    S = int(rs.choice([3, 70, 130]))
    shuffle = bool(rs.random() < 0.5)
    hub = bool(rs.random() < 0.25) and nnz >= 3 * n - 2
    thin = bool(rs.random() < 0.25)
    redraws = 0
    while True:
        Q = pattern_Q(n, nnz, int(rs.integers(1 << 30)), hub=hub, thin=thin)
        if accepted(Q):
            break
        redraws += 1
        assert redraws < 100
    Q.setflags(write=False)
    p = Problem(f"random{k}", Q, int(rs.integers(1 << 30)), int(rs.integers(1 << 40)), int(rs.integers(1 << 30)) if shuffle else None)
    return p, variant, S, redraws


def replicas_of(S):
    return tuple(sorted({0, min(63, S - 1), S - 1}))


# ---------------------------------------------------------------------------------------------------------------------------
# what the GPU tests compare with the oracle: (problem, variant, replicas, per-replica tips); the CPU test checks that every
# one of these is a good input before a GPU sees it
# ---------------------------------------------------------------------------------------------------------------------------
SPARSE_DRIVER_RUNS = (("tiny10", "sparse"), ("tiny10", "sparse_rescaled"), ("odd7", "sparse_rescaled"), ("odd21", "sparse_rescaled"),
                      ("tiny10", "bigtree"))
LAYOUT_RUNS = (("even12_parity", "ks"), ("even12_parity", "bf"), ("slots24_96", "bf"))      # parity tips; the n + n^2 counting layout
SITE_CASES = ("odd7", "odd21")


def compared_runs():
    runs = [(problem(c), v, REPLICAS, False) for c in GENERATED for v in ("bigtree", "plain")]
    runs += [(problem(c), v, REPLICAS, False) for c, v in SPARSE_DRIVER_RUNS]
    runs += [(problem("top32_over"), "bigtree", REPLICAS, False)]
    runs += [(problem(c), v, REPLICAS, False) for c, v in LAYOUT_RUNS]
    runs += [(problem(c), "bigtree", REPLICAS, True) for c in SITE_CASES]
    return runs


# ---------------------------------------------------------------------------------------------------------------------------
# the classes, asserted where the cases are defined (tests/test_sparse_patterns_cpu.py repeats them)
# ---------------------------------------------------------------------------------------------------------------------------
def check_case(name):
    Q = case_Q(name)
    n = Q.shape[0]
    B, Bc = chain_matrices(Q)
    assert accepted(Q, over_fill=name == "top32_over"), name
    assert np.count_nonzero(Bc) == CASES[name]["nnz"], name
    off = np.count_nonzero(B) - n
    rows = np.count_nonzero(Bc, axis=1)
    if name == "ring5":
        assert np.count_nonzero(Bc) == 12 == int(0.5 * 25) and off == 7
    if name == "pad9":
        assert rows.max() == 9 and np.count_nonzero(rows == 2) >= 4
    if name == "thin13":
        assert rows.min() == 2 and np.count_nonzero(Bc, axis=0).min() == 2
    if name == "odd21":
        assert off == 79 <= WT_MAX_SLOTS
    if name in ("slots24_96", "slots24_97"):
        assert off == (WT_MAX_SLOTS if name == "slots24_96" else WT_MAX_SLOTS + 1)
    if name == "even12_parity":
        assert Q[0, 1] != 0.0 and Q[1, 0] == 0.0 and np.count_nonzero(B) <= WT_MAX_SLOTS           # ks parameter columns divide by Q[0, 1]; the n + n^2 layout counts a == c as slots too
    if name == "top31":
        assert np.count_nonzero(Bc) == 480 == int(0.5 * 31 * 31) and rows.max() == 31
    if name == "top32_half":
        assert np.count_nonzero(Bc) == 512 == 0.5 * 32 * 32
    if name == "top32_over":
        assert np.count_nonzero(Bc) == 513
    if name == "tri8":
        assert np.count_nonzero(np.tril(Bc, -1)) == 1 and Bc[n - 1, 0] != 0 and one_way_entries(Bc) == off
    if name == "tiny10":
        assert np.count_nonzero(B) == n * n and np.all(B > 0) and np.count_nonzero(Bc) == 34
        assert np.all((B <= SPARSE_THRESHOLD) == (Bc == 0))


for _name in CASES:
    check_case(_name)
