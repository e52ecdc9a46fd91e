"""The classes of the matrix-exponential path (phm_exp.hip: the sumstatEXP sampler in its two mappings, the four transition-matrix
kernels): the host's choices restated from phm_expm_api.cpp / phm_exp.hip, and the cases of tests/test_gpu_exp_classes.py.
TEST INFRASTRUCTURE ONLY.

The device reports neither its group nor its grid, so the formulas are copied here and pinned by tests/test_exp_classes_cpu.py,
which also asserts of every case the property that makes it a case.  No oracle result is computed here."""
import math

import numpy as np

from phylomap_amd import synth

EXP_BLOCK = 256                      # phm_exp.h
WAVES_PER_BLOCK = EXP_BLOCK // 64
ITEMS_PER_WAVE_TARGET = 8192         # launch_exp_tiles: group = clamp(E * tiles / 8192, 1, 16)
GROUP_MAX = 16
BRANCH_BLOCKS_MAX = 2048             # exp_one_device: branch_blocks = min((E * tiles + 3) / 4, 2048)
EXP_KL = 12                          # jump times per lane kept in LDS (phm_exp.hip); more: the wave's global scratch rows
UNIF_CAP = 300                       # newunifSample's cap (phm_exp.h)
EIGEN_N_MAX, PADE_N_MAX = 256, 128   # phm_expm_eigen / phm_expm_pade refuse more
EIGEN_MFMA_GRID, PADE_MFMA_GRID = 2048, 1024
MAPS_OFF, MAPS_COUNT, MAPS_WRITE = 0, 1, 2      # phm_maps.h; a maps=True call is a sizing call (count) and a filling call (write)


# ---- the sampler's launch ------------------------------------------------------------------------------------------------------

def tiles_of(N):
    return (N + 63) // 64


def group_sizes(count, group):
    """branches per item along one tile: [group, group, ..., the rest]"""
    return [min(group, count - q0) for q0 in range(0, count, group)]


def branch_launch(n_edge, N):
    """exp_tiles_branch_kernel of one sumstatEXP call on one device:
      group          launch_exp_tiles: max(1, min(16, n_edge * tiles / 8192))
      branch_blocks  exp_one_device: min((n_edge * tiles + 3) / 4, 2048), four waves each
      items          ceil(n_edge / group) * tiles, walked with stride gridDim.x * 4"""
    tiles = tiles_of(N)
    group = max(1, min(GROUP_MAX, n_edge * tiles // ITEMS_PER_WAVE_TARGET))
    blocks = min((n_edge * tiles + 3) // 4, BRANCH_BLOCKS_MAX)
    sizes = group_sizes(n_edge, group)
    items = len(sizes) * tiles
    waves = blocks * WAVES_PER_BLOCK
    return dict(tiles=tiles, group=group, blocks=blocks, sizes=sizes, short_last=sizes[-1] < group, items=items, waves=waves,
                second_trip=items > waves, second_items=max(0, items - waves))


def smallest_N(n_edge, group):
    """the smallest sample count whose launch has ``group`` branches per item: one lane into the first tile count that does"""
    tiles = -(-group * ITEMS_PER_WAVE_TARGET // n_edge)
    return (tiles - 1) * 64 + 1


def branch_form(n, maps):
    """(NS, modes) of exp_tiles_branch_kernel<NS, MODE> (with_producer_form): 2..4 states compiled in, more at run time"""
    return (n if n <= 4 else 0), ((MAPS_COUNT, MAPS_WRITE) if maps else (MAPS_OFF,))


def replica_form(n):
    """the kernel of the replicas mapping"""
    return f"exp_sample_kernel<{n}>" if n <= 4 else "exp_wide_kernel"


# ---- the transition-matrix kernels ---------------------------------------------------------------------------------------------

def eigen_mpb(n):
    """matrices per workgroup of expm_eigen_kernel: 256 / n^2, at least one"""
    return max(1, EXP_BLOCK // (n * n))


def eigen_grid(n, n_t):
    mpb = eigen_mpb(n)
    return (n_t + mpb - 1) // mpb


def eigen_batches(n):
    """n_t on either side of every edge of the workgroup's share"""
    mpb = eigen_mpb(n)
    return sorted({1, mpb - 1, mpb, mpb + 1, 2 * mpb + 1} - {0}) if mpb > 1 else [1, 3]


def mfma_grid(route, n_t):
    """grid of expm_eigen_mfma_kernel / expm_pade_mfma_kernel: workgroup b takes matrices b, b + grid, ..."""
    return min(n_t, EIGEN_MFMA_GRID if route == "eigen" else PADE_MFMA_GRID)


def pade_squarings(Q, t):
    """pade_squarings (phm_internal.h), arma::expmat's choice: exponent(log2 ||Q t||_inf) + 1, at least 0"""
    norm = float(np.max(np.sum(np.abs(np.asarray(Q) * t), axis=1)))
    l2 = math.log2(norm) if norm > 0.0 else 0.0
    return max(0, math.frexp(l2)[1] + 1)


# ---- models and trees ----------------------------------------------------------------------------------------------------------

def symmetric(Q):
    Q = (Q + Q.T) / 2
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(1))
    return Q


def model(n):
    """a rate matrix with a real spectrum: C1's, a symmetric 3-state one, C2's hidden-rates one, symmetric dense beyond"""
    if n == 2:
        return synth.config_Q(1)
    if n == 3:
        return symmetric(np.array([[-.3, .2, .1], [.05, -.15, .1], [.2, .2, -.4]]))
    if n == 4:
        return synth.config_Q(2)
    return symmetric(synth.dense_Q(n, 0.005, 0.03, seed=n))


def pade_model(n):
    """the Pade route needs no real spectrum: unsymmetric"""
    if n == 3:
        return np.array([[-.3, .2, .1], [.05, -.15, .1], [.2, .2, -.4]])
    return synth.dense_Q(n, 0.005, 0.03, seed=1000 + n)


def rate_of(Q):
    return float(np.max(np.abs(np.diag(Q))))


def problem(n, tips, seed):
    Q = model(n)
    pid = np.full(n, 1.0 / n)
    return synth.make_tree(tips, Q, 1.25 * rate_of(Q), seed, pid), Q, pid


def with_edge_lengths(z, lens):
    """``z`` with new edge lengths and initial paths of those lengths (two halves, the tip state at the end of a tip branch), so
    that the tree still validates; the sampler itself reads the lengths and the tip states only"""
    lens = np.asarray(lens, dtype=np.float64)
    edge = np.asarray(z["edge"])
    T = len(z["states"])
    out = dict(z)
    out["edge.length"] = lens
    paths = [synth.initial_path(float(lens[r]), int(z["states"][edge[r, 1] - 1]) if edge[r, 1] <= T else 1, 2) for r in range(edge.shape[0])]
    out["maps"] = [p[0] for p in paths]
    out["mapnames"] = [p[1] for p in paths]
    return out


def fx_exp(z):
    """binary exponent of max(tree length, 1) (exp_prepare): a segment is rounded to the nearest multiple of 2^(fx_exp - 61)"""
    return math.frexp(max(float(np.sum(z["edge.length"])), 1.0))[1]


def tiles_atol(out, z, n):
    """the absolute term of the tiles mapping's dwell bar, per sample: its segments (jumps + edges) half a fixed-point unit each"""
    segments = out[:, n:].sum(1) + len(z["edge.length"])
    return segments * 2.0 ** (fx_exp(z) - 62)


# ---- 1, 2: state counts and sample counts ---------------------------------------------------------------------------------------
STATE_COUNTS = (3, 6, 33, 64)        # exp_sample_kernel<3>; the run-time forms at 6, between 21 and 60, and a full wave of rows
STATE_N = 150
SAMPLE_COUNTS = (1, 64, 65, 257)     # one sample; exactly one tile; one lane into a second tile; a second workgroup
SAMPLE_STATES = (3, 6)
SAMPLE_MAPS_N = (1, 65)


def state_case(n):
    return problem(n, 12, 900 + n)


# ---- 3, 4: branch groups --------------------------------------------------------------------------------------------------------
# name -> (states, tree, group, N; None: the smallest N with that group)
GROUP_CASES = {
    "n2_pairs": (2, "c1", 2, 5312),          # 83 tiles: 99 full groups
    "n3_pairs": (3, "t40", 2, 13504),        # 211 tiles
    "n4_fives": (4, "t40", 5, None),         # 78 = 15 x 5 + 3: a short last group, and 16 items per tile on 8 192 waves
    "n6_fives": (6, "t40", 5, None),         # the same for the run-time form
    "n2_cap": (2, "c1", 16, 42368),          # 662 tiles: the cap; 198 = 12 x 16 + 6
}
GROUP_MAPS_CASES = ("n2_pairs", "n3_pairs", "n4_fives", "n6_fives")      # again with maps at the smallest N with group >= 2


def group_tree(n, tree):
    if tree == "c1":
        z, Q, pid, _ = synth.config_problem(1)
        return z, Q, pid
    return problem(n, 40, 0x40 + n)


def group_case(name, maps=False):
    """(z, Q, pid, N)"""
    n, tree, group, N = GROUP_CASES[name]
    z, Q, pid = group_tree(n, tree)
    E = len(z["edge.length"])
    if maps:
        N = smallest_N(E, 2)
    elif N is None:
        N = smallest_N(E, group)
    return z, Q, pid, N


# ---- 5, 6: long branches, the heavy branch and the cap ---------------------------------------------------------------------------
LONG_STATES = (3, 6, 64)
LONG_RT_INNER = (0.0, 0.3, 2.0, 10.0, 13.0, 25.0)                 # rate * t of the six internal edges, in row order
LONG_RT_TIPS = (0.05, 1.0, 3.0, 6.0, 12.0, 16.0, 40.0)            # and of the tip edges but the last, which is the heavy one
HEAVY_RT, CAP_RT = 230.0, 400.0
BRINK_RT, BRINK_SEED = 300.0, 1004   # one sample whose draw on the heavy branch takes exactly UNIF_CAP jumps: the last legal row of the table
LONG_TREE_SEED = 3
HEAVY_JUMPS = 200
LONG_TWIN_N = 64


def long_N(n):
    return 256 if n == 3 else 128


def long_case(n, heavy=HEAVY_RT):
    """(z, Q, pid, heavy edge row): 8 tips, 14 edges, rate * t from 0 (an internal edge) to ``heavy`` (the last tip edge)"""
    Q = model(n)
    pid = np.full(n, 1.0 / n)
    z = synth.make_tree(8, Q, 9.0, LONG_TREE_SEED, pid)
    edge = np.asarray(z["edge"])
    inner = [r for r in range(14) if edge[r, 1] > 8]
    tip = [r for r in range(14) if edge[r, 1] <= 8]
    rt = np.zeros(14)
    rt[inner] = LONG_RT_INNER
    rt[tip] = LONG_RT_TIPS + (heavy,)
    return with_edge_lengths(z, rt / rate_of(Q)), Q, pid, tip[-1]


# ---- a node draw on the boundary of its running sum -----------------------------------------------------------------------------
# The node draw takes the first state j with u * total <= w_0 + ... + w_j.  Equality has probability 2^-52 per draw unless the
# weights have few bits: on a 600-tip ladder with every tip in state 3 and this branch length the unscaled pruning pass leaves the
# root's row at a few dozen units of the smallest denormal, so that u * total rounds onto a running sum in one sample of ten.
TIE_STATES, TIE_TIPS, TIE_STATE, TIE_RT, TIE_N = 6, 600, 3, 0.7712060585836085, 256


def ladder_case(n=TIE_STATES, tips=TIE_TIPS, rt=TIE_RT, state=TIE_STATE):
    """(z, Q, pid): the caterpillar (internal node k hangs tip k and node k + 1), every edge of length rt / rate"""
    Q = model(n)
    edges = []
    for k in range(tips - 1):
        node = tips + 1 + k
        edges.append((node, k + 1))
        edges.append((node, node + 1) if k < tips - 2 else (node, tips))
    z = {"edge": np.asarray(edges, dtype=np.int32), "Nnode": tips - 1, "states": np.full(tips, state, dtype=np.int32)}
    return with_edge_lengths(z, np.full(len(edges), rt / rate_of(Q))), Q, np.full(n, 1.0 / n)


# ---- 7, 8: the transition-matrix kernels ------------------------------------------------------------------------------------------
EIGEN_STATES = (3, 5, 11, 15, 16, 65, 128, 256)
PADE_STATES = (3, 5, 65, 96, 128)
MFMA_STATES = (17, 64)
MFMA_BATCH = {"eigen": EIGEN_MFMA_GRID + 5, "pade": PADE_MFMA_GRID + 6}


def eigen_times(n, n_t):
    """0 and 1e-6 wherever the batch has room for them"""
    pool = np.concatenate([[0.0, 1e-6], np.random.default_rng(n).exponential(3.0, max(n_t, 2))])
    return pool[2:3] if n_t == 1 else pool[:n_t]


def pade_times(Q):
    """no time, a norm of 1.2 (no squaring), 1e-6 (the exponent of log2 of a small norm: six squarings), ordinary ones, 200"""
    norm = float(np.max(np.sum(np.abs(Q), axis=1)))
    return np.array([0.0, 1.2 / norm, 1e-6, 0.4, 3.0, 200.0])


def mfma_times(route, n):
    """a batch that gives the first workgroups a second matrix; the special times are the first matrices and the second ones"""
    grid = EIGEN_MFMA_GRID if route == "eigen" else PADE_MFMA_GRID
    t = np.random.default_rng(n).exponential(3.0, MFMA_BATCH[route])
    special = [0.0, 1e-6] + ([200.0] if route == "pade" else [])
    t[:len(special)] = special
    t[grid:grid + len(special)] = special
    return t


# ---- coverage: every template instantiation and both mappings by a named case ------------------------------------------------------
def covered_forms():
    """{(NS, MODE): case name} over the group cases, plain and with maps"""
    out = {}
    for name in GROUP_CASES:
        ns, modes = branch_form(GROUP_CASES[name][0], False)
        out.setdefault((ns, modes[0]), name)
    for name in GROUP_MAPS_CASES:
        ns, modes = branch_form(GROUP_CASES[name][0], True)
        for m in modes:
            out.setdefault((ns, m), name + "+maps")
    return out
