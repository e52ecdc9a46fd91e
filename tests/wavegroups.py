"""How many consecutive branches one wave item covers in the persistent kernels of the exact sampler (sm_branch_kernel, DESIGN.md
sections 19 and 20) and of the forward simulation under many models (simm_level_kernel, section 22), restated from the host code,
and the complete 32-tip tree the grouped simulation runs on.  TEST INFRASTRUCTURE ONLY.

The device does not report its group, so the three formulas are copied here and pinned by tests/test_wave_groups_cpu.py; whoever
retunes one of them gets a failing CPU test that says which GPU shapes have to move with it."""
import numpy as np

WAVES_PER_BLOCK = 4                  # SM_BLOCK / 64 (phm_sample.h) and SIMM_BLOCK / 64 (phm_simm.h)
ITEMS_PER_WAVE_TARGET = 8192         # the divisor of both group formulas
GROUP_MAX = 16
BRANCH_BLOCKS_MAX = 2048             # the launch of a flush in phm_sample_api.cpp, the chain chunk in phm_gibbs_api.cpp
LEVEL_BLOCKS_MAX = 65536             # launch_simulate_models in phm_simm.hip


# The shapes of tests/test_gpu_wave_groups.py; tests/test_wave_groups_cpu.py asserts what each of them reaches.
SAMPLE_D = 3470                      # sample_histories on the 24-tip tree: 10 evaluations x 55 tiles, the last of 14 draws;
SAMPLE_KS = {False: (5, 2), True: (10, 2)}    # (models, sites) crossed / paired by site_of_model: 10 evaluations either way
LONG_D = 160000                      # sample_histories on the 6-tip long-branch tree, 3 models: 3 x 2 500 tiles
SIM_KR = (3, 16500)                  # simulate_histories_models on complete_tree(): 49 500 histories, 774 tiles
GIBBS_CHAINS, GIBBS_SITES = 11420, 3  # posterior_rates, joint: 179 waves of chains x 3 sites, 36 idle lanes per site
CHUNK_SAMPLE, CHUNK_SIM, CHUNK_GIBBS = 64, 64, 2048      # expect_chunk of the ungrouped runs they are compared with


def group_sizes(count, group):
    """branches per item along one tile: [group, group, ..., the rest]"""
    return [min(group, count - q0) for q0 in range(0, count, group)]


def sampler_launch(n_edge, n_tiles):
    """One flush of phm_sample_histories_models (tile form) or one chunk of chains of phm_gibbs_rates (packed form).
      group          launch_sm_sample, phm_sample.hip: max(1, min(16, n_edge * n_tiles / 8192))
      branch_blocks  phm_sample_api.cpp (the launch of a flush) and phm_gibbs_api.cpp: min((n_edge * n_tiles + 3) / 4, 2048)
      items          sm_branch_kernel: ceil(n_edge / group) * n_tiles, walked with stride gridDim.x * 4"""
    group = max(1, min(GROUP_MAX, n_edge * n_tiles // ITEMS_PER_WAVE_TARGET))
    blocks = min((n_edge * n_tiles + 3) // 4, BRANCH_BLOCKS_MAX)
    sizes = group_sizes(n_edge, group)
    items = len(sizes) * n_tiles
    waves = blocks * WAVES_PER_BLOCK
    return dict(group=group, sizes=sizes, short_last=sizes[-1] < group, items=items, waves=waves, second_trip=items > waves,
                second_items=max(0, items - waves))


def tiles_of_sample(n_eval, D, expect_chunk=0):
    """tiles of the flushes of a sample_histories call whose evaluations fit one chunk of models and sites (a tile: 64 draws of
    one evaluation; sm_tiles_max of phm_sample_host.h: Tc_max = min(tiles, expect_chunk))"""
    total = n_eval * ((D + 63) // 64)
    cap = min(total, expect_chunk) if expect_chunk > 0 else total
    return [min(cap, total - t0) for t0 in range(0, total, cap)]


def tiles_of_gibbs(chains, S, expect_chunk=0):
    """tiles of the chunks of chains of a posterior_rates call with S evaluations per chain (phm_gibbs_api.cpp: Kc_max chains
    rounded up to 64 per chunk, nt = S * Kp / 64)"""
    kc_max = (chains + 63) // 64 * 64
    if expect_chunk > 0:
        kc_max = min(kc_max, (expect_chunk + 63) // 64 * 64)
    return [S * ((min(kc_max, chains - c0) + 63) // 64) for c0 in range(0, chains, kc_max)]


def level_counts(edge):
    """edges by the depth of their parent, the root's first (depth_levels, phm_sched.cpp)"""
    edge = np.asarray(edge)
    T = edge.shape[0] // 2 + 1
    parent_of = {int(c): int(p) for p, c in edge}
    depth = {T + 1: 0}

    def d(v):
        if v not in depth:
            depth[v] = d(parent_of[v]) + 1
        return depth[v]

    return np.bincount([d(int(p)) for p in edge[:, 0]]).tolist()


def simulate_launches(level_edges, n_hist, expect_chunk=0):
    """The depth-level launches of one chunk of n_hist histories of phm_simulate_histories_models.
      group   launch_simulate_models, phm_simm.hip: max(1, min(16, level_edges * n_tiles / 8192)), then min(group, expect_chunk)
      blocks  same function: min((items + 3) / 4, 65536)"""
    n_tiles = (n_hist + 63) // 64
    out = []
    for cnt in level_edges:
        group = max(1, min(GROUP_MAX, cnt * n_tiles // ITEMS_PER_WAVE_TARGET))
        if expect_chunk > 0:
            group = min(group, expect_chunk)
        sizes = group_sizes(cnt, group)
        items = len(sizes) * n_tiles
        waves = min((items + 3) // 4, LEVEL_BLOCKS_MAX) * WAVES_PER_BLOCK
        out.append(dict(edges=cnt, group=group, sizes=sizes, short_last=sizes[-1] < group, items=items, waves=waves,
                        second_trip=items > waves))
    return out


def complete_tree(levels=5, seed=32, shuffle=False):
    """The complete binary tree of 2^levels tips: levels of 2, 4, ..., 2^levels edges, the widest level a tree of its size can
    have.  Tips 1 .. T, root T + 1, internal nodes numbered and edge rows emitted in pre-order (ape's cladewise order); branch
    lengths uniform(0.05, 0.6) from ``seed``, row 5 of the pre-order set to zero; ``shuffle``: the edge rows permuted."""
    T = 1 << levels
    edges = []
    nxt = [T + 1, 1]                                       # next internal id, next tip id

    def grow(parent, depth):
        for _ in range(2):
            if depth == levels:
                child = nxt[1]
                nxt[1] += 1
                edges.append((parent, child))
            else:
                nxt[0] += 1
                child = nxt[0]
                edges.append((parent, child))
                grow(child, depth + 1)

    grow(T + 1, 1)
    edge = np.asarray(edges, dtype=np.int32)
    rng = np.random.default_rng(seed)
    lens = rng.uniform(0.05, 0.6, edge.shape[0])
    lens[5] = 0.0
    if shuffle:
        perm = rng.permutation(edge.shape[0])
        edge, lens = edge[perm], lens[perm]
    return edge, lens
