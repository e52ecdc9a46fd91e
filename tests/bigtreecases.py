"""Inputs of the tests that push the exact one-shot calls past 65 535 tips, level steps, rows, sites and models (the limit of a
grid's y and z dimensions, at which every launcher of the family cuts its work and hands the next launch an offset):
tests/test_level_ref_cpu.py and tests/test_gpu_launch_splits.py.  TEST INFRASTRUCTURE ONLY.

``balanced(D)``: a perfectly balanced binary tree of 2^D tips in ape numbering (tips 1 .. T, the root T + 1), the tips' and the
other internal nodes' numbers dealt by a seeded permutation and the edge table shuffled.  At D = 17: 131 072 tips, 131 071 internal
nodes, 262 142 edge rows, height levels of 65 536, 32 768, ..., 1 nodes -- the smallest tree with more than 65 535 steps in one
level.  Branch lengths come from a table of 16 distinct positive values (15 of uniform(0.02, 0.6) and one long 3.0), so a reference
needs 16 matrix exponentials; exactly three edges have length 0: a tip edge, the edge into a cherry parent and an edge at mid
height, no two of them at one node.

The models are ``branchrowscases.models`` (non-symmetric, a tenth of the rates structurally zero), the tips
``branchrowscases.sites`` (uniform, a tenth missing), the 4-state observe map ``branchrowscases.parity``.  ``many_sites`` and
``many_models`` are the inputs on the 6-tip tree of ``manymodelscases``: 65 537 sites gathered from a pool of distinct tip sets and
65 537 models, the last three copies of the first three."""
import numpy as np

import branchrowscases as bc
import manymodelscases

GRID_MAX = 65535                                                              # LL_GRID_Y, AW_GRID_MAX, BR_GRID_MAX
BIG_D = 17
TABLE_LONG = 3.0
PAST = GRID_MAX + 2                                                           # 65 537 sites or models: launches of 65 535 and 2


def length_table(seed=0xB16):
    """the 16 distinct positive branch lengths"""
    t = np.append(np.random.default_rng(seed).uniform(0.02, 0.6, 15), TABLE_LONG)
    assert np.unique(t).size == 16
    return t


def balanced(D=BIG_D, seed=0xB16):
    """(z, info): the tree as the api takes it and, in ``info``, ``zero`` (the three edge rows of length 0: tip edge, edge into
    a cherry parent, edge at mid height), ``table`` (the 16 lengths) and ``root``"""
    T = 1 << D
    rs = np.random.default_rng(seed + D)
    # heap positions h = 1 .. 2T - 1: children 2h and 2h + 1, leaves T .. 2T - 1
    ids = np.zeros(2 * T, dtype=np.int64)
    ids[1] = T + 1
    ids[2:T] = T + 2 + rs.permutation(T - 2)
    ids[T:] = 1 + rs.permutation(T)
    h = np.arange(2, 2 * T)
    table = length_table(seed)
    lens = table[rs.integers(0, 16, h.size)]
    mid = D // 2
    zero_h = [T + 5, T // 2 + T // 4 + 3, (1 << mid) + (1 << mid) // 3]       # a leaf, a cherry parent, a node at depth D // 2
    assert len({x for z in zero_h for x in (z, z // 2)}) == 6                 # no node meets two of them
    lens[np.asarray(zero_h) - 2] = 0.0
    perm = rs.permutation(h.size)
    edge = np.stack([ids[h // 2], ids[h]], axis=1)[perm].astype(np.int32)
    lens = lens[perm].copy()
    where = np.empty(h.size, dtype=np.int64)
    where[perm] = np.arange(h.size)
    z = {"edge": edge, "edge.length": lens, "Nnode": T - 1, "states": np.ones(T, dtype=np.int32)}
    return z, {"zero": [int(where[x - 2]) for x in zero_h], "table": table, "root": T + 1}


def problem(n, K, S=2, D=BIG_D, seed=0):
    """(z, info, Qs [K, n, n], pid [K, n], tips [S, T], observe) on the balanced tree; parity observe at 4 states"""
    z, info = balanced(D)
    observe = bc.parity(n) if n == 4 else None
    Qs, pid = bc.models(n, K)
    tips = bc.sites(n, 1 << D, S, observe, seed=seed)
    return z, info, Qs, pid, tips, observe


def many_sites(n, S=PAST, pool=2048):
    """(sets [pool, 6], index [S]): site s has the tips sets[index[s]]; a tenth of the tips missing; the last three sites are
    the first three again.  The pool is what a reference has to be asked for"""
    rs = np.random.default_rng(0xB1700 + n)
    sets = rs.integers(1, n + 1, (pool, manymodelscases.T)).astype(np.int32)
    sets[rs.random(sets.shape) < 0.1] = 0
    index = rs.integers(0, pool, S)
    index[S - 3:] = index[:3]
    return sets, index


def many_models(n, K=PAST):
    """(Qs [K, n, n], pid [K, n]): the last three models are the first three again"""
    Qs, pid = bc.models(n, K - 3, seed=17)
    return np.concatenate([Qs, Qs[:3]]), np.concatenate([pid, pid[:3]])
