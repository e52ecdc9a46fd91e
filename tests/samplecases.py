"""Inputs shared by the CPU and GPU tests of the exact sampler over many models.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from phylomap_amd import synth

PARITY = (1, 2, 1, 2)


def tree(n_tips=24, seed=5, long_branch=6.0, shuffle=False):
    """a random tree with one zero-length branch and one branch of length ``long_branch``; ``shuffle``: edge rows permuted (no
    longer a pre-order)"""
    edge, lens = synth.random_tree(n_tips, 0.3, seed)
    lens = lens.copy()
    lens[3] = 0.0
    if long_branch is not None:
        lens[7] = long_branch
    if shuffle:
        perm = np.random.default_rng(seed).permutation(edge.shape[0])
        edge, lens = edge[perm], lens[perm]
    return edge, lens


def as_z(edge, lens, tips):
    return {"edge": edge, "edge.length": lens, "Nnode": edge.shape[0] // 2, "states": np.asarray(tips, dtype=np.int32)}


def random_Q(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    Q = rng.uniform(0.1, 1.0, (n, n)) * scale
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q


def hidden_Q(scale=1.0):
    return synth.make2sQ(.3, .2, .4, .5, 2.0) * scale


def tips_for(edge, lens, Q, seed, observe=None, missing=0.0):
    """tips simulated under Q, seen through ``observe``, a fraction ``missing`` of them set to 0"""
    n = Q.shape[0]
    y = synth.simulate_tips(edge, lens, Q, np.full(n, 1.0 / n), seed).astype(np.int64)
    if observe is not None:
        y = np.asarray(observe)[y - 1]
    if missing > 0.0:
        rng = np.random.default_rng(seed + 1000)
        k = max(1, int(round(missing * y.size)))
        y[rng.choice(y.size, k, replace=False)] = 0
    return y.astype(np.int32)
