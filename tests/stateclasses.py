"""Inputs shared by the CPU and GPU tests of the state-count dispatch classes ("Dispatch classes"): the
long-branch problem, mu t_b = 800 on one branch for any n.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from phylomap_amd import synth

LONG_N = (5, 8, 9, 16, 17, 32, 33, 64)
B_LONG = 4


def long_Q(n, seed):
    """rates uniform(0.2, 1), a fifth of the entries zero, +0.05 on the cyclic superdiagonal, the largest row sum scaled to 10"""
    rs = np.random.default_rng(seed)
    Q = rs.uniform(0.2, 1.0, (n, n))
    Q[rs.random((n, n)) < 0.2] = 0.0
    idx = np.arange(n)
    Q[idx, (idx + 1) % n] += 0.05
    Q[idx, idx] = 0.0
    Q *= 10.0 / Q.sum(axis=1).max()
    Q[idx, idx] = -Q.sum(axis=1)
    return Q


def long_branch(n):
    """(edge, lens, Q, pid, tips [2, 6]): a 6-tip tree whose branch ``B_LONG`` has mu t_b = 800 > 745, so e^(-mu t) is not
    representable; two sites of random tips in 1 .. n, one tip of the second site missing"""
    edge, lens = synth.random_tree(6, 0.3, 9)
    lens = lens.copy()
    lens[B_LONG] = 80.0
    Q = long_Q(n, 0x10B0 + n)
    rs = np.random.default_rng(0x10C0 + n)
    tips = rs.integers(1, n + 1, (2, 6)).astype(np.int32)
    tips[1, 2] = 0
    return edge, lens, Q, np.arange(1.0, n + 1.0), tips
