"""Inputs and plain-numpy restatements shared by the CPU and GPU tests of the per-branch expectations under many rate matrices
(phm_expected_branch_stats_models).  TEST INFRASTRUCTURE ONLY.

Trees: a 40-tip random tree, E = 78 (four full runs of 16 edge rows and a ragged run of 14), its rows shuffled and one branch of
length 0; and the 6-tip tree of ``manymodelscases``, E = 10 (a single ragged run).  Models: random non-symmetric rate matrices
with a tenth of the entries structurally zero, the rates of model k multiplied by a log-normal factor.  Sites: random tips that
``observe`` can show, a few of them missing.

``sum_in_run_order`` and ``label_reduce`` are the two documented orders of addition, in plain double arithmetic."""
import numpy as np

import exactref
import manymodelscases
from phylomap_amd import synth

SC_RUN = 16                                                                   # phm_scores.h
ZERO_EDGE = 29                                                                # the 40-tip tree's branch of length 0
EDGE_LIST = [77, 0, 16, 15, 16, 31, 32]                                       # out of order, a repeat, both sides of two run edges


def tree40():
    edge, lens = synth.random_tree(40, 0.5, 0xB27)
    perm = np.random.default_rng(0xB27).permutation(edge.shape[0])
    edge, lens = edge[perm], lens[perm].copy()
    lens[ZERO_EDGE] = 0.0
    assert edge.shape[0] == 78
    return {"edge": edge, "edge.length": lens, "Nnode": 39, "states": np.ones(40, dtype=np.int32)}


def tree6():
    return manymodelscases.z_of()


def parity(n):
    """the observe map that shows a state up to parity"""
    return (np.arange(n) % 2 + 1).astype(np.int32)


def models(n, K, seed=0):
    """(Qs [K, n, n], pid [K, n]): the rates of model k spread log-normally around a common scale"""
    rs = np.random.default_rng(0xB2700 + 100 * n + seed)
    Qs = rs.uniform(0.05, 1.0, (K, n, n)) * min(1.0, 4.0 / n)
    Qs[rs.random((K, n, n)) < 0.1] = 0.0
    idx = np.arange(n)
    Qs[:, idx, (idx + 1) % n] += 0.05 * min(1.0, 4.0 / n)                     # never a whole row of zeros
    Qs *= np.exp(rs.normal(0.0, 0.5, K))[:, None, None]
    Qs[:, idx, idx] = 0.0
    Qs[:, idx, idx] = -Qs.sum(axis=2)
    return Qs, rs.uniform(0.2, 1.0, (K, n))


def sites(n, T, S=3, observe=None, seed=0, missing=0.1):
    """S tip sets of what ``observe`` can show (1..n without it), a few tips missing (0)"""
    rs = np.random.default_rng(0xB2800 + 100 * n + T + seed)
    true = rs.integers(0, n, (S, T))
    tips = (true + 1 if observe is None else np.asarray(observe)[true]).astype(np.int32)
    tips[rs.random(tips.shape) < missing] = 0
    return tips


def owner(K, S):
    """a site_of_model that names every site, in no order"""
    return ((np.arange(K) * 5 + 1) % S).astype(np.int32)


def weights(n, labels):
    """[L, n + n(n-1)] weights of [L, n, n] labels in natural (from, to) orientation, in ``expected_sumstat``'s column order:
    (i, i) weighs E[dwell_i], (i, j) weighs E[N_ij]"""
    labels = np.asarray(labels, dtype=np.float64)
    if labels.ndim == 2:
        labels = labels[None]
    idx = np.arange(n)
    return np.concatenate([labels[:, idx, idx], np.stack([labels[:, i, j] for i, j in exactref.columns(n)], axis=1)], axis=1)


def sum_in_run_order(rows):
    """[..., E, C] rows by edge row -> [..., C] totals in the documented order: per run of 16 edge rows acc = 0.0, then every row
    added in edge order; then tot = 0.0, then every run's total added in run order"""
    rows = np.asarray(rows, dtype=np.float64)
    E = rows.shape[-2]
    tot = np.zeros(rows.shape[:-2] + rows.shape[-1:])
    for r0 in range(0, E, SC_RUN):
        acc = np.zeros_like(tot)
        for b in range(r0, min(E, r0 + SC_RUN)):
            acc = acc + rows[..., b, :]
        tot = tot + acc
    return tot


def label_reduce(rows, labels):
    """[..., C] full rows and [L, n, n] labels -> [..., L]: acc = 0.0; for col in 0 .. C - 1: acc = acc + w[col] * row[col], the
    product and the sum rounded separately"""
    rows = np.asarray(rows, dtype=np.float64)
    C = rows.shape[-1]
    n = int(round(C ** 0.5))
    w = weights(n, labels)
    acc = np.zeros(rows.shape[:-1] + (w.shape[0],))
    with np.errstate(invalid="ignore"):
        for col in range(C):
            acc = acc + w[:, col] * rows[..., col, None]
    return acc


def twin(z, Qs, pid, tips, observe=None):
    """exactref.expected(per_branch=True) per model, cross: (branch [K, S, E, C], loglik [K, S]); an impossible evaluation is
    -inf.  ``pid``: [n] shared or [K, n]"""
    pid = np.atleast_2d(np.asarray(pid, dtype=np.float64))
    br, ll = [], []
    for k in range(len(Qs)):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            _, l, b = exactref.expected(z["edge"], z["edge.length"], Qs[k], pid[k if pid.shape[0] > 1 else 0], tips, observe,
                                        per_branch=True)
        br.append(b)
        ll.append(np.where(np.isfinite(l), l, -np.inf))
    return np.array(br), np.array(ll)
