"""Parametrised rate matrices for ``api.fit_ml``: a ``RateModel`` is (n states, p parameters, theta -> Q, parameter names).

Builders: ``er(n)`` (one rate), ``sym(n)`` (q_ij = q_ji), ``ard(n)`` (every off-diagonal entry its own rate, row-major order),
``index_model(index_matrix)`` (corHMM's ``rate.mat`` convention: 0 = structurally zero, c >= 1 = parameter c) and
``hidden_rates(k)`` (``synth.make2sQ``'s l01, l10, rkappas, lkappas, gammas: 2 + 3k parameters, n = 2k + 2).

Labels for ``api.expected_branch_stats_models``: ``count_labels(n, pairs)`` and ``observed_change_labels(observe)``.
"""
from __future__ import annotations

import numpy as np


class RateModel:
    """``Q(theta)`` -> [n, n] generator; ``Qs(thetas)`` -> [K, n, n] for a [K, p] array of parameter vectors.
    ``dQ_dlog(theta)`` -> [p, n, n], the derivative of the off-diagonal entries in log theta (diagonal entries: minus the row
    sums), by the chain rule where it is known exactly (index models) and by a central difference otherwise."""

    def __init__(self, n, names, q_of_theta, index=None):
        self.n = int(n)
        self.names = list(names)
        self.p = len(self.names)
        self._q = q_of_theta
        self.index = index                       # index models: [n, n] ints, 0 = zero, c = parameter c (1-based)

    def Q(self, theta):
        theta = np.asarray(theta, dtype=np.float64).reshape(-1)
        if theta.size != self.p:
            raise ValueError(f"{self.p} parameters expected")
        Q = np.array(self._q(theta), dtype=np.float64)
        np.fill_diagonal(Q, 0.0)
        np.fill_diagonal(Q, -Q.sum(axis=1))
        return Q

    def Qs(self, thetas):
        thetas = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
        if self.index is not None:               # vectorised over the models
            K = thetas.shape[0]
            table = np.concatenate([np.zeros((K, 1)), thetas], axis=1)
            Q = table[:, self.index]
            idx = np.arange(self.n)
            Q[:, idx, idx] = 0.0
            Q[:, idx, idx] = -Q.sum(axis=2)
            return Q
        return np.stack([self.Q(t) for t in thetas])

    def dQ_dlog(self, theta):
        theta = np.asarray(theta, dtype=np.float64).reshape(-1)
        out = np.zeros((self.p, self.n, self.n))
        for c in range(self.p):
            if self.index is not None:
                out[c] = np.where(self.index == c + 1, theta[c], 0.0)
            else:
                h = 1e-6
                up, dn = theta.copy(), theta.copy()
                up[c] *= np.exp(h)
                dn[c] *= np.exp(-h)
                out[c] = (self.Q(up) - self.Q(dn)) / (2 * h)
            np.fill_diagonal(out[c], 0.0)
        return out

    def score(self, theta, stats):
        """The exact score in log theta from one row of expected statistics (n dwell columns, then the off-diagonal counts row
        by row; summed over the sites of a joint fit): g_c = sum_ij dq_ij / dlog theta_c (E[N_ij] / q_ij - E[dwell_i]).  An
        entry with q_ij = 0 has E[N_ij] = 0 and contributes nothing."""
        n = self.n
        stats = np.asarray(stats, dtype=np.float64).reshape(-1)
        Q = self.Q(theta)
        dQ = self.dQ_dlog(theta)
        off = ~np.eye(n, dtype=bool)
        counts = np.zeros((n, n))
        counts[off] = stats[n:]                       # row-major over the off-diagonal entries: the column order
        live = off & (Q > 0.0)
        ratio = np.zeros((n, n))
        ratio[live] = counts[live] / Q[live]
        term = np.where(live, ratio - stats[:n, None], 0.0)
        return np.array([float(np.sum(np.where(dQ[c] != 0.0, dQ[c] * term, 0.0))) for c in range(self.p)])


def index_model(index_matrix, names=None):
    """corHMM's ``rate.mat``: an n x n integer matrix, 0 (or a negative / NA-like value) = structurally zero, c >= 1 = the c-th
    parameter; the diagonal is ignored.  Every parameter 1..p must own at least one entry."""
    idx = np.array(index_matrix, dtype=np.int64)
    if idx.ndim != 2 or idx.shape[0] != idx.shape[1]:
        raise ValueError("index matrix must be square")
    idx = np.where(idx > 0, idx, 0)
    np.fill_diagonal(idx, 0)
    p = int(idx.max())
    if p < 1 or set(np.unique(idx[idx > 0])) != set(range(1, p + 1)):
        raise ValueError("parameters must be numbered 1..p without gaps")
    names = [f"q{c}" for c in range(1, p + 1)] if names is None else list(names)
    return RateModel(idx.shape[0], names, lambda th: np.concatenate([[0.0], th])[idx], index=idx)


def er(n):
    """Equal rates: one parameter."""
    return index_model(np.ones((n, n), dtype=np.int64) - np.eye(n, dtype=np.int64), ["rate"])


def sym(n):
    """Symmetric: q_ij = q_ji, n(n-1)/2 parameters in the order (0,1), (0,2), .., (n-2,n-1)."""
    idx = np.zeros((n, n), dtype=np.int64)
    names, c = [], 0
    for i in range(n):
        for j in range(i + 1, n):
            c += 1
            idx[i, j] = idx[j, i] = c
            names.append(f"q{i}{j}")
    return index_model(idx, names)


def ard(n):
    """All rates different: n(n-1) parameters, the off-diagonal entries in row-major order."""
    idx = np.zeros((n, n), dtype=np.int64)
    names, c = [], 0
    for i in range(n):
        for j in range(n):
            if i != j:
                c += 1
                idx[i, j] = c
                names.append(f"q{i}{j}")
    return index_model(idx, names)


def hidden_rates(k):
    """``synth.make2sQ(l01, l10, rkappas, lkappas, gammas)`` with k hidden regimes: n = 2k + 2 states, 2 + 3k parameters
    (l01, l10, rkappa_1..k, lkappa_1..k, gamma_1..k).  Tips are observed up to parity: fit with ``observe = (1, 2, 1, 2, ..)``."""
    from .synth import make2sQ
    names = ["l01", "l10"] + [f"rkappa{i}" for i in range(1, k + 1)] + [f"lkappa{i}" for i in range(1, k + 1)] + \
            [f"gamma{i}" for i in range(1, k + 1)]
    return RateModel(2 * k + 2, names, lambda th: make2sQ(th[0], th[1], th[2:2 + k], th[2 + k:2 + 2 * k], th[2 + 2 * k:2 + 3 * k]))


def count_labels(n, pairs):
    """A 0/1 label for ``api.expected_branch_stats_models``: [n, n] with 1 at every (from, to) of ``pairs`` (0-based states), so
    that the labelled sum is the expected number of those transitions on a branch.  A pair (i, i) counts E[dwell_i]."""
    w = np.zeros((int(n), int(n)))
    for i, j in pairs:
        if not (0 <= int(i) < n and 0 <= int(j) < n):
            raise ValueError("pairs must name states in 0..n-1")
        w[int(i), int(j)] = 1.0
    return w


def observed_change_labels(observe):
    """One label that counts the changes between different OBSERVED classes of a hidden-state or codon model: [n, n] with 1 at
    (i, j) where ``observe[i] != observe[j]`` (a non-synonymous change when ``observe`` maps codons to amino acids; a change of the
    observed character, not of the hidden regime, in a hidden-rates model).  ``observe``: the n 1-based observations of the states,
    as given to ``api.expected_branch_stats_models``."""
    obs = np.asarray(observe, dtype=np.int64).reshape(-1)
    return (obs[:, None] != obs[None, :]).astype(np.float64)
