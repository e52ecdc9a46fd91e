"""Python twin of the posterior sampler of rates at 9..64 states (phm_gibbs_rates_wide), written from the
spec: ``gibbsref.run``'s loop of ``samplemodelsref.sample_models(draws=1, replica_offset=i)``, but with the update taken from the
chain's SUMMED statistics row in one pass over the index matrix (O(n^2) per chain instead of O(p S n^2), so 64 states stay
testable).  The Gamma draw and its stream are ``gibbsref.Stream``'s.

TEST INFRASTRUCTURE ONLY.
"""
import math

import numpy as np

import gibbsref
import samplemodelsref


def banded_index(n):
    """an index matrix of two parameters with structural zeros everywhere off the two neighbouring diagonals: i -> i + 1 is
    parameter 1, i + 1 -> i parameter 2"""
    idx = np.zeros((n, n), dtype=np.int64)
    for i in range(n - 1):
        idx[i, i + 1], idx[i + 1, i] = 1, 2
    return idx


def sum_rows(rows):
    """the rows added one after the other, first to last: the order in which the device sums a chain's sites"""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    acc = np.zeros(rows.shape[1])
    for row in rows:
        acc = acc + row
    return acc


def update(index, theta, T, prior, theta_max, seed, chain, rep):
    """One chain's Gamma update from its summed row T [n + n(n-1)]: one pass over the off-diagonal entries (i, j) in row-major
    order adds T[n + i (n-1) + (j > i ? j-1 : j)] to N_c and T[i] to W_c for c = index[i, j] >= 1; then the draws for c ascending.
    Returns (theta', rejected [p])."""
    index = np.asarray(index)
    n = index.shape[0]
    theta = np.array(theta, dtype=np.float64)
    p = theta.size
    N, W = [0.0] * p, [0.0] * p
    T = [float(v) for v in T]
    for i in range(n):
        for j in range(n):
            c = int(index[i, j])
            if i == j or c < 1:
                continue
            N[c - 1] += T[n + i * (n - 1) + (j - 1 if j > i else j)]
            W[c - 1] += T[i]
    rej = np.zeros(p, dtype=np.int64)
    for c in range(p):
        fresh = gibbsref.Stream(seed, gibbsref.ENT_RATE | c, chain, rep).gamma(float(prior[c][0]) + N[c], 1 / (float(prior[c][1]) + W[c]))
        if fresh > theta_max or not fresh > 0.0:
            rej[c] += 1
        else:
            theta[c] = fresh
    return theta, rej


def run(edge, edge_length, index, theta0, prior, theta_max, pid, sites, iters, observe=None, site_of_chain=None, thin=1, seed=0,
        replica_offset=0):
    """The whole driver: theta [rows, C, p], loglik [rows, C], stats [rows, C, cols], rejected [C, p], status [C]."""
    index = np.asarray(index)
    n = index.shape[0]
    theta = np.array(theta0, dtype=np.float64)
    Cn, p = theta.shape
    prior = np.asarray(prior, dtype=np.float64)
    if prior.ndim == 2:
        prior = np.broadcast_to(prior, (Cn,) + prior.shape)
    sites = np.atleast_2d(np.asarray(sites))
    cols = n + n * (n - 1)
    rows = -(-iters // thin)
    out_t, out_l, out_s = np.full((rows, Cn, p), np.nan), np.full((rows, Cn), np.nan), np.full((rows, Cn, cols), np.nan)
    rejected, status = np.zeros((Cn, p), dtype=np.int64), np.zeros(Cn, dtype=np.int64)
    for i in range(iters):
        Qs = np.stack([gibbsref.build_Q(index, t) for t in theta])
        r = samplemodelsref.sample_models(edge, edge_length, Qs, pid, sites, 1, observe=observe, site_of_model=site_of_chain,
                                          seed=seed, replica_offset=i + replica_offset)
        st = r["stats"][..., 0, :].reshape(Cn, -1, cols)                   # [C, S_eval, cols]
        ll = r["loglik"].reshape(Cn, -1)
        for k in range(Cn):
            tot = float(sum_rows(ll[k][:, None])[0])
            if not math.isfinite(tot):
                status[k] = 1
            if status[k]:
                continue
            T = sum_rows(st[k])
            if i % thin == 0:
                out_t[i // thin, k], out_l[i // thin, k], out_s[i // thin, k] = theta[k], tot, T
            theta[k], rej = update(index, theta[k], T, prior[k], theta_max, seed, k, i + replica_offset)
            rejected[k] += rej
    return dict(theta=out_t, loglik=out_l, stats=out_s, rejected=rejected, status=status)
