"""Python twin of the ancestral states per model (phm_ancestral_models).  Written from the spec, not from
phm_ancestral.hip.

* marginals: ``exactref.expected(..., nodes=True)``'s node posteriors (``marginal`` takes them from the same ``exactref.passes``
  without the branch integrals nobody asked for: the identical numbers);
* joint reconstruction: the five rules of section 21 in numpy on ``exactref``'s P (scipy ``expm``), vectorised over the sites:
  tips M = the 0/1 tip vector; edge b: w(c) = P[a, c] M_c(c), m_b(a) = max, ptr_b(a) = the smallest c attaining it; parent
  M_p = m_b0 m_b1 rescaled by a power of two; root r = pid M_root, the first maximal state; down x_c = ptr_b(x_parent).

``joint`` also returns the smallest relative decision margin (best - second best) / best over every (edge, parent state) and the
root, and ``assignment_logp`` prices ANY full assignment.  TEST INFRASTRUCTURE ONLY.
"""
import math

import numpy as np

import exactref


def marginal(edge, edge_length, Q, pid, states, observe=None, P=None):
    """(node posteriors [S, T + Nnode, n], loglik [S]): what ``exactref.expected(nodes=True)`` returns for them.  P: the
    [E, n, n] transition matrices when the caller has them already (scipy ``expm`` otherwise)."""
    r = exactref.passes(edge, edge_length, Q, pid, states, observe, P=P)
    NT = np.asarray(edge).shape[0] + 1
    n = np.asarray(Q).shape[0]
    post = np.zeros((r["loglik"].shape[0], NT, n))
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(1, NT + 1):
            ol = r["O"][k] * r["L"][k]
            post[:, k - 1] = ol / ol.sum(axis=1, keepdims=True)
    return post, r["loglik"]


def _margin(w):
    """smallest (best - second best) / best over the last axis' maxima ([..., n] -> scalar); all-zero rows do not count"""
    s = np.sort(w, axis=-1)
    best, second = s[..., -1], s[..., -2]
    ok = best > 0
    if not np.any(ok):
        return math.inf
    return float(np.min((best[ok] - second[ok]) / best[ok]))


def joint(edge, edge_length, Q, pid, states, observe=None, P=None):
    """Joint reconstruction per site.  Returns (x [S, T + Nnode] 1-based states by node id (0 where the site is impossible),
    logp [S], margin)."""
    edge = np.asarray(edge, dtype=np.int64)
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    E = edge.shape[0]
    T = E // 2 + 1
    kids, root, order = exactref._children(edge, T)
    if P is None:
        P = np.stack([exactref.expm(Q * float(t)) for t in edge_length])
    tipL = exactref.tip_vectors(states, n, observe)
    S = tipL.shape[0]
    M, sM, ptr = {}, {}, {}
    for k in range(T):
        M[k + 1], sM[k + 1] = tipL[:, k, :], np.zeros(S)
    margin = math.inf
    for b in reversed(order):                            # children before parents
        p = int(edge[b, 0])
        if p in M:
            continue
        b0, b1 = kids[p]
        c0, c1 = int(edge[b0, 1]), int(edge[b1, 1])
        if c0 not in M or c1 not in M:
            continue
        m = []
        for bb, c in ((b0, c0), (b1, c1)):
            w = P[bb][None, :, :] * M[c][:, None, :]     # [S, a, c']
            margin = min(margin, _margin(w))
            ptr[bb] = np.argmax(w, axis=2)               # the first maximal c'
            m.append(np.max(w, axis=2))
        M[p], s = exactref._rescale(m[0] * m[1])
        sM[p] = s + sM[c0] + sM[c1]
    pid = np.asarray(pid, dtype=np.float64)
    pid = pid / np.sum(pid)
    r = pid[None, :] * M[root]
    margin = min(margin, _margin(r))
    x = np.zeros((S, 2 * T - 1), dtype=np.int64)
    x[:, root - 1] = np.argmax(r, axis=1)
    best = np.max(r, axis=1)
    with np.errstate(divide="ignore"):
        logp = np.log(best) + sM[root] * math.log(2.0)
    for b in order:                                      # parents before children
        p, c = int(edge[b, 0]), int(edge[b, 1])
        x[:, c - 1] = ptr[b][np.arange(S), x[:, p - 1]]
    x = x + 1
    x[~(best > 0)] = 0
    return x, logp, margin


def assignment_logp(edge, edge_length, Q, pid, states, x, observe=None, P=None):
    """log p(states of all nodes = x, tips | Q, pid) per site for the full assignment x [S, T + Nnode] (1-based, by node id);
    -inf where a tip's state contradicts its observation (or x holds a 0)."""
    edge = np.asarray(edge, dtype=np.int64)
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    E = edge.shape[0]
    T = E // 2 + 1
    if P is None:
        P = np.stack([exactref.expm(Q * float(t)) for t in edge_length])
    x = np.atleast_2d(np.asarray(x, dtype=np.int64))
    tipL = exactref.tip_vectors(states, n, observe)
    S = tipL.shape[0]
    _, root, _ = exactref._children(edge, T)
    pid = np.asarray(pid, dtype=np.float64)
    pid = pid / np.sum(pid)
    bad = np.any(x < 1, axis=1)
    x0 = np.where(x < 1, 0, x - 1)
    with np.errstate(divide="ignore"):
        lp = np.log(pid[x0[:, root - 1]])
        for b in range(E):
            p, c = int(edge[b, 0]), int(edge[b, 1])
            lp = lp + np.log(P[b][x0[:, p - 1], x0[:, c - 1]])
        for k in range(T):
            lp = lp + np.log(tipL[np.arange(S), k, x0[:, k]])
    lp[bad] = -math.inf
    return lp


def brute_force(edge, edge_length, Q, pid, states, observe=None):
    """All n^(2T-1) assignments of ONE site by enumeration (unscaled products): (best assignment 1-based -- the first maximal one
    in the order that has the root's state slowest is not defined here, so ties must not occur --, log of the maximum,
    marginals [T + Nnode, n], log p(tips))."""
    edge = np.asarray(edge, dtype=np.int64)
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    E = edge.shape[0]
    NT = E + 1
    T = E // 2 + 1
    P = np.stack([exactref.expm(Q * float(t)) for t in edge_length])
    tipL = exactref.tip_vectors(states, n, observe)[0]
    _, root, _ = exactref._children(edge, T)
    pid = np.asarray(pid, dtype=np.float64)
    pid = pid / np.sum(pid)
    grid = np.indices((n,) * NT, dtype=np.int8).reshape(NT, -1)        # [node, assignment]
    p = pid[grid[root - 1]]
    for b in range(E):
        p = p * P[b][grid[int(edge[b, 0]) - 1], grid[int(edge[b, 1]) - 1]]
    for k in range(T):
        p = p * tipL[k][grid[k]]
    best = int(np.argmax(p))
    total = p.sum()
    marg = np.stack([np.bincount(grid[k], weights=p, minlength=n) for k in range(NT)]) / total
    return grid[:, best] + 1, math.log(p[best]), marg, math.log(total)
