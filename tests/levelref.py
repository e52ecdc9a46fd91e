"""Plain numpy reference of the exact one-shot family on LARGE trees (DESIGN.md sections 13 and 21), vectorised over the nodes of
a level where ``exactref`` and ``ancref`` walk node by node: the up pass runs over the height levels, the down pass and the
traceback over the depth levels, the branch integrals over the edges of equal length.  Written from the specification, not from
the kernels and not from the per-node twins; tests/test_level_ref_cpu.py holds it to them on small trees.  Any binary tree given
as an ape edge table (tips 1 .. T) is served.  TEST INFRASTRUCTURE ONLY.

* P(t) = scipy ``expm(Q t)``, once per DISTINCT branch length;
* every L, O, F and M vector is rescaled by ``exactref._rescale``'s exact power of two, its base-2 exponent kept beside it;
* branch integral: the Van Loan tensor J_g[a, i, j, b] = (int_0^t P(s) E_ij P(t - s) ds)[a, b], the upper right block of
  expm([[Q, E_ij], [0, Q]] t), once per distinct length, contracted with F_b and L_c over the edges of that length;
* joint reconstruction: section 21's five rules (max-product up, first maximal state, traceback), with the smallest relative
  decision margin (best - second best) / best per site, and the price of ANY full assignment (``assignment_logp``).
"""
import math

import numpy as np
from scipy.linalg import expm

import exactref


class Tree:
    """Level structure of an edge table: ``up[h - 1]`` the internal nodes of height h with ``kid0`` / ``kid1`` their two edge rows
    (the lower row first); ``down[d - 1]`` the edge rows whose child has depth d, with ``sib`` the sibling's edge row"""

    def __init__(self, edge):
        edge = np.asarray(edge, dtype=np.int64)
        E = edge.shape[0]
        self.edge, self.E, self.T, self.NT = edge, E, E // 2 + 1, E + 1
        order = np.argsort(edge[:, 0], kind="stable")
        b0, b1 = order[0::2], order[1::2]
        assert np.array_equal(edge[b0, 0], edge[b1, 0]), "every internal node needs two children"
        self.kid0 = np.full(self.NT + 1, -1, dtype=np.int64)
        self.kid1 = np.full(self.NT + 1, -1, dtype=np.int64)
        self.kid0[edge[b0, 0]], self.kid1[edge[b1, 0]] = b0, b1
        self.sib = np.empty(E, dtype=np.int64)
        self.sib[b0], self.sib[b1] = b1, b0
        is_child = np.zeros(self.NT + 1, dtype=bool)
        is_child[edge[:, 1]] = True
        roots = np.flatnonzero(~is_child[1:]) + 1
        assert roots.size == 1 and roots[0] > self.T
        self.root = int(roots[0])
        self.down = []
        front = np.array([self.root])
        while True:
            front = front[front > self.T]
            if front.size == 0:
                break
            rows = np.concatenate([self.kid0[front], self.kid1[front]])
            self.down.append(rows)
            front = edge[rows, 1]
        assert sum(r.size for r in self.down) == E
        height = np.zeros(self.NT + 1, dtype=np.int64)
        for rows in reversed(self.down):
            np.maximum.at(height, edge[rows, 0], height[edge[rows, 1]] + 1)
        self.height = height
        self.up = [np.flatnonzero(height == h) for h in range(1, int(height.max()) + 1)]


def _classes(Q, lens):
    """(P [G, n, n], g [E]): P(t) of every distinct length and each edge's class"""
    uniq, g = np.unique(np.asarray(lens, dtype=np.float64), return_inverse=True)
    return np.stack([expm(Q * float(t)) for t in uniq]), g.reshape(-1), uniq


def _van_loan(Q, t):
    """J[a, i, j, b] of one length"""
    n = Q.shape[0]
    J = np.zeros((n, n, n, n))
    if t == 0.0:
        return J
    big = np.zeros((2 * n, 2 * n))
    big[:n, :n] = Q
    big[n:, n:] = Q
    for i in range(n):
        for j in range(n):
            big[:n, n:] = 0.0
            big[i, n + j] = 1.0
            J[:, i, j, :] = expm(big * t)[:n, n:]
    return J


def _apply(P, v):
    """P [k, n, n] on v [k, S, n] -> [k, S, n]: sum_j P[a, j] v[j]"""
    return np.einsum("kij,ksj->ksi", P, v)


def _pid(pid):
    pid = np.asarray(pid, dtype=np.float64)
    return pid / np.sum(pid)


def expected(edge, edge_length, Q, pid, states, observe=None, per_branch=True, nodes=True, block=8192):
    """dict: loglik [S]; with ``nodes`` post [S, NT, n]; with ``per_branch`` branch [S, E, n + n(n-1)] in ``exactref.expected``'s
    columns and stats [S, cols] (the rows added by numpy over the edge axis)"""
    tr = edge if isinstance(edge, Tree) else Tree(edge)
    e = tr.edge
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    P, g, uniq = _classes(Q, edge_length)
    tipL = exactref.tip_vectors(states, n, observe)                          # [S, T, n]
    S = tipL.shape[0]
    L = np.zeros((tr.NT + 1, S, n))
    sL = np.zeros((tr.NT + 1, S))
    L[1:tr.T + 1] = tipL.transpose(1, 0, 2)
    for p in tr.up:
        b0, b1 = tr.kid0[p], tr.kid1[p]
        v = _apply(P[g[b0]], L[e[b0, 1]]) * _apply(P[g[b1]], L[e[b1, 1]])
        L[p], s = exactref._rescale(v)
        sL[p] = s + sL[e[b0, 1]] + sL[e[b1, 1]]
    pid = _pid(pid)
    lam = L[tr.root] @ pid
    with np.errstate(divide="ignore"):
        out = {"loglik": np.log(lam) + sL[tr.root] * math.log(2.0)}
    if not (per_branch or nodes):
        return out
    O = np.zeros_like(L)
    sO = np.zeros_like(sL)
    F = np.zeros((tr.E, S, n))
    sF = np.zeros((tr.E, S))
    O[tr.root] = pid
    for b in tr.down:
        p, c, sb = e[b, 0], e[b, 1], tr.sib[b]
        cs = e[sb, 1]
        F[b], s = exactref._rescale(O[p] * _apply(P[g[sb]], L[cs]))
        sF[b] = s + sO[p] + sL[cs]
        O[c], s = exactref._rescale(np.einsum("kji,ksj->ksi", P[g[b]], F[b]))
        sO[c] = s + sF[b]
    if nodes:
        ol = O[1:] * L[1:]
        with np.errstate(divide="ignore", invalid="ignore"):
            out["post"] = (ol / ol.sum(axis=2, keepdims=True)).transpose(1, 0, 2)
    if per_branch:
        pairs = exactref.columns(n)
        ii = np.arange(n)
        pi, pj = np.array([i for i, _ in pairs]), np.array([j for _, j in pairs])
        qcol = Q[pi, pj]
        branch = np.zeros((S, tr.E, n + len(pairs)))
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            inv_lam = 1.0 / lam
        for k, t in enumerate(uniq):
            J = _van_loan(Q, float(t)).reshape(n, n * n * n)
            rows = np.flatnonzero(g == k)
            for r0 in range(0, rows.size, block):
                b = rows[r0:r0 + block]
                c = e[b, 1]
                FJ = (F[b].reshape(-1, n) @ J).reshape(b.size, S, n, n, n)    # [b, S, i, j, b']
                I = np.einsum("esijb,esb->esij", FJ, L[c])
                f = np.ldexp(inv_lam[None, :], (sF[b] + sL[c] - sL[tr.root][None, :]).astype(np.int64))   # [b, S]
                branch[:, b, :n] = (I[:, :, ii, ii] * f[:, :, None]).transpose(1, 0, 2)
                branch[:, b, n:] = (I[:, :, pi, pj] * qcol[None, None, :] * f[:, :, None]).transpose(1, 0, 2)
        out["branch"] = branch
        out["stats"] = branch.sum(axis=1)
    return out


def _margin(w):
    """smallest (best - second best) / best over the last axis' maxima, per site: w [k, S, ..., n] -> [S]; all-zero rows do not
    count"""
    s = np.sort(w, axis=-1)
    best, second = s[..., -1], s[..., -2]
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.where(best > 0, (best - second) / best, np.inf)
    m = np.moveaxis(m, 1, 0)
    return m.reshape(m.shape[0], -1).min(axis=1)


def joint(edge, edge_length, Q, pid, states, observe=None):
    """Joint reconstruction per site: (x [S, NT] 1-based states by node id, 0 where the site is impossible; logp [S]; margin [S])"""
    tr = edge if isinstance(edge, Tree) else Tree(edge)
    e = tr.edge
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    P, g, _ = _classes(Q, edge_length)
    tipL = exactref.tip_vectors(states, n, observe)
    S = tipL.shape[0]
    M = np.zeros((tr.NT + 1, S, n))
    sM = np.zeros((tr.NT + 1, S))
    M[1:tr.T + 1] = tipL.transpose(1, 0, 2)
    ptr = np.zeros((tr.E, S, n), dtype=np.int8)
    margin = np.full(S, np.inf)
    for p in tr.up:
        m = []
        for b in (tr.kid0[p], tr.kid1[p]):
            w = P[g[b]][:, None, :, :] * M[e[b, 1]][:, :, None, :]            # [k, S, a, c']
            margin = np.minimum(margin, _margin(w))
            ptr[b] = np.argmax(w, axis=3)                                    # the first maximal c'
            m.append(np.max(w, axis=3))
        M[p], s = exactref._rescale(m[0] * m[1])
        sM[p] = s + sM[e[tr.kid0[p], 1]] + sM[e[tr.kid1[p], 1]]
    r = _pid(pid)[None, :] * M[tr.root]                                      # [S, n]
    margin = np.minimum(margin, _margin(r[None]))
    best = r.max(axis=1)
    with np.errstate(divide="ignore"):
        logp = np.log(best) + sM[tr.root] * math.log(2.0)
    x = np.zeros((tr.NT + 1, S), dtype=np.int64)
    x[tr.root] = np.argmax(r, axis=1)
    site = np.arange(S)[None, :]
    for b in tr.down:
        x[e[b, 1]] = ptr[b[:, None], site, x[e[b, 0]]]
    x = x[1:].T + 1
    x[~(best > 0)] = 0
    return x, logp, margin


def assignment_logp(edge, edge_length, Q, pid, states, x, observe=None):
    """log p(states of all nodes = x, tips | Q, pid) per site for the full assignment x [S, NT] (1-based, by node id); -inf where
    a tip's state contradicts its observation or x holds a 0.  The edges' terms are added pairwise by ``np.sum``"""
    tr = edge if isinstance(edge, Tree) else Tree(edge)
    e = tr.edge
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    P, g, _ = _classes(Q, edge_length)
    x = np.atleast_2d(np.asarray(x, dtype=np.int64))
    tipL = exactref.tip_vectors(states, n, observe)
    S = tipL.shape[0]
    bad = np.any(x < 1, axis=1)
    x0 = np.where(x < 1, 0, x - 1)
    with np.errstate(divide="ignore"):
        lp = np.log(_pid(pid)[x0[:, tr.root - 1]])
        lp = lp + np.log(P[g[None, :], x0[:, e[:, 0] - 1], x0[:, e[:, 1] - 1]]).sum(axis=1)
        lp = lp + np.log(tipL[np.arange(S)[:, None], np.arange(tr.T)[None, :], x0[:, :tr.T]]).sum(axis=1)
    lp[bad] = -math.inf
    return lp
