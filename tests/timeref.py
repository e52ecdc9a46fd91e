"""Python twin of the exact expectations through time (phm_expected_through_time): the state posterior at
points inside branches, the expected lineages in each state at depth boundaries, and E[dwell_i], E[N_ij] per depth bin.  Written
from the spec on top of ``exactref.passes`` (exactref itself is not changed): P(s) from scipy.linalg.expm, sub-branch integrals by
``exactref.integral_unif`` or, as a second route, ``exactref.integral_vanloan``.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
from scipy.linalg import expm

import exactref


def depths(edge, edge_length):
    """[T + Nnode] depth by ape node id - 1: d(root) = 0, d(child) = d(parent) + t_b (one addition per node: any parent-first
    order gives these bits)"""
    edge = np.asarray(edge, dtype=np.int64)
    E = edge.shape[0]
    _, root, order = exactref._children(edge, E // 2 + 1)
    d = np.zeros(E + 1)
    for b in order:
        d[edge[b, 1] - 1] = d[edge[b, 0] - 1] + float(edge_length[b])
    return d


def _ends(edge, edge_length):
    edge = np.asarray(edge, dtype=np.int64)
    d = depths(edge, edge_length)
    return d[edge[:, 0] - 1], d[edge[:, 1] - 1], np.asarray(edge_length, dtype=np.float64)


def crossings(edge, edge_length, bounds):
    """[(k, b, s)] by boundary, then edge row: branch b counts at tau_k when d_p < tau <= d_c, at s = tau - d_p (t_b when
    tau >= d_c); tau = 0 adds (k, lowest root branch row, 0), the root as one lineage"""
    edge = np.asarray(edge, dtype=np.int64)
    dp, dc, t = _ends(edge, edge_length)
    root = int(np.setdiff1d(edge[:, 0], edge[:, 1])[0])
    root_b = int(np.nonzero(edge[:, 0] == root)[0][0])
    out = []
    for k, tau in enumerate(bounds):
        tau = float(tau)
        if tau == 0.0:
            out.append((k, root_b, 0.0))
        for b in range(edge.shape[0]):
            if dp[b] < tau <= dc[b]:
                out.append((k, b, t[b] if tau >= dc[b] else min(tau - dp[b], t[b])))
    return out


def sub_branches(edge, edge_length, bounds):
    """[(k, b, s1, s2)] by (bin, edge row): the part of branch b inside bin k = [tau_k, tau_{k+1}); s1 = 0 when tau_k <= d_p, else
    tau_k - d_p; s2 = t_b when tau_{k+1} >= d_c, else tau_{k+1} - d_p (both at most t_b); kept when d_p < tau_{k+1},
    d_c > tau_k and s2 > s1"""
    edge = np.asarray(edge, dtype=np.int64)
    dp, dc, t = _ends(edge, edge_length)
    out = []
    for k in range(len(bounds) - 1):
        lo, hi = float(bounds[k]), float(bounds[k + 1])
        for b in range(edge.shape[0]):
            if not (dp[b] < hi and dc[b] > lo):
                continue
            s1 = 0.0 if lo <= dp[b] else min(lo - dp[b], t[b])
            s2 = t[b] if hi >= dc[b] else min(hi - dp[b], t[b])
            if s2 > s1:
                out.append((k, b, s1, s2))
    return out


def _forward(r, Q, b, s):
    """a = P(s)^T F_b rescaled, its exponent (sF_b included)"""
    a, e = exactref._rescale(r["F"][b] @ expm(Q * s))
    return a, e + r["sF"][b]


def _backward(r, Q, edge, edge_length, b, s):
    """beta = P(t_b - s) L_c rescaled, its exponent (sL_c included)"""
    c = int(edge[b, 1])
    v, e = exactref._rescale(r["L"][c] @ expm(Q * (float(edge_length[b]) - s)).T)
    return v, e + r["sL"][c]


def _posterior(r, Q, edge, edge_length, b, s):
    a, _ = _forward(r, Q, b, s)
    v, _ = _backward(r, Q, edge, edge_length, b, s)
    x = a * v
    return x / x.sum(axis=1, keepdims=True)


def through_time(edge, edge_length, Q, pid, states, bounds=None, points=None, observe=None, route="unif"):
    """dict: loglik [S]; with bounds, occupancy [S, K, n] and (K >= 2) bins [S, K - 1, n + n(n-1)]; with points = (edge rows,
    positions), points [S, P, n]"""
    edge = np.asarray(edge, dtype=np.int64)
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    r = exactref.passes(edge, edge_length, Q, pid, states, observe)
    S = r["loglik"].shape[0]
    out = {"loglik": r["loglik"]}
    if bounds is not None:
        K = len(bounds)
        occ = np.zeros((S, K, n))
        for k, b, s in crossings(edge, edge_length, bounds):
            occ[:, k] += _posterior(r, Q, edge, edge_length, b, s)
        out["occupancy"] = occ
        if K >= 2:
            integral = exactref.integral_unif if route == "unif" else exactref.integral_vanloan
            pairs = exactref.columns(n)
            qcol = np.array([Q[i, j] for i, j in pairs])
            bins = np.zeros((S, K - 1, n + len(pairs)))
            for k, b, s1, s2 in sub_branches(edge, edge_length, bounds):
                a, ea = _forward(r, Q, b, s1)
                v, ev = _backward(r, Q, edge, edge_length, b, s2)
                I = integral(Q, s2 - s1, a, v)
                f = np.ldexp(1.0 / r["lam"], (ea + ev - r["sL"][r["root"]]).astype(np.int64))
                bins[:, k, :n] += np.einsum("sii->si", I) * f[:, None]
                bins[:, k, n:] += np.stack([I[:, i, j] for i, j in pairs], axis=1) * qcol[None, :] * f[:, None]
            out["bins"] = bins
    if points is not None:
        pe, pp = points
        out["points"] = np.stack([_posterior(r, Q, edge, edge_length, int(b), float(s)) for b, s in zip(pe, pp)], axis=1)
    return out


def lineages(edge, edge_length, bounds):
    """[K] branches alive at each bound by the crossing rule (the root counts at 0)"""
    cnt = np.zeros(len(bounds))
    for k, _, _ in crossings(edge, edge_length, bounds):
        cnt[k] += 1
    return cnt
