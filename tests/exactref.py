"""Python twin of the exact conditional expectations (phm_expected_stats): E[dwell_i | tips, Q] and
E[N_ij | tips, Q] per site and per branch, log p(tips | Q) and the marginal posterior of every node's state.  Written from the
spec, not from phm_expect.hip.  Two independent routes to the branch integral

    I_b[i, j] = int_0^t F_b^T P(s) E_ij P(t - s) L_c ds

* ``route="vanloan"``: the upper right block of expm([[Q, E_ij], [0, Q]] t) for every (i, j) (Van Loan 1978), contracted with
  F_b and L_c;
* ``route="unif"``: uniformization, I_b = sum_{l + r <= M_b} w_{l+r} u_l v_r^T with u_l = (B^T)^l F_b, v_r = B^r L_c,
  w_m = pois(m + 1; mu t_b) / mu, B = I + Q / mu, mu = max_i(-q_ii), truncated where the omitted Poisson mass is <= 2^-60.

Vectorised over sites with numpy.  Every partial likelihood vector is rescaled by a power of two to a maximum in [1/2, 1) per
(node, site), its base-2 exponent kept beside it; a branch's factor 2^(eF + eL - e_root) / lambda is exact up to one division.  TEST INFRASTRUCTURE ONLY.
"""
import math

import numpy as np
from scipy.linalg import expm

TAIL = 2.0 ** -60


def poisson_weights(x):
    """pmf of Poisson(x) at 0 .. K, computed outward from the mode with p_mode = 1 and normalised by the sum (no lgamma, so
    x in the thousands keeps full relative precision), and M: the first m with sum_{k >= m + 2} pmf(k) <= 2^-60.
    Returns (pmf[0 .. M + 1], M)."""
    if x <= 0.0:
        return np.array([1.0, 0.0]), 0
    mode = int(math.floor(x))
    hi = mode + int(math.ceil(12.0 * math.sqrt(x))) + 40
    lo = max(0, mode - int(math.ceil(12.0 * math.sqrt(x))) - 40)
    r = np.zeros(hi + 1)
    r[mode] = 1.0
    for k in range(mode, hi):
        r[k + 1] = r[k] * x / (k + 1)
    for k in range(mode, lo, -1):
        r[k - 1] = r[k] * k / x
    p = r / np.sum(r)
    tail = np.cumsum(p[::-1])[::-1]                      # tail[k] = sum_{j >= k} p_j, small terms first
    M = 0
    while M + 2 <= hi and tail[M + 2] > TAIL:
        M += 1
    return p[:M + 2], M


def _children(edge, T):
    kids = {}
    for b in range(edge.shape[0]):
        kids.setdefault(int(edge[b, 0]), []).append(b)
    children = set(int(c) for c in edge[:, 1])
    root = next(int(p) for p in edge[:, 0] if int(p) not in children)
    order = []                                           # pre-order of the edges
    stack = list(reversed(kids[root]))
    while stack:
        b = stack.pop()
        order.append(b)
        c = int(edge[b, 1])
        if c > T:
            stack += list(reversed(kids[c]))
    return kids, root, order


def tip_vectors(states, n, observe=None):
    """[S, T, n] 0/1 tip vectors: L(a) = 1 if observe[a] == y (identity when None), all ones for y = 0 (missing)."""
    states = np.atleast_2d(np.asarray(states, dtype=np.int64))
    obs = np.arange(1, n + 1) if observe is None else np.asarray(observe, dtype=np.int64)
    L = (obs[None, None, :] == states[:, :, None]).astype(np.float64)
    L[states == 0] = 1.0
    return L


def _rescale(v):
    """v scaled by 2^-e (exact) to a maximum in [1/2, 1) per site; e (integer-valued, 0 for an all-zero vector)"""
    _, e = np.frexp(v.max(axis=-1))
    e = np.where(v.max(axis=-1) > 0, e, 0)
    return np.ldexp(v, -e[..., None]), e.astype(np.float64)


def passes(edge, edge_length, Q, pid, states, observe=None, P=None):
    """Up and down passes.  Returns a dict: L, sL (node id -> [S, n], [S] base-2 exponents), O, sO (same), F, sF (edge row
    -> ...), P [E, n, n], loglik [S], lam [S] (p(tips) = lam 2^sL[root]), root."""
    edge = np.asarray(edge, dtype=np.int64)
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    E = edge.shape[0]
    T = E // 2 + 1
    kids, root, order = _children(edge, T)
    if P is None:
        P = np.stack([expm(Q * float(t)) for t in edge_length])
    tipL = tip_vectors(states, n, observe)
    S = tipL.shape[0]
    L, sL = {}, {}
    for k in range(T):
        L[k + 1], sL[k + 1] = tipL[:, k, :], np.zeros(S)
    for b in reversed(order):                            # children before parents
        p = int(edge[b, 0])
        if p in L:
            continue
        b0, b1 = kids[p]
        c0, c1 = int(edge[b0, 1]), int(edge[b1, 1])
        if c0 not in L or c1 not in L:
            continue
        v = np.einsum("ij,sj->si", P[b0], L[c0]) * np.einsum("ij,sj->si", P[b1], L[c1])
        L[p], s = _rescale(v)
        sL[p] = s + sL[c0] + sL[c1]
    pid = np.asarray(pid, dtype=np.float64)
    pid = pid / np.sum(pid)                              # the root prior, normalised (as the simulation draws the root state)
    lam = L[root] @ pid
    with np.errstate(divide="ignore"):
        loglik = np.log(lam) + sL[root] * math.log(2.0)
    O, sO = {root: np.broadcast_to(pid, (S, n)).copy()}, {root: np.zeros(S)}
    F, sF = {}, {}
    for b in order:
        p, c = int(edge[b, 0]), int(edge[b, 1])
        sib = kids[p][1] if kids[p][0] == b else kids[p][0]
        cs = int(edge[sib, 1])
        f, s = _rescale(O[p] * np.einsum("ij,sj->si", P[sib], L[cs]))
        F[b], sF[b] = f, s + sO[p] + sL[cs]
        o, s = _rescale(np.einsum("ji,sj->si", P[b], f))
        O[c], sO[c] = o, s + sF[b]
    return dict(L=L, sL=sL, O=O, sO=sO, F=F, sF=sF, P=P, loglik=loglik, lam=lam, root=root, order=order)


def transition_unif(Q, t):
    """P(t) = sum_m pois(m; mu t) B^m, B = I + Q / mu, mu = max_i(-q_ii): every term is non-negative, so nothing cancels, and no
    Pade enters.  Truncated where the omitted Poisson mass is <= 2^-60 (``poisson_weights``).  ``passes(..., P=...)`` takes a
    stack of these in place of scipy's expm."""
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    mu = float(np.max(-np.diag(Q)))
    if mu <= 0.0 or float(t) <= 0.0:
        return np.eye(n)
    B = np.eye(n) + Q / mu
    p, M = poisson_weights(mu * float(t))
    P = np.zeros((n, n))
    Bm = np.eye(n)
    for m in range(M + 2):
        if p[m] > 0.0:
            P += p[m] * Bm
        Bm = Bm @ B
    return P


def integral_unif(Q, t, F, Lc):
    """I[s, i, j] by uniformization (module docstring), F, Lc [S, n]."""
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    mu = float(np.max(-np.diag(Q)))
    B = np.eye(n) + Q / mu
    p, M = poisson_weights(mu * float(t))
    w = p[1:M + 2] / mu                                  # w_m = pois(m + 1) / mu, m = 0 .. M
    U = np.empty((M + 1,) + F.shape)
    V = np.empty((M + 1,) + Lc.shape)
    U[0], V[0] = F, Lc
    for m in range(M):
        U[m + 1] = U[m] @ B                              # (B^T u)^T = u^T B
        V[m + 1] = V[m] @ B.T
    idx = np.arange(M + 1)
    H = np.where(idx[:, None] + idx[None, :] <= M, w[np.minimum(idx[:, None] + idx[None, :], M)], 0.0)
    Y = np.einsum("lr,rsn->lsn", H, V)
    return np.einsum("lsi,lsj->sij", U, Y)


def integral_vanloan(Q, t, F, Lc):
    """I[s, i, j] from expm([[Q, E_ij], [0, Q]] t) (module docstring)."""
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    out = np.empty((F.shape[0], n, n))
    big = np.zeros((2 * n, 2 * n))
    big[:n, :n] = Q
    big[n:, n:] = Q
    for i in range(n):
        for j in range(n):
            big[:n, n:] = 0.0
            big[i, n + j] = 1.0
            G = expm(big * float(t))[:n, n:]
            out[:, i, j] = np.einsum("sa,ab,sb->s", F, G, Lc)
    return out


def columns(n):
    """(from, to) of the off-diagonal count columns in man/sumstatMCMC.Rd:18 order: row by row, the diagonal skipped"""
    return [(i, j) for i in range(n) for j in range(n) if i != j]


def expected(edge, edge_length, Q, pid, states, observe=None, route="unif", per_branch=False, nodes=False):
    """Returns (stats [S, n + n(n-1)], loglik [S][, branch [S, E, cols]][, node_post [S, T + Nnode, n]])."""
    edge = np.asarray(edge, dtype=np.int64)
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    E = edge.shape[0]
    T = E // 2 + 1
    r = passes(edge, edge_length, Q, pid, states, observe)
    S = r["loglik"].shape[0]
    integral = integral_unif if route == "unif" else integral_vanloan
    pairs = columns(n)
    qcol = np.array([Q[i, j] for i, j in pairs])
    branch = np.zeros((S, E, n + len(pairs)))
    for b in range(E):
        c = int(edge[b, 1])
        I = integral(Q, edge_length[b], r["F"][b], r["L"][c])
        f = np.ldexp(1.0 / r["lam"], (r["sF"][b] + r["sL"][c] - r["sL"][r["root"]]).astype(np.int64))
        branch[:, b, :n] = np.einsum("sii->si", I) * f[:, None]
        branch[:, b, n:] = np.stack([I[:, i, j] for i, j in pairs], axis=1) * qcol[None, :] * f[:, None]
    out = [branch.sum(axis=1), r["loglik"]]
    if per_branch:
        out.append(branch)
    if nodes:
        post = np.zeros((S, 2 * T - 1, n))
        for k in range(1, 2 * T):
            ol = r["O"][k] * r["L"][k]                   # = O L exp(sO + sL - loglik), normalised without the log scales
            post[:, k - 1] = ol / ol.sum(axis=1, keepdims=True)
        out.append(post)
    return tuple(out)


def felsenstein_loglik(edge, edge_length, Q, pid, states, observe=None):
    """log p(tips | Q) by a plain unscaled pruning pass with scipy's expm, one site at a time (small trees only)."""
    edge = np.asarray(edge, dtype=np.int64)
    n = np.asarray(Q).shape[0]
    E = edge.shape[0]
    T = E // 2 + 1
    kids, root, order = _children(edge, T)
    tipL = tip_vectors(states, n, observe)
    out = []
    for s in range(tipL.shape[0]):
        def lik(node):
            if node <= T:
                return tipL[s, node - 1]
            v = np.ones(n)
            for b in kids[node]:
                v = v * (expm(np.asarray(Q) * float(edge_length[b])) @ lik(int(edge[b, 1])))
            return v
        pid = np.asarray(pid, dtype=np.float64)
        out.append(math.log(float(pid @ lik(root) / np.sum(pid))))
    return np.array(out)
