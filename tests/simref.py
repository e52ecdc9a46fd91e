"""Python twin of the forward simulator, written from R/sourceme.R:346-414 (sample2statehistory /
samplethebranch) and the spec, not from phm_sim.hip: Gillespie waiting times along every branch in a pre-order walk, every
random number addressed by (block, entity, 0xFFFFFFFF, global replica) on the Philox4x32-7 stream of the sampler.  Vectorised
over replicas with numpy (the arithmetic is elementwise IEEE binary64, so each replica's numbers are those of a scalar walk);
the scalar building blocks are pyref's.  Also: the closed-form expectations the simulator is pinned to.

TEST INFRASTRUCTURE ONLY.
"""
import numpy as np
from scipy.linalg import expm

import pyref

SIM_ITER = 0xFFFFFFFF
MAX_JUMPS = 9999                 # more jumps than this on one branch: PHM_ERR_CAPACITY
_M32 = np.uint64(0xFFFFFFFF)
_INV = np.asarray(pyref._INV, dtype=np.float64)
_LOGC = np.asarray(pyref._LOGC, dtype=np.float64)


class JumpCapError(RuntimeError):
    def __init__(self, edge_row):
        super().__init__(f"more than {MAX_JUMPS} jumps on edge row {edge_row + 1}")
        self.edge_row = edge_row


def philox_v(c0, c1, c2, c3, key, rounds=pyref.STREAM_ROUNDS):
    """pyref.philox over arrays of counters (uint64 holding 32-bit words)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3))
    k0, k1 = key
    for _ in range(rounds):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)) & _M32, p1 & _M32, \
                         ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)) & _M32, p0 & _M32
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def word(seed, d, entity, reps):
    """the 32 random bits of draw d (same for every replica) of stream (entity, SIM_ITER, replica)"""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    o = philox_v(np.full(reps.shape, d >> 2), np.full(reps.shape, entity), np.full(reps.shape, SIM_ITER), reps, key)
    return o[d & 3]


def u01_v(x):
    return (x.astype(np.float64) + 0.5) * 2.0 ** -32


def neglog_v(k):
    """pyref.neglog_u32 elementwise"""
    y = k.astype(np.float64) * 2.0 + 1.0
    f, e = np.frexp(y)
    top = (e == 33) & (f >= 0.99609375)
    j = ((f - 0.5) * 256.0).astype(np.int64)
    c = 0.501953125 + j.astype(np.float64) * 0.00390625
    r = np.where(top, f - 1.0, (f - c) * _INV[j])
    c0 = np.where(top, 0.0, _LOGC[j])
    ee = np.where(top, 0.0, (e - 33).astype(np.float64))
    p = np.full(k.shape, 1.0 / 7.0)
    p = p * r - 1.0 / 6.0
    p = p * r + 0.2
    p = p * r - 0.25
    p = p * r + 1.0 / 3.0
    p = p * r - 0.5
    p = p * r * r + r
    return -(ee * 6.93147180369123816490e-01 + (c0 + (p + ee * 1.90821492927058770002e-10)))


def left_sum(w):
    """left-to-right sum over the last axis"""
    t = w[..., 0].copy()
    for j in range(1, w.shape[-1]):
        t = t + w[..., j]
    return t


def categorical_v(w, total, u):
    """first j with u * total <= w_0 + .. + w_j (pyref.sample), rows of w per replica"""
    thr = u * total
    cum = w[:, 0].copy()
    idx = (thr > cum).astype(np.int64)
    for j in range(1, w.shape[1] - 1):
        cum = cum + w[:, j]
        idx += (thr > cum)
    return idx


def walk_order(edge, n_tips):
    """the edge rows in the order the library walks them: row order when it is a pre-order, else a depth-first pre-order
    taking children in row order"""
    E = edge.shape[0]
    children = set(int(c) for c in edge[:, 1])
    root = next(int(p) for p in edge[:, 0] if int(p) not in children)
    seen = {root}
    ok = True
    for r in range(E):
        if int(edge[r, 0]) not in seen:
            ok = False
            break
        seen.add(int(edge[r, 1]))
    if ok:
        return list(range(E)), root
    kids = {}
    for r in range(E):
        kids.setdefault(int(edge[r, 0]), []).append(r)
    order, stack = [], [kids[root][1], kids[root][0]]
    while stack:
        r = stack.pop()
        order.append(r)
        c = int(edge[r, 1])
        if c > n_tips:
            stack += [kids[c][1], kids[c][0]]
    return order, root


def simulate(edge, edge_length, Q, pid, R, seed, replica_offset=0, observe=None):
    """R histories; returns (tips [R, T] 1-based observed, stats [R, n + n*n + 1], nodes [R, T + Nnode] 1-based true states),
    the layouts of phm_simulate_histories.  Raises JumpCapError where the library returns PHM_ERR_CAPACITY."""
    edge = np.asarray(edge, dtype=np.int64)
    edge_length = np.asarray(edge_length, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    pid = np.asarray(pid, dtype=np.float64)
    n = Q.shape[0]
    E = edge.shape[0]
    T = E // 2 + 1
    order, root = walk_order(edge, T)
    qoff = Q.copy()
    np.fill_diagonal(qoff, 0.0)
    diag = np.diag(Q)
    inv = np.array([1.0 / (-q) if q < 0.0 else 0.0 for q in diag])
    tot = left_sum(qoff)
    reps = np.arange(R, dtype=np.uint64) + np.uint64(replica_offset)
    nodes = np.zeros((R, 2 * T - 1), dtype=np.int64)
    dwell = np.zeros((R, n))
    cnt = np.zeros((R, n, n), dtype=np.int64)
    u = u01_v(word(seed, 0, root, reps))
    P = np.broadcast_to(pid, (R, n))
    root_state = categorical_v(P, left_sum(P), u)
    nodes[:, root - 1] = root_state
    for b in order:
        t = edge_length[b]
        ent = (1 << 30) | b
        s = nodes[:, edge[b, 0] - 1].copy()
        pos = np.zeros(R)
        active = np.arange(R)
        j = 0
        while active.size:
            absorb = inv[s[active]] == 0.0
            a = active[absorb]
            dwell[a, s[a]] += t - pos[a]
            m = active[~absorb]
            if m.size == 0:
                break
            gap = inv[s[m]] * neglog_v(word(seed, 2 * j, ent, reps[m]))
            dab = pos[m] + gap
            fin = ~(dab < t)
            f = m[fin]
            dwell[f, s[f]] += gap[fin] - (dab[fin] - t)
            g = m[~fin]
            dwell[g, s[g]] += gap[~fin]
            if g.size and j == MAX_JUMPS:
                raise JumpCapError(b)
            if g.size:
                ug = u01_v(word(seed, 2 * j + 1, ent, reps[g]))
                nx = categorical_v(qoff[s[g]], tot[s[g]], ug)
                cnt[g, s[g], nx] += 1
                s[g] = nx
                pos[g] = dab[~fin]
            active = g
            j += 1
        nodes[:, edge[b, 1] - 1] = s
    omap = np.arange(1, n + 1) if observe is None else np.asarray(observe, dtype=np.int64)
    tips = omap[nodes[:, :T]].astype(np.int32)
    stats = np.concatenate([dwell, cnt.reshape(R, n * n).astype(np.float64), root_state[:, None].astype(np.float64)], axis=1)
    return tips, stats, (nodes + 1).astype(np.int32)


# ---- closed forms --------------------------------------------------------------------------------------------------------
def expectations(edge, edge_length, Q, pid):
    """E[dwell_i] = sum_b int_0^{t_b} (p_parent e^{Qu})_i du (Van Loan: expm([[Q, I], [0, 0]] t), upper right block),
    E[N_ij] = q_ij E[dwell_i], P(tip = j) = (pid e^{Q depth(tip)})_j.  Returns (dwell [n], counts [n, n], tip_p [T, n])."""
    edge = np.asarray(edge, dtype=np.int64)
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    E = edge.shape[0]
    T = E // 2 + 1
    order, root = walk_order(edge, T)
    p0 = np.asarray(pid, dtype=np.float64) / np.sum(pid)
    dist = {root: p0}
    dwell = np.zeros(n)
    big = np.zeros((2 * n, 2 * n))
    big[:n, :n] = Q
    big[:n, n:] = np.eye(n)
    for b in order:
        t = float(edge_length[b])
        pp = dist[int(edge[b, 0])]
        dwell += pp @ expm(big * t)[:n, n:]
        dist[int(edge[b, 1])] = pp @ expm(Q * t)
    counts = Q * dwell[:, None]
    np.fill_diagonal(counts, 0.0)
    tip_p = np.stack([dist[i + 1] for i in range(T)])
    return dwell, counts, tip_p


def zscores(tips, stats, edge, edge_length, Q, pid, observe=None):
    """|z| of the sample means of every dwell column, every off-diagonal count column (sample sd) and every (tip, reported
    state) frequency (binomial sd) against the closed forms; columns whose expectation and sample are both zero are left out."""
    n = np.asarray(Q).shape[0]
    R = stats.shape[0]
    dwell, counts, tip_p = expectations(edge, edge_length, Q, pid)
    z = []
    for col, want in list(enumerate(dwell)) + [(n + i * n + j, counts[i, j]) for i in range(n) for j in range(n) if i != j]:
        x = stats[:, col]
        sd = x.std(ddof=1)
        if sd == 0.0 and want == 0.0 and np.all(x == 0.0):
            continue
        z.append(abs(x.mean() - want) / max(sd / np.sqrt(R), 1e-300))
    omap = np.arange(1, n + 1) if observe is None else np.asarray(observe)
    for k in np.unique(omap):
        p = tip_p[:, omap == k].sum(axis=1)
        f = (tips == k).mean(axis=0)
        sd = np.sqrt(np.maximum(p * (1 - p), 1e-300) / R)
        z.extend(np.abs(f - p) / sd)
    return np.asarray(z)
