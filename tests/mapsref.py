"""Python twin of the stochastic maps: simref.simulate and pyref.sumstatEXP restated so that they record
every branch's segments, built from those modules' primitives (streams, variates, categorical rules, matrix helpers).  Each
returns the usual outputs plus the maps in the library's layout: ``off`` int64 [R*E + 1] (row r*E + b = history r on edge
row b), ``dwell`` float64 and ``state`` int32 (1-based) per segment, parent end first.
TEST INFRASTRUCTURE ONLY.
"""
import numpy as np

import pyref
import simref


def _pack(rows, R, E):
    """rows[(r, b)] = list of (dwell, state0) -> (off, dwell, state)"""
    cnt = np.zeros(R * E, dtype=np.int64)
    for (r, b), segs in rows.items():
        cnt[r * E + b] = len(segs)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    dwell = np.zeros(off[-1])
    state = np.zeros(off[-1], dtype=np.int32)
    for (r, b), segs in rows.items():
        k = off[r * E + b]
        for i, (x, s) in enumerate(segs):
            dwell[k + i] = x
            state[k + i] = s + 1
    return off, dwell, state


def simulate(edge, edge_length, Q, pid, R, seed, replica_offset=0, observe=None):
    """simref.simulate with the segments recorded: (tips, stats, nodes, (off, dwell, state)).  The statistics are summed from
    the same numbers in the same walk order as simref's."""
    edge = np.asarray(edge, dtype=np.int64)
    edge_length = np.asarray(edge_length, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    pid = np.asarray(pid, dtype=np.float64)
    n = Q.shape[0]
    E = edge.shape[0]
    T = E // 2 + 1
    order, root = simref.walk_order(edge, T)
    qoff = Q.copy()
    np.fill_diagonal(qoff, 0.0)
    inv = np.array([1.0 / (-q) if q < 0.0 else 0.0 for q in np.diag(Q)])
    tot = simref.left_sum(qoff)
    reps = np.arange(R, dtype=np.uint64) + np.uint64(replica_offset)
    nodes = np.zeros((R, 2 * T - 1), dtype=np.int64)
    dwell = np.zeros((R, n))
    cnt = np.zeros((R, n, n), dtype=np.int64)
    P = np.broadcast_to(pid, (R, n))
    root_state = simref.categorical_v(P, simref.left_sum(P), simref.u01_v(simref.word(seed, 0, root, reps)))
    nodes[:, root - 1] = root_state
    rows = {}
    for b in order:
        t = edge_length[b]
        ent = (1 << 30) | b
        s = nodes[:, edge[b, 0] - 1].copy()
        pos = np.zeros(R)
        segs = [[] for _ in range(R)]

        def add(idx, x):
            dwell[idx, s[idx]] += x
            for i, v in zip(idx.tolist(), np.broadcast_to(x, idx.shape).tolist()):
                segs[i].append((v, int(s[i])))

        active = np.arange(R)
        j = 0
        while active.size:
            absorb = inv[s[active]] == 0.0
            a = active[absorb]
            add(a, t - pos[a])
            m = active[~absorb]
            if m.size == 0:
                break
            gap = inv[s[m]] * simref.neglog_v(simref.word(seed, 2 * j, ent, reps[m]))
            dab = pos[m] + gap
            fin = ~(dab < t)
            add(m[fin], gap[fin] - (dab[fin] - t))
            g = m[~fin]
            add(g, gap[~fin])
            if g.size and j == simref.MAX_JUMPS:
                raise simref.JumpCapError(b)
            if g.size:
                nx = simref.categorical_v(qoff[s[g]], tot[s[g]], simref.u01_v(simref.word(seed, 2 * j + 1, ent, reps[g])))
                cnt[g, s[g], nx] += 1
                s[g] = nx
                pos[g] = dab[~fin]
            active = g
            j += 1
        nodes[:, edge[b, 1] - 1] = s
        for r in range(R):
            rows[(r, b)] = segs[r]
    omap = np.arange(1, n + 1) if observe is None else np.asarray(observe, dtype=np.int64)
    tips = omap[nodes[:, :T]].astype(np.int32)
    stats = np.concatenate([dwell, cnt.reshape(R, n * n).astype(np.float64), root_state[:, None].astype(np.float64)], axis=1)
    return tips, stats, (nodes + 1).astype(np.int32), _pack(rows, R, E)


def sumstatEXP(z, Q, pid, N, nen, nodelist, root, L, R, dv, seed, replica, rescale=False, jumps=None):
    """pyref.sumstatEXP (maketreelistEXP :3001-3051, newunifSample :93-208) with the segments recorded: (out, (off, dwell,
    state)).  Same draws in the same order; out is summed in edge-row order as pyref's.  ``jumps``: a dict that receives the
    number of jumps, virtual ones included, of every (sample, edge row)."""
    n = len(Q)
    E = len(z["edge"])
    T = len(z["states"])
    e1 = [int(r[0]) for r in z["edge"]]
    e2 = [int(r[1]) for r in z["edge"]]
    tl = [float(x) for x in z["edge.length"]]
    rate = -1.0 * min(Q[i][i] for i in range(n))
    B2 = [[(1.0 if i == j else 0.0) + Q[i][j] / rate for j in range(n)] for i in range(n)]
    rng = pyref.Rng(seed, replica)
    P = [pyref.matexp(L, R, dv, tl[b]) for b in range(E)]
    PL = [[0.0] * n for _ in range(2 * T - 1)]
    for i in range(T):
        PL[i][int(z["states"][i]) - 1] = 1.0
    for i in range(T - 1):                                                   # the pruning pass in nen order
        ea, eb = nen[2 * i] - 1, nen[2 * i + 1] - 1
        va = pyref.matvec_lr(P[ea], PL[e2[ea] - 1])
        vb = pyref.matvec_lr(P[eb], PL[e2[eb] - 1])
        row = [va[c] * vb[c] for c in range(n)]
        if rescale:
            sm = row[0]
            for c in range(1, n):
                sm += row[c]
            row = [x / sm for x in row]
        PL[e1[ea] - 1] = row
    out = [[0.0] * (n + n * (n - 1)) for _ in range(N)]
    rows = {}
    chains = {}                                                              # end state -> [B^k e_end], shared by every branch
    ks = [] if jumps is not None else None
    for it in range(N):
        rm = [0] * (2 * T - 1)
        for i in range(T):
            rm[i] = int(z["states"][i]) - 1
        rm[root - 1] = pyref.sample([pid[c] * PL[root - 1][c] for c in range(n)], rng.u(it, pyref.ENT_NODE | (root - 1), 0))
        for node in nodelist:
            j = e2.index(node)
            rm[node - 1] = pyref.sample([P[j][rm[e1[j] - 1]][c] * PL[node - 1][c] for c in range(n)],
                                        rng.u(it, pyref.ENT_NODE | (node - 1), 0))
        for b in range(E):
            segs = _unif_segments(rm[e1[b] - 1], rm[e2[b] - 1], tl[b], P[b], B2, rate, n, lambda d: rng.u(it, pyref.ENT_BUNIF | b, d),
                                  chains, ks)
            if jumps is not None:
                jumps[(it, b)] = ks.pop()
            for i in range(1, len(segs)):
                x, y = segs[i - 1][1], segs[i][1]
                out[it][n + x * (n - 1) + (y - 1 if x < y else y)] += 1.0
            for d, s in segs:
                out[it][s] += d
            rows[(it, b)] = segs
    return out, _pack(rows, N, E)


def _unif_segments(a, e, t, Pb, B2, rate, n, u, chains=None, ks=None):
    """newunifSample(a, e, t, P_b[a, e]) as a list of (dwell, state0), virtual jumps dropped; u(d) is draw d of the branch.
    ``chains``: a dict that keeps the rows B^k e_end between calls (the same numbers; 64 states would recompute 300 products of
    4 096 terms per branch otherwise); ``ks``: a list that receives the number of jumps drawn"""
    tp = Pb[a][e]
    dr = 0
    rU = u(dr); dr += 1
    lam = rate * t
    pk = pyref.pexp(-lam)
    cum = pk / tp if a == e else 0.0
    beta = chains.get(e) if chains is not None else None
    if beta is None:
        beta = [[0.0] * n]
        beta[0][e] = 1.0
        if chains is not None:
            chains[e] = beta
    k = 0
    while not cum > rU:
        k += 1
        assert k <= 300
        if len(beta) <= k:
            beta.append(pyref.matvec_lr(B2, beta[k - 1]))
        pk = pk * lam / float(k)
        cum += pk * beta[k][a] / tp
    if ks is not None:
        ks.append(k)
    if k == 0 or (k == 1 and a == e):
        return [(t - 0.0, a)]
    if k == 1:
        tj = t * u(dr)
        return [(tj - 0.0, a), (t - tj, e)]
    times = []
    for _ in range(k):
        times.append(t * u(dr)); dr += 1
    times.sort()
    dom = [a] + [0] * (k - 1) + [e]
    for i in range(1, k):
        w = [B2[dom[i - 1]][c] * beta[k - i][c] for c in range(n)]
        total = w[0]
        for x in w[1:]:
            total += x
        x = u(dr); dr += 1
        cumw, pick = 0.0, None
        for c in range(n):                                                   # sampleOnce :81-90
            cumw += w[c] / total
            if x < cumw:
                pick = c
                break
        assert pick is not None
        dom[i] = pick
    segs, tprev, sprev = [], 0.0, a
    for i in range(1, k + 1):
        if dom[i - 1] != dom[i]:
            segs.append((times[i - 1] - tprev, sprev))
            tprev, sprev = times[i - 1], dom[i]
    segs.append((t - tprev, sprev))
    return segs
