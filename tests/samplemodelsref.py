"""Python twin of the exact sampler of histories over many rate matrices and sites (DESIGN.md section 19,
phm_sample_histories_models), written from the spec, not from phm_sample.hip: ``exactref.passes`` per model for P_k(t_b) and the
partial likelihoods, then the top-down draw of every node (tips included) and the end-point-conditioned uniformization sampler
of every branch -- jump count from the series' own total with no exp(-x) and no division by P[a, e], jump times from normalised
exponential spacings, states from B and the end-state table beta.  Every random number is addressed by (seed, entity, global
evaluation id site * K + model, draw index + replica_offset) on the sampler's Philox4x32-7 streams.  Vectorised over the draws
of one evaluation with numpy (elementwise IEEE binary64, so each draw's numbers are those of a scalar walk).

TEST INFRASTRUCTURE ONLY.
"""
import numpy as np
from scipy.linalg import expm

import exactref
import pyref
import simref

SCALE_UP = 2.0 ** 512
SCALE_DOWN = 2.0 ** -512
TAIL = 2.0 ** -60
M_CAP = 1 << 17
MAX_JUMP_MEAN = 32768.0


def stop_index(x):
    """M(x): section 18's stopping index as a function of x = mu t alone.  r_0 = 1, r_m = r_{m-1} (x / m), S_m = r_0 + .. + r_m
    (both divided by 2^512 whenever r passes 2^512); the first m >= 1 with x < m + 1 and r_{m+1} <= 2^-60 S_m (1 - x / (m + 2))."""
    if not x > 0.0:
        return 0
    r, S = x, 1.0 + x
    for m in range(1, M_CAP):
        rn = r * (x / float(m + 1))
        if x < float(m + 1) and rn <= TAIL * S * (1.0 - x / float(m + 2)):
            return m
        r = rn
        S += r
        if r > SCALE_UP:
            r *= SCALE_DOWN
            S *= SCALE_DOWN
    return M_CAP


def model_table(Q, depth):
    """mu, B = I + Q / mu (I when mu = 0) and beta [depth + 1, n, n], beta[m][c, e] = (B^m)[c, e] by beta_{m+1} = B beta_m with
    unfused left-to-right sums."""
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    mu = float(np.max(-np.diag(Q)))
    B = np.eye(n) + Q / mu if mu > 0.0 else np.eye(n)
    beta = np.empty((depth + 1, n, n))
    beta[0] = np.eye(n)
    for m in range(depth):
        acc = B[:, 0, None] * beta[m][0, None, :]
        for j in range(1, n):
            acc = acc + B[:, j, None] * beta[m][j, None, :]
        beta[m + 1] = acc
    return mu, B, beta


def jump_count_series(x, ba):
    """First pass of a branch: ba [>= M + 1, D] = beta_m[a] per draw.  Returns (S [D], M, R): the series' own total
    S = sum_{m <= M(x)} r_m beta_m[a] accumulated ascending, and the number R of divisions by 2^512 it went through, so that
    S e^-x 2^(512 R) = P[a, e]."""
    r, Sp = 1.0, 1.0
    Sa = ba[0].astype(np.float64).copy()
    R = M = 0
    m = 1
    while True:
        rn = r * (x / float(m))
        if m >= 2 and x < float(m) and rn <= TAIL * Sp * (1.0 - x / float(m + 1)):
            break
        r = rn
        Sp += r
        Sa = Sa + r * ba[m]
        M = m
        if r > SCALE_UP:
            r *= SCALE_DOWN
            Sp *= SCALE_DOWN
            Sa = Sa * SCALE_DOWN
            R += 1
        m += 1
    return Sa, M, R


def _ldexp(v, e):
    with np.errstate(under="ignore"):
        return np.ldexp(v, e)


def jump_count(x, ba, u):
    """N [D]: the first m with u S <= cum_m (a partial sum taken before a later division by 2^512 is compared after the
    divisions that followed it)."""
    Sa, M, R = jump_count_series(x, ba)
    thr = u * Sa
    cum = ba[0].astype(np.float64).copy()
    N = np.full(u.shape, M, dtype=np.int64)
    found = thr <= _ldexp(cum, -512 * R)
    N[found] = 0
    r, rho = 1.0, 0
    for m in range(1, M + 1):
        if np.all(found):
            break
        r = r * (x / float(m))
        cum = cum + r * ba[m]
        if r > SCALE_UP:
            r *= SCALE_DOWN
            cum = cum * SCALE_DOWN
            rho += 1
        hit = ~found & (thr <= _ldexp(cum, -512 * (R - rho)))
        N[hit] = m
        found |= hit
    return N, Sa, R


class _Rng:
    def __init__(self, seed, eval_id, reps):
        self.key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        self.it = np.full(reps.shape, eval_id, dtype=np.uint64)
        self.reps = reps.astype(np.uint64)

    def words(self, ent, d):
        """the 32 random bits of draw d (a scalar or one index per draw) of stream (ent, evaluation, draw)"""
        d = np.broadcast_to(np.asarray(d, dtype=np.uint64), self.reps.shape)
        o = simref.philox_v(d >> np.uint64(2), np.full(self.reps.shape, ent, dtype=np.uint64), self.it, self.reps, self.key)
        return np.choose((d & np.uint64(3)).astype(np.int64), o)

    def u(self, ent, d):
        return simref.u01_v(self.words(ent, d))

    def e(self, ent, d):
        return simref.neglog_v(self.words(ent, d))


def sample_evaluation(edge, edge_length, Q, pid, tips, observe, eval_id, D, seed=0, replica_offset=0, P=None):
    """D histories of one evaluation.  Returns None when the tips are impossible, else a dict: stats [D, n + n(n-1)], nodes
    [D, T + Nnode] 1-based true states, loglik, and the maps as rows (d, b): seg_off [D * E + 1], seg_dwell, seg_state (1-based)."""
    edge = np.asarray(edge, dtype=np.int64)
    el = np.asarray(edge_length, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    E = edge.shape[0]
    T = E // 2 + 1
    cols = n + n * (n - 1)
    r = exactref.passes(edge, el, Q, pid, np.asarray(tips).reshape(1, -1), observe, P=P)
    loglik = float(r["loglik"][0])
    if not np.isfinite(loglik):
        return None
    Pm, L = r["P"], r["L"]
    pidn = np.asarray(pid, dtype=np.float64) / np.sum(pid)
    mu = float(np.max(-np.diag(Q)))
    if mu * float(np.max(el)) > MAX_JUMP_MEAN:
        raise ValueError("max(-q_ii) * t_b above 32768")
    mu, B, beta = model_table(Q, stop_index(mu * float(np.max(el))))
    rng = _Rng(seed, eval_id, np.arange(D, dtype=np.int64) + replica_offset)
    state = np.zeros((D, 2 * T - 1), dtype=np.int64)
    root = r["root"]
    w = pidn[None, :] * L[root][0][None, :] * np.ones((D, 1))
    state[:, root - 1] = simref.categorical_v(w, simref.left_sum(w), rng.u(pyref.ENT_NODE | (root - 1), 0))
    for b in r["order"]:                                   # parents before children; every child takes its draw, tips too
        p, c = int(edge[b, 0]), int(edge[b, 1])
        w = Pm[b][state[:, p - 1], :] * L[c][0][None, :]
        state[:, c - 1] = simref.categorical_v(w, simref.left_sum(w), rng.u(pyref.ENT_NODE | (c - 1), 0))
    stats = np.zeros((D, cols))
    ev_lane, ev_edge, ev_dwell, ev_state = [], [], [], []
    lanes = np.arange(D)

    def segment(b, sel, st, v):
        np.add.at(stats, (lanes[sel], st[sel]), v[sel])
        ev_lane.append(lanes[sel]); ev_edge.append(np.full(int(np.sum(sel)), b)); ev_dwell.append(v[sel]); ev_state.append(st[sel] + 1)

    def count(sel, frm, to):
        col = n + frm * (n - 1) + np.where(to > frm, to - 1, to)
        np.add.at(stats, (lanes[sel], col[sel]), 1.0)

    every = np.ones(D, dtype=bool)
    for b in range(E):
        a, e = state[:, int(edge[b, 0]) - 1], state[:, int(edge[b, 1]) - 1]
        t = float(el[b])
        x = mu * t
        if not x > 0.0:
            segment(b, every, a, np.full(D, t))
            continue
        ent = pyref.ENT_BUNIF | b
        N, Sa, _ = jump_count(x, beta[:, a, e], rng.u(ent, 0))
        if np.any(~(Sa > 0.0)):
            raise ZeroDivisionError(f"edge row {b + 1}: an impossible pair of end states was drawn")
        Nmax = int(N.max())
        Ex = np.zeros((Nmax + 2, D))
        for i in range(1, Nmax + 2):
            Ex[i] = rng.e(ent, i)
        G = np.zeros(D)
        for i in range(1, Nmax + 2):
            G = np.where(i <= N + 1, G + Ex[i], G)
        prev, sprev = a.copy(), a.copy()
        tprev, c = np.zeros(D), np.zeros(D)
        for i in range(1, Nmax + 1):
            active = i <= N
            c = np.where(active, c + Ex[i], c)
            di = e.copy()
            inner = i < N
            if np.any(inner):
                mrow = np.clip(N - i, 0, None)
                w = B[prev, :] * beta[mrow[:, None], np.arange(n)[None, :], e[:, None]]
                idx = simref.categorical_v(w, simref.left_sum(w), rng.u(ent, N + 1 + i))
                di = np.where(inner, idx, di)
            change = active & (prev != di)
            if np.any(change):
                with np.errstate(invalid="ignore", divide="ignore"):
                    ti = t * (c / G)
                segment(b, change, sprev, ti - tprev)
                count(change, sprev, di)
                tprev = np.where(change, ti, tprev)
                sprev = np.where(change, di, sprev)
            prev = np.where(active, di, prev)
        segment(b, every, sprev, t - tprev)
    lane = np.concatenate(ev_lane); eb = np.concatenate(ev_edge)
    key = lane * E + eb
    order = np.argsort(key, kind="stable")
    seg_off = np.zeros(D * E + 1, dtype=np.int64)
    np.cumsum(np.bincount(key, minlength=D * E), out=seg_off[1:])
    return dict(stats=stats, nodes=state + 1, loglik=loglik, seg_off=seg_off, seg_dwell=np.concatenate(ev_dwell)[order],
                seg_state=np.concatenate(ev_state)[order].astype(np.int32))


def sample_models(edge, edge_length, Qs, pid, sites, draws, observe=None, site_of_model=None, seed=0, replica_offset=0):
    """The whole call: returns a dict with stats [K, S, D, cols], loglik [K, S], nodes [K, S, D, NT] and the maps (off, dwell,
    state) over histories h = e D + d in evaluation order; the S axis is absent with ``site_of_model``.  An impossible evaluation:
    -inf, NaN statistics, zero nodes, empty map rows."""
    Qs = np.asarray(Qs, dtype=np.float64)
    if Qs.ndim == 2:
        Qs = Qs[None]
    K, n = Qs.shape[0], Qs.shape[1]
    sites = np.atleast_2d(np.asarray(sites))
    S = sites.shape[0]
    pid = np.atleast_2d(np.asarray(pid, dtype=np.float64))
    E = np.asarray(edge).shape[0]
    NT = E + 1
    D = int(draws)
    cols = n + n * (n - 1)
    evals = [(k, int(site_of_model[k])) for k in range(K)] if site_of_model is not None else [(k, s) for k in range(K) for s in range(S)]
    stats = np.full((len(evals), D, cols), np.nan)
    nodes = np.zeros((len(evals), D, NT), dtype=np.int32)
    loglik = np.full(len(evals), -np.inf)
    offs, dwell, state = [np.zeros(1, dtype=np.int64)], [], []
    base = 0
    el = np.asarray(edge_length, dtype=np.float64)
    P_of = {}                                              # a model's P(t_b), once for all its sites
    for i, (k, s) in enumerate(evals):
        if k not in P_of:
            P_of = {k: expm(Qs[k][None, :, :] * el[:, None, None])}
        r = sample_evaluation(edge, edge_length, Qs[k], pid[k if pid.shape[0] > 1 else 0], sites[s], observe, s * K + k, D, seed,
                              replica_offset, P=P_of[k])
        if r is None:
            offs.append(np.full(D * E, base, dtype=np.int64))
            continue
        stats[i], nodes[i], loglik[i] = r["stats"], r["nodes"], r["loglik"]
        offs.append(r["seg_off"][1:] + base)
        base += int(r["seg_off"][-1])
        dwell.append(r["seg_dwell"]); state.append(r["seg_state"])
    shape = (K,) if site_of_model is not None else (K, S)
    return dict(stats=stats.reshape(shape + (D, cols)), nodes=nodes.reshape(shape + (D, NT)), loglik=loglik.reshape(shape),
                off=np.concatenate(offs), dwell=np.concatenate(dwell) if dwell else np.zeros(0),
                state=np.concatenate(state) if state else np.zeros(0, dtype=np.int32))
