"""Stochastic maps of sampled and simulated histories (DESIGN.md sections 14 and 15): what ``api.simulate_histories(..., maps=True)``,
``api.sumstatEXP(..., maps=True)`` and the fixed-Q MCMC drivers (``api.sumstatMCMC(..., maps=True)`` and its kin) return, the
reference's helpers around a history (R/sourceme.R:1-60: ``makemappededge``, ``nodestatesmake``, ``divtophy``), and the summaries
through time of section 16 (``node_depths``, ``Maps.through_time``, ``Maps.states_at``).

Row ``r * E + b`` is history r's map on edge row b: segments ``off[k]:off[k+1]`` of ``dwell`` (time) and ``state`` (1-based,
the ``mapnames`` convention), from the parent end to the child end.  From the MCMC drivers, history ``h = s * J + j`` is chain s
at the j-th of the J recorded iterations (``map_iters[j]``)."""
from __future__ import annotations

import numpy as np


class Maps:
    """R histories x E edge rows of segments: ``off`` int64 [R*E + 1], ``dwell`` float64 and ``state`` int32 [off[-1]]."""

    def __init__(self, off, dwell, state, n_edge):
        self.off = np.asarray(off, dtype=np.int64)
        self.dwell = np.asarray(dwell, dtype=np.float64)
        self.state = np.asarray(state, dtype=np.int32)
        self.n_edge = int(n_edge)
        if self.n_edge < 1 or (self.off.size - 1) % self.n_edge:
            raise ValueError("off must hold R * n_edge + 1 offsets")
        if self.dwell.size != self.off[-1] or self.state.size != self.off[-1]:
            raise ValueError("dwell and state must hold off[-1] segments")

    @property
    def n_hist(self):
        return (self.off.size - 1) // self.n_edge

    def __len__(self):
        return self.n_hist

    def counts(self):
        """segments per row, [R, E]"""
        return np.diff(self.off).reshape(self.n_hist, self.n_edge)

    def branch(self, r, b):
        """(dwell, state) of history r on edge row b (0-based)"""
        k = int(r) * self.n_edge + int(b)
        lo, hi = self.off[k], self.off[k + 1]
        return self.dwell[lo:hi], self.state[lo:hi]

    def history(self, r):
        """history r as a phm_tree triple: (map_off int32 [E + 1] from 0, maps, mapnames)"""
        lo, hi = self.off[int(r) * self.n_edge], self.off[(int(r) + 1) * self.n_edge]
        off = self.off[int(r) * self.n_edge:(int(r) + 1) * self.n_edge + 1] - lo
        return off.astype(np.int32), self.dwell[lo:hi], self.state[lo:hi]

    def mapped_edge(self, n):
        """[R, E, n] time spent in each state on each edge (makemappededge); segments added in row order"""
        rows = np.repeat(np.arange(self.off.size - 1), np.diff(self.off))
        out = np.zeros((self.off.size - 1, int(n)))
        np.add.at(out, (rows, self.state.astype(np.int64) - 1), self.dwell)
        return out.reshape(self.n_hist, self.n_edge, int(n))

    def _cumulative(self):
        """c[k]: the dwell of segments off[row] .. k of segment k's row, added in row order"""
        cnt = np.diff(self.off)
        start = self.off[:-1]
        c = self.dwell.copy()
        for j in range(1, int(cnt.max(initial=0))):
            idx = start[cnt > j] + j
            c[idx] = c[idx - 1] + self.dwell[idx]
        return c

    def _state_at(self, c, rows, s):
        """state of row rows[i] at s[i] from its parent end: segment k with c[k-1] < s <= c[k] (the first at s = 0, the last past
        the row's end)"""
        cnt = np.diff(self.off)[rows]
        if np.any(cnt < 1):
            raise ValueError("a row without segments has no state")
        start = self.off[rows]
        k = np.zeros(rows.size, dtype=np.int64)
        for j in range(int(cnt.max(initial=1)) - 1):
            live = j < cnt - 1
            k += live & (c[np.where(live, start + j, 0)] < s)
        return self.state[start + k]

    def states_at(self, edge_rows, positions):
        """[R, P] the state (1-based) of every history at each point: 0-based edge row, distance from the parent end (DESIGN.md
        section 16: the segment k with c[k-1] < s <= c[k], c the row's cumulative dwell in row order; s = 0 gives the first)"""
        b = np.asarray(edge_rows, dtype=np.int64).reshape(-1)
        s = np.asarray(positions, dtype=np.float64).reshape(-1)
        R, E = self.n_hist, self.n_edge
        rows = (np.arange(R)[:, None] * E + b[None, :]).ravel()
        return self._state_at(self._cumulative(), rows, np.tile(s, R)).reshape(R, b.size)

    def through_time(self, z, bounds, n):
        """Per history, the quantities whose expectations ``api.expected_through_time`` gives:
        ``(occupancy [R, K, n], bins [R, K - 1, n + n(n-1)])`` -- the lineages in each state at each bound, and the dwell in each
        state and the transitions (man/sumstatMCMC.Rd:18 column order) within depths [bounds[k], bounds[k+1]).  A branch counts at
        tau when d_parent < tau <= d_child, at s = tau - d_parent (t_b when tau >= d_child); bound 0 counts the root's state (the
        first segment of its lowest branch row).  A segment's dwell is split among the bins its depth interval overlaps; a
        transition belongs to the bin holding its depth."""
        edge = np.asarray(z["edge"], dtype=np.int64)
        E = edge.shape[0]
        if E != self.n_edge:
            raise ValueError("the tree and the maps have different edge counts")
        tau = np.asarray(bounds, dtype=np.float64).reshape(-1)
        K, n, R = tau.size, int(n), self.n_hist
        el = np.asarray(z["edge.length"], dtype=np.float64)
        d = node_depths(z)
        dp, dc = d[edge[:, 0] - 1], d[edge[:, 1] - 1]
        c = self._cumulative()
        hist = np.arange(R)
        occ = np.zeros((R, K, n))
        root = int(np.setdiff1d(edge[:, 0], edge[:, 1])[0])
        root_b = int(np.nonzero(edge[:, 0] == root)[0][0])
        for k, t in enumerate(tau):
            if t == 0.0:
                np.add.at(occ, (hist, k, self.state[self.off[hist * E + root_b]] - 1), 1.0)
            bs = np.nonzero((dp < t) & (t <= dc))[0]
            if bs.size:
                s = np.where(t >= dc[bs], el[bs], np.minimum(t - dp[bs], el[bs]))
                st = self._state_at(c, (hist[:, None] * E + bs[None, :]).ravel(), np.tile(s, R)) - 1
                np.add.at(occ, (np.repeat(hist, bs.size), k, st), 1.0)
        bins = np.zeros((R, max(K - 1, 0), n + n * (n - 1)))
        if K < 2 or self.dwell.size == 0:
            return occ, bins
        row = np.repeat(np.arange(self.off.size - 1), np.diff(self.off))
        h, b = row // E, row % E
        idx = np.arange(self.dwell.size)
        first = idx == self.off[row]
        lo = dp[b] + np.where(first, 0.0, c[np.maximum(idx - 1, 0)])
        hi = dp[b] + c
        st = self.state.astype(np.int64) - 1
        for k in range(K - 1):
            ov = np.minimum(hi, tau[k + 1]) - np.maximum(lo, tau[k])
            m = ov > 0
            np.add.at(bins, (h[m], k, st[m]), ov[m])
        nxt = np.nonzero(row[:-1] == row[1:])[0]                        # segment -> the next one of its row: a transition
        j = np.searchsorted(tau, hi[nxt], side="right") - 1
        a, z_ = st[nxt], st[nxt + 1]
        col = n + a * (n - 1) + np.where(z_ < a, z_, z_ - 1)
        ok = (j >= 0) & (j < K - 1)
        np.add.at(bins, (h[nxt][ok], j[ok], col[ok]), 1.0)
        return occ, bins

    def node_states(self):
        """[R, E, 2] (parent state, child state) of every edge (nodestatesmake): the first and the last segment of each row"""
        if np.any(np.diff(self.off) < 1):
            raise ValueError("a row without segments has no end states")
        first = self.state[self.off[:-1]]
        last = self.state[self.off[1:] - 1]
        return np.stack([first, last], axis=-1).reshape(self.n_hist, self.n_edge, 2)


def node_depths(z):
    """[n_tips + Nnode] depth of every node by ape node id (index id - 1): 0 at the root, a child's depth its parent's plus the edge
    length -- one addition per node, so these are the depths phm_expected_through_time uses, bit for bit."""
    edge = np.asarray(z["edge"], dtype=np.int64)
    el = np.asarray(z["edge.length"], dtype=np.float64)
    N = edge.shape[0] + 1
    kids = [[] for _ in range(N + 1)]
    for b in range(edge.shape[0]):
        kids[edge[b, 0]].append(b)
    stack = [int(np.setdiff1d(edge[:, 0], edge[:, 1])[0])]
    d = np.zeros(N)
    while stack:
        p = stack.pop()
        for b in kids[p]:
            c = int(edge[b, 1])
            d[c - 1] = d[p - 1] + el[b]
            stack.append(c)
    return d


def history_tree(z, maps, r, n=None, observe=None):
    """A copy of the tree ``z`` carrying history ``r`` of ``maps`` (divtophy): ``maps`` / ``mapnames`` per edge row,
    ``node.states`` [E, 2], ``mapped.edge`` [E, n] and ``states`` = the history's tip states (mapped through ``observe`` when
    given: the simulator's reported tips).  ``n`` defaults to the largest state in the history.  The result is a valid input tree
    of sumstatMCMC / SPARSEsumstatMCMC / sumstatEXP."""
    edge = np.asarray(z["edge"])
    E = edge.shape[0]
    if E != maps.n_edge:
        raise ValueError("the tree and the maps have different edge counts")
    off, dwell, state = maps.history(r)
    n = int(state.max()) if n is None else int(n)
    out = dict(z)
    out["maps"] = [dwell[off[b]:off[b + 1]].copy() for b in range(E)]
    out["mapnames"] = [state[off[b]:off[b + 1]].copy() for b in range(E)]
    ns = np.stack([state[off[:-1]], state[off[1:] - 1]], axis=1).astype(np.int32)
    out["node.states"] = ns
    me = np.zeros((E, n))
    rows = np.repeat(np.arange(E), np.diff(off))
    np.add.at(me, (rows, state.astype(np.int64) - 1), dwell)
    out["mapped.edge"] = me
    T = E - int(z["Nnode"]) + 1
    tips = np.zeros(T, dtype=np.int32)
    is_tip = edge[:, 1] <= T
    tips[edge[is_tip, 1] - 1] = ns[is_tip, 1]
    if observe is not None:
        tips = np.asarray(observe, dtype=np.int32)[tips - 1]
    out["states"] = tips
    return out
