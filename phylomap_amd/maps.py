"""Stochastic maps of sampled and simulated histories (DESIGN.md sections 14 and 15): what ``api.simulate_histories(..., maps=True)``,
``api.sumstatEXP(..., maps=True)`` and the fixed-Q MCMC drivers (``api.sumstatMCMC(..., maps=True)`` and its kin) return, and the
reference's helpers around a history (R/sourceme.R:1-60: ``makemappededge``, ``nodestatesmake``, ``divtophy``).

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

    def node_states(self):
        """[R, E, 2] (parent state, child state) of every edge (nodestatesmake): the first and the last segment of each row"""
        if np.any(np.diff(self.off) < 1):
            raise ValueError("a row without segments has no end states")
        first = self.state[self.off[:-1]]
        last = self.state[self.off[1:] - 1]
        return np.stack([first, last], axis=-1).reshape(self.n_hist, self.n_edge, 2)


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
