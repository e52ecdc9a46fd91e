"""Helpers around ``api.ancestral_states_models`` (DESIGN.md sections 21 and 23): model weights, model-averaged node posteriors,
the node id of a clade's ancestor and node posteriors collapsed onto what is observed.  numpy only, no device."""
from __future__ import annotations

import numpy as np


def akaike_weights(loglik, n_params):
    """Akaike weights of K models: w_k proportional to exp(-(AIC_k - min AIC) / 2), AIC_k = 2 n_params_k - 2 loglik_k.
    ``n_params``: K values, or one shared by every model.  A model with ``loglik`` = -inf gets weight 0 (all -inf: ValueError)."""
    ll = np.asarray(loglik, dtype=np.float64).reshape(-1)
    aic = 2.0 * np.broadcast_to(np.asarray(n_params, dtype=np.float64), ll.shape) - 2.0 * ll
    if not np.any(np.isfinite(aic)):
        raise ValueError("every model has loglik = -inf")
    w = np.where(np.isfinite(aic), np.exp(-0.5 * (aic - np.min(aic[np.isfinite(aic)]))), 0.0)
    return w / np.sum(w)


def model_average(node_post, weights=None, axis=0):
    """Weighted mean of ``node_post`` over its model axis.  ``weights``: one non-negative value per model, normalised here
    (``akaike_weights``); None: equal weights, as for a posterior sample of Q.  A model of weight 0 is left out, so it may hold
    NaN (an impossible evaluation).  Nothing here is particular to node posteriors: any array with a model axis is averaged the
    same way, ``api.expected_branch_stats_models``' ``branch`` ([K, S, n_sel, C] or [K, n_sel, C]) included -- the per-branch
    expectations under rate uncertainty."""
    post = np.moveaxis(np.asarray(node_post, dtype=np.float64), axis, 0)
    K = post.shape[0]
    w = np.full(K, 1.0) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.size != K:
        raise ValueError("weights must have one entry per model")
    if np.any(w < 0.0) or not np.sum(w) > 0.0:
        raise ValueError("weights must be non-negative with a positive sum")
    w = w / np.sum(w)
    out = np.zeros(post.shape[1:])
    for k in range(K):
        if w[k] > 0.0:
            out += w[k] * post[k]
    return out


def average_over_models(values, weights=None):
    """``model_average`` over the leading K axis, under the name the through-time results use: any part of
    ``api.expected_through_time_models`` (``occupancy``, ``bins``, ``point_post``; [K, S, ...] or [K, ...]) averaged with
    ``akaike_weights`` or, ``weights`` None, equally as for a posterior sample of Q.  One function: this is ``model_average``."""
    return model_average(values, weights, axis=0)


def collapse_states(node_post, observe):
    """Node posteriors of the OBSERVED character: ``node_post`` [..., n] summed over the states that share an observation -- the
    amino acid behind the codons, the observed character behind hidden-rate classes.  ``observe``: the n 1-based observations of
    the states, as given to ``api.ancestral_states_models``.  Returns [..., n_obs], n_obs = max(observe); a NaN row (an impossible
    evaluation) stays NaN.  The joint reconstruction needs no function: ``observe[joint_states - 1]`` where ``joint_states`` > 0."""
    post = np.asarray(node_post, dtype=np.float64)
    obs = np.asarray(observe, dtype=np.int64).reshape(-1)
    if post.ndim < 1 or obs.size != post.shape[-1]:
        raise ValueError("observe must have one entry per state of node_post")
    if obs.size == 0 or np.any(obs < 1):
        raise ValueError("observe must hold 1-based observations")
    out = np.zeros(post.shape[:-1] + (int(obs.max()),))
    for i, o in enumerate(obs):                         # state order: the sums do not depend on how the states are grouped
        out[..., o - 1] += post[..., i]
    return out


def mrca(z, tips):
    """Ape node id of the most recent common ancestor of the 1-based tip ids ``tips`` in the tree ``z`` (``z['edge']``,
    ``z['Nnode']``); a single tip is its own ancestor.  The id can go into ``api.ancestral_states_models(nodes=...)``."""
    edge = np.asarray(z["edge"], dtype=np.int64)
    T = edge.shape[0] - int(z["Nnode"]) + 1
    tips = [int(t) for t in np.atleast_1d(tips)]
    if not tips or any(t < 1 or t > T for t in tips):
        raise ValueError(f"tips must be ids in 1..{T}")
    parent = {int(c): int(p) for p, c in edge}

    def path(v):                                        # v, its parent, ..., the root
        out = [v]
        while out[-1] in parent:
            out.append(parent[out[-1]])
        return out

    common = path(tips[0])
    for t in tips[1:]:
        on = set(path(t))
        common = [v for v in common if v in on]
    return common[0]
