"""Python twin of phm_loglik_models: log p(tips_s | Q_k, pid_k) for K models, one model at a time through
``exactref.passes`` (scipy ``expm``, numpy passes) -- an independent text, not a restatement of phm_loglik.hip.  Also the exact
score in log theta from ``exactref.expected``, the check no fit code produces.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import exactref


def loglik_models(edge, edge_length, Qs, pid, states, observe=None, site_of_model=None):
    """[K, S] (cross) or [K] (paired: model k on site ``site_of_model[k]``).  ``pid``: n values or [K, n]."""
    Qs = np.asarray(Qs, dtype=np.float64)
    states = np.atleast_2d(np.asarray(states))
    pid = np.atleast_2d(np.asarray(pid, dtype=np.float64))
    K = Qs.shape[0]
    out = np.zeros(K) if site_of_model is not None else np.zeros((K, states.shape[0]))
    for k in range(K):
        y = states if site_of_model is None else states[int(site_of_model[k])][None]
        with np.errstate(divide="ignore", invalid="ignore"):
            ll = exactref.passes(edge, edge_length, Qs[k], pid[k if pid.shape[0] > 1 else 0], y, observe)["loglik"]
        ll = np.where(np.isfinite(ll), ll, -np.inf)
        out[k] = ll[0] if site_of_model is not None else ll
    return out


def batch(edge, edge_length, pid, states, observe=None, per_site=False):
    """the callable ``fit.fit`` takes: joint over the sites (summed) or one problem per site"""
    def f(Qs, owner):
        if per_site:
            return loglik_models(edge, edge_length, Qs, pid, states, observe, site_of_model=owner)
        return loglik_models(edge, edge_length, Qs, pid, states, observe).sum(axis=1)
    return f


def exact_score(model, theta, stats):
    """g_c = sum_ij dq_ij / dlog theta_c (E[N_ij] / q_ij - E[dwell_i]) from one row of expected statistics (n dwell columns, then
    the off-diagonal counts row by row).  Entries with q_ij = 0 have E[N_ij] = 0 and contribute nothing."""
    n = model.n
    Q = model.Q(theta)
    dQ = model.dQ_dlog(theta)
    dwell = np.asarray(stats[:n])
    g = np.zeros(model.p)
    for c in range(model.p):
        for col, (i, j) in enumerate(exactref.columns(n)):
            if dQ[c, i, j] != 0.0:
                g[c] += dQ[c, i, j] * (stats[n + col] / Q[i, j] - dwell[i])
    return g
