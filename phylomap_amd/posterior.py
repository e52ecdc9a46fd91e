"""What one does with the traces of ``api.posterior_rates``: the rate matrices of a trace row as the driver
builds them, summaries with split-R-hat over the chains of one site, and DIC.
"""
from __future__ import annotations

import numpy as np


def rate_matrices(model, thetas):
    """[K, n, n] generators of an index model for [K, p] parameter vectors, bit for bit the matrices phm_gibbs_rates evaluates:
    q_ij = theta_c for ``model.index[i, j] = c``, 0 for a structural zero, and the diagonal minus the row's off-diagonal entries
    summed left to right (``RateModel.Qs`` leaves the order of that sum to numpy, which pairs the terms from 8 states on)."""
    if getattr(model, "index", None) is None:
        raise ValueError("an index model is needed")
    thetas = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
    K, n = thetas.shape[0], model.n
    table = np.concatenate([np.zeros((K, 1)), thetas], axis=1)
    Q = table[:, np.asarray(model.index)]
    idx = np.arange(n)
    Q[:, idx, idx] = 0.0
    row = np.zeros((K, n))
    for j in range(n):
        row = row + Q[:, :, j]
    Q[:, idx, idx] = -row
    return Q


def split_rhat(x):
    """Split-R-hat (Gelman et al., BDA3 section 11.4) of x [iterations, chains]: every chain cut in halves, B the between- and W
    the within-sequence variance of the 2 * chains sequences of length L, sqrt(((L - 1) / L W + B / L) / W).  NaN with fewer than
    four iterations; 1 when W = B = 0."""
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[0] // 2
    if L < 2:
        return float("nan")
    seq = np.concatenate([x[:L], x[x.shape[0] - L:]], axis=1)               # [L, 2 chains]
    means = seq.mean(axis=0)
    W = float(seq.var(axis=0, ddof=1).mean())
    B = L * float(means.var(ddof=1))
    if W == 0.0:
        return 1.0 if B == 0.0 else float("inf")
    return float(np.sqrt(((L - 1) / L * W + B / L) / W))


def summary(trace, burn=0, probs=(0.025, 0.5, 0.975)):
    """Summaries of a trace [rows, chains, p] (``result["theta"]``, or the result dict itself; a per-site result
    [rows, S, chains, p] is summarised site by site and every value gets a leading site axis) after dropping the first ``burn``
    rows: mean [p], sd [p] (over all kept draws, ddof = 1), quantiles [len(probs), p], rhat [p] (split-R-hat over the chains) and
    n, the number of kept draws.  Chains that failed (NaN rows) are left out."""
    x = np.asarray(trace["theta"] if isinstance(trace, dict) else trace, dtype=np.float64)
    if x.ndim == 4:
        parts = [summary(x[:, s], burn, probs) for s in range(x.shape[1])]
        return {k: np.stack([q[k] for q in parts]) for k in parts[0]}
    if x.ndim != 3:
        raise ValueError("trace must be [rows, chains, p]")
    x = x[int(burn):]
    x = x[:, ~np.isnan(x).any(axis=(0, 2))]
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("no draws left")
    flat = x.reshape(-1, x.shape[2])
    return dict(mean=flat.mean(axis=0), sd=flat.std(axis=0, ddof=1) if flat.shape[0] > 1 else np.full(x.shape[2], np.nan),
                quantiles=np.quantile(flat, probs, axis=0), rhat=np.array([split_rhat(x[:, :, c]) for c in range(x.shape[2])]),
                n=flat.shape[0])


def dic_from(loglik, D):
    """(DIC, D, pD) from the kept log-likelihoods and D = -2 log p(tips | posterior-mean theta): pD = mean(-2 l) - D,
    DIC = D + 2 pD (tools/squamate_dic/run_dic.py's definition)."""
    pD = float(np.mean(-2.0 * np.asarray(loglik, dtype=np.float64))) - float(D)
    return float(D) + 2.0 * pD, float(D), pD


def dic(result, burn, z, pid, sites=None, observe=None, **opt):
    """DIC of a joint ``api.posterior_rates`` result: the chains that ran are pooled, the first ``burn`` rows dropped, and D is
    evaluated at the posterior-mean theta through ``api.loglik_models`` (summed over the sites).  Returns a dict: DIC, D, pD,
    theta_mean.  A per-site result gives one value per site (paired evaluation)."""
    from . import api
    model = result["model"]
    th, ll = np.asarray(result["theta"])[int(burn):], np.asarray(result["loglik"])[int(burn):]
    if not result.get("per_site", False):
        th, ll = th[:, None], ll[:, None]                                   # one "site": the joint problem
    S = th.shape[1]
    ok = ~np.isnan(ll).any(axis=0)                                          # [S, chains]
    mean = np.stack([th[:, s][:, ok[s]].reshape(-1, model.p).mean(axis=0) for s in range(S)])
    Qs = rate_matrices(model, mean)
    if result.get("per_site", False):
        at = api.loglik_models(z, Qs, pid, sites=sites, observe=observe, site_of_model=np.arange(S, dtype=np.int32), **opt)
    else:
        at = api.loglik_models(z, Qs, pid, sites=sites, observe=observe, **opt).sum(axis=1)
    vals = [dic_from(ll[:, s][:, ok[s]], -2.0 * float(at[s])) for s in range(S)]
    out = dict(DIC=np.array([v[0] for v in vals]), D=np.array([v[1] for v in vals]), pD=np.array([v[2] for v in vals]),
               theta_mean=mean)
    return out if result.get("per_site", False) else {k: v[0] for k, v in out.items()}


def predictive_rows(result, burn=0, draws=None):
    """The theta rows ``predictive`` simulates under: the rows of ``result["theta"]`` after the first ``burn``, over all chains
    (and sites), flattened row-major to [N, p]; ``draws`` = M thins them evenly to rows ``(j N) // M``, j = 0 .. M - 1."""
    th = np.asarray(result["theta"], dtype=np.float64)
    th = th[int(burn):].reshape(-1, th.shape[-1])
    N = th.shape[0]
    if N < 1:
        raise ValueError("no draws left")
    if draws is not None:
        M = int(draws)
        if M < 1 or M > N:
            raise ValueError(f"draws must be in 1..{N}")
        th = th[(np.arange(M, dtype=np.int64) * N) // M]
    if not np.all(np.isfinite(th)):
        raise ValueError("the selected rows hold a chain that failed (NaN rates)")
    return th


def predictive(result, z, pid, burn=0, draws=None, observe=None, **opt):
    """Posterior-predictive replicates of an ``api.posterior_rates`` result: one dataset simulated forward under every kept draw
    of the rates, all in one ``api.simulate_histories_models`` call (R = 1, the models across the lanes).  The rows are
    ``predictive_rows(result, burn, draws)``.  Returns a dict: theta [M, p], tips [M, n_tips] (1-based, through ``observe``) and
    stats [M, n + n*n + 1] in ``api.simulate_histories``' columns.  Row m is ``api.simulate_histories(z, Q(theta[m]), pid, 1,
    replica_offset=replica_offset + m)``'s.  Options: seed, replica_offset, device, devices."""
    from . import api
    th = predictive_rows(result, burn, draws)
    tips, stats = api.simulate_histories_models(z, rate_matrices(result["model"], th), pid, 1, observe=observe, **opt)[:2]
    return dict(theta=th, tips=tips[:, 0], stats=stats[:, 0])


def ppp(t_obs, t_rep):
    """Posterior-predictive p-value of a test quantity: mean(t_rep > t_obs) + mean(t_rep == t_obs) / 2 over the replicates
    (ties count half, so a discrete quantity is not biased towards either tail)."""
    t_rep = np.asarray(t_rep, dtype=np.float64).reshape(-1)
    if t_rep.size < 1:
        raise ValueError("no replicates")
    return float(np.mean(t_rep > t_obs) + 0.5 * np.mean(t_rep == t_obs))
