"""Maximum-likelihood fit of a parametrised rate matrix over a BATCHED likelihood.  numpy only.

``fit(batch, model, ...)`` takes the likelihood as a callable ``batch(Qs [K, n, n], owner [K]) -> [K]`` -- the log-likelihood of
model k on problem ``owner[k]`` (``api.loglik_models`` on the device; ``tests/fitref.py`` on the CPU) -- and runs every start of
every problem in lock-step: each iteration gathers what every live run needs into ONE call of ``batch``.

The optimiser works in x = log(theta) and minimises phi = -log l by BFGS:

* gradient by central differences, ``h = 1e-4`` in log theta: error eps_l / h + O(h^2), about 1e-7 for |log l| ~ 1e2;
* a step is d = -H g with max|d_i| capped at 2 (a factor e^2 per rate and iteration), clipped to the box; the line search is a
  ladder alpha = 1, 1/4, 1/16, 1/64 (Armijo, c1 = 1e-4), all four rungs evaluated in the same call together with the 2p
  gradient points around the FIRST rung.  When the first rung is accepted (the usual case) the run has its next gradient
  already; when a lower rung is accepted its next contribution to the call is the 2p gradient points alone; when none is, the
  inverse Hessian is reset and the ladder shrinks by 256, and a run whose steps fall below 1e-10 stops unconverged;
* box bounds in log theta, default ``log(rate0) + (log 1e-6, log 1e4)`` with rate0 = number of tips / tree length: components on
  a bound whose gradient points outward are held (their direction entries zeroed) and left out of the convergence test
  ``max |g_i| <= gtol``; a parameter that ends on a bound is reported in ``at_bound``, not an error;
* a start whose first evaluation is not finite is dropped (its entry of ``starts`` keeps ``-inf``); a candidate that is not
  finite simply fails the line search.

``gradient="exact"`` replaces the difference gradient by the exact score
g_c = sum_ij dq_ij / dlog theta_c (E[N_ij] / q_ij - E[dwell_i]) (``RateModel.score``) from a batched statistics callable
``batch_stats(Qs, owner) -> (loglik [K], stats [K, cols])``.  All four rungs of the ladder go through that one call, so whichever
rung is accepted brings its gradient with it: an iteration is 4 evaluations (statistics included) where ``"fd"`` makes 2p + 4
likelihood evaluations, there is no gradient-only call after a lower rung, and ``gtol`` is no longer held up at the 1e-7 of the
differences.  ``"fd"`` stays the default and is what it was bit for bit.

Start 0 is deterministic (every rate = rate0); the others are log-normal around it (sigma = 1 in log theta) from the Philox
stream of ``seed``, the same for every problem, so a fit is reproducible bit for bit.
"""
from __future__ import annotations

import math

import numpy as np

from .synth import PhiloxStream

H_FD = 1e-4
LADDER = (1.0, 0.25, 0.0625, 0.015625)
STEP_CAP = 2.0
C1 = 1e-4
DEFAULT_BOUNDS = (1e-6, 1e4)          # times rate0


def start_points(p, rate0, starts, seed, lo, hi):
    """[starts, p] in log theta: row 0 = log(rate0), the rest N(log rate0, 1) by Box-Muller on PhiloxStream(seed, 11), clipped."""
    rs = PhiloxStream(int(seed), stream=11)
    X = np.full((starts, p), math.log(rate0))
    for r in range(1, starts):
        for c in range(p):
            u1, u2 = rs.uniform(), rs.uniform()
            X[r, c] += math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)
    return np.clip(X, lo, hi)


class _Run:
    __slots__ = ("prob", "x", "f", "g", "H", "d", "state", "scale", "fresh", "prev", "iters", "converged", "alive")

    def __init__(self, prob, x, p):
        self.prob, self.x, self.f, self.g = prob, x.copy(), None, None
        self.H, self.d = np.eye(p), None
        self.state = "grad"            # "grad": needs the gradient at x; "search": has a direction; "done"
        self.scale = 1.0               # multiplies the ladder
        self.fresh = True              # H is still the identity (scaled at the first update)
        self.prev = None               # (x, g) of the point the last accepted step left
        self.iters, self.converged, self.alive = 0, False, True


def _fd_points(x, p):
    pts = np.repeat(x[None], 2 * p, axis=0)
    for c in range(p):
        pts[2 * c, c] += H_FD
        pts[2 * c + 1, c] -= H_FD
    return pts


def _fd_grad(vals, p):
    """gradient of phi = -log l from the 2p values of log l"""
    return np.array([-(vals[2 * c] - vals[2 * c + 1]) / (2.0 * H_FD) for c in range(p)])


def _held(x, g, lo, hi):
    """components on a bound whose descent direction -g points out of the box"""
    return ((x <= lo) & (g > 0.0)) | ((x >= hi) & (g < 0.0))


def _advance(r, g, lo, hi, gtol):
    """the gradient at r.x has arrived: BFGS update from the previous point, convergence test, next direction"""
    if not np.all(np.isfinite(g)):
        r.g = g
        r.state = "done"
        return
    if r.prev is not None:
        s, y = r.x - r.prev[0], g - r.prev[1]
        sy = float(s @ y)
        if sy > 1e-12 * float(np.linalg.norm(s) * np.linalg.norm(y)) and sy > 0.0:
            if r.fresh:
                r.H = np.eye(s.size) * (sy / float(y @ y))
                r.fresh = False
            rho = 1.0 / sy
            V = np.eye(s.size) - rho * np.outer(s, y)
            r.H = V @ r.H @ V.T + rho * np.outer(s, s)
        r.prev = None
    r.g = g
    held = _held(r.x, g, lo, hi)
    if not np.any(~held) or float(np.max(np.abs(g[~held]))) <= gtol:
        r.converged = True
        r.state = "done"
        return
    free = ~held
    d = np.zeros_like(g)
    d[free] = -(r.H[np.ix_(free, free)] @ g[free])
    if not (float(d @ g) < 0.0):                       # not a descent direction: steepest descent
        d = np.where(free, -g, 0.0)
        r.H, r.fresh = np.eye(g.size), True
    m = float(np.max(np.abs(d)))
    if m > STEP_CAP:
        d *= STEP_CAP / m
    r.d = d
    r.state = "search"


def fit(batch, model, n_problems, rate0, starts=8, seed=0, gtol=1e-5, max_iter=200, bounds=None, gradient="fd", batch_stats=None):
    """Fits ``model`` on ``n_problems`` problems at once.  ``bounds``: (lower, upper) for theta, scalars or p values each
    (default ``DEFAULT_BOUNDS`` times ``rate0``).  Returns a dict with a leading problem axis: theta [P, p], Q [P, n, n],
    loglik [P], aic [P] (2p - 2 log l), iterations [P], converged [P], at_bound [P, p], grad [P, p] (the last finite-difference
    gradient of log l in log theta; the exact score with ``gradient="exact"``), starts {"loglik": [P, R], "theta": [P, R, p]},
    calls (batched calls made), evals (models evaluated over all calls).  ``gradient="exact"`` needs ``batch_stats`` (module
    docstring) and does not use ``batch``."""
    p, P, R = model.p, int(n_problems), int(starts)
    if R < 1:
        raise ValueError("starts must be >= 1")
    if gradient not in ("fd", "exact"):
        raise ValueError('gradient must be "fd" or "exact"')
    exact = gradient == "exact"
    if exact and batch_stats is None:
        raise ValueError('gradient="exact" needs batch_stats')
    b = (DEFAULT_BOUNDS[0] * rate0, DEFAULT_BOUNDS[1] * rate0) if bounds is None else bounds
    lo = np.log(np.broadcast_to(np.asarray(b[0], dtype=np.float64), (p,))).copy()
    hi = np.log(np.broadcast_to(np.asarray(b[1], dtype=np.float64), (p,))).copy()
    X0 = start_points(p, rate0, R, seed, lo, hi)
    runs = [_Run(s, X0[r], p) for s in range(P) for r in range(R)]
    calls = evals = 0
    for _ in range(int(max_iter)):
        rows, owner, plan = [], [], []
        for r in runs:
            if r.state == "done":
                continue
            k0 = len(rows)
            if exact:                                      # the point itself, or the ladder: each brings its own score
                pts = r.x[None] if r.state == "grad" else np.clip(r.x[None] + np.outer(np.array(LADDER) * r.scale, r.d), lo, hi)
            elif r.state == "grad":
                pts = _fd_points(r.x, p)
                if r.f is None:
                    pts = np.concatenate([r.x[None], pts])
            else:
                cand = np.clip(r.x[None] + np.outer(np.array(LADDER) * r.scale, r.d), lo, hi)
                pts = np.concatenate([cand, _fd_points(cand[0], p)])
            rows.extend(pts)
            owner.extend([r.prob] * len(pts))
            plan.append((r, k0, len(pts)))
        if not plan:
            break
        thetas = np.exp(np.asarray(rows))
        evals += len(rows)
        if exact:
            vals, stats = batch_stats(model.Qs(thetas), np.asarray(owner, dtype=np.int32))
            vals, stats = np.asarray(vals, dtype=np.float64), np.asarray(stats, dtype=np.float64)
        else:
            vals = np.asarray(batch(model.Qs(thetas), np.asarray(owner, dtype=np.int32)), dtype=np.float64)
        calls += 1
        for r, k0, cnt in plan:
            v = vals[k0:k0 + cnt]
            if exact and r.state == "grad":
                if r.f is None:
                    r.f = -float(v[0])
                    if not math.isfinite(r.f):             # impossible under this start: dropped
                        r.alive, r.state = False, "done"
                        continue
                _advance(r, -model.score(thetas[k0], stats[k0]), lo, hi, gtol)
                continue
            if r.state == "grad":
                if r.f is None:
                    r.f = -float(v[0])
                    v = v[1:]
                    if not math.isfinite(r.f):         # impossible under this start: dropped
                        r.alive, r.state = False, "done"
                        continue
                _advance(r, _fd_grad(v, p), lo, hi, gtol)
                continue
            C = len(LADDER)
            cand = np.clip(r.x[None] + np.outer(np.array(LADDER) * r.scale, r.d), lo, hi)
            taken = -1
            for c in range(C):
                fc = -float(v[c])
                if math.isfinite(fc) and fc <= r.f + C1 * float(r.g @ (cand[c] - r.x)) and np.any(cand[c] != r.x):
                    taken = c
                    break
            if taken < 0:
                if not r.fresh:
                    r.H, r.fresh, r.scale = np.eye(p), True, 1.0
                    _advance(r, r.g, lo, hi, gtol)
                else:
                    r.scale *= LADDER[-1] / 4.0
                    if r.scale * float(np.max(np.abs(r.d))) < 1e-10:
                        r.state = "done"
                continue
            r.prev = (r.x, r.g)
            r.x, r.f = cand[taken], -float(v[taken])
            r.iters += 1
            if taken == 0:
                r.scale = min(1.0, r.scale * 16.0)
            if exact:
                _advance(r, -model.score(thetas[k0 + taken], stats[k0 + taken]), lo, hi, gtol)
            elif taken == 0:
                _advance(r, _fd_grad(v[C:], p), lo, hi, gtol)
            else:
                r.state = "grad"

    out = dict(theta=np.zeros((P, p)), Q=np.zeros((P, model.n, model.n)), loglik=np.full(P, -np.inf), aic=np.full(P, np.inf),
               iterations=np.zeros(P, dtype=np.int64), converged=np.zeros(P, dtype=bool), at_bound=np.zeros((P, p), dtype=bool),
               grad=np.full((P, p), np.nan), starts=dict(loglik=np.full((P, R), -np.inf), theta=np.zeros((P, R, p))), calls=calls, evals=evals)
    for s in range(P):
        mine = runs[s * R:(s + 1) * R]
        best = None
        for k, r in enumerate(mine):
            out["starts"]["theta"][s, k] = np.exp(r.x)
            if r.alive and r.f is not None:
                out["starts"]["loglik"][s, k] = -r.f
                if best is None or r.f < best.f:
                    best = r
        r = best if best is not None else mine[0]
        out["theta"][s] = np.exp(r.x)
        out["Q"][s] = model.Q(out["theta"][s])
        if best is not None:
            out["loglik"][s] = -r.f
            out["aic"][s] = 2.0 * p + 2.0 * r.f
            out["grad"][s] = -r.g if r.g is not None else np.nan
        out["iterations"][s], out["converged"][s] = r.iters, r.converged
        out["at_bound"][s] = (r.x <= lo + 1e-12) | (r.x >= hi - 1e-12)
    return out


def information(batch_stats, model, theta, owner, h=1e-4):
    """Observed information of log l in log theta at ``theta`` ([P, p], or [p] for one problem), problem ``owner[i]`` for row i:
    J = -d score / d log theta by central differences of the exact score at theta exp(+-h e_c) -- one call of ``batch_stats`` with
    2p models per problem -- symmetrised.  Truncation O(h^2) = 1e-8; rounding about 1e-10 / h = 1e-6 for a score good to 1e-10.
    Returns [P, p, p] (or [p, p])."""
    th = np.asarray(theta, dtype=np.float64)
    one = th.ndim == 1
    th = np.atleast_2d(th)
    P, p = th.shape
    owner = np.asarray(owner, dtype=np.int32).reshape(-1)
    x = np.log(th)
    pts = np.concatenate([_fd_points_h(x[i], p, h) for i in range(P)])
    thetas = np.exp(pts)
    _, stats = batch_stats(model.Qs(thetas), np.repeat(owner, 2 * p))
    stats = np.asarray(stats, dtype=np.float64)
    J = np.zeros((P, p, p))
    for i in range(P):
        g = np.array([model.score(thetas[i * 2 * p + k], stats[i * 2 * p + k]) for k in range(2 * p)])
        for c in range(p):
            J[i, c] = -(g[2 * c] - g[2 * c + 1]) / (2.0 * h)
        J[i] = 0.5 * (J[i] + J[i].T)
    return J[0] if one else J


def _fd_points_h(x, p, h):
    pts = np.repeat(x[None], 2 * p, axis=0)
    for c in range(p):
        pts[2 * c, c] += h
        pts[2 * c + 1, c] -= h
    return pts


INFO_NOISE = 1e-6                     # what central differences (h = 1e-4) of a score good to 1e-10 resolve in an entry of J


def standard_errors(batch_stats, model, theta, owner, at_bound, h=1e-4):
    """Wald standard errors in log theta from ``information`` for theta [P, p]: cov_log [P, p, p] = J^-1 over the parameters that
    are not on a bound (those are left out of the inversion; their rows, columns, se and interval are NaN), se_log [P, p] =
    sqrt(diag), ci [P, p, 2] = theta exp(-+1.96 se_log), se_ok [P], information [P, p, p].  A J that is not positive definite
    over the free parameters -- its smallest eigenvalue not above ``INFO_NOISE`` max(1, max |J_ij|), what the differences can tell
    from zero: a flat direction -- gives NaN throughout and se_ok = False, not an exception."""
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    at_bound = np.atleast_2d(np.asarray(at_bound, dtype=bool))
    P, p = theta.shape
    J = np.atleast_3d(information(batch_stats, model, theta, owner, h=h)).reshape(P, p, p)
    cov = np.full((P, p, p), np.nan)
    ok = np.zeros(P, dtype=bool)
    for i in range(P):
        free = ~at_bound[i]
        if not np.any(free) or not np.all(np.isfinite(J[i][np.ix_(free, free)])):
            continue
        Jf = J[i][np.ix_(free, free)]
        if float(np.min(np.linalg.eigvalsh(Jf))) <= INFO_NOISE * max(1.0, float(np.max(np.abs(Jf)))):
            continue
        cov[i][np.ix_(free, free)] = np.linalg.inv(Jf)
        ok[i] = True
    se = np.sqrt(np.einsum("kii->ki", cov))
    ci = np.stack([theta * np.exp(-1.96 * se), theta * np.exp(1.96 * se)], axis=-1)
    return dict(cov_log=cov, se_log=se, ci=ci, se_ok=ok, information=J)


def first_problem(r):
    """the result of a one-problem fit without its leading axis"""
    out = {k: (v[0] if isinstance(v, np.ndarray) else v) for k, v in r.items()}
    out["starts"] = {k: v[0] for k, v in r["starts"].items()}
    return out


def sample_thetas(result, M, seed=0):
    """``M`` draws of theta = exp(N(log theta_hat, cov_log)) from the result of a one-problem ``fit_ml(se=True)``: the models a
    caller hands to ``api.sample_histories`` for stochastic maps under rate uncertainty.  The normals are Box-Muller pairs
    (sqrt(-2 log u1) cos(2 pi u2), then the sine) over ``PhiloxStream(seed, 12)``, taken draw by draw and, within a draw, free
    parameter by free parameter, and coloured by the lower Cholesky factor of cov_log over the free parameters.  A parameter on
    a bound (NaN standard error) is held at theta_hat.  Raises ValueError when ``se_ok`` is false.  Returns [M, p]."""
    theta = np.asarray(result["theta"], dtype=np.float64)
    if theta.ndim != 1:
        raise ValueError("sample_thetas takes the result of one problem (index a per-site result first)")
    if "se_ok" not in result or not bool(np.all(result["se_ok"])):
        raise ValueError("the fit has no usable covariance (se_ok is false): no draws")
    cov = np.asarray(result["cov_log"], dtype=np.float64).reshape(theta.size, theta.size)
    free = np.isfinite(np.asarray(result["se_log"], dtype=np.float64).reshape(-1))
    pf = int(np.sum(free))
    M = int(M)
    out = np.repeat(theta[None], M, axis=0)
    if pf == 0 or M < 1:
        return out
    chol = np.linalg.cholesky(cov[np.ix_(free, free)])
    rng = PhiloxStream(seed, 12)
    total = M * pf
    z = np.empty(total + (total & 1))
    for i in range(0, z.size, 2):
        rad = math.sqrt(-2.0 * math.log(rng.uniform()))
        ang = 2.0 * math.pi * rng.uniform()
        z[i], z[i + 1] = rad * math.cos(ang), rad * math.sin(ang)
    z = z[:total].reshape(M, pf)
    out[:, free] = np.exp(np.log(theta[free])[None] + z @ chol.T)
    return out
