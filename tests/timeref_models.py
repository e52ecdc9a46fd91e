"""Python twin of the exact expectations through time under many rate matrices (DESIGN.md section 28,
phm_expected_through_time_models): ``timeref.through_time`` once per model, stacked.  timeref itself is not changed.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import timeref


def through_time_models(edge, edge_length, Qs, pid, states, bounds=None, points=None, observe=None, site_of_model=None):
    """dict: loglik [K, S]; with bounds, occupancy [K, S, n_bounds, n] and (two bounds or more) bins
    [K, S, n_bounds - 1, n + n(n-1)]; with points = (edge rows, positions), points [K, S, P, n].  ``pid``: n values shared by the
    models, or [K, n].  ``site_of_model``: model k on row ``site_of_model[k]`` of ``states`` alone; the S axis is then absent."""
    Qs = np.asarray(Qs, dtype=np.float64)
    if Qs.ndim == 2:
        Qs = Qs[None]
    K = Qs.shape[0]
    pid = np.atleast_2d(np.asarray(pid, dtype=np.float64))
    states = np.atleast_2d(np.asarray(states))
    per_model = []
    for k in range(K):
        tips = states if site_of_model is None else states[int(site_of_model[k])][None]
        per_model.append(timeref.through_time(edge, edge_length, Qs[k], pid[k if pid.shape[0] > 1 else 0], tips, bounds=bounds,
                                              points=points, observe=observe))
    out = {key: np.stack([r[key] for r in per_model]) for key in per_model[0]}
    if site_of_model is not None:
        out = {key: v[:, 0] for key, v in out.items()}
    return out
