"""R-level API of phylomap, mirrored in Python (the reference's R toolchain is not available here).

Same names, argument order and meaning as the R wrappers: ``sumstatMCMC(z,Q,pid,Omega,N)``
(R/sumstatMCMC.R:21-29), ``sumstatMCMC_bigtree`` (R/sumstatMCMC_bigtree.R), ``SPARSEsumstatMCMC``
(R/SPARSEsumstatMCMC.R:21-29) and ``sumstatEXP(z,Q,pid,N)`` (R/sumstatEXP.R:21-33).  Each computes the
derived arguments exactly where the R wrapper does (``nen``, ``nodelist``, ``root``, ``B``; EXP:
``eigen``/``solve``) and then calls the C-ABI entry point that replaces the corresponding ``.Call``
(R/RcppExports.R:4-22).  Returns the N x (n + n(n-1)) matrix of man/sumstatMCMC.Rd:18.

Extra keyword arguments (``seed``, ``n_replicas``, ...) map onto ``phm_options``; with the defaults a
call is a drop-in for the R function (one chain, one tip vector).
"""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from . import _lib
from .treeorder import makenodelist, myreorder, pruningwiseedgeorder  # noqa: F401  (Python twins of phm_tree_orders)


_MCMC_VARIANT = {"phm_maketreelistMCMC": _lib.PHM_MCMC, "phm_maketreelistMCMC_bigtree": _lib.PHM_MCMC_BIGTREE,
                 "phm_SPARSEmaketreelistMCMC": _lib.PHM_MCMC_SPARSE, "phm_maketreelistMCMCks_sweep": _lib.PHM_MCMC_KS,
                 "phm_maketreelistMCMCbf_sweep": _lib.PHM_MCMC_BF}


def _one_model(Q, pid):
    """(n, Q column-major, pid) of one model as the library takes them"""
    Q = np.asfortranarray(np.asarray(Q, dtype=np.float64))
    return Q.shape[0], Q, np.ascontiguousarray(pid, dtype=np.float64)


def _model_args(Q, pid, Omega):
    """(n, the model run of every sweep's head): n, Q column-major, pid, B = I + Q / Omega (R/sumstatMCMC.R:25), Omega"""
    n, Q, pid = _one_model(Q, pid)
    B = np.asfortranarray(np.eye(n) + Q / Omega)
    return n, (n, _lib._p(Q, C.c_double), _lib._p(pid, C.c_double), _lib._p(B, C.c_double), float(Omega))


def _sweep_head(z, Q, pid, Omega, N, sites=None):
    """(tree, n, head) of a one-tree sweep; the head: tree, model run, nen, nodelist, root (R/sumstatMCMC.R:22-24, native O(E))
    and N.  ``_lib._p``'s pointers keep their arrays alive; the caller holds the tree, which owns the struct's arrays."""
    n, model = _model_args(Q, pid, Omega)
    nen, nodelist, root = _lib.tree_orders(z)
    ft = _lib.FlatTree(z, sites)
    return ft, n, (C.byref(ft.c),) + model + (_lib._p(nen, C.c_int32), _lib._p(nodelist, C.c_int32), root, int(N))


def _mcmc(fn_name, z, Q, pid, Omega, N, sites=None, maps=False, map_iters=None, **opt):
    """``sites``: optional S x n_tips matrix of 1-based tip states -- S sites of an alignment on the same tree, one chain each
    (``n_replicas = S``, ``tips_per_replica``); the initial paths of ``z`` must be compatible with every site (e.g. internal
    segments in a state from which every tip state is reachable).  ``maps=True``: returns ``(out, maps)`` with the chains'
    histories at the 0-based iterations ``map_iters`` (default: every iteration) as a ``maps.Maps`` -- history ``s * J + j`` is
    chain s at ``map_iters[j]`` (phm_maketreelistMCMC_maps: a sizing call, then a filling call; the (tile, branch) mapping)."""
    L = _lib.load()
    if sites is not None:
        sites = np.ascontiguousarray(np.asarray(sites).round(), dtype=np.int32)
        opt = dict(opt, n_replicas=sites.shape[0], tips_per_replica=True)
    ft, n, head = _sweep_head(z, Q, pid, Omega, N, sites)
    o = _lib.make_options(**opt)
    S = max(1, int(o.n_replicas))
    cols = _lib.stat_cols(n, {"phm_maketreelistMCMCks_sweep": "ks", "phm_maketreelistMCMCbf_sweep": "bf"}.get(fn_name, "plain"))
    single = bool(o.reduce) or S == 1
    out = np.zeros((N, cols), order="F") if single else np.zeros((S, cols, N))
    if not maps:
        _lib.check(getattr(L, fn_name)(*head, C.byref(o), _lib._p(out, C.c_double)))
        return out if single else out.transpose(0, 2, 1)
    if map_iters is None:
        its, J = None, int(N)
    else:
        its = np.ascontiguousarray(np.atleast_1d(map_iters), dtype=np.int32)
        J = int(its.size)
    args = (_MCMC_VARIANT[fn_name],) + head + (_lib._p(its, C.c_int32) if its is not None else None, 0 if its is None else J,
                                              C.byref(o), _lib._p(out, C.c_double))
    m = _two_phase_maps(L.phm_maketreelistMCMC_maps, args, S * J, ft.E)
    return (out if single else out.transpose(0, 2, 1)), m


def sumstatMCMC(z, Q, pid, Omega, N, maps=False, map_iters=None, **opt):
    """R/sumstatMCMC.R:21-29 -> phm_maketreelistMCMC.  ``maps=True``: ``(out, maps)`` with the sampled histories at the 0-based
    iterations ``map_iters`` (default: all), as for every fixed-Q MCMC driver below."""
    return _mcmc("phm_maketreelistMCMC", z, Q, pid, Omega, N, maps=maps, map_iters=map_iters, **opt)


def sumstatMCMC_bigtree(z, Q, pid, Omega, N, maps=False, map_iters=None, **opt):
    """R/sumstatMCMC_bigtree.R -> phm_maketreelistMCMC_bigtree (row-normalised partial likelihoods)."""
    return _mcmc("phm_maketreelistMCMC_bigtree", z, Q, pid, Omega, N, maps=maps, map_iters=map_iters, **opt)


def SPARSEsumstatMCMC(z, Q, pid, Omega, N, maps=False, map_iters=None, **opt):
    """R/SPARSEsumstatMCMC.R:21-29 -> phm_SPARSEmaketreelistMCMC."""
    return _mcmc("phm_SPARSEmaketreelistMCMC", z, Q, pid, Omega, N, maps=maps, map_iters=map_iters, **opt)


def sumstatMCMCks_sweep(z, Q, pid, Omega, N, maps=False, map_iters=None, **opt):
    """The tree sweep of ``sumstatMCMCks`` (R/sumstatMCMCks.R, src/phylomap.cpp:1802-1872) with Q held FIXED:
    hidden-rates Q of even size (``synth.make2sQ``), tips observed only up to parity and re-sampled every sweep,
    n x n transition counters including self pairs, result layout of man/sumstatMCMCks.Rd:19.  ``sumstatMCMCks`` below
    adds the per-iteration Gibbs/MH updates of Q (src/phylomap.cpp:1862-1866) and is the drop-in for the R function."""
    return _mcmc("phm_maketreelistMCMCks_sweep", z, Q, pid, Omega, N, maps=maps, map_iters=map_iters, **opt)


def sumstatMCMCbf_sweep(z, Q, pid, Omega, N, maps=False, map_iters=None, **opt):
    """The tree sweep of ``sumstatMCMCbf`` (treesamplebf, src/phylomap.cpp:1169-1179) with Q held FIXED, for ANY number of
    states: tips observed, row-normalised pruning, every consecutive pair of segment states counted -- self pairs, i.e.
    virtual jumps, included (shortenerbf :1010-1014) -- into n x n counters.  Columns: n dwell sums, n*n counts (row-major
    from, to), Q[0,1], Q[1,0], root state (0-based); at n = 2 that is the layout of R/sumstatMCMCbf.R:33."""
    return _mcmc("phm_maketreelistMCMCbf_sweep", z, Q, pid, Omega, N, maps=maps, map_iters=map_iters, **opt)


def _qupdate(fn_name, z, Q, pid, Omega, N, prior, kind, **opt):
    L = _lib.load()
    _tree, n, head = _sweep_head(z, Q, pid, Omega, N)
    prior = np.ascontiguousarray(prior, dtype=np.float64)
    o = _lib.make_options(**opt)
    out = np.zeros((N, _lib.stat_cols(n, kind)), order="F")
    _lib.check(getattr(L, fn_name)(*head, _lib._p(prior, C.c_double), int(prior.size), C.byref(o), _lib._p(out, C.c_double)))
    return out


def sumstatMCMCbf(z, Q, pid, Omega, N, prior, **opt):
    """R/sumstatMCMCbf.R:19-35 -> phm_maketreelistMCMCbf: two-state model, rates re-drawn after every sweep.
    Columns: time 0, time 1, n00, n01, n10, n11, l01, l10, root_state (R/sumstatMCMCbf.R:33).  ``Q`` is not modified."""
    return _qupdate("phm_maketreelistMCMCbf", z, Q, pid, Omega, N, prior, "bf", **opt)


def sumstatMCMCks(z, Q, pid, Omega, N, prior, **opt):
    """R/sumstatMCMCks.R:19-33 -> phm_maketreelistMCMCks: hidden-rates model with k regimes (n = 2k+2), all 2+3k rate
    parameters updated after every sweep.  Layout man/sumstatMCMCks.Rd:19.  ``Q`` is not modified."""
    return _qupdate("phm_maketreelistMCMCks", z, Q, pid, Omega, N, prior, "ks", **opt)


def sumstatMCMC2sDICt(z, Q, pid, Omega, N, prior, **opt):
    """R/sumstatMCMC2sDICt.R -> phm_maketreelistMCMC2sDICt: ``sumstatMCMCbf`` plus log p(y|Q) (matrix exponentiation) per
    iteration; columns time 0, time 1, n00, n01, n10, n11, l01, l10, root_state, log(p(y|Q))."""
    return _qupdate("phm_maketreelistMCMC2sDICt", z, Q, pid, Omega, N, prior, "bfdic", **opt)


def sumstatMCMCksDICt(z, Q, pid, Omega, N, prior, **opt):
    """R/sumstatMCMCksDICt.R -> phm_maketreelistMCMCksDICt: ``sumstatMCMCks`` plus log p(y|Q) per iteration (last column)."""
    return _qupdate("phm_maketreelistMCMCksDICt", z, Q, pid, Omega, N, prior, "ksdic", **opt)


def _qupdate_mt(fn_name, treelist, Q, pid, Omega, N, prior, kind, **opt):
    L = _lib.load()
    n, model = _model_args(Q, pid, Omega)
    orders = [_lib.tree_orders(z) for z in treelist]                 # R/sumstatMCMCmt.R:37-46, one row per tree
    nen_m = np.asfortranarray(np.stack([o[0] for o in orders]), dtype=np.int32)
    nodelist_m = np.asfortranarray(np.stack([o[1] for o in orders]), dtype=np.int32)
    roots = np.ascontiguousarray([o[2] for o in orders], dtype=np.int32)
    prior = np.ascontiguousarray(prior, dtype=np.float64)
    ftl = _lib.FlatTreeList(treelist)
    o = _lib.make_options(**opt)
    out = np.zeros((N, _lib.stat_cols(n, kind)), order="F")
    _lib.check(getattr(L, fn_name)(ftl.c, ftl.n, *model, _lib._p(nen_m, C.c_int32), _lib._p(nodelist_m, C.c_int32),
                                   _lib._p(roots, C.c_int32), int(N), _lib._p(prior, C.c_double), int(prior.size), C.byref(o),
                                   _lib._p(out, C.c_double)))
    return out


def sumstatMCMCmt(treelist, Q, pid, Omega, N, prior, **opt):
    """R/sumstatMCMCmt.R:29-52 -> phm_maketreelistMCMCmt: two-state model over a list of trees (same tips, different
    topologies / branch lengths); every iteration sweeps every tree, keeps one drawn uniformly and updates the rates from
    it.  Columns: time_0, time_1, n00, n01, n10, n11, l01, l10, tree_number (0-based, as the reference stores it)."""
    return _qupdate_mt("phm_maketreelistMCMCmt", treelist, Q, pid, Omega, N, prior, "bf", **opt)


def sumstatMCMCksmt(treelist, Q, pid, Omega, N, prior, **opt):
    """R/sumstatMCMCksmt.R -> phm_maketreelistMCMCksmt: hidden-rates model (n = 2k+2) over a list of trees; ``prior`` has
    8 entries (l01, l10, kappa, gamma shape/rate pairs).  Columns as ``sumstatMCMCks`` with tree_number last."""
    return _qupdate_mt("phm_maketreelistMCMCksmt", treelist, Q, pid, Omega, N, prior, "ks", **opt)


def eigen_decompose(Q):
    """R/sumstatEXP.R:26-29: lefts = eigen(Q)$vectors, rights = solve(lefts), d = diag(values) (real spectrum only)."""
    vals, vecs = np.linalg.eig(np.asarray(Q, dtype=np.float64))
    if np.max(np.abs(np.imag(vals))) > 0:
        raise ValueError("Q has complex eigenvalues; the reference's matexp handles a real spectrum only")
    lefts = np.real(vecs)
    rights = np.linalg.solve(lefts, np.eye(lefts.shape[0]))
    return lefts, rights, np.diag(np.real(vals))


def sumstatEXP(z, Q, pid, N, eig=None, maps=False, **opt):
    """R/sumstatEXP.R:21-33 -> phm_maketreelistEXP.  ``eig`` = (lefts, rights, d) overrides the eigendecomposition
    R/sumstatEXP.R:26-29 computes (LAPACK results differ between machines in the last bits).  ``maps=True``: returns
    ``(out, maps)`` with the N sampled histories as a ``maps.Maps`` (phm_maketreelistEXP_maps: a sizing call, then a filling
    call; the (tile, branch) mapping)."""
    L = _lib.load()
    n, Q, pid = _one_model(Q, pid)
    nen, nodelist, root = _lib.tree_orders(z)
    lefts, rights, d = (np.asfortranarray(np.asarray(a, dtype=np.float64)) for a in (eigen_decompose(Q) if eig is None else eig))
    ft = _lib.FlatTree(z)
    o = _lib.make_options(**opt)
    out = np.zeros((N, _lib.stat_cols(n)), order="F")
    args = (C.byref(ft.c), n, _lib._p(Q, C.c_double), _lib._p(pid, C.c_double), _lib._p(nen, C.c_int32),
            _lib._p(nodelist, C.c_int32), root, int(N), _lib._p(lefts, C.c_double), _lib._p(rights, C.c_double),
            _lib._p(d, C.c_double), C.byref(o), _lib._p(out, C.c_double))
    if not maps:
        _lib.check(L.phm_maketreelistEXP(*args))
        return out
    return out, _two_phase_maps(L.phm_maketreelistEXP_maps, args, int(N), ft.E)


def _two_phase_maps(fn, args, R, E):
    """the sizing call (writes the offsets), then the filling call into arrays of that size"""
    from .maps import Maps
    off = np.zeros(R * E + 1, dtype=np.int64)
    _lib.check(fn(*args, _lib._p(off, C.c_int64), 0, None, None))
    total = int(off[-1])
    dwell = np.empty(max(total, 1))
    state = np.empty(max(total, 1), dtype=np.int32)
    _lib.check(fn(*args, _lib._p(off, C.c_int64), total, _lib._p(dwell, C.c_double), _lib._p(state, C.c_int32)))
    return Maps(off, dwell[:total], state[:total], E)


def expm_eigen(lefts, rights, d, t, device=-1, mfma=False):
    """Batched P_b = |L diag(exp(d t_b)) R| (matexp, src/phylomap.cpp:2964-2968). Returns (P[n_t,n,n], kernel_ms).
    ``mfma=True`` (16 < n <= 64) runs the product on the matrix cores (last-bit differences)."""
    L = _lib.load()
    lefts, rights, d = (np.asfortranarray(np.asarray(a, dtype=np.float64)) for a in (lefts, rights, d))
    t = np.ascontiguousarray(t, dtype=np.float64)
    n = lefts.shape[0]
    out = np.zeros((t.size, n, n))
    ms = C.c_double(0.0)
    fn = L.phm_expm_eigen_mfma if mfma else L.phm_expm_eigen
    _lib.check(fn(n, _lib._p(lefts, C.c_double), _lib._p(rights, C.c_double), _lib._p(d, C.c_double),
                                _lib._p(t, C.c_double), int(t.size), int(device), _lib._p(out, C.c_double), C.byref(ms)))
    return out, ms.value


def expm_pade(Q, t, device=-1, mfma=False):
    """Batched expmat(Q t_b), Pade(6) scaling-and-squaring. Returns (P[n_t,n,n], kernel_ms).
    ``mfma=True`` (16 < n <= 64): every matrix product on the matrix cores (agrees to rounding, not bit for bit)."""
    L = _lib.load()
    Q = np.asfortranarray(np.asarray(Q, dtype=np.float64))
    t = np.ascontiguousarray(t, dtype=np.float64)
    n = Q.shape[0]
    out = np.zeros((t.size, n, n))
    ms = C.c_double(0.0)
    fn = L.phm_expm_pade_mfma if mfma else L.phm_expm_pade
    _lib.check(fn(n, _lib._p(Q, C.c_double), _lib._p(t, C.c_double), int(t.size), int(device),
                               _lib._p(out, C.c_double), C.byref(ms)))
    return out, ms.value


def _observe(observe, n):
    """``observe`` as the library takes it: None, or the n observed states as int32"""
    obs = None if observe is None else np.ascontiguousarray(observe, dtype=np.int32)
    if obs is not None and obs.size != n:
        raise ValueError("observe must have one entry per state")
    return obs


def _pid_rows(pid, n, K, per="model"):
    """pid as [1, n] (shared) or [K, n]"""
    pid = np.ascontiguousarray(np.atleast_2d(np.asarray(pid, dtype=np.float64)))
    if pid.shape[1] != n or pid.shape[0] not in (1, K):
        raise ValueError(f"pid must have n entries, shared or one row per {per}")
    return pid


def _model_batch(Qs, pid, site_of_model=None):
    """A batch of models as the many-model entry points take it: (K, n, Qf, pid, som) with Qf [K, n, n], each matrix
    column-major and the model slowest, pid [1, n] or [K, n], som None ("cross") or K int32 site indices ("paired")."""
    Qs = np.asarray(Qs, dtype=np.float64)
    if Qs.ndim == 2:
        Qs = Qs[None]
    if Qs.ndim != 3 or Qs.shape[1] != Qs.shape[2]:
        raise ValueError("Qs must be [K, n, n]")
    K, n = Qs.shape[0], Qs.shape[1]
    Qf = np.ascontiguousarray(Qs.transpose(0, 2, 1))
    pid = _pid_rows(pid, n, K)
    som = None
    if site_of_model is not None:
        som = np.ascontiguousarray(site_of_model, dtype=np.int32).reshape(-1)
        if som.size != K:
            raise ValueError("site_of_model must have one entry per model")
    return K, n, Qf, pid, som


def _tips_tree(z, sites, observe, n, opt):
    """What the calls on observed tips share: the tree with its tip states (``z['states']``, or one row of ``sites`` per site),
    ``observe`` and the options.  ``pt`` holds the arrays the tree points into."""
    if sites is None:
        tips = np.asarray(z["states"]).reshape(1, -1)
    else:
        tips = np.atleast_2d(np.asarray(sites))
        opt = dict(opt, n_replicas=tips.shape[0], tips_per_replica=True)
    pt = _lib.PlainTree(z, tips)
    if pt.states.shape[1] != pt.T:
        raise ValueError(f"tip states must have {pt.T} columns")
    obs = _observe(observe, n)
    o = _lib.make_options(**opt)
    S = max(1, int(o.n_replicas))                  # without sites: n_replicas sites that share z['states']
    return SimpleNamespace(pt=pt, tree=pt.c, obs=obs, opt=o, E=pt.E, T=pt.T, NT=pt.NT, S=S)


def _models_on_tips(z, Qs, pid, sites, observe, site_of_model, opt):
    """(n, a, shape, head) of a many-model call on observed tips: ``_tips_tree``'s ``a`` (hold it: it owns the tree), the
    outputs' leading shape, (K,) paired or (K, S) cross, and the eight arguments every such entry point begins with."""
    K, n, Qf, pid, som = _model_batch(Qs, pid, site_of_model)
    a = _tips_tree(z, sites, observe, n, opt)
    head = (C.byref(a.tree), n, K, _lib._p(Qf, C.c_double), _lib._p(pid, C.c_double), pid.shape[0], _lib._p(a.obs, C.c_int32),
            _lib._p(som, C.c_int32))
    return n, a, (K,) if som is not None else (K, a.S), head


def _start_rate(z, n_tips):
    """tips / tree length: the rate around which a fit and a posterior sample start"""
    return n_tips / float(np.sum(np.asarray(z["edge.length"], dtype=np.float64)))


def simulate_histories(z, Q, pid, R, observe=None, nodes=False, maps=False, **opt):
    """``R`` independent forward simulations of the chain along the tree of ``z`` (sample2statehistory, R/sourceme.R:346-414)
    -> phm_simulate_histories.  Reads ``z['edge']``, ``z['edge.length']`` and ``z['Nnode']`` only.  ``observe``: n values in
    1..n, the tip state reported for each true state (simulate_4_state_tree's parity map is (1, 2, 1, 2)).
    Returns ``(tips, stats)`` or, with ``nodes=True``, ``(tips, stats, nodes)``: tips [R, n_tips] 1-based (ready for the
    samplers' ``sites=``), stats [R, n + n*n + 1] (dwell per state, jump counts n x n row-major (from, to), root state 0-based),
    nodes [R, n_tips + Nnode] 1-based true states by ape node id.  Options: seed, replica_offset, device, devices.
    ``maps=True`` appends the R histories as a ``maps.Maps`` (true states; phm_simulate_histories_maps: a sizing call, then a
    filling call): ``(tips, stats[, nodes], maps)``."""
    L = _lib.load()
    n, Q, pid = _one_model(Q, pid)
    pt = _lib.PlainTree(z)
    obs = _observe(observe, n)
    R = int(R)
    o = _lib.make_options(n_replicas=R, **opt)
    tips = np.zeros((max(R, 1), pt.T), dtype=np.int32)
    nst = np.zeros((max(R, 1), pt.NT), dtype=np.int32) if nodes else None
    stats = np.zeros((max(R, 1), _lib.stat_cols(n, "simulate")), order="F")
    args = (C.byref(pt.c), n, _lib._p(Q, C.c_double), _lib._p(pid, C.c_double), _lib._p(obs, C.c_int32), C.byref(o),
            _lib._p(tips, C.c_int32), _lib._p(nst, C.c_int32), _lib._p(stats, C.c_double))
    res = (tips, stats, nst) if nodes else (tips, stats)
    if not maps:
        _lib.check(L.phm_simulate_histories(*args))
        return res
    return res + (_two_phase_maps(L.phm_simulate_histories_maps, args, max(R, 1), pt.E),)


def simulate_state_tree(z, Q, pid, observe=None, **opt):
    """simulate_2_state_tree / simulate_4_state_tree (R/simulate_2_state_tree.R, R/simulate_4_state_tree.R) for any tree and
    model: one simulated history, and ``z`` returned with its tips replaced by the simulated (observed) states and its tip
    branches re-initialised to two half-length pieces (synth.with_tip_states).  ``observe=(1, 2, 1, 2)`` is the 4-state
    function's parity map."""
    from . import synth
    tips, _ = simulate_histories(z, Q, pid, 1, observe=observe, **opt)
    return synth.with_tip_states(z, tips[0])


def simulate_histories_models(z, Qs, pid, R, observe=None, nodes=False, maps=False, **opt):
    """``R`` forward simulations under EACH of K rate matrices in one call ->
    phm_simulate_histories_models: one replicate dataset per posterior draw of the rates (``posterior.predictive``), R bootstrap
    replicates under each of K fits, one dataset per prior draw.  ``Qs``: [K, n, n] (or one [n, n]); ``pid``: n values shared by
    the models or [K, n], used as given.  History h = k R + r is ``simulate_histories(z, Qs[k], pid[k], 1,
    replica_offset=replica_offset + h)``'s, bit for bit in tips, nodes, counts, root state and maps; the dwell sums agree with it
    to 1e-12 of the tree length (64-bit fixed-point accumulators: the same bits whatever the chunks and devices are).
    Returns ``(tips, stats)``: tips [K, R, n_tips] 1-based (seen through ``observe``), stats [K, R, n + n*n + 1] in
    ``simulate_histories``' columns; ``nodes=True`` appends [K, R, n_tips + Nnode] 1-based true states, ``maps=True`` the H = K R
    histories as a ``maps.Maps`` (a sizing call, then a filling call).  Options: seed, replica_offset, device, devices."""
    L = _lib.load()
    K, n, Qf, pid, _ = _model_batch(Qs, pid)
    pt = _lib.PlainTree(z)
    obs = _observe(observe, n)
    R = int(R)
    Rr = max(R, 1)                                                    # R < 1 is refused by the library; the arrays stay valid
    o = _lib.make_options(**opt)
    tips = np.zeros((K, Rr, pt.T), dtype=np.int32)
    nst = np.zeros((K, Rr, pt.NT), dtype=np.int32) if nodes else None
    stats = np.zeros((_lib.stat_cols(n, "simulate"), K, Rr))         # column slowest, history fastest within it
    args = (C.byref(pt.c), n, K, _lib._p(Qf, C.c_double), _lib._p(pid, C.c_double), pid.shape[0], _lib._p(obs, C.c_int32), R,
            C.byref(o), _lib._p(tips, C.c_int32), _lib._p(nst, C.c_int32), _lib._p(stats, C.c_double))
    res = (tips, np.moveaxis(stats, 0, -1)) + ((nst,) if nodes else ())
    if not maps:
        _lib.check(L.phm_simulate_histories_models(*args, None, 0, None, None))
        return res
    return res + (_two_phase_maps(L.phm_simulate_histories_models, args, K * Rr, pt.E),)


def expected_sumstat(z, Q, pid, sites=None, observe=None, per_branch=False, nodes=False, **opt):
    """Exact E[dwell_i | tips, Q] and E[N_ij | tips, Q] -> phm_expected_stats: what the samplers'
    posterior means converge to, with no sampling.  Reads ``z['edge']``, ``z['edge.length']``, ``z['Nnode']`` and, without
    ``sites``, ``z['states']``.  ``sites``: S x n_tips tip states (0 = missing, else 1..n; e.g. the tips of
    ``simulate_histories``), one site per row.  ``observe``: n values in 1..n, the tip state each true state is seen as.
    Returns ``(stats, loglik)``, plus ``branch`` with ``per_branch=True`` and ``nodes`` with ``nodes=True``: stats
    [S, n + n(n-1)] in man/sumstatMCMC.Rd:18 column order, loglik [S] = log p(tips | Q), branch [S, n_edge, n + n(n-1)] by
    edge row, nodes [S, n_tips + Nnode, n] = P(state of node | tips) by ape node id.  Options: device, devices."""
    L = _lib.load()
    n, Q, pid = _one_model(Q, pid)
    a = _tips_tree(z, sites, observe, n, opt)
    S, cols = a.S, _lib.stat_cols(n)
    stats = np.zeros((S, cols), order="F")
    ll = np.zeros(S)
    br = np.zeros((S, a.E, cols), order="F") if per_branch else None
    post = np.zeros((S, a.NT, n), order="F") if nodes else None
    _lib.check(L.phm_expected_stats(C.byref(a.tree), n, _lib._p(Q, C.c_double), _lib._p(pid, C.c_double),
                                    _lib._p(a.obs, C.c_int32), C.byref(a.opt), _lib._p(stats, C.c_double), _lib._p(ll, C.c_double),
                                    _lib._p(br, C.c_double), _lib._p(post, C.c_double)))
    out = [stats, ll]
    if per_branch:
        out.append(br)
    if nodes:
        out.append(post)
    return tuple(out)


def expected_through_time(z, Q, pid, bounds=None, points=None, sites=None, observe=None, **opt):
    """Exact state probabilities and expected statistics through time -> phm_expected_through_time.
    Depth runs from the root: 0 there, a child's depth is its parent's plus the edge length (``maps.node_depths``).
    ``bounds``: K >= 1 strictly increasing depths >= 0, giving ``occupancy`` [S, K, n] (the expected number of lineages in each
    state at each bound; a node at a bound counts through its parent branch, bound 0 counts the root) and, with K >= 2, ``bins``
    [S, K - 1, n + n(n-1)] (E[dwell_i] and E[N_ij] within depths [bounds[k], bounds[k+1]) in ``expected_sumstat``'s columns).
    ``points``: (edge_rows, positions), 0-based edge rows and distances from the parent end (0 <= position <= t_b), giving
    ``points`` [S, P, n] = P(state at the point | tips).  ``loglik`` [S] always.  ``z``, ``sites``, ``observe`` and the options
    are ``expected_sumstat``'s.  Returns a dict of those keys."""
    L = _lib.load()
    n, Q, pid = _one_model(Q, pid)
    a = _tips_tree(z, sites, observe, n, opt)
    S = a.S
    out = {}
    bnd = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.float64).reshape(-1)
    K = 0 if bnd is None else bnd.size
    occ = out["occupancy"] = np.zeros((S, K, n), order="F") if K >= 1 else None
    bins = out["bins"] = np.zeros((S, K - 1, _lib.stat_cols(n)), order="F") if K >= 2 else None
    pe = pp = post = None
    if points is not None:
        pe = np.ascontiguousarray(points[0], dtype=np.int32).reshape(-1)
        pp = np.ascontiguousarray(points[1], dtype=np.float64).reshape(-1)
        if pe.size != pp.size:
            raise ValueError("points: as many edge rows as positions")
        post = out["points"] = np.zeros((S, pe.size, n), order="F")
    ll = out["loglik"] = np.zeros(S)
    _lib.check(L.phm_expected_through_time(C.byref(a.tree), n, _lib._p(Q, C.c_double), _lib._p(pid, C.c_double),
                                           _lib._p(a.obs, C.c_int32), C.byref(a.opt), K, _lib._p(bnd, C.c_double),
                                           _lib._p(occ, C.c_double), _lib._p(bins, C.c_double), 0 if pe is None else pe.size,
                                           _lib._p(pe, C.c_int32), _lib._p(pp, C.c_double), _lib._p(post, C.c_double),
                                           _lib._p(ll, C.c_double)))
    return {k: v for k, v in out.items() if v is not None}


def loglik_models(z, Qs, pid, sites=None, observe=None, site_of_model=None, **opt):
    """log p(tips_s | Q_k, pid_k) for K rate matrices in one call (DESIGN.md sections 17 and 26) -> phm_loglik_models (2..8 states,
    the models across the lanes) or phm_expected_stats_models_wide with no statistics asked for (9..64 states, one state per lane,
    batched over models and sites; the same values bit for bit): the likelihood a fit evaluates.  ``Qs``: [K, n, n] (or
    one n x n matrix).  ``pid``: n values shared by every model, or [K, n].  ``z``, ``sites``, ``observe`` and the options are
    ``expected_sumstat``'s.  ``site_of_model`` None ("cross"): every model on every site, returns [K, S].  ``site_of_model`` = K
    0-based site indices ("paired"): model k on its own site alone, returns [K].  An impossible evaluation is ``-inf``."""
    L = _lib.load()
    n, a, shape, head = _models_on_tips(z, Qs, pid, sites, observe, site_of_model, opt)
    out = np.zeros(shape)
    if n > 8:
        _lib.check(L.phm_expected_stats_models_wide(*head, C.byref(a.opt), None, _lib._p(out, C.c_double)))
    else:
        _lib.check(L.phm_loglik_models(*head, C.byref(a.opt), _lib._p(out, C.c_double)))
    return out


def expected_sumstat_models(z, Qs, pid, sites=None, observe=None, site_of_model=None, **opt):
    """Exact E[dwell_i | tips_s, Q_k] and E[N_ij | tips_s, Q_k] with log p(tips_s | Q_k) for K rate matrices in one call
    (DESIGN.md sections 18 and 26) -> phm_expected_stats_models (2..8 states: ``expected_sumstat`` with the models across the
    lanes) or phm_expected_stats_models_wide (9..64 states: one state per lane, batched over models and sites; a model that leaves
    no state is served there too).  Every argument is ``loglik_models``'.  Returns ``(stats, loglik)``: [K, S, n + n(n-1)] and
    [K, S] ("cross"), or [K, n + n(n-1)] and [K] with ``site_of_model`` ("paired").  ``loglik`` is ``loglik_models``' value bit
    for bit; an impossible evaluation is ``-inf`` with a row of NaN."""
    L = _lib.load()
    n, a, shape, head = _models_on_tips(z, Qs, pid, sites, observe, site_of_model, opt)
    ll = np.zeros(shape)
    stats = np.zeros((_lib.stat_cols(n),) + shape)                 # column slowest, evaluation (site fastest) within it
    fn = L.phm_expected_stats_models_wide if n > 8 else L.phm_expected_stats_models
    _lib.check(fn(*head, C.byref(a.opt), _lib._p(stats, C.c_double), _lib._p(ll, C.c_double)))
    return np.moveaxis(stats, 0, -1), ll


def expected_branch_stats_models(z, Qs, pid, sites=None, observe=None, site_of_model=None, edges=None, labels=None, **opt):
    """Exact E[dwell_i | tips_s, Q_k] and E[N_ij | tips_s, Q_k] PER BRANCH for K rate matrices in one call
    -> phm_expected_branch_stats_models, 2..64 states: where on the tree the changes happened under the models of a fit and its
    uncertainty (``fit.sample_thetas``) or of a posterior sample of Q -- ``expected_sumstat(per_branch=True)`` with the models
    batched.  ``Qs``, ``pid``, ``z``, ``sites``, ``observe``, ``site_of_model`` and the options are ``loglik_models``'.
    ``edges``: 0-based edge rows of ``z['edge']`` in any order, repeats allowed (default: every row in row order); the output
    follows the list.  ``labels``: None for full rows, or [L, n, n] (or one [n, n]) weight matrices in natural (from, to)
    orientation -- entry (i, i) weighs E[dwell_i], entry (i, j) E[N_ij] -- for L labelled sums per branch, reduced on the device
    (``ratemodel.count_labels``, ``ratemodel.observed_change_labels``): what a codon or hidden-rates model is asked for, where a
    full row is thousands of values.  Returns ``(branch, loglik)``: [K, S, n_sel, C] and [K, S] ("cross"), or [K, n_sel, C] and
    [K] with ``site_of_model`` ("paired"); C = n + n(n-1) in ``expected_sumstat``'s columns, or L.  ``loglik`` is
    ``loglik_models``' value bit for bit; an impossible evaluation is ``-inf`` with NaN rows.  The rows of all edges, added in
    runs of 16 edge rows, are ``expected_sumstat_models``' totals bit for bit, and a labelled sum is the plain double sum
    ``acc = acc + w[col] * row[col]`` over the full row's columns bit for bit.  ``ancestral.model_average`` averages ``branch``
    over the models."""
    L = _lib.load()
    n, a, shape, head = _models_on_tips(z, Qs, pid, sites, observe, site_of_model, opt)
    sel = None
    if edges is not None:
        sel = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1)
    n_sel = a.E if sel is None else sel.size
    lab = None
    if labels is not None:
        lab = np.asarray(labels, dtype=np.float64)
        if lab.ndim == 2:
            lab = lab[None]
        if lab.ndim != 3 or lab.shape[1:] != (n, n):
            raise ValueError("labels must be [L, n, n]")
        lab = np.ascontiguousarray(lab.transpose(0, 2, 1))           # column-major per matrix, as Qs
    cols = _lib.stat_cols(n) if lab is None else lab.shape[0]
    ll = np.zeros(shape)
    br = np.zeros((cols, max(n_sel, 1)) + shape)                     # column slowest, evaluation (site fastest) within an entry
    _lib.check(L.phm_expected_branch_stats_models(*head, C.byref(a.opt), n_sel, _lib._p(sel, C.c_int32), 0 if lab is None else lab.shape[0],
                                                  _lib._p(lab, C.c_double), _lib._p(br, C.c_double), _lib._p(ll, C.c_double)))
    return np.moveaxis(br, (0, 1), (-1, -2)), ll


ThroughTimeModels = namedtuple("ThroughTimeModels", ["loglik", "occupancy", "bins", "point_post"])


def expected_through_time_models(z, Qs, pid, sites=None, observe=None, site_of_model=None, bounds=None, points=None, labels=None,
                                 batched=False, **opt):
    """Exact state probabilities and expected statistics through time for K rate matrices in one call (DESIGN.md sections 28
    and 29) -> phm_expected_through_time_models, 2..64 states: WHEN the changes happened under the models of a fit and its
    uncertainty (``fit.sample_thetas``) or of a posterior sample of Q -- ``expected_through_time`` with the models batched (2..8
    states: the models across the lanes and one plan of depths, crossings and sub-branches for all of them; 9..64 states: served
    one model after another).  ``batched=True`` sends a call at 9..64 states to phm_expected_through_time_models_wide instead:
    one state per lane, batched over models, sites and items, one plan for all, a model that leaves no state served; its values
    agree with the default's within ``expected_through_time``'s bars.  The default stays model by model so that recorded values
    hold bit for bit; at 2..8 states ``batched`` changes nothing.  ``Qs``, ``pid``, ``z``, ``sites``, ``observe``,
    ``site_of_model`` and the options are ``loglik_models``'; ``bounds`` and ``points`` are ``expected_through_time``'s.
    ``labels``: None, or [L, n, n] (or one [n, n]) weight matrices in natural (from, to) orientation, as
    ``expected_branch_stats_models`` takes them, for L labelled sums per bin reduced on the device; it needs ``batched=True`` at
    9..64 states (labelled bins are not built for 2..8 states).  Returns the named tuple
    ``(loglik, occupancy, bins, point_post)``: [K, S] (``loglik_models``' values bit for bit), [K, S, n_bounds, n],
    [K, S, n_bounds - 1, n + n(n-1)] in ``expected_sumstat``'s columns ([K, S, n_bounds - 1, L] with ``labels``) and
    [K, S, n_points, n]; with ``site_of_model`` the S axis is absent; a part that was not asked for (no ``bounds``, fewer than
    two, no ``points``) is ``None``.  An impossible evaluation is ``-inf`` with NaN rows.  ``ancestral.average_over_models``
    averages any of them over the models."""
    L = _lib.load()
    n, a, shape, head = _models_on_tips(z, Qs, pid, sites, observe, site_of_model, opt)
    wide = bool(batched) and n > 8
    lab = None
    if labels is not None:
        if n <= 8:
            raise ValueError("labels: labelled bins are not built for 2..8 states")
        if not wide:
            raise ValueError("labels needs batched=True at 9..64 states")
        lab = np.asarray(labels, dtype=np.float64)
        if lab.ndim == 2:
            lab = lab[None]
        if lab.ndim != 3 or lab.shape[1:] != (n, n):
            raise ValueError("labels must be [L, n, n]")
        lab = np.ascontiguousarray(lab.transpose(0, 2, 1))           # column-major per matrix, as Qs
    bnd = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.float64).reshape(-1)
    nb = 0 if bnd is None else bnd.size
    occ = np.zeros((n, nb) + shape) if nb >= 1 else None             # column slowest, evaluation (site fastest) within a row
    bins = np.zeros((_lib.stat_cols(n) if lab is None else lab.shape[0], nb - 1) + shape) if nb >= 2 else None
    pe = pp = post = None
    if points is not None:
        pe = np.ascontiguousarray(points[0], dtype=np.int32).reshape(-1)
        pp = np.ascontiguousarray(points[1], dtype=np.float64).reshape(-1)
        if pe.size != pp.size:
            raise ValueError("points: as many edge rows as positions")
        post = np.zeros((n, pe.size) + shape)
    ll = np.zeros(shape)
    tail = (_lib._p(occ, C.c_double), _lib._p(bins, C.c_double), 0 if pe is None else pe.size, _lib._p(pe, C.c_int32),
            _lib._p(pp, C.c_double), _lib._p(post, C.c_double), _lib._p(ll, C.c_double))
    if wide:
        _lib.check(L.phm_expected_through_time_models_wide(*head, C.byref(a.opt), nb, _lib._p(bnd, C.c_double),
                                                           0 if lab is None else lab.shape[0], _lib._p(lab, C.c_double), *tail))
    else:
        _lib.check(L.phm_expected_through_time_models(*head, C.byref(a.opt), nb, _lib._p(bnd, C.c_double), *tail))

    def rows_last(x):
        return None if x is None else np.moveaxis(x, (0, 1), (-1, -2))
    return ThroughTimeModels(ll, rows_last(occ), rows_last(bins), rows_last(post))


def sample_histories(z, Qs, pid, draws, sites=None, observe=None, site_of_model=None, nodes=False, maps=False, **opt):
    """``draws`` exact, independent histories given the tips for each of K rate matrices (and each site) in one call (DESIGN.md
    sections 19 and 24) -> phm_sample_histories_models (2..8 states, the models across the lanes of the tree passes) or
    phm_sample_histories_models_wide (9..64 states, one state per lane there): stochastic maps under the models of a fit and its uncertainty
    (``fit.sample_thetas``), of per-dataset fits or of a posterior sample of Q.  No burn-in, no jump cap (max(-q_ii) t_b up to
    32 768), missing tips and ``observe`` maps allowed; 2..64 states.  ``Qs``, ``pid``, ``z``, ``sites``, ``observe`` and
    ``site_of_model`` are ``loglik_models``'.  Returns ``(stats, loglik)``: [K, S, draws, n + n(n-1)] in ``expected_sumstat``'s
    columns and [K, S] (``loglik_models``' values bit for bit); with ``site_of_model`` the S axis is absent.  ``nodes=True``
    appends [K, S, draws, n_tips + Nnode] 1-based TRUE states by ape node id, tips included (a missing tip and the hidden state
    behind ``observe`` come out sampled).  ``maps=True`` appends the histories as a ``maps.Maps`` (a sizing call, then a filling
    call) whose history index is h = (k S + s) draws + d.  An impossible evaluation (``-inf``) has NaN statistics, zero nodes and
    empty map rows.  Options: seed, replica_offset, device, devices."""
    L = _lib.load()
    n, a, shape, head = _models_on_tips(z, Qs, pid, sites, observe, site_of_model, opt)
    D = int(draws)
    ll = np.zeros(shape)
    hshape = shape + (max(D, 1),)
    stats = np.zeros((_lib.stat_cols(n),) + hshape)                  # column slowest, history fastest within it
    nst = np.zeros(hshape + (a.NT,), dtype=np.int32) if nodes else None
    args = head + (D, C.byref(a.opt), _lib._p(stats, C.c_double), _lib._p(ll, C.c_double), _lib._p(nst, C.c_int32))
    res = (np.moveaxis(stats, 0, -1), ll) + ((nst,) if nodes else ())
    fn = L.phm_sample_histories_models_wide if n > 8 else L.phm_sample_histories_models
    if not maps:
        _lib.check(fn(*args, None, 0, None, None))
        return res
    return res + (_two_phase_maps(fn, args, int(np.prod(hshape)), a.E),)


AncestralStates = namedtuple("AncestralStates", ["loglik", "node_post", "joint_states", "joint_logp", "nodes"])


def ancestral_states_models(z, Qs, pid, sites=None, observe=None, site_of_model=None, nodes=None, marginal=True, joint=True,
                            **opt):
    """Ancestral states under K rate matrices in one call for 2..64 states (DESIGN.md sections 21 and 23) -> phm_ancestral_models
    (2..8 states, the models across the lanes) or phm_ancestral_models_wide (9..64 states, one state per lane): the marginal
    posterior of every reported node's state and the JOINT reconstruction, the one assignment of all nodes that maximises
    p(states, tips_s | Q_k, pid_k) (Pupko et al. 2000).  ``Qs``, ``pid``, ``z``, ``sites``, ``observe`` and ``site_of_model`` are
    ``loglik_models``'.  ``nodes``: 1-based ape node ids to report, tips and duplicates allowed (``ancestral.mrca`` names a
    clade's ancestor); None: every node in id order.  Returns the named tuple
    ``(loglik, node_post, joint_states, joint_logp, nodes)``: [K, S] (``loglik_models``' values bit for bit), [K, S, J, n],
    [K, S, J] 1-based TRUE states (a missing tip and the hidden state behind ``observe`` come out reconstructed) and [K, S]; with
    ``site_of_model`` the S axis is absent.  ``marginal=False`` / ``joint=False`` leave that part out (``None``; the other part is
    the same bit for bit).  ``nodes`` echoes the ids reported.  An impossible evaluation (``-inf``) has NaN posteriors, zero
    states and ``joint_logp`` = ``-inf``.  Behind an ``observe`` map (codons -> amino acids, hidden-rate classes -> the observed
    character) ``ancestral.collapse_states(node_post, observe)`` sums the posterior per observation and ``observe[x - 1]`` maps
    ``joint_states``.  Options: device, devices."""
    if not marginal and not joint:
        raise ValueError("marginal and joint are both False: nothing to compute")
    L = _lib.load()
    n, a, shape, head = _models_on_tips(z, Qs, pid, sites, observe, site_of_model, opt)
    sel = None
    if nodes is not None:
        sel = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
        if sel.size == 0:
            raise ValueError("nodes must name at least one node (None: every node)")
    J = a.NT if sel is None else sel.size
    ll = np.zeros(shape)
    post = np.zeros(shape + (J, n)) if marginal else None
    states = np.zeros(shape + (J,), dtype=np.int32) if joint else None
    jl = np.zeros(shape) if joint else None
    fn = L.phm_ancestral_models_wide if n > 8 else L.phm_ancestral_models
    _lib.check(fn(*head, _lib._p(sel, C.c_int32), 0 if sel is None else sel.size, C.byref(a.opt), _lib._p(ll, C.c_double),
                  _lib._p(post, C.c_double), _lib._p(states, C.c_int32), _lib._p(jl, C.c_double)))
    ids = np.arange(1, a.NT + 1, dtype=np.int32) if sel is None else sel.copy()
    return AncestralStates(ll, post, states, jl, ids)


def fit_ml(z, model, pid, sites=None, observe=None, per_site=False, starts=8, seed=0, gtol=1e-5, max_iter=200, bounds=None,
           gradient="fd", se=False, **opt):
    """Maximum-likelihood fit of a parametrised rate matrix (``ratemodel.RateModel``) to the tips, by ``fit.fit`` over
    ``loglik_models``: every iteration evaluates all starts' (and, with ``per_site=True``, all sites') gradient points and
    line-search candidates in one call.  Joint fit over the sites (default): cross mode summed over the sites.
    ``per_site=True``: one fit per site in lock-step, paired mode; every result gets a leading site axis.  Returns ``fit.fit``'s
    dict (theta, Q, loglik, aic, iterations, converged, at_bound, grad, starts, calls, evals).
    ``gradient="exact"``: the score from ``expected_sumstat_models`` at the line-search candidates replaces the 2p difference
    points.  ``se=True`` adds ``fit.standard_errors``' keys: cov_log [p, p], se_log [p], ci [p, 2] and
    se_ok, from the observed information in log theta (one call of 2p models per problem)."""
    from . import fit as _fit
    a = _tips_tree(z, sites, observe, model.n, opt)
    S, rate0 = a.S, _start_rate(z, a.T)
    if per_site:
        def batch(Qs, owner):
            return loglik_models(z, Qs, pid, sites=sites, observe=observe, site_of_model=owner, **opt)

        def batch_stats(Qs, owner):
            st, ll = expected_sumstat_models(z, Qs, pid, sites=sites, observe=observe, site_of_model=owner, **opt)
            return ll, st
    else:
        def batch(Qs, owner):
            return loglik_models(z, Qs, pid, sites=sites, observe=observe, **opt).sum(axis=1)

        def batch_stats(Qs, owner):
            st, ll = expected_sumstat_models(z, Qs, pid, sites=sites, observe=observe, **opt)
            return ll.sum(axis=1), st.sum(axis=1)
    P = S if per_site else 1
    r = _fit.fit(batch, model, P, rate0, starts=starts, seed=seed, gtol=gtol, max_iter=max_iter, bounds=bounds,
                 gradient=gradient, batch_stats=batch_stats if gradient == "exact" else None)
    if se:
        r.update(_fit.standard_errors(batch_stats, model, r["theta"], np.arange(P, dtype=np.int32), r["at_bound"]))
    return r if per_site else _fit.first_problem(r)


def posterior_rates(z, model, pid, prior, iters, chains=4, sites=None, observe=None, per_site=False, theta0=None, theta_max=None,
                    thin=1, stats=True, **opt):
    """Posterior sample of the rates of an index model (``ratemodel.er`` / ``sym`` / ``ard`` / ``index_model``) by exact data
    augmentation for 2..64 states (DESIGN.md sections 20 and 25) -> phm_gibbs_rates (2..8 states, one chain per lane) or
    phm_gibbs_rates_wide (9..64 states, one site of a chain per lane; with ``per_site=True`` a chain has one site and a wave one
    live lane): the Bayesian counterpart of ``fit_ml``.  ``chains`` chains run in lock-step; every iteration draws an exact
    history given the tips and the chain's rates (``sample_histories``'
    sampler: no burn-in of the history, no jump cap) and then every rate from its Gamma full conditional.
    ``prior``: Gamma (shape, rate) per parameter, [p, 2] (or one pair for all) shared by the chains, or [C, p, 2].
    Joint (default): every chain sees all the sites; C = chains.  ``per_site=True``: ``chains`` chains per site in one call
    (paired mode), C = S * chains, chain s * chains + r on site s, and every result gets a leading site axis after the rows.
    ``theta0``: [C, p] starts (default ``fit.start_points`` around tips / tree length, the same for every site).
    ``theta_max``: a truncation of the prior -- every rate is confined to (0, theta_max], a draw of the conditional above it is
    rejected and the old value kept (default 100 * tips / tree length); it also bounds the sampler's table:
    (most rates in a row) * theta_max * (longest branch) <= 32 768.
    Returns a dict: theta [rows, C, p] (row r = iteration r * thin; row 0 the starts), loglik [rows, C] (``loglik_models``'
    value of the row's theta bit for bit, summed over the sites when joint: what DIC needs), stats [rows, C, n + n(n-1)] (the
    history drawn under the row's theta in ``expected_sumstat``'s columns: the posterior of N_ij and dwell_i under rate
    uncertainty; ``stats=False`` leaves it out), rejected [C, p], status [C] (1: impossible tips, NaN rows), theta_max, thin,
    site_of_chain and model.  Iteration i's history of chain k is ``sample_histories(posterior.rate_matrices(model, theta[i]),
    draws=1, replica_offset=i + replica_offset)``'s, so node states and maps of any iteration can be redrawn after the fact.
    Options: seed, replica_offset, device, devices."""
    from . import fit as _fit
    if getattr(model, "index", None) is None:
        raise ValueError("posterior_rates needs an index model (ratemodel.er, sym, ard or index_model)")
    L = _lib.load()
    n, p = model.n, model.p
    a = _tips_tree(z, sites, observe, n, opt)
    S, rate0 = a.S, _start_rate(z, a.T)
    theta_max = 100.0 * rate0 if theta_max is None else float(theta_max)
    per = int(chains)
    if per < 1:
        raise ValueError("chains must be >= 1")
    Cn = S * per if per_site else per
    som = np.ascontiguousarray(np.repeat(np.arange(S, dtype=np.int32), per)) if per_site else None
    if theta0 is None:
        lo, hi = math.log(_fit.DEFAULT_BOUNDS[0] * rate0), math.log(theta_max)
        th0 = np.exp(_fit.start_points(p, min(rate0, theta_max), per, opt.get("seed", 0), lo, hi))
        th0 = np.minimum(th0, theta_max)
        if per_site:
            th0 = np.tile(th0, (S, 1))
    else:
        th0 = np.asarray(theta0, dtype=np.float64)
    th0 = np.ascontiguousarray(th0, dtype=np.float64).reshape(-1, p)
    if th0.shape[0] != Cn:
        raise ValueError(f"theta0 must be [{Cn}, {p}]")
    pr = np.asarray(prior, dtype=np.float64)
    if pr.ndim == 1:
        pr = np.tile(pr.reshape(1, 2), (p, 1))
    if pr.ndim == 2:
        pr = pr[None]
    if pr.shape[1:] != (p, 2) or pr.shape[0] not in (1, Cn):
        raise ValueError("prior must be [p, 2] (shared) or [C, p, 2]")
    pr = np.ascontiguousarray(pr)
    pid = _pid_rows(pid, n, Cn, per="chain")
    idx = np.ascontiguousarray(np.asarray(model.index, dtype=np.int32).T)     # column-major
    iters, thin = int(iters), int(thin)
    rows = max(1, -(-iters // max(thin, 1)))
    theta = np.zeros((rows, Cn, p))
    ll = np.zeros((rows, Cn))
    st = np.zeros((rows, Cn, _lib.stat_cols(n))) if stats else None
    rej = np.zeros((Cn, p), dtype=np.int32)
    status = np.zeros(Cn, dtype=np.int32)
    fn = L.phm_gibbs_rates_wide if n > 8 else L.phm_gibbs_rates
    _lib.check(fn(C.byref(a.tree), n, _lib._p(idx, C.c_int32), p, Cn, _lib._p(th0, C.c_double),
                  _lib._p(pr, C.c_double), pr.shape[0], theta_max, _lib._p(pid, C.c_double), pid.shape[0],
                  _lib._p(a.obs, C.c_int32), _lib._p(som, C.c_int32), iters, thin, C.byref(a.opt),
                  _lib._p(theta, C.c_double), _lib._p(ll, C.c_double), _lib._p(st, C.c_double),
                  _lib._p(rej, C.c_int32), _lib._p(status, C.c_int32)))
    out = dict(theta=theta, loglik=ll, stats=st, rejected=rej, status=status)
    if per_site:
        lead = dict(theta=1, loglik=1, stats=1, rejected=0, status=0)         # axes before the chain axis
        out = {k: (None if v is None else v.reshape(v.shape[:lead[k]] + (S, per) + v.shape[lead[k] + 1:])) for k, v in out.items()}
    out.update(theta_max=theta_max, thin=thin, site_of_chain=som, model=model, per_site=bool(per_site), chains=per)
    return out
