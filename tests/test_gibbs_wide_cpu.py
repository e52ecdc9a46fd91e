"""The posterior sampler of rates at 9..64 states without a device (phm_gibbs_rates_wide): where the symbol is
declared and bound, every refusal of the entry point before its first device call by status and message, the one-pass update from
the summed row against ``gibbsref.update`` bit for bit, a short run of the Python twin (tests/gibbswideref.py) and the
``ValueError`` for a model without an index.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gibbsref
import gibbswideref
import samplecases as sc
from phylomap_amd import _lib, api, posterior, ratemodel, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = "phm_gibbs_rates_wide"
NARROW = "phm_gibbs_rates"


def banded(n):
    return ratemodel.index_model(gibbswideref.banded_index(n))


def test_symbol_is_declared_apart_and_bound_like_the_narrow_one():
    L = _lib.load()
    assert hasattr(L, WIDE) and _lib.EXT2_EXPORTS == [WIDE]
    assert WIDE not in _lib.EXPORTS and WIDE not in _lib.EXT_EXPORTS
    assert L.phm_version() == 300
    assert list(getattr(L, WIDE).argtypes) == list(getattr(L, NARROW).argtypes)
    inc = os.path.join(ROOT, "include")
    for name in ("phylomap_hip.h", "phylomap_hip_ext.h"):
        assert WIDE not in open(os.path.join(inc, name)).read()
    ext2 = open(os.path.join(inc, "phylomap_hip_ext2.h")).read()
    assert re.findall(r"\b(phm_[A-Za-z0-9_]+)\s*\(", ext2) == [WIDE] and '#include "phylomap_hip_ext.h"' in ext2
    assert "2..64 states" in api.posterior_rates.__doc__


def _raw(z, model, C_=3, theta0=None, prior=None, n_prior=None, theta_max=50.0, pid=None, S=2, observe=None, soc=None, iters=4,
         thin=1, index=None, n_states=None, n_params=None, stats=True, null=None):
    """one call of the wide entry point with the tree's tips tiled S times -> (status, message)"""
    n = model.n if n_states is None else n_states
    p = model.p if n_params is None else n_params
    idx = np.ascontiguousarray(np.asarray(model.index if index is None else index, dtype=np.int32).T)
    th0 = np.ascontiguousarray(np.full((C_, p), 0.5) if theta0 is None else theta0, dtype=np.float64)
    pr = np.ascontiguousarray(np.ones((1, p, 2)) if prior is None else prior, dtype=np.float64)
    pid = np.ascontiguousarray(np.full(n, 1.0 / n) if pid is None else pid, dtype=np.float64)
    pt = _lib.PlainTree(z, np.tile(z["states"], (S, 1)))
    obs = None if observe is None else np.ascontiguousarray(observe, dtype=np.int32)
    so = None if soc is None else np.ascontiguousarray(soc, dtype=np.int32)
    o = _lib.make_options(n_replicas=S, tips_per_replica=True)
    rows = max(1, -(-iters // max(thin, 1)))
    cols = n + n * (n - 1)
    theta, ll = np.zeros((rows, C_, p)), np.zeros((rows, C_))
    sts = np.zeros((rows, C_, cols)) if stats else None
    rej, status = np.zeros((C_, p), dtype=np.int32), np.zeros(C_, dtype=np.int32)
    a = dict(tree=C.byref(pt.c), index=_lib._p(idx, C.c_int32), theta0=_lib._p(th0, C.c_double), prior=_lib._p(pr, C.c_double),
             pid=_lib._p(pid, C.c_double), theta=_lib._p(theta, C.c_double), loglik=_lib._p(ll, C.c_double),
             rejected=_lib._p(rej, C.c_int32), status=_lib._p(status, C.c_int32))
    if null is not None:
        a[null] = None
    L = _lib.load()
    code = getattr(L, WIDE)(a["tree"], n, a["index"], p, C_, a["theta0"], a["prior"], pr.shape[0] if n_prior is None else n_prior,
                            theta_max, a["pid"], 1, _lib._p(obs, C.c_int32), _lib._p(so, C.c_int32), iters, thin, C.byref(o),
                            a["theta"], a["loglik"], _lib._p(sts, C.c_double), a["rejected"], a["status"])
    return code, L.phm_last_error().decode()


def test_refusals_need_no_device():
    L = _lib.load()
    z4, _, _, _ = synth.config_problem(2, n_tips=16)
    z = dict(z4, states=np.ones(16, dtype=np.int32))
    m = ratemodel.sym(9)
    for null in ("tree", "index", "theta0", "prior", "pid", "theta", "loglik", "rejected", "status"):
        st, msg = _raw(z, m, null=null)
        assert st == 1 and msg.startswith(WIDE + ": NULL argument"), (null, st, msg)
    # the state count: 2..8 belong to the narrow entry point, anything outside 2..64 is bad input
    m8 = ratemodel.er(8)
    st, msg = _raw(z, m8)
    assert st == 2 and msg.startswith(WIDE + ":") and msg.endswith("go to " + NARROW)
    assert _raw(z, ratemodel.er(2))[0] == 2
    st, msg = _raw(z, ratemodel.er(65))
    assert st == 1 and msg.startswith(WIDE + ":") and "2..64" in msg
    st, msg = _raw(z, m, n_states=1)
    assert st == 1 and "2..64" in msg
    assert _raw(z, m, C_=0, theta0=np.zeros((1, m.p)))[0] == 1
    st, msg = _raw(z, m, n_params=0)
    assert st == 1 and "n_params" in msg
    assert _raw(z, m, n_params=73, theta0=np.full((3, 73), 0.5), prior=np.ones((1, 73, 2)))[0] == 1      # above n (n - 1) = 72
    # index with a gap in 1..p: parameter 3 owns nothing
    st, msg = _raw(z, m, index=np.where(m.index == 3, 2, m.index))
    assert st == 1 and msg.startswith(WIDE + ":") and "parameter 3" in msg
    st, msg = _raw(z, m, index=np.where(m.index == 6, m.p + 1, m.index))                                 # an entry beyond p
    assert st == 1 and f"parameter {m.p + 1}" in msg
    pr = np.ones((1, m.p, 2))
    pr[0, 4, 0] = 0.0
    st, msg = _raw(z, m, prior=pr)
    assert st == 1 and "parameter 5" in msg
    pr = np.ones((3, m.p, 2))
    pr[2, 1, 1] = -1.0
    st, msg = _raw(z, m, prior=pr)
    assert st == 1 and "parameter 2" in msg and "row 2" in msg
    st, msg = _raw(z, m, prior=np.ones((2, m.p, 2)))                                                      # n_prior neither 1 nor C
    assert st == 1 and "n_prior" in msg
    th = np.full((3, m.p), 0.5)
    th[1, 2] = 0.0
    st, msg = _raw(z, m, theta0=th)
    assert st == 1 and "chain 1" in msg and "parameter 3" in msg
    th[1, 2] = 51.0                                                                                       # above theta_max = 50
    st, msg = _raw(z, m, theta0=th)
    assert st == 1 and "chain 1" in msg and "theta_max" in msg
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        st, msg = _raw(z, m, theta_max=bad)
        assert st == 1 and "theta_max" in msg
    st, msg = _raw(z, m, iters=0)
    assert st == 1 and "iters" in msg
    st, msg = _raw(z, m, thin=0)
    assert st == 1 and "thin" in msg
    st, msg = _raw(z, m, soc=[0, 2, 1])                                                                   # S = 2
    assert st == 1 and "chain 1" in msg
    st, msg = _raw(z, m, soc=[0, -1, 1])
    assert st == 1 and "chain 1" in msg
    assert _raw(z, m, observe=[1, 2, 1, 2, 1, 2, 1, 2, 10])[0] == 1                                       # ll_validate's checks follow
    assert _raw(z, m, pid=[0.5, 0.5, -0.1, 0.1, 0, 0, 0, 0, 0])[0] != 0
    assert _raw(dict(z, states=np.full(16, 10, dtype=np.int32)), m)[0] == 1                               # a tip state above n
    # theta_max bounds the uniformization rate: 8 rates in a row * theta_max * longest branch <= 32768
    tmax = float(np.max(z["edge.length"]))
    st, msg = _raw(z, m, theta_max=32768.0 / (8 * tmax) * 1.01)
    assert st == 2 and msg.startswith(WIDE + ":") and "theta_max" in msg and "= 8)" in msg
    b17 = banded(17)                                                                                      # at most 2 rates in a row
    st, msg = _raw(z, b17, theta_max=32768.0 / (2 * tmax) * 1.01)
    assert st == 2 and "theta_max" in msg and "= 2)" in msg
    if L.phm_device_count() == 0:                                                                         # a valid call gets as far as the device
        assert _raw(z, m, theta_max=32768.0 / (8 * tmax) * 0.99)[0] == 3
        assert _raw(z, ratemodel.er(9))[0] == 3
        assert _raw(z, ratemodel.sym(64), theta_max=5.0)[0] == 3                                        # 63 rates in a row
        assert _raw(z, b17, soc=[0, 1, 1], stats=False, thin=3)[0] == 3


def test_the_narrow_entry_point_keeps_its_messages():
    z, _, _, _ = synth.config_problem(2, n_tips=16)
    z9 = dict(z, states=np.ones(16, dtype=np.int32))
    import test_gibbs_cpu
    st, msg = test_gibbs_cpu._raw(z9, ratemodel.er(9))
    assert st == 2 and msg == "phm_gibbs_rates: more than 8 states are not supported"
    st, msg = test_gibbs_cpu._raw(z, ratemodel.sym(4), n_states=1)
    assert st == 1 and msg == "phm_gibbs_rates: n_states must be in 2..8"


def test_a_model_without_an_index_is_refused():
    z, _, pid, _ = synth.config_problem(2, n_tips=16)
    with pytest.raises(ValueError, match="index model"):
        api.posterior_rates(z, ratemodel.hidden_rates(1), pid, [1.0, 1.0], 10)


@pytest.mark.parametrize("model", [ratemodel.er(9), ratemodel.sym(9), banded(17)], ids=["er9", "sym9", "banded17"])
def test_one_pass_update_is_gibbsrefs_on_the_summed_row(model):
    n, p = model.n, model.p
    rng = np.random.default_rng(n * 100 + p)
    for chain in range(4):
        T = np.concatenate([rng.uniform(0.1, 30.0, n), rng.integers(0, 40, n * (n - 1)).astype(np.float64)])
        theta = rng.uniform(0.05, 2.0, p)
        prior = rng.uniform(0.5, 3.0, (p, 2))
        theta_max = 1.0 if chain == 3 else 50.0                             # the last one rejects some
        got, rej = gibbswideref.update(model.index, theta, T, prior, theta_max, 11, chain, 7 + chain)
        want, rej_want = gibbsref.update(model.index, theta, T[None], prior, theta_max, 11, chain, 7 + chain)
        assert np.array_equal(got, want) and np.array_equal(rej, rej_want)
    Q = posterior.rate_matrices(model, theta[None])[0]
    assert np.array_equal(Q, gibbsref.build_Q(model.index, theta))


@pytest.fixture(scope="module")
def twin_run():
    edge, lens = synth.random_tree(12, 0.3, 4)
    m = ratemodel.er(9)
    Q = m.Q([0.15])
    sites = np.stack([sc.tips_for(edge, lens, Q, 8 + s) for s in range(3)])
    th0 = np.array([[0.3], [0.05]])
    kw = dict(pid=np.full(9, 1 / 9), sites=sites, iters=4, seed=3)
    loose = gibbswideref.run(edge, lens, m.index, th0, np.ones((1, 2)), 25.0, **kw)
    tight = gibbswideref.run(edge, lens, m.index, np.minimum(th0, 0.04), np.ones((1, 2)), 0.05, **kw)
    return lens, th0, loose, tight


def test_twin_run(twin_run):
    lens, th0, r, tight = twin_run
    S, n = 3, 9
    assert r["theta"].shape == (4, 2, 1) and r["stats"].shape == (4, 2, n * n) and np.all(r["status"] == 0)
    assert np.all(np.abs(r["stats"][:, :, :n].sum(axis=2) - S * lens.sum()) <= 1e-12 * S * lens.sum())     # dwell: S * tree length
    assert np.all(r["stats"][:, :, n:] == np.round(r["stats"][:, :, n:])) and np.all(np.isfinite(r["loglik"]))
    assert np.all(r["theta"] > 0.0) and np.all(r["theta"] <= 25.0) and np.all(r["rejected"] == 0)
    assert np.array_equal(r["theta"][0], th0)                                                              # row 0 is the start
    assert len(np.unique(r["theta"][:, 0, 0])) == 4                                                        # every iteration moves
    assert np.all(tight["theta"] <= 0.05) and np.all(tight["theta"] > 0.0)                                 # never exceeded,
    assert tight["rejected"].sum() > 0                                                                     # and draws are rejected
