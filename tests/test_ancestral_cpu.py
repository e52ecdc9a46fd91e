"""Ancestral states per model without a device: the Python twin (tests/ancref.py) against the enumeration
of all n^(2T-1) assignments, the C-ABI checks of phm_ancestral_models that run before any device call, and
phylomap_amd/ancestral.py.  No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest

import ancref
from phylomap_amd import _lib, ancestral, api, synth


def _random_Q(n, rs):
    """a random non-symmetric rate matrix (every rate its own, `ard`-like)"""
    Q = rs.uniform(0.05, 1.0, (n, n))
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q


CASES = [(T, n, seed, False) for T in (5, 6) for n in (2, 3, 4) for seed in (0, 1, 2)] + [(6, 4, 3, True)]


@pytest.mark.parametrize("T,n,seed,observed", CASES)
def test_twin_against_enumeration(T, n, seed, observed):
    rs = np.random.default_rng(1000 * T + 100 * n + seed)
    edge, lens = synth.random_tree(T, 0.6, 7 * T + n + seed)
    Q, pid = _random_Q(n, rs), rs.uniform(0.2, 1.0, n)
    observe = (np.arange(n) % 2 + 1) if observed else None
    tips = rs.integers(1, (2 if observed else n) + 1, T)
    tips[rs.random(T) < 0.25] = 0                                             # missing tips
    tips = tips[None]
    bx, blogp, bmarg, bll = ancref.brute_force(edge, lens, Q, pid, tips, observe)
    x, logp, margin = ancref.joint(edge, lens, Q, pid, tips, observe)
    post, ll = ancref.marginal(edge, lens, Q, pid, tips, observe)
    print(f"T={T} n={n} seed={seed} observe={observed}: margin {margin:.3g}, |logp - enumeration| {abs(logp[0] - blogp):.3g}, "
          f"max |marginal - enumeration| {np.max(np.abs(post[0] - bmarg)):.3g}")
    assert margin > 1e-9                                                       # no tie: the maximiser is unique
    assert np.array_equal(x[0], bx)
    assert abs(logp[0] - blogp) <= 1e-12 * max(1.0, abs(blogp))
    assert np.max(np.abs(post[0] - bmarg)) <= 1e-12
    assert abs(ll[0] - bll) <= 1e-12 * max(1.0, abs(bll))
    assert logp[0] <= ll[0]
    # the price of the twin's own assignment is its maximum, and any other assignment is no better
    assert abs(ancref.assignment_logp(edge, lens, Q, pid, tips, x, observe)[0] - blogp) <= 1e-12 * max(1.0, abs(blogp))
    other = x.copy()
    other[0, T] = other[0, T] % n + 1
    assert ancref.assignment_logp(edge, lens, Q, pid, tips, other, observe)[0] < logp[0]


def test_twin_marginal_is_exactrefs_node_posterior():
    import exactref
    rs = np.random.default_rng(5)
    edge, lens = synth.random_tree(12, 0.5, 3)
    Q, pid = _random_Q(3, rs), np.array([1.0, 2.0, 3.0])
    tips = rs.integers(0, 4, (4, 12))
    want = exactref.expected(edge, lens, Q, pid, tips, nodes=True)
    got, ll = ancref.marginal(edge, lens, Q, pid, tips)
    assert np.array_equal(got, want[2]) and np.array_equal(ll, want[1])


def _raw(z, Qs, pid, S=2, sel=None, n_sel=None, tree=True, q=True, post=True, states=True, logp=True, ll=True):
    Qs = np.asarray(Qs, dtype=np.float64)
    K, n = Qs.shape[0], Qs.shape[1]
    Qf = np.ascontiguousarray(Qs.transpose(0, 2, 1))
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    pt = _lib.PlainTree(z, np.tile(z["states"], (S, 1)))
    t, T = pt.c, pt.T
    o = _lib.make_options(n_replicas=S, tips_per_replica=True)
    sel = None if sel is None else np.ascontiguousarray(sel, dtype=np.int32)
    J = 2 * T - 1 if sel is None else sel.size
    n_sel = (0 if sel is None else sel.size) if n_sel is None else n_sel
    lik = np.zeros(K * S) if ll else None
    npost = np.zeros(K * S * J * n) if post else None
    js = np.zeros(K * S * J, dtype=np.int32) if states else None
    jl = np.zeros(K * S) if logp else None
    L = _lib.load()
    status = L.phm_ancestral_models(C.byref(t) if tree else None, n, K, _lib._p(Qf, C.c_double) if q else None,
                                    _lib._p(pid, C.c_double), pid.size // n, None, None, _lib._p(sel, C.c_int32), n_sel,
                                    C.byref(o), _lib._p(lik, C.c_double), _lib._p(npost, C.c_double), _lib._p(js, C.c_int32),
                                    _lib._p(jl, C.c_double))
    return status, L.phm_last_error().decode()


def test_c_abi_checks_need_no_device():
    L = _lib.load()
    assert "phm_ancestral_models" in _lib.EXPORTS and hasattr(L, "phm_ancestral_models")
    assert L.phm_version() == 300
    z, Q, pid, _ = synth.config_problem(2, n_tips=16)
    Qs = np.stack([Q, 2 * Q, 3 * Q])
    NT = 31
    assert _raw(z, Qs, pid, tree=False)[0] == 1
    assert _raw(z, Qs, pid, q=False)[0] == 1
    assert _raw(z, Qs, pid, ll=False)[0] == 1
    st, msg = _raw(z, Qs, pid, post=False, states=False, logp=False)
    assert st == 1 and "both NULL" in msg
    st, msg = _raw(z, Qs, pid, states=False)                                   # joint_logp alone
    assert st == 1 and "joint_logp needs joint_states" in msg
    st, msg = _raw(z, Qs, pid, sel=[17, 3, 0])
    assert st == 1 and "node_sel[2]" in msg
    st, msg = _raw(z, Qs, pid, sel=[NT + 1, 3])
    assert st == 1 and "node_sel[0]" in msg
    st, msg = _raw(z, Qs, pid, n_sel=-1)
    assert st == 1 and "n_sel" in msg
    st, msg = _raw(z, Qs, pid, n_sel=2)                                        # node_sel NULL
    assert st == 1 and "node_sel is NULL" in msg
    bad = Qs.copy()
    bad[2, 0, 3], bad[2, 0, 1] = -0.05, bad[2, 0, 1] + 0.05                  # ll_validate's checks come first
    st, msg = _raw(z, bad, pid)
    assert st == 1 and msg.startswith("model 2")
    z9 = dict(z, states=np.ones(16, dtype=np.int32))
    st, msg = _raw(z9, synth.dense_Q(9, 0.01, 0.04)[None], np.ones(9))
    assert st == 2 and "8 states" in msg
    if L.phm_device_count() == 0:                                              # a valid call gets as far as the device
        assert _raw(z, Qs, pid)[0] == 3
        assert _raw(z, Qs, pid, sel=[17, 1, 17, NT], post=False, logp=False)[0] == 3
        assert _raw(z, Qs, pid, states=False, logp=False)[0] == 3


def test_python_layer_refuses_nothing_to_compute():
    z, Q, pid, _ = synth.config_problem(2, n_tips=16)
    with pytest.raises(ValueError):
        api.ancestral_states_models(z, Q, pid, marginal=False, joint=False)
    assert api.AncestralStates._fields == ("loglik", "node_post", "joint_states", "joint_logp", "nodes")


def test_akaike_weights():
    w = ancestral.akaike_weights([-10.0, -11.0, -10.0], [1, 1, 2])
    raw = np.array([1.0, math.exp(-1.0), math.exp(-1.0)])                      # delta AIC 0, 2, 2
    np.testing.assert_allclose(w, raw / raw.sum(), rtol=1e-15)
    w = ancestral.akaike_weights([-1e4, -np.inf, -1e4 - math.log(2.0)], 3)
    np.testing.assert_allclose(w, [2.0 / 3.0, 0.0, 1.0 / 3.0], rtol=1e-12)
    assert w[1] == 0.0
    with pytest.raises(ValueError):
        ancestral.akaike_weights([-np.inf, -np.inf], 1)


def test_model_average():
    post = np.array([[[0.2, 0.8], [1.0, 0.0]], [[0.6, 0.4], [0.0, 1.0]], [[np.nan, np.nan], [np.nan, np.nan]]])   # [K=3, J=2, n=2]
    got = ancestral.model_average(post, [3.0, 1.0, 0.0])
    np.testing.assert_allclose(got, [[0.3, 0.7], [0.75, 0.25]], rtol=1e-15)
    np.testing.assert_allclose(ancestral.model_average(post[:2]), [[0.4, 0.6], [0.5, 0.5]], rtol=1e-15)
    assert np.all(np.isnan(ancestral.model_average(post)))                     # equal weights reach the NaN model
    moved = np.moveaxis(post, 0, 1)                                            # the model axis second
    np.testing.assert_allclose(ancestral.model_average(moved, [3.0, 1.0, 0.0], axis=1), got, rtol=1e-15)
    with pytest.raises(ValueError):
        ancestral.model_average(post, [1.0, 1.0])
    with pytest.raises(ValueError):
        ancestral.model_average(post, [1.0, -1.0, 1.0])


def test_mrca():
    # ((1,2)8,(3,(4,5)10)9)7 with 6 hanging off the root: 11 is the root
    edge = np.array([[11, 7], [11, 6], [7, 8], [7, 9], [8, 1], [8, 2], [9, 3], [9, 10], [10, 4], [10, 5]])
    z = {"edge": edge, "Nnode": 5}
    assert ancestral.mrca(z, [4, 5]) == 10
    assert ancestral.mrca(z, [3, 5]) == 9
    assert ancestral.mrca(z, [1, 2]) == 8
    assert ancestral.mrca(z, [2, 4]) == 7
    assert ancestral.mrca(z, [5, 6]) == 11
    assert ancestral.mrca(z, 3) == 3 and ancestral.mrca(z, [3, 3]) == 3       # a single tip
    assert ancestral.mrca(z, [1, 2, 3, 4, 5, 6]) == 11                         # all tips: the root
    with pytest.raises(ValueError):
        ancestral.mrca(z, [0, 2])
    with pytest.raises(ValueError):
        ancestral.mrca(z, [7])
