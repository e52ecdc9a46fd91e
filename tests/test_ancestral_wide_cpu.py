"""Ancestral states per model at 9..64 states without a device: the C-ABI checks of
phm_ancestral_models_wide that run before any device call, the Python twin (tests/ancref.py) against the enumeration of all n^5
assignments of a 3-tip tree at 9, 12 and 16 states, and ancestral.collapse_states.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import ancref
from phylomap_amd import _lib, ancestral, synth


def _random_Q(n, rs):
    """a random non-symmetric rate matrix (every rate its own, `ard`-like), rates scaled so that branches stay informative"""
    Q = rs.uniform(0.05, 1.0, (n, n)) * 4.0 / n
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q


def _raw(z, Qs, pid, S=2, sel=None, n_sel=None, tree=True, q=True, p=True, post=True, states=True, logp=True, ll=True):
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
    status = L.phm_ancestral_models_wide(C.byref(t) if tree else None, n, K, _lib._p(Qf, C.c_double) if q else None,
                                         _lib._p(pid, C.c_double) if p else None, pid.size // n, None, None,
                                         _lib._p(sel, C.c_int32), n_sel, C.byref(o), _lib._p(lik, C.c_double),
                                         _lib._p(npost, C.c_double), _lib._p(js, C.c_int32), _lib._p(jl, C.c_double))
    return status, L.phm_last_error().decode()


def test_symbol_and_version():
    L = _lib.load()
    assert "phm_ancestral_models_wide" in _lib.EXPORTS and hasattr(L, "phm_ancestral_models_wide")
    assert L.phm_version() == 300


def test_c_abi_checks_need_no_device():
    L = _lib.load()
    n, T = 9, 16
    NT = 2 * T - 1
    edge, lens = synth.random_tree(T, 0.5, 3)
    z = {"edge": edge, "edge.length": lens, "Nnode": T - 1, "states": np.ones(T, dtype=np.int32)}
    rs = np.random.default_rng(3)
    Qs = np.stack([_random_Q(n, rs) for _ in range(3)])
    pid = np.ones(n)
    for missing in ("tree", "q", "p", "ll"):
        st, msg = _raw(z, Qs, pid, **{missing: False})
        assert st == 1 and "NULL argument" in msg, missing
    st, msg = _raw(z, Qs, pid, post=False, states=False, logp=False)
    assert st == 1 and "both NULL" in msg
    st, msg = _raw(z, Qs, pid, states=False)                                   # joint_logp alone
    assert st == 1 and "joint_logp needs joint_states" in msg
    st, msg = _raw(z, Qs, pid, n_sel=-1)
    assert st == 1 and "n_sel must be >= 0" in msg
    st, msg = _raw(z, Qs, pid, n_sel=2)                                        # node_sel NULL
    assert st == 1 and "node_sel is NULL" in msg
    st, msg = _raw(z, Qs, pid, sel=[17, 3, 0])
    assert st == 1 and "node_sel[2]" in msg
    st, msg = _raw(z, Qs, pid, sel=[NT + 1, 3])
    assert st == 1 and "node_sel[0]" in msg
    bad = Qs.copy()
    bad[2, 0, 3], bad[2, 0, 1] = -0.05, bad[2, 0, 1] + 0.05                  # ll_validate's checks come first
    st, msg = _raw(z, bad, pid, sel=[0])
    assert st == 1 and msg.startswith("model 2")
    for every in (True, False):                                                # 8 states: the narrow entry point's
        st, msg = _raw(z, synth.dense_Q(8, 0.01, 0.04)[None], np.ones(8), sel=None if every else [1])
        assert st == 2 and "go to phm_ancestral_models" in msg and msg.startswith("phm_ancestral_models_wide: ")
    st, msg = _raw(z, synth.dense_Q(65, 0.01, 0.04)[None], np.ones(65))
    assert st == 1 and "2..64" in msg
    if L.phm_device_count() == 0:                                              # a valid call gets as far as the device
        assert _raw(z, Qs, pid)[0] == 3
        assert _raw(z, Qs, pid, sel=[17, 1, 17, NT], post=False, logp=False)[0] == 3
        assert _raw(z, Qs, pid, states=False, logp=False)[0] == 3


# (n, seed, a missing tip, parity observe)
CASES = [(9, 0, False, False), (9, 1, True, False), (12, 0, False, True), (12, 1, False, False), (16, 0, False, False),
         (16, 1, True, True)]


@pytest.mark.parametrize("n,seed,missing,observed", CASES)
def test_twin_against_enumeration(n, seed, missing, observed):
    T = 3
    rs = np.random.default_rng(0xB31 + 100 * n + seed)
    edge, lens = synth.random_tree(T, 0.6, 7 * n + seed)
    Q, pid = _random_Q(n, rs), rs.uniform(0.2, 1.0, n)
    observe = (np.arange(n) % 2 + 1) if observed else None
    tips = rs.integers(1, (2 if observed else n) + 1, T)
    if missing:
        tips[1] = 0
    tips = tips[None]
    bx, blogp, bmarg, bll = ancref.brute_force(edge, lens, Q, pid, tips, observe)
    x, logp, margin = ancref.joint(edge, lens, Q, pid, tips, observe)
    post, ll = ancref.marginal(edge, lens, Q, pid, tips, observe)
    print(f"n={n} seed={seed} missing={missing} observe={observed}: margin {margin:.3g}, |logp - enumeration| "
          f"{abs(logp[0] - blogp):.3g}, max |marginal - enumeration| {np.max(np.abs(post[0] - bmarg)):.3g}")
    assert margin > 1e-9                                                       # no tie: the maximiser is unique
    assert np.array_equal(x[0], bx)
    assert abs(logp[0] - blogp) <= 1e-12 * max(1.0, abs(blogp))
    assert np.max(np.abs(post[0] - bmarg)) <= 1e-12
    assert abs(ll[0] - bll) <= 1e-12 * max(1.0, abs(bll))
    assert logp[0] <= ll[0]


def test_collapse_states():
    observe = [1, 2, 1, 3]
    post = np.array([[0.1, 0.2, 0.3, 0.4], [0.5, 0.0, 0.25, 0.25], [np.nan] * 4])
    got = ancestral.collapse_states(post, observe)
    assert got.shape == (3, 3)
    assert np.array_equal(got[:2], np.array([[0.1 + 0.3, 0.2, 0.4], [0.75, 0.0, 0.25]]))
    assert np.all(np.isnan(got[2]))
    deep = ancestral.collapse_states(np.tile(post[:2], (2, 5, 1, 1)), observe)   # leading axes pass through
    assert deep.shape == (2, 5, 2, 3) and np.array_equal(deep[1, 4], got[:2])
    ident = ancestral.collapse_states(post[:2], [1, 2, 3, 4])
    assert np.array_equal(ident, post[:2])
    states = np.array([[3, 1, 4], [2, 2, 1]])                                  # the joint reconstruction: observe[x - 1]
    assert np.array_equal(np.asarray(observe)[states - 1], [[1, 1, 3], [2, 2, 1]])
    with pytest.raises(ValueError):
        ancestral.collapse_states(post, [1, 2, 1])
    with pytest.raises(ValueError):
        ancestral.collapse_states(post, [0, 1, 1, 2])
