"""The Python twin (tests/exactref.py) at the state counts that tests/test_gpu_state_classes.py adds: its two routes against each
other at n = 5, 6, 7, 9, and on the long-branch input (mu t_b = 800) its log-likelihood with scipy's P against the same passes
with the uniformised P, which no Pade enters.  The second is the condition under which the twin alone stays well inside the
device's bar of 1e-12 max(1, |l|).  No GPU needed."""
import numpy as np
import pytest

import exactref
import stateclasses
from phylomap_amd import synth


def _models(n, seed):
    """one generator of test_gpu_scores._models: rates in (0.02, 1.5), a fifth of the entries structurally zero"""
    rs = np.random.default_rng(seed)
    Q = rs.uniform(0.02, 1.5, (n, n)) * rs.uniform(0.2, 3.0)
    Q[rs.random((n, n)) < 0.2] = 0.0
    idx = np.arange(n)
    Q[idx, (idx + 1) % n] += 0.05
    Q[idx, idx] = 0.0
    Q[idx, idx] = -Q.sum(axis=1)
    return Q


@pytest.mark.parametrize("n", [5, 6, 7, 9])
def test_van_loan_and_uniformization_routes_agree(n):
    Q = _models(n, 0x5C0 + n) if n <= 8 else synth.dense_Q(n, 0.05, 0.2)
    edge, lens = synth.random_tree(6, 1.0, 0xE0 + n)
    pid = np.arange(1.0, n + 1.0)
    tips = np.random.default_rng(n).integers(0, n + 1, (4, 6))
    a = exactref.expected(edge, lens, Q, pid, tips, per_branch=True)
    b = exactref.expected(edge, lens, Q, pid, tips, route="vanloan", per_branch=True)
    scale = np.max(np.abs(b[0]))
    worst = 0.0
    for x, y in ((a[0], b[0]), (a[2], b[2])):
        allow = 1e-10 * np.abs(y) + 1e-14 * scale
        worst = max(worst, float(np.max(np.abs(x - y) / allow)))
        assert np.all(np.abs(x - y) <= allow)
    print(f"n={n}: routes differ by {worst:.3g} of the allowance")
    assert np.array_equal(a[1], b[1])


def test_transition_unif_is_a_transition_matrix_and_agrees_with_expm_on_ordinary_branches():
    from scipy.linalg import expm
    for n in (2, 5, 9, 33):
        Q = stateclasses.long_Q(n, n)
        for t in (0.0, 1e-6, 0.03, 0.4, 2.5):
            P = exactref.transition_unif(Q, t)
            assert np.all(P >= 0.0)
            np.testing.assert_allclose(P.sum(axis=1), 1.0, rtol=0, atol=1e-14)
            np.testing.assert_allclose(P, expm(Q * t), rtol=0, atol=1e-13)     # scipy: a few squarings of entries <= 1
    assert np.array_equal(exactref.transition_unif(np.zeros((3, 3)), 1.0), np.eye(3))


@pytest.mark.parametrize("n", stateclasses.LONG_N)
def test_long_branch_loglik_does_not_depend_on_the_pade(n):
    edge, lens, Q, pid, tips = stateclasses.long_branch(n)
    mu = float(np.max(-np.diag(Q)))
    assert mu * lens[stateclasses.B_LONG] == pytest.approx(800.0, rel=1e-12) and mu * lens.max() > 745.0
    assert exactref.poisson_weights(mu * lens.max())[1] > 1000
    P = np.stack([exactref.transition_unif(Q, t) for t in lens])
    np.testing.assert_allclose(P.sum(axis=2), 1.0, rtol=0, atol=1e-13)
    a = exactref.passes(edge, lens, Q, pid, tips)["loglik"]
    b = exactref.passes(edge, lens, Q, pid, tips, P=P)["loglik"]
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    print(f"n={n}: scipy's P against the uniformised P: max |d loglik| / max(1, |loglik|) = {err.max():.3g}")
    assert np.all(np.isfinite(b)) and np.all(err <= 1e-13)
