"""Every state-count dispatch class of the exact (no-sampling) entry points on the device ("Dispatch
classes"): the lane kernels' instantiations for n = 5, 6, 7, the wide kernel's three classes at their first, an inner and their
unpadded last n (9, 16 | 17, 32 | 33, 64), the run-time-n paths of the log-likelihood, score, sampler and Gibbs kernels at
n = 5, 6, 7, and a branch at mu t_b = 800 -- e^(-mu t) not representable, a Poisson sum of over a thousand terms -- in every
class.  The checkers and their bars are the existing tests', imported, not copied: statistics and per-branch values 1e-12
relative with the floor of 1e-14 x tree length, log-likelihood 1e-12 max(1, |l|), posteriors 1e-13, counts, node states and map
offsets exactly."""
import functools
import math

import numpy as np
import pytest

import exactref
import fitref
import samplecases as sc
import stateclasses
import test_gpu_gibbs as gibbs
import test_gpu_sample_models as sample
import test_gpu_scores as scores
import test_gpu_time as through
import timeref
from phylomap_amd import api, synth
from test_gpu_expected import _check, _tips
from test_gpu_loglik_models import _bar as ll_bar

pytestmark = pytest.mark.gpu

LANE = (5, 6, 7)                         # one template instantiation each, none run by the six state counts of the other tests
WIDE = (9, 16, 17, 32, 33, 64)           # NP = 16 | 32 | 64: first of the class and the unpadded last


def _model(n, seed=0):
    return scores._models(n, 1, 0x5C00 + 16 * n + seed)[0] if n <= 8 else synth.dense_Q(n, 0.01, 0.04)


def _observe(n):
    return np.arange(n) % 2 + 1


@pytest.mark.parametrize("S", [1, 130])
@pytest.mark.parametrize("n", LANE + WIDE)
def test_expected_sumstat_against_the_uniformization_twin(n, S):
    """S = 130: real sites in several site groups of every NP class; S = 1: all but one lane of a block is padding"""
    Q = _model(n)
    z = scores._tree(24, 0x5C10 + n, True)
    pid = np.arange(1.0, n + 1.0)
    tips = _tips(z, Q, pid, S, seed=100 * n + S, observe=_observe(n))
    st, ll, br, post = _check(z, Q, pid, tips, observe=_observe(n), what=f"expected_sumstat n={n} S={S}")
    lens = np.asarray(z["edge.length"])
    np.testing.assert_allclose(br[:, :, :n].sum(axis=2), np.broadcast_to(lens, (S, lens.size)), rtol=1e-12, atol=0)
    np.testing.assert_allclose(st[:, :n].sum(axis=1), lens.sum(), rtol=1e-12)
    st2, ll2 = api.expected_sumstat(z, Q, pid, sites=tips, observe=_observe(n))
    assert np.array_equal(st2, st) and np.array_equal(ll2, ll)      # without per-branch / node outputs: the same bits


@pytest.mark.parametrize("n", LANE)
def test_expected_sumstat_against_the_van_loan_twin(n):
    Q = _model(n, 1)
    z = scores._tree(24, 0x5C20 + n, True)
    pid = np.ones(n)
    for observe in (None, _observe(n)):
        _check(z, Q, pid, _tips(z, Q, pid, 63, seed=7 + n, observe=observe), observe=observe, route="vanloan", rtol=1e-9,
               what=f"Van Loan n={n} observe={'parity' if observe is not None else 'none'}")


@pytest.mark.parametrize("n", [5, 7, 9, 16, 33])
def test_expected_through_time_against_the_twin(n):
    Q = _model(n, 2)
    z = through._tree(16, 0x5C30 + n, True)
    pid = np.arange(1.0, n + 1.0)
    observe = _observe(n)
    bounds, points = through._bounds(z), through._points(z)
    length = float(np.sum(z["edge.length"]))
    tips = through._tips(z, Q, pid, 63, seed=100 * n + 63, observe=observe)
    got = api.expected_through_time(z, Q, pid, bounds=bounds, points=points, sites=tips, observe=observe)
    want = timeref.through_time(z["edge"], z["edge.length"], Q, pid, tips, bounds=bounds, points=points, observe=observe)
    bins = np.abs(got["bins"] - want["bins"]) / (1e-12 * np.abs(want["bins"]) + 1e-14 * length)
    print(f"expected_through_time n={n}: error / allowance: occupancy {np.max(np.abs(got['occupancy'] - want['occupancy'])) / 1e-12:.3g}, "
          f"points {np.max(np.abs(got['points'] - want['points'])) / 1e-12:.3g}, bins {bins.max():.3g}")
    through._close(got["occupancy"], want["occupancy"], 0.0, 1e-12)
    through._close(got["points"], want["points"], 0.0, 1e-12)
    through._close(got["bins"], want["bins"], 1e-12, 1e-14 * length)
    st, ll = api.expected_sumstat(z, Q, pid, sites=tips, observe=observe)
    assert np.array_equal(got["loglik"], ll)
    through._close(got["bins"].sum(axis=1), st, 1e-11, 1e-14 * length)    # the bins cover the whole depth: their sum is the total


@pytest.mark.parametrize("n,K", [(n, K) for n in LANE for K in (1, 63, 64, 130)] + [(n, 2) for n in (9, 16, 17, 33)])
def test_models_entry_points_against_the_twins(n, K):
    """loglik_models against fitref.loglik_models and expected_sumstat_models against exactref.expected per model, with
    per-model pid, in cross and paired mode; the two device calls agree on the log-likelihood bit for bit.  A 16-tip tree and
    three sites: the twin takes one model at a time, 130 of them here."""
    z = scores._tree(16, 0x5C40 + n, True)
    length = float(np.sum(z["edge.length"]))
    observe = _observe(n)
    tips = scores._sites(16, n, 3, 7 * n, observe)
    Qs = scores._models(n, K, 100 * n + K) if n <= 8 else scores._wide_models(n, K, 0xA0 + n)
    rs = np.random.default_rng(K)
    pid = rs.uniform(0.1, 1.0, (K, n))
    som = rs.integers(0, 3, K)
    want, ll_want = scores._twin(z, Qs, pid, tips, observe)
    got, ll = api.expected_sumstat_models(z, Qs, pid, sites=tips, observe=observe)
    llm = api.loglik_models(z, Qs, pid, sites=tips, observe=observe)
    assert got.shape == (K, 3, n * n) and ll.shape == (K, 3) and np.array_equal(ll, llm)
    w = scores._bar(got, want, ll, ll_want, length)
    v = ll_bar(llm, fitref.loglik_models(z["edge"], z["edge.length"], Qs, pid, tips, observe))
    print(f"models n={n} K={K}: stats error / allowance {w[0]:.3g}, max |d loglik| / max(1, |loglik|): "
          f"expected_sumstat_models {w[1]:.3g}, loglik_models {v:.3g}")
    ok = np.isfinite(ll)
    np.testing.assert_allclose(got[ok][:, :n].sum(axis=1), length, rtol=1e-12)
    pst, pll = api.expected_sumstat_models(z, Qs, pid, sites=tips, observe=observe, site_of_model=som)
    pllm = api.loglik_models(z, Qs, pid, sites=tips, observe=observe, site_of_model=som)
    assert pst.shape == (K, n * n) and pll.shape == (K,) and np.array_equal(pll, pllm)
    scores._bar(pst, want[np.arange(K), som], pll, ll_want[np.arange(K), som], length)
    ll_bar(pllm, fitref.loglik_models(z["edge"], z["edge.length"], Qs, pid, tips, observe, site_of_model=som))
    assert np.array_equal(pll, ll[np.arange(K), som]) and np.array_equal(pst, got[np.arange(K), som], equal_nan=True)


@pytest.mark.parametrize("n", LANE + (9, 16, 17, 33))
def test_models_entry_points_against_expected_sumstat(n):
    """every rate positive: both calls give expected_sumstat's log-likelihood per model bit for bit"""
    z = scores._tree(24, 0x5C50 + n, True)
    length = float(np.sum(z["edge.length"]))
    K = 70 if n <= 8 else 2
    Qs = scores._positive(scores._models(n, K, 9 * n) if n <= 8 else scores._wide_models(n, K, 0xB0))
    pid = np.arange(1.0, n + 1.0)
    tips = scores._sites(24, n, 3, n, None)
    got, ll = api.expected_sumstat_models(z, Qs, pid, sites=tips)
    assert np.array_equal(ll, api.loglik_models(z, Qs, pid, sites=tips))
    ref = [api.expected_sumstat(z, Qs[k], pid, sites=tips) for k in range(K)]
    assert np.array_equal(ll, np.stack([r[1] for r in ref]))
    w = scores._bar(got, np.stack([r[0] for r in ref]), ll, ll, length)
    print(f"models n={n}: stats against expected_sumstat: error / allowance {w[0]:.3g}")


@pytest.mark.parametrize("n,K,S,D,second", [(5, 3, 2, 64, False), (6, 65, 1, 1, True), (7, 1, 2, 130, False)])
def test_sample_histories_against_the_twin(n, K, S, D, second):
    """``second``: shuffled edge rows, 10 % missing tips and a prior per model.  Seeds: none changed so far (the rule of
    test_gpu_sample_models' docstring: a flipped draw changes that case's seed and is recorded here)."""
    edge, lens = sc.tree(shuffle=second)
    assert lens.min() == 0.0
    Qs = sample.models(n, K, 100 * n + K)
    sites = np.stack([sc.tips_for(edge, lens, Qs[0], 50 + s, None, 0.1 if second else 0.0) for s in range(S)])
    z = sc.as_z(edge, lens, sites[0])
    sample.check_against_twin(z, Qs, sample.pids(n, K, second, n + K), sites, D, seed=1000 + n * K + D)


@pytest.mark.parametrize("n,Cn,joint", [(5, 63, False), (6, 64, True), (7, 130, False)])
def test_posterior_rates_lock_step(n, Cn, joint):
    gibbs.check_rows(gibbs.run(n, Cn, joint, True, 1))


# ---- a branch at mu t_b = 800 in every class -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long(n):
    edge, lens, Q, pid, tips = stateclasses.long_branch(n)
    assert float(np.max(-np.diag(Q))) * lens[stateclasses.B_LONG] > 745.0
    return sc.as_z(edge, lens, tips[0]), Q, pid, tips


@pytest.mark.parametrize("n", stateclasses.LONG_N)
def test_long_branch_expected_sumstat(n):
    z, Q, pid, tips = _long(n)
    st, ll, br, post = _check(z, Q, pid, tips, what=f"long branch n={n}")
    P = np.stack([exactref.transition_unif(Q, t) for t in z["edge.length"]])
    want = exactref.passes(z["edge"], z["edge.length"], Q, pid, tips, P=P)["loglik"]
    print(f"long branch n={n}: loglik against the uniformised P: {ll_bar(ll, want):.3g} (bar 1e-12)")
    np.testing.assert_allclose(br[:, :, :n].sum(axis=2), np.broadcast_to(z["edge.length"], (2, 10)), rtol=1e-12, atol=0)


@pytest.mark.parametrize("n", [5, 8])
def test_long_branch_models_entry_points(n):
    z, Q, pid, tips = _long(n)
    Qs = np.stack([Q, Q / 100.0, Q / 1000.0])
    length = float(np.sum(z["edge.length"]))
    got, ll = api.expected_sumstat_models(z, Qs, pid, sites=tips)
    assert np.array_equal(ll, api.loglik_models(z, Qs, pid, sites=tips))
    ref = [api.expected_sumstat(z, Qs[k], pid, sites=tips) for k in range(3)]
    assert np.array_equal(ll, np.stack([r[1] for r in ref]))
    w = scores._bar(got, np.stack([r[0] for r in ref]), ll, ll, length)
    want, ll_want = scores._twin(z, Qs, pid, tips, None)
    v = scores._bar(got, want, ll, ll_want, length)
    print(f"long branch models n={n}: stats error / allowance: against expected_sumstat {w[0]:.3g}, against the twin {v[0]:.3g}; "
          f"max |d loglik| / max(1, |loglik|) = {v[1]:.3g}")


def test_long_branch_sample_histories():
    n, D = 5, 64
    z, Q, pid, tips = _long(n)
    Qs = np.stack([Q, Q / 100.0, Q / 1000.0])
    stats, ll, nodes, m = sample.check_against_twin(z, Qs, pid / pid.sum(), tips[:1], D, seed=78)
    E = len(z["edge.length"])
    seg = m.counts().reshape(3, D, E)[0, :, stateclasses.B_LONG].astype(np.float64)
    _, _, br = api.expected_sumstat(z, Q, pid, sites=tips[:1], per_branch=True)
    want = 1.0 + float(br[0, stateclasses.B_LONG, n:].sum())
    zed = abs(seg.mean() - want) / (seg.std(ddof=1) / math.sqrt(D))
    print(f"long branch sample_histories n={n}: mean segments {seg.mean():.1f}, exact {want:.1f}, |z| = {zed:.2f}")
    assert seg.mean() > 300 and zed < 5.0
