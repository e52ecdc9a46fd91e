"""The batched posterior sampler of rates without a device: the C-ABI refusals of phm_gibbs_rates by status and
message, the restated Gamma draw, a run of the Python twin (tests/gibbsref.py), ``posterior.summary`` / ``posterior.dic`` on
synthetic traces with known answers and the ``ValueError`` for a model without an index.  No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest

import gibbsref
import samplecases as sc
from phylomap_amd import _lib, api, posterior, ratemodel, synth


def _raw(z, model, C_=3, theta0=None, prior=None, n_prior=None, theta_max=50.0, pid=None, S=2, observe=None, soc=None, iters=4,
         thin=1, index=None, n_states=None, n_params=None, stats=True):
    n = model.n if n_states is None else n_states
    p = model.p if n_params is None else n_params
    idx = np.ascontiguousarray(np.asarray(model.index if index is None else index, dtype=np.int32).T)
    th0 = np.ascontiguousarray(np.full((C_, p), 0.5) if theta0 is None else theta0, dtype=np.float64)
    pr = np.ascontiguousarray(np.ones((1, p, 2)) if prior is None else prior, dtype=np.float64)
    pid = np.ascontiguousarray(np.full(n, 1.0 / n) if pid is None else pid, dtype=np.float64)
    pt = _lib.PlainTree(z, np.tile(z["states"], (S, 1)))
    t = pt.c
    obs = None if observe is None else np.ascontiguousarray(observe, dtype=np.int32)
    so = None if soc is None else np.ascontiguousarray(soc, dtype=np.int32)
    o = _lib.make_options(n_replicas=S, tips_per_replica=True)
    rows = max(1, -(-iters // max(thin, 1)))
    cols = n + n * (n - 1)
    theta, ll = np.zeros((rows, C_, p)), np.zeros((rows, C_))
    sts = np.zeros((rows, C_, cols)) if stats else None
    rej, status = np.zeros((C_, p), dtype=np.int32), np.zeros(C_, dtype=np.int32)
    L = _lib.load()
    code = L.phm_gibbs_rates(C.byref(t), n, _lib._p(idx, C.c_int32), p, C_, _lib._p(th0, C.c_double), _lib._p(pr, C.c_double),
                             pr.shape[0] if n_prior is None else n_prior, theta_max, _lib._p(pid, C.c_double), 1,
                             _lib._p(obs, C.c_int32), _lib._p(so, C.c_int32), iters, thin, C.byref(o), _lib._p(theta, C.c_double),
                             _lib._p(ll, C.c_double), _lib._p(sts, C.c_double), _lib._p(rej, C.c_int32), _lib._p(status, C.c_int32))
    return code, L.phm_last_error().decode()


def test_c_abi_checks_need_no_device():
    L = _lib.load()
    assert "phm_gibbs_rates" in _lib.EXPORTS and hasattr(L, "phm_gibbs_rates")
    assert L.phm_version() == 300 and callable(api.posterior_rates)
    z, _, _, _ = synth.config_problem(2, n_tips=16)                         # 4 states
    m = ratemodel.sym(4)
    # index with a gap in 1..p: parameter 3 owns nothing
    gap = np.where(m.index == 3, 2, m.index)
    st, msg = _raw(z, m, index=gap)
    assert st == 1 and "parameter 3" in msg
    st, msg = _raw(z, m, index=np.where(m.index == 6, 7, m.index))          # an entry beyond p
    assert st == 1 and "parameter 7" in msg
    pr = np.ones((1, m.p, 2))
    pr[0, 4, 0] = 0.0
    st, msg = _raw(z, m, prior=pr)
    assert st == 1 and "parameter 5" in msg
    pr = np.ones((3, m.p, 2))
    pr[2, 1, 1] = -1.0
    st, msg = _raw(z, m, prior=pr)
    assert st == 1 and "parameter 2" in msg and "row 2" in msg
    assert _raw(z, m, prior=np.ones((2, m.p, 2)))[0] == 1                   # n_prior neither 1 nor C
    th = np.full((3, m.p), 0.5)
    th[1, 2] = 0.0
    st, msg = _raw(z, m, theta0=th)
    assert st == 1 and "chain 1" in msg and "parameter 3" in msg
    th[1, 2] = 51.0                                                          # above theta_max = 50
    st, msg = _raw(z, m, theta0=th)
    assert st == 1 and "chain 1" in msg and "theta_max" in msg
    st, msg = _raw(z, m, iters=0)
    assert st == 1 and "iters" in msg
    st, msg = _raw(z, m, thin=0)
    assert st == 1 and "thin" in msg
    st, msg = _raw(z, m, soc=[0, 2, 1])                                     # S = 2
    assert st == 1 and "chain 1" in msg
    st, msg = _raw(z, m, soc=[0, -1, 1])
    assert st == 1 and "chain 1" in msg
    assert _raw(z, m, observe=[1, 2, 1, 5])[0] == 1                         # ll_validate's checks follow
    assert _raw(z, m, pid=[0.5, 0.5, -0.1, 0.1])[0] != 0
    m9 = ratemodel.er(9)
    z9 = dict(z, states=np.ones(16, dtype=np.int32))
    st, msg = _raw(z9, m9)
    assert st == 2 and "8 states" in msg
    # theta_max bounds the uniformization rate: 3 rates in a row * theta_max * longest branch <= 32768
    tmax = float(np.max(z["edge.length"]))
    st, msg = _raw(z, m, theta_max=32768.0 / (3 * tmax) * 1.01)
    assert st == 2 and "theta_max" in msg
    if L.phm_device_count() == 0:                                            # a valid call gets as far as the device
        assert _raw(z, m, theta_max=32768.0 / (3 * tmax) * 0.99)[0] == 3
        assert _raw(z, m)[0] == 3
        assert _raw(z, m, soc=[0, 1, 1], stats=False, thin=3)[0] == 3


def test_hidden_rates_is_refused():
    z, _, pid, _ = synth.config_problem(2, n_tips=16)
    with pytest.raises(ValueError, match="index model"):
        api.posterior_rates(z, ratemodel.hidden_rates(1), pid, [1.0, 1.0], 10)
    with pytest.raises(ValueError):
        posterior.rate_matrices(ratemodel.hidden_rates(1), np.ones((1, 5)))


@pytest.mark.parametrize("shape", [0.3, 1.0, 7.5])
def test_restated_gamma_moments(shape):
    # mean shape * scale, variance shape * scale^2; the standard errors of the two estimates from the Gamma's own moments:
    # var(x) = k s^2, var((x - m)^2) = mu_4 - var^2 = (3 k^2 + 6 k) s^4 - k^2 s^4 = (2 k^2 + 6 k) s^4
    M, scale = 20000, 0.7
    x = np.array([gibbsref.Stream(11, gibbsref.ENT_RATE | 1, d, 5).gamma(shape, scale) for d in range(M)])
    assert np.all(x > 0.0)
    z_mean = (x.mean() - shape * scale) / math.sqrt(shape * scale ** 2 / M)
    z_var = (x.var(ddof=1) - shape * scale ** 2) / math.sqrt((2 * shape ** 2 + 6 * shape) * scale ** 4 / M)
    print(f"shape {shape}: z(mean) = {z_mean:.2f}, z(var) = {z_var:.2f}")
    assert abs(z_mean) < 5.0 and abs(z_var) < 5.0


def test_rate_matrices_are_the_twins():
    for m in (ratemodel.ard(2), ratemodel.sym(3), ratemodel.er(8), ratemodel.index_model([[0, 1, 0, 2], [1, 0, 3, 0], [0, 2, 0, 1], [3, 0, 1, 0]])):
        th = np.random.default_rng(m.n).uniform(0.05, 2.0, (5, m.p))
        Q = posterior.rate_matrices(m, th)
        assert np.array_equal(Q, np.stack([gibbsref.build_Q(m.index, t) for t in th]))
        assert np.allclose(Q, m.Qs(th), rtol=1e-15, atol=0.0)


@pytest.fixture(scope="module")
def twin_run():
    edge, lens = synth.random_tree(12, 0.3, 4)
    m = ratemodel.ard(2)
    tips = sc.tips_for(edge, lens, m.Q([0.4, 0.7]), 8)
    th0 = np.array([[0.3, 0.5], [1.0, 0.2]])
    args = (edge, lens, m.index, th0, np.ones((2, 2)))
    kw = dict(pid=[0.5, 0.5], sites=tips[None], iters=6, site_of_chain=[0, 0], seed=3)
    tight = (edge, lens, m.index, np.minimum(th0, 0.5), np.ones((2, 2)))
    return lens, gibbsref.run(*args, theta_max=25.0, **kw), gibbsref.run(*tight, theta_max=0.55, **kw)


def test_twin_run(twin_run):
    lens, r, tight = twin_run
    assert r["theta"].shape == (6, 2, 2) and np.all(r["status"] == 0)
    assert np.all(np.abs(r["stats"][:, :, :2].sum(axis=2) - lens.sum()) <= 1e-12 * lens.sum())   # the dwell columns sum to the tree length
    assert np.all(r["stats"][:, :, 2:] == np.round(r["stats"][:, :, 2:])) and np.all(np.isfinite(r["loglik"]))
    assert np.all(r["theta"] > 0.0) and np.all(r["theta"] <= 25.0) and np.all(r["rejected"] == 0)
    assert np.array_equal(r["theta"][0], np.array([[0.3, 0.5], [1.0, 0.2]]))                      # row 0 is the start
    assert len(np.unique(r["theta"][:, 0, 0])) == 6                                               # and every iteration moves
    assert np.all(tight["theta"] <= 0.55) and np.all(tight["theta"] > 0.0)                        # a tiny theta_max: never exceeded,
    assert tight["rejected"].sum() > 0                                                            # and draws are rejected


def test_summary_and_dic_on_synthetic_traces():
    rows, chains = 200, 4
    t = np.arange(rows, dtype=np.float64)
    base = np.where(t % 2 == 0, -1.0, 1.0)                                  # mean 0, the same in both halves of a chain
    x = np.zeros((rows, chains, 2))
    x[:, :, 0] = 3.0 + base[:, None]                                        # identical chains
    x[:, :, 1] = base[:, None] + 10.0 * np.arange(chains)[None, :]          # chains that sit apart
    s = posterior.summary(x, probs=(0.5,))
    assert s["n"] == rows * chains and np.allclose(s["mean"], [3.0, 15.0])
    assert abs(s["sd"][0] - math.sqrt(rows * chains / (rows * chains - 1.0))) < 1e-12
    assert s["quantiles"].shape == (1, 2)
    # identical sequences: B = 0, R-hat = sqrt((L - 1) / L); apart: W = L / (L - 1), B = L var(means)
    Lh = rows // 2
    assert abs(s["rhat"][0] - math.sqrt((Lh - 1) / Lh)) < 1e-12
    W = Lh / (Lh - 1.0)
    B = Lh * np.var(np.repeat(10.0 * np.arange(chains), 2), ddof=1)
    assert abs(s["rhat"][1] - math.sqrt(((Lh - 1) / Lh * W + B / Lh) / W)) < 1e-12 and s["rhat"][1] > 5
    assert np.allclose(posterior.summary(x, burn=100)["mean"], [3.0, 15.0])
    x4 = np.stack([x, x + 1.0], axis=1)                                     # a per-site trace [rows, S, chains, p]
    s4 = posterior.summary(x4)
    assert s4["mean"].shape == (2, 2) and np.allclose(s4["mean"][1], [4.0, 16.0])
    xn = x.copy()
    xn[50:, 2] = np.nan                                                     # a failed chain is left out
    assert posterior.summary(xn)["n"] == rows * 3
    # DIC: loglik values -10, -12 -> mean(-2 l) = 22; D = 20 -> pD = 2, DIC = 24
    val, D, pD = posterior.dic_from(np.array([[-10.0, -12.0], [-12.0, -10.0]]), 20.0)
    assert (val, D, pD) == (24.0, 20.0, 2.0)
