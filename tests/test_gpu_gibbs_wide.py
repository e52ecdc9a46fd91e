"""The posterior sampler of rates at 9..64 states on the device (phm_gibbs_rates_wide / api.posterior_rates).

Lock-step equivalence, as tests/test_gpu_gibbs.py has it for 2..8 states: for every recorded row i the DRIVER'S OWN theta^(i) goes
back through the public calls -- the row's counts are ``api.sample_histories(draws=1, replica_offset=i)``'s summed over the sites
exactly, its dwell sums agree with theirs (added sites ascending) within 1e-12 * S * tree length, its log-likelihood is
``api.loglik_models``' summed sites ascending bit for bit, and the twin's one-pass update (tests/gibbswideref.py) of the driver's
own ``stats`` row gives theta^(i+1) within 1e-12 relative.  The shapes are the smallest at which the sites mapping (a tile = 64
consecutive sites of one chain) can go wrong: the first and last unpadded state count of every lane class and the codon model's
61; 1, 3, 64, 65 (a second tile with one live lane, the last chain's included) and 130 sites; 1 and 3 chains; paired mode, where a
tile has one live lane.  Then: chunks, devices, ``stats=False`` and ``replica_offset``; a tight theta_max; an impossible site
that fails one chain alone; and the scheme itself against a posterior computed by quadrature, which no code under test enters.

Every test here fails on a library without the entry point: ``api.posterior_rates`` raises above 8 states there."""
import functools
import math

import numpy as np
import pytest

import gibbswideref
import samplecases as sc
from phylomap_amd import api, posterior, ratemodel, synth

pytestmark = pytest.mark.gpu

ITERS = 4
STATES = [9, 16, 17, 32, 33, 61, 64]
KEYS = ("theta", "loglik", "stats", "rejected", "status")


def model_of(n):
    return {9: ratemodel.er, 16: ratemodel.sym, 32: ratemodel.er, 61: ratemodel.er, 64: ratemodel.sym}.get(
        n, lambda k: ratemodel.index_model(gibbswideref.banded_index(k)))(n)


def rate_scale(m):
    """4 / (most rates in a row): a state's total rate does not grow with n"""
    return 4.0 / int(np.max(np.sum(np.asarray(m.index) > 0, axis=1)))


def parity(n):
    return tuple(1 + (i % 2) for i in range(n))


@functools.lru_cache(maxsize=None)
def problem(n, S, observe=False):
    """a 24-tip tree with shuffled edges and one zero-length branch, S sites; observe: parity map and 10 % missing tips"""
    edge, lens = sc.tree(shuffle=True)
    assert lens.min() == 0.0
    m = model_of(n)
    obs = parity(n) if observe else None
    Q = m.Q(np.linspace(0.2, 0.5, m.p) * rate_scale(m))
    sites = np.stack([sc.tips_for(edge, lens, Q, 70 + s, obs, 0.1 if observe else 0.0) for s in range(S)])
    assert not observe or np.any(sites == 0)
    return sc.as_z(edge, lens, sites[0]), m, obs, sites, np.full(n, 1.0 / n)


def flat(res, Cn):
    """the result with one chain axis, whatever the mode"""
    out = {}
    for k in KEYS:
        v = res[k]
        if v is None:
            out[k] = None
            continue
        lead = 0 if k in ("rejected", "status") else 1
        out[k] = v.reshape(v.shape[:lead] + (Cn,) + v.shape[lead + (2 if res["per_site"] else 1):])
    return out


@functools.lru_cache(maxsize=None)
def run(n, Cn, S, joint=True, per_chain_prior=False, thin=1, tmax_factor=20.0, expect_chunk=0, devices=None, replica_offset=0,
        stats=True, observe=False):
    """joint: Cn chains on all S sites; paired: Cn / S chains on each of S sites"""
    z, m, obs, sites, pid = problem(n, S, observe)
    s = rate_scale(m)
    rng = np.random.default_rng(1000 * n + 10 * Cn + S)
    theta_max = tmax_factor * s
    th0 = rng.uniform(0.1, min(1.5, tmax_factor), (Cn, m.p)) * s
    prior = rng.uniform(0.5, 3.0, (Cn, m.p, 2)) if per_chain_prior else np.tile([1.5, 2.0], (m.p, 1))
    prior = prior * np.array([1.0, 1.0 / s])                                 # the rate of the prior on the scale of the rates
    seed = 40 + n + Cn + S
    opt = {} if devices is None else {"devices": list(devices)}
    if expect_chunk:
        opt["expect_chunk"] = expect_chunk
    res = api.posterior_rates(z, m, pid, prior, ITERS, chains=Cn if joint else Cn // S, sites=sites, observe=obs, per_site=not joint,
                              theta0=th0, theta_max=theta_max, thin=thin, seed=seed, replica_offset=replica_offset, stats=stats, **opt)
    som = res["site_of_chain"]
    assert (som is None) == joint and (joint or (np.bincount(som).min() == Cn // S and Cn // S * S == Cn))
    return dict(flat(res, Cn), z=z, m=m, obs=obs, sites=sites, pid=pid, prior=np.broadcast_to(prior, (Cn, m.p, 2)), seed=seed, som=som,
                theta_max=theta_max, thin=thin, C=Cn, offset=replica_offset)


def check_rows(r):
    """every recorded row of run r against the public calls and the twin's update of the driver's own row; returns
    (dwell bitwise, theta bitwise)"""
    m, z, n, Cn = r["m"], r["z"], r["m"].n, r["C"]
    cols = n + n * (n - 1)
    tree_len = float(np.sum(z["edge.length"]))
    rows = r["theta"].shape[0]
    assert rows == -(-ITERS // r["thin"]) and np.all(r["status"] == 0)
    kw = dict(sites=r["sites"], observe=r["obs"], site_of_model=r["som"])
    dwell_bits, theta_bits, worst_dwell, worst_theta = True, True, 0.0, 0.0
    for row in range(rows):
        i = row * r["thin"]
        th = r["theta"][row]
        Qs = posterior.rate_matrices(m, th)
        st, ll = api.sample_histories(z, Qs, r["pid"], 1, seed=r["seed"], replica_offset=i + r["offset"], **kw)
        st = st[..., 0, :].reshape(Cn, -1, cols)                             # [C, sites of the chain, cols]
        Sn = st.shape[1]
        got = r["stats"][row]
        assert np.array_equal(st[:, :, n:].sum(axis=1), got[:, n:])
        dw = np.zeros((Cn, n))
        for s in range(Sn):                                                  # sites ascending
            dw = dw + st[:, s, :n]
        worst_dwell = max(worst_dwell, float(np.max(np.abs(dw - got[:, :n]))))
        dwell_bits = dwell_bits and np.array_equal(dw, got[:, :n])
        assert np.all(np.abs(got[:, :n].sum(axis=1) - Sn * tree_len) <= 1e-12 * Sn * tree_len)
        llm = api.loglik_models(z, Qs, r["pid"], **kw).reshape(Cn, -1)
        tot = np.zeros(Cn)
        for s in range(Sn):
            tot = tot + llm[:, s]
        assert np.array_equal(tot, r["loglik"][row]) and np.array_equal(ll.reshape(Cn, -1), llm)
        if r["thin"] == 1 and row + 1 < rows:
            for k in range(Cn):
                want, _ = gibbswideref.update(m.index, th[k], got[k], r["prior"][k], r["theta_max"], r["seed"], k, i + r["offset"])
                nxt = r["theta"][row + 1, k]
                worst_theta = max(worst_theta, float(np.max(np.abs(nxt - want) / want)))
                theta_bits = theta_bits and np.array_equal(nxt, want)
    print(f"n={n} C={Cn} S={Sn}: max |dwell - sample_histories'| = {worst_dwell:.3g} (bound {1e-12 * Sn * tree_len:.3g}), bitwise = "
          f"{dwell_bits}; max relative theta difference to the twin's update = {worst_theta:.3g}, bitwise = {theta_bits}")
    assert worst_dwell <= 1e-12 * Sn * tree_len
    assert worst_theta <= 1e-12
    assert np.all(r["theta"] > 0.0) and np.all(r["theta"] <= r["theta_max"])
    return dwell_bits, theta_bits


@pytest.mark.parametrize("n", STATES)
def test_every_state_count_class(n):
    check_rows(run(n, 3, 3, per_chain_prior=n % 2 == 0))


@pytest.mark.parametrize("per_chain_prior", [False, True])
@pytest.mark.parametrize("n", [9, 33])
def test_shared_and_per_chain_priors(n, per_chain_prior):
    check_rows(run(n, 3, 3, per_chain_prior=per_chain_prior))


@pytest.mark.parametrize("S", [1, 3, 64, 65, 130])
@pytest.mark.parametrize("n", [9, 33])
def test_every_site_count(n, S):
    """one lane, a part of a tile, a full tile, a second tile with ONE live lane (the last chain's last tile reaches past the
    evaluations if an idle lane loads anything) and a third tile"""
    check_rows(run(n, 3, S, per_chain_prior=True))


@pytest.mark.parametrize("n", [9, 33])
def test_one_chain_at_65_sites(n):
    check_rows(run(n, 1, 65))


@pytest.mark.parametrize("n", [9, 33])
def test_paired_mode(n):
    """2 chains per site over 3 sites: a chain has one site, so a tile has one live lane"""
    check_rows(run(n, 6, 3, joint=False, per_chain_prior=True))


@pytest.mark.parametrize("n", [9, 33])
def test_thinned_rows_are_the_full_runs(n):
    r, full = run(n, 3, 3, thin=2), run(n, 3, 3)
    check_rows(r)
    for k in ("theta", "loglik", "stats"):
        assert np.array_equal(r[k], full[k][::2])
    assert np.array_equal(r["rejected"], full["rejected"])


def test_parity_observe_with_missing_tips():
    r = run(16, 3, 3, per_chain_prior=True, observe=True)
    assert set(np.unique(r["sites"])) == {0, 1, 2}
    check_rows(r)


@pytest.mark.parametrize("joint", [True, False])
@pytest.mark.parametrize("n", [9, 33])
def test_chunks_and_devices_change_no_bit(n, joint):
    Cn, S = (3, 65) if joint else (6, 3)
    base = run(n, Cn, S, joint=joint, per_chain_prior=True)
    for kw in (dict(expect_chunk=1), dict(devices=(0, 0))):
        other = run(n, Cn, S, joint=joint, per_chain_prior=True, **kw)
        for k in KEYS:
            assert np.array_equal(base[k], other[k]), (kw, k)


@pytest.mark.parametrize("n", [9, 33])
def test_replica_offset_and_stats_off(n):
    base = run(n, 3, 3)
    shifted = run(n, 3, 3, replica_offset=5)                                 # histories and rates at iteration + 5
    check_rows(shifted)
    assert np.array_equal(shifted["theta"][0], base["theta"][0]) and not np.array_equal(shifted["theta"][1], base["theta"][1])
    bare = run(n, 3, 3, stats=False)
    assert bare["stats"] is None
    for k in ("theta", "loglik", "rejected", "status"):
        assert np.array_equal(base[k], bare[k]), k


def test_tight_theta_max_rejects():
    r = run(9, 3, 3, tmax_factor=0.12)
    assert r["rejected"].sum() > 0 and np.all(r["theta"] <= r["theta_max"])
    check_rows(r)                                                            # the kept values are the twin's too


def block_problem():
    """two blocks that no rate joins, states 1..5 and 6..9, and tips of both: 64 sites inside the first block, one inside the
    second; a root prior without the second block makes that one site impossible"""
    edge, lens = sc.tree(shuffle=True)
    plain = sc.tree()                                                        # the same tree in cladewise rows, which the simulation walks
    idx = np.zeros((9, 9), dtype=np.int64)
    idx[:5, :5], idx[5:, 5:] = 1, 2
    np.fill_diagonal(idx, 0)
    m = ratemodel.index_model(idx)
    Q = m.Q([0.4, 0.3])
    first, second = np.r_[np.full(5, 0.2), np.zeros(4)], np.r_[np.zeros(5), np.full(4, 0.25)]
    sites = np.stack([synth.simulate_tips(*plain, Q, second if s == 40 else first, 300 + s) for s in range(65)]).astype(np.int32)
    assert sites[40].min() >= 6 and np.delete(sites, 40, axis=0).max() <= 5
    return edge, lens, m, sites, first, np.full(9, 1.0 / 9)


def test_an_impossible_site_fails_its_chain_alone_joint():
    edge, lens, m, sites, first, both = block_problem()
    z = sc.as_z(edge, lens, sites[0])
    Cn, dead = 3, 1
    pid = np.stack([first if k == dead else both for k in range(Cn)])        # chain 1 cannot start in the second block
    th0 = np.random.default_rng(3).uniform(0.1, 1.0, (Cn, 2))
    res = api.posterior_rates(z, m, pid, [1.0, 1.0], ITERS, chains=Cn, sites=sites, theta0=th0, theta_max=20.0, seed=9)
    f = flat(res, Cn)
    live = np.arange(Cn) != dead
    assert f["status"][dead] == 1 and f["status"].sum() == 1 and np.all(f["rejected"][dead] == 0)
    assert np.all(np.isnan(f["theta"][:, dead])) and np.all(np.isnan(f["loglik"][:, dead])) and np.all(np.isnan(f["stats"][:, dead]))
    assert np.all(np.isfinite(f["theta"][:, live])) and np.all(np.isfinite(f["loglik"][:, live])) and np.all(np.isfinite(f["stats"][:, live]))
    # the live chains against the public calls; the dead chain stays in the redraw with its start (it moves nothing of theirs)
    tree_len, n = float(lens.sum()), 9
    prior = np.ones((2, 2))
    for row in range(ITERS):
        th = np.where(np.isnan(f["theta"][row]), th0, f["theta"][row])
        Qs = posterior.rate_matrices(m, th)
        st, ll = api.sample_histories(z, Qs, pid, 1, sites=sites, seed=9, replica_offset=row)
        assert np.isneginf(ll[dead, 40]) and np.all(np.isfinite(np.delete(ll[dead], 40)))
        st = st[:, :, 0, :]
        got = f["stats"][row]
        assert np.array_equal(st[live][:, :, n:].sum(axis=1), got[live][:, n:])
        dw, tot = np.zeros((Cn, n)), np.zeros(Cn)
        for s in range(65):
            dw, tot = dw + st[:, s, :n], tot + ll[:, s]
        assert np.all(np.abs(dw[live] - got[live][:, :n]) <= 1e-12 * 65 * tree_len)
        assert np.array_equal(tot[live], f["loglik"][row][live])
        if row + 1 < ITERS:
            for k in np.flatnonzero(live):
                want, _ = gibbswideref.update(m.index, th[k], got[k], prior, 20.0, 9, int(k), row)
                assert np.all(np.abs(f["theta"][row + 1, k] - want) <= 1e-12 * want)


def test_an_impossible_site_fails_its_chain_alone_paired():
    edge, lens, m, sites, first, _ = block_problem()
    z = sc.as_z(edge, lens, sites[0])
    three = sites[[0, 40, 1]]                                                # chain 1 sits on the site of the second block
    th0 = np.random.default_rng(4).uniform(0.1, 1.0, (3, 2))
    res = api.posterior_rates(z, m, first, [1.0, 1.0], ITERS, chains=1, sites=three, per_site=True, theta0=th0, theta_max=20.0, seed=9)
    f = flat(res, 3)
    assert np.array_equal(f["status"], [0, 1, 0]) and np.all(f["rejected"][1] == 0)
    assert np.all(np.isnan(f["theta"][:, 1])) and np.all(np.isnan(f["loglik"][:, 1])) and np.all(np.isnan(f["stats"][:, 1]))
    som = res["site_of_chain"]
    # paired: evaluation ids are site * C + chain, so the live chains are redrawn inside the same three-chain call
    for row in range(ITERS):
        th = np.where(np.isnan(f["theta"][row]), th0, f["theta"][row])
        st, ll = api.sample_histories(z, posterior.rate_matrices(m, th), first, 1, sites=three, site_of_model=som, seed=9,
                                      replica_offset=row)
        assert np.isneginf(ll[1])
        for k in (0, 2):
            assert np.array_equal(st[k, 0, 9:], f["stats"][row, k, 9:]) and ll[k] == f["loglik"][row, k]
            assert np.all(np.abs(st[k, 0, :9] - f["stats"][row, k, :9]) <= 1e-12 * float(lens.sum()))
            if row + 1 < ITERS:
                want, _ = gibbswideref.update(m.index, th[k], f["stats"][row, k], np.ones((2, 2)), 20.0, 9, k, row)
                assert np.all(np.abs(f["theta"][row + 1, k] - want) <= 1e-12 * want)


def grid_moments(z, sites, pid, theta_max, G):
    """E theta, E theta^2 and the posterior sd on a midpoint grid of G rates over (0, theta_max]: loglik_models (summed over the
    sites) x the Gamma(1, 1) prior density"""
    m = ratemodel.er(9)
    g = (np.arange(G) + 0.5) * (theta_max / G)
    ll = api.loglik_models(z, posterior.rate_matrices(m, g[:, None]), pid, sites=sites).sum(axis=1)
    logw = ll - g                                                            # Gamma(1, 1): density exp(-theta)
    w = np.exp(logw - logw.max())
    w /= w.sum()
    e1, e2 = float(w @ g), float(w @ g ** 2)
    return e1, e2, math.sqrt(e2 - e1 ** 2), math.sqrt(float(w @ g ** 4) - e2 ** 2)


def test_the_scheme_against_quadrature():
    m = ratemodel.er(9)
    edge, lens = sc.tree(shuffle=True)
    pid = np.full(9, 1.0 / 9)
    Q = m.Q([0.1])
    sites = np.stack([sc.tips_for(edge, lens, Q, 31 + s) for s in range(8)])
    z = sc.as_z(edge, lens, sites[0])
    theta_max, Cn, iters, burn = 0.5, 64, 300, 100
    e1, e2, sd1, sd2 = grid_moments(z, sites, pid, theta_max, 800)
    c1, c2, _, _ = grid_moments(z, sites, pid, theta_max, 400)
    assert abs(e1 - c1) < 1e-3 * sd1 and abs(e2 - c2) < 1e-3 * sd2           # the grid is converged: halving its step moves nothing
    assert e1 + 6 * sd1 < theta_max                                          # and the truncation is far in the tail
    th0 = np.exp(np.random.default_rng(8).uniform(math.log(0.01), math.log(0.4), (Cn, 1)))      # dispersed starts
    res = api.posterior_rates(z, m, pid, [1.0, 1.0], iters, chains=Cn, sites=sites, theta0=th0, theta_max=theta_max, seed=77)
    assert np.all(res["status"] == 0)
    th = res["theta"][burn:, :, 0]
    for name, x, want in (("E theta", th, e1), ("E theta^2", th ** 2, e2)):
        per_chain = x.mean(axis=0)
        est, se = float(per_chain.mean()), float(per_chain.std(ddof=1)) / math.sqrt(Cn)
        zed = (est - want) / se
        print(f"{name}: driver {est:.6f} +- {se:.6f}, quadrature {want:.6f}, z = {zed:.2f}")
        assert abs(zed) < 5.0, name
    s = posterior.summary(res, burn=burn)
    assert np.all(s["rhat"] < 1.05)
    d = posterior.dic(res, burn, z, pid, sites=sites)
    assert np.isfinite(d["DIC"]) and abs(d["DIC"] - (d["D"] + 2.0 * d["pD"])) < 1e-9 and d["theta_mean"].shape == (1,)
    pp = posterior.predictive(res, z, pid, burn=burn, draws=16, seed=5)
    assert pp["tips"].shape == (16, 24) and pp["tips"].min() >= 1 and pp["tips"].max() <= 9
