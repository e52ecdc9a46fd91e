"""Ancestral states under many rate matrices at 9..64 states on the device (phm_ancestral_models_wide):
the first state count of every lane class, its unpadded last and the codon model's 61; cross and paired mode, shuffled edge tables
with a zero-length branch, observe maps, shared and per-model root priors.  loglik against loglik_models and the node posteriors
against expected_sumstat(nodes=True) BIT FOR BIT; posteriors and the joint reconstruction against the Python twin
(tests/ancref.py) by value (independent of ties) and exactly (after asserting the twin's decision margin); node selection, parts,
chunks and devices bit for bit; an impossible model, P = I, and a tree deep enough that the unscaled products underflow."""
import math

import numpy as np
import pytest

import ancref
import exactref
from phylomap_amd import api, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def one_blas_thread():
    """the twin multiplies n x n matrices thousands of times: a BLAS thread pool only gets in its way"""
    try:
        import threadpoolctl
    except ImportError:
        yield
        return
    with threadpoolctl.threadpool_limits(limits=1):
        yield


def _tree(T, seed, shuffled, mean=0.5):
    """pre-ordered edge table, or shuffled with one zero-length branch"""
    edge, lens = synth.random_tree(T, mean, seed)
    if shuffled:
        rs = np.random.default_rng(seed)
        perm = rs.permutation(edge.shape[0])
        edge, lens = edge[perm], lens[perm].copy()
        lens[int(rs.integers(edge.shape[0]))] = 0.0
    return {"edge": edge, "edge.length": lens, "Nnode": T - 1, "states": np.ones(T, dtype=np.int32)}


def _random_Qs(K, n, rs, lo=0.05, hi=1.0):
    """random non-symmetric rate matrices, the rates scaled by 4 / n so that a state's total rate does not grow with n and the
    branches stay informative"""
    Qs = rs.uniform(lo, hi, (K, n, n)) * 4.0 / n
    for Q in Qs:
        np.fill_diagonal(Q, 0.0)
        np.fill_diagonal(Q, -Q.sum(axis=1))
    return Qs


def _tips(z, Q, pid, S, seed, observe=None, missing=0.1):
    tips, _ = api.simulate_histories(z, Q, pid, S, observe=observe, seed=seed)
    rs = np.random.default_rng(seed)
    tips[rs.random(tips.shape) < missing] = 0
    return tips


def _twin(z, Qs, pid, tips, observe, som, models):
    """per model of `models`: node posteriors [.., NT, n], joint states [.., NT], joint logp, loglik, P and the smallest decision
    margin; cross: [k][S, ...], paired: [k][1, ...] on the model's own site"""
    pid = np.atleast_2d(pid)
    out = {"post": {}, "x": {}, "logp": {}, "ll": {}, "P": {}, "margin": math.inf}
    for k in models:
        y = tips if som is None else tips[int(som[k])][None]
        pk = pid[k if pid.shape[0] > 1 else 0]
        P = np.stack([exactref.expm(Qs[k] * float(t)) for t in z["edge.length"]])
        out["P"][k] = P
        out["post"][k], out["ll"][k] = ancref.marginal(z["edge"], z["edge.length"], Qs[k], pk, y, observe, P=P)
        out["x"][k], out["logp"][k], m = ancref.joint(z["edge"], z["edge.length"], Qs[k], pk, y, observe, P=P)
        out["margin"] = min(out["margin"], m)
    return out


def _rel(err, scale):
    return err / np.maximum(1.0, np.abs(scale))


def _check_values(what, z, Qs, pid, tips, observe, som, got, tw, exact):
    """the value checks of the joint reconstruction (independent of ties) and, with `exact`, equality of the states"""
    pid2 = np.atleast_2d(pid)
    n = Qs.shape[1]
    T = tips.shape[1]
    obs = np.arange(1, n + 1) if observe is None else np.asarray(observe)
    worst_price, worst_logp, differ = 0.0, 0.0, 0
    for k in tw["x"]:
        y = tips if som is None else tips[int(som[k])][None]
        pk = pid2[k if pid2.shape[0] > 1 else 0]
        dev_x = got.joint_states[k] if som is None else got.joint_states[k][None]
        dev_lp = np.atleast_1d(got.joint_logp[k])
        dev_ll = np.atleast_1d(got.loglik[k])
        price = ancref.assignment_logp(z["edge"], z["edge.length"], Qs[k], pk, y, dev_x, observe, P=tw["P"][k])
        worst_price = max(worst_price, float(np.max(_rel(tw["logp"][k] - price, tw["logp"][k]))))
        worst_logp = max(worst_logp, float(np.max(_rel(np.abs(dev_lp - tw["logp"][k]), tw["logp"][k]))))
        seen = obs[dev_x[:, :T] - 1]                                            # what each reconstructed tip state is observed as
        assert np.all((y == 0) | (seen == y)), (what, k)
        assert np.all(dev_lp <= dev_ll), (what, k)
        differ += int(np.sum(dev_x != tw["x"][k]))
    print(f"{what}: twin's price of the device's assignment below the twin's maximum by {worst_price:.3g} (allowed 1e-10), "
          f"joint_logp error {worst_logp:.3g} (allowed 1e-12), smallest decision margin {tw['margin']:.3g}, "
          f"states that differ from the twin's {differ}")
    assert worst_price <= 1e-10
    assert worst_logp <= 1e-12
    if exact:
        assert differ == 0


def _check_post(what, z, Qs, pid, tips, observe, som, got, tw, nodes=None):
    """three models: the one-model route of section 13 bit for bit, the twin within 1e-13, rows summing to 1 within 1e-12"""
    pid2 = np.atleast_2d(pid)
    rows = slice(None) if nodes is None else np.asarray(nodes) - 1
    worst, worst_sum, differ = 0.0, 0.0, 0
    for k in sorted(tw["post"])[:3]:
        y = tips if som is None else tips[int(som[k])][None]
        pk = pid2[k if pid2.shape[0] > 1 else 0]
        dev = got.node_post[k] if som is None else got.node_post[k][None]
        one = api.expected_sumstat(z, Qs[k], pk, sites=y, observe=observe, nodes=True)[2][:, rows]
        differ += int(np.sum(dev != one))
        worst = max(worst, float(np.max(np.abs(dev - tw["post"][k][:, rows]))))
        worst_sum = max(worst_sum, float(np.max(np.abs(dev.sum(axis=-1) - 1.0))))
    print(f"{what}: node posteriors: values that differ from expected_sumstat(nodes=True) {differ}, error / allowance: twin "
          f"{worst / 1e-13:.3g}, row sums {worst_sum / 1e-12:.3g}")
    assert differ == 0
    assert worst <= 1e-13
    assert worst_sum <= 1e-12


# (K, S, paired, shuffled + zero-length branch, parity observe, per-model pid); 15 evaluations do not fill a wave at 16 or 32 lanes
SHAPES = [(1, 1, False, False, False, False), (3, 5, False, True, True, True), (5, 3, True, False, False, False)]
MANY = (130, 1, True, True, False, False)                  # more models than any chunk of 64 or 128
CASES = [(n, s) for n in (9, 16, 17, 32, 33, 61, 64) for s in SHAPES] + [(n, MANY) for n in (9, 17, 33)]


@pytest.mark.parametrize("n,shape", CASES, ids=lambda v: f"K{v[0]}-S{v[1]}-{'paired' if v[2] else 'cross'}" if isinstance(v, tuple)
                         else f"n{v}")
def test_lane_classes_against_the_twin(n, shape):
    K, S, paired, shuffled, observed, per_model_pid = shape
    seed = 0xB31 + 100 * n + K + S
    rs = np.random.default_rng(seed)
    z = _tree(24, seed, shuffled)
    Qs = _random_Qs(K, n, rs)
    pid = rs.uniform(0.2, 1.0, (K, n)) if per_model_pid else np.arange(1.0, n + 1.0)
    observe = (np.arange(n) % 2 + 1) if observed else None
    tips = _tips(z, Qs[0], np.ones(n), S, seed, observe=observe)
    som = rs.integers(0, S, K) if paired else None
    got = api.ancestral_states_models(z, Qs, pid, sites=tips, observe=observe, site_of_model=som)
    what = f"n={n} K={K} S={S} {'paired' if paired else 'cross'}"
    want_shape = (K,) if paired else (K, S)
    assert got.loglik.shape == want_shape and got.node_post.shape == want_shape + (47, n)
    assert got.joint_states.shape == want_shape + (47,) and got.joint_logp.shape == want_shape
    assert np.array_equal(got.nodes, np.arange(1, 48))
    assert np.all(np.isfinite(got.loglik))
    assert np.array_equal(got.loglik, api.loglik_models(z, Qs, pid, sites=tips, observe=observe, site_of_model=som))
    assert np.all((got.joint_states >= 1) & (got.joint_states <= n))
    tw = _twin(z, Qs, pid, tips, observe, som, range(K) if K <= 5 else (0, 64, 129))
    _check_post(what, z, Qs, pid, tips, observe, som, got, tw)
    assert tw["margin"] > 1e-9, (what, tw["margin"])                           # a condition on the inputs: no decision near a tie
    _check_values(what, z, Qs, pid, tips, observe, som, got, tw, exact=True)


@pytest.mark.parametrize("n", [9, 33])
def test_more_sites_than_a_workgroup_walks(n):
    """70 sites per model: a workgroup's groups walk four sites each through the staged matrices (64 sites a workgroup at 16 lanes,
    16 at 64), so the site axis crosses both the walk and the tile, and the last tile is partly empty"""
    K, S = 2, 70
    seed = 0xB31 + 100 * n + K + S
    rs = np.random.default_rng(seed)
    z = _tree(24, seed, True)
    Qs = _random_Qs(K, n, rs)
    pid = rs.uniform(0.2, 1.0, (K, n))
    tips = _tips(z, Qs[0], np.ones(n), S, seed)
    got = api.ancestral_states_models(z, Qs, pid, sites=tips)
    assert np.all(np.isfinite(got.loglik))
    assert np.array_equal(got.loglik, api.loglik_models(z, Qs, pid, sites=tips))
    tw = _twin(z, Qs, pid, tips, None, None, range(K))
    what = f"n={n} K={K} S={S} cross"
    _check_post(what, z, Qs, pid, tips, None, None, got, tw)
    assert tw["margin"] > 1e-9, (what, tw["margin"])
    _check_values(what, z, Qs, pid, tips, None, None, got, tw, exact=True)
    paired = api.ancestral_states_models(z, Qs[[1] * S], pid[[1] * S], sites=tips, site_of_model=np.arange(S))
    for a, b in zip(paired[:4], got[:4]):                                     # model 1 on every site, one model per site
        assert np.array_equal(a, b[1])


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("n", [9, 33])
def test_selection_parts_chunks_and_devices_change_no_bit(n):
    rs = np.random.default_rng(40 + n)
    z = _tree(24, 41 + n, True)
    K, S = 5, 3
    Qs = _random_Qs(K, n, rs)
    pid = rs.uniform(0.2, 1.0, (K, n))
    observe = np.arange(n) % 2 + 1
    tips = _tips(z, Qs[0], np.ones(n), S, 42 + n, observe=observe)
    for som in (None, rs.integers(0, S, K)):
        kw = dict(sites=tips, observe=observe, site_of_model=som)
        whole = api.ancestral_states_models(z, Qs, pid, **kw)
        assert np.all(np.isfinite(whole.loglik))
        root = 25                                                              # random_tree numbers the root T + 1
        nodes = [root, 7, 31, 31]
        rows = np.asarray(nodes) - 1
        part = api.ancestral_states_models(z, Qs, pid, nodes=nodes, **kw)
        assert np.array_equal(part.nodes, nodes)
        assert np.array_equal(part.loglik, whole.loglik) and np.array_equal(part.joint_logp, whole.joint_logp)
        assert np.array_equal(part.node_post, whole.node_post[..., rows, :])
        assert np.array_equal(part.joint_states, whole.joint_states[..., rows])
        m = api.ancestral_states_models(z, Qs, pid, joint=False, **kw)
        assert m.joint_states is None and m.joint_logp is None
        assert np.array_equal(m.loglik, whole.loglik) and np.array_equal(m.node_post, whole.node_post)
        j = api.ancestral_states_models(z, Qs, pid, marginal=False, **kw)
        assert j.node_post is None
        assert np.array_equal(j.loglik, whole.loglik) and np.array_equal(j.joint_states, whole.joint_states)
        assert np.array_equal(j.joint_logp, whole.joint_logp)
        for opt in ({"expect_chunk": 2}, {"devices": [0, 0]}):
            assert _same(api.ancestral_states_models(z, Qs, pid, **kw, **opt), whole), opt


def test_an_impossible_model_among_five():
    """a block-diagonal Q (states 1..4 and 5..9 never meet) with tips in both blocks"""
    rs = np.random.default_rng(9)
    z = _tree(24, 9, False)
    n, K = 9, 5
    Qs = _random_Qs(K, n, rs)
    pid = rs.uniform(0.2, 1.0, n)
    tips = _tips(z, Qs[0], pid, 2, 10)
    tips[:, :2] = [1, 9]                                                       # both blocks are seen in both sites
    plain = api.ancestral_states_models(z, Qs, pid, sites=tips)
    split = Qs.copy()
    split[2, :4, 4:] = 0.0
    split[2, 4:, :4] = 0.0
    np.fill_diagonal(split[2], 0.0)
    np.fill_diagonal(split[2], -split[2].sum(axis=1))
    got = api.ancestral_states_models(z, split, pid, sites=tips)
    assert np.all(got.loglik[2] == -np.inf) and np.all(got.joint_logp[2] == -np.inf)
    assert np.all(np.isnan(got.node_post[2])) and np.all(got.joint_states[2] == 0)
    assert np.array_equal(got.loglik, api.loglik_models(z, split, pid, sites=tips))
    keep = np.arange(K) != 2
    assert np.all(np.isfinite(got.loglik[keep]))
    for a, b in zip(got[:4], plain[:4]):
        assert np.array_equal(a[keep], b[keep])


def test_a_model_that_leaves_no_state():
    """Q = 0 (P = I) with every tip in state 2: every node in state 2, one-hot posteriors, the joint maximum is pid(2).  pid(2) is
    a power of two, so the posterior's own sum is one and its reciprocal is exact."""
    rs = np.random.default_rng(11)
    z = _tree(24, 11, False)
    n = 9
    pid = np.full(n, 3.0 / 32.0)
    pid[1] = 0.25
    still = np.concatenate([np.zeros((1, n, n)), _random_Qs(1, n, rs)])
    same = np.full((1, 24), 2)
    got = api.ancestral_states_models(z, still, pid, sites=same)
    assert np.all(got.joint_states[0] == 2)
    assert np.array_equal(got.node_post[0, 0], np.tile(np.eye(n)[1], (47, 1)))
    # log pid(2) up to the rounding of log and of the exponent's product with ln 2: a few ulp of values of order 1
    assert abs(got.joint_logp[0, 0] - math.log(0.25)) <= 1e-12
    assert abs(got.loglik[0, 0] - math.log(0.25)) <= 1e-12


def test_rescaling_on_a_deep_tree():
    """2 000 tips: the unscaled max-products underflow (the joint maximum is far below 1e-308)"""
    n, K = 9, 3
    rs = np.random.default_rng(2000)
    z = _tree(2000, 2000, False, mean=0.3)
    Qs = _random_Qs(K, n, rs, 0.1, 0.6)
    pid = np.arange(1.0, n + 1.0)
    tips = _tips(z, Qs[0], pid, 1, 2001)
    nodes = [2001, 5, 2002, 2500, 3000, 3500, 3998, 3999]
    got = api.ancestral_states_models(z, Qs, pid, sites=tips)
    assert np.all(got.joint_logp < math.log(1e-308)) and np.all(np.isfinite(got.joint_logp))
    assert np.array_equal(got.loglik, api.loglik_models(z, Qs, pid, sites=tips))
    tw = _twin(z, Qs, pid, tips, None, None, range(K))
    assert tw["margin"] > 1e-9, tw["margin"]
    _check_values("2000 tips", z, Qs, pid, tips, None, None, got, tw, exact=True)
    sel = api.ancestral_states_models(z, Qs, pid, sites=tips, nodes=nodes)
    rows = np.asarray(nodes) - 1
    assert np.array_equal(sel.node_post, got.node_post[:, :, rows])
    assert np.array_equal(sel.joint_states, got.joint_states[:, :, rows]) and np.array_equal(sel.joint_logp, got.joint_logp)
    _check_post("2000 tips, 8 selected nodes", z, Qs, pid, tips, None, None, sel, tw, nodes=nodes)
