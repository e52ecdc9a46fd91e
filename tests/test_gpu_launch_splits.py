"""The exact one-shot calls past 65 535 tips, level steps, rows, edges, sites and models: the limit of a grid's y and z dimensions, at
which every launcher of the family cuts its work and hands the next launch an offset (t0, k0, r0, e0, j0).  No other test makes
any of them take its second step.

The balanced tree of 131 072 tips (tests/bigtreecases.py) crosses the splits of the tree at once.  With cap = 65 535:
* tips, 131 072 = cap + cap + 2: three launches of ``launch_ex_tips``, ``launch_ll_tips`` and ``launch_aw_tips`` (t0);
* height level 1 has 65 536 cherries = cap + 1: the second launch of ``launch_ex_up``, ``launch_ll_up``, ``an_up_kernel`` and of
  ``aw_level_steps`` over the up lists has exactly one step (k0);
* the depth levels of 131 072 and 262 144 edges take 3 and 5 launches of ``launch_ex_down``, the ``sc_down_kernel`` loop,
  ``an_trace_kernel`` and ``aw_level_steps`` over the down lists (k0);
* NT = 262 143 posterior rows: five launches of ``launch_ex_post`` (r0), of ``launch_an_post`` and of ``aw_post`` (j0);
* E = 262 142 edges: five launches of ``LlLanes::expm`` at 2 and 4 states, where ``ll_edges_per_launch`` is the cap itself (e0); at
  5 states the Pade workspace allows 5 242 edges a launch and the cap does not bind;
* the branch stage of ``phm_expected_branch_stats_models``: ``br_edges_per_launch`` is the cap at 4 and at 9 states with these few
  evaluations (five launches); the one-model call's ``ne_max`` is the cap at 2 states alone (its 256 MB scratch allows 32 768 edges
  at 4 states and 6 472 at 9), which is why ``expected_sumstat`` is also run at 2 states here.
The 6-tip tree carries 65 537 sites (``Sc_max = min(S, cap)`` in ``ll_plan`` and ``aw_plan``: chunks of 65 535 and 2 sites, the
sites on the grid's z dimension) and 65 537 models (``Kc_max <= AW_GRID_MAX`` in ``aw_plan``: chunks of 65 535 and 2 models at 9
states; at 2 states the models lie across the lanes of the x dimension and only the size is new).
tests/test_level_ref_cpu.py restates these launch counts from the plans' formulas.  NOT reached on this tree: the run caps of
``phm_scores_api.cpp`` and ``phm_scores_wide_api.cpp`` (16 384 runs of 16 edges, far below the cap).

Every result is compared with the level-vectorised numpy reference (tests/levelref.py, held to the per-node twins by
tests/test_level_ref_cpu.py) at the project's bars: log-likelihood 1e-12 max(1, |l|); per-branch rows and totals 1e-12 |want| +
1e-14 x tree length; node posteriors 1e-13; joint log-probability 1e-12 relative; the reference's price of the device's joint
assignment within 1e-10 of the reference's maximum; joint states equal (the reference's decision margins exceed 1e-9, asserted in
tests/test_level_ref_cpu.py and again here).  These trees are also where the base-2 exponents of the scaled vectors get large
(sL about -4e5 at 9 states)."""
import functools
import math

import numpy as np
import pytest

import bigtreecases as big
import branchrowscases as bc
import exactref
import levelref
from phylomap_amd import _lib, api

pytestmark = pytest.mark.gpu
LOG_TINY = math.log(1e-308)


@pytest.fixture(scope="module", autouse=True)
def one_blas_thread():
    """the references multiply small matrices many times: a BLAS thread pool only gets in the way"""
    try:
        import threadpoolctl
    except ImportError:
        yield
        return
    with threadpoolctl.threadpool_limits(limits=1):
        yield


# ---- inputs and references, computed once and never changed ----
@functools.lru_cache(maxsize=None)
def _tree():
    return levelref.Tree(big.balanced()[0]["edge"])


@functools.lru_cache(maxsize=None)
def _problem(n):
    """K = 3 models across the lanes (2 .. 8 states), K = 2 with a state per lane (9 states); S = 2 sites"""
    p = big.problem(n, 3 if n <= 8 else 2)
    for a in (p[0]["edge"], p[0]["edge.length"]) + p[2:5]:
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _ref(n, k, full):
    """levelref.expected of model k: loglik alone, or with branch rows, totals and node posteriors"""
    z, _, Qs, pid, tips, observe = _problem(n)
    r = levelref.expected(_tree(), z["edge.length"], Qs[k], pid[k], tips, observe, per_branch=full, nodes=full)
    for a in r.values():
        a.setflags(write=False)
    return r


def _ref_loglik(n, k):
    return (_ref(n, k, True) if n in (4, 9) else _ref(n, k, False))["loglik"]


@functools.lru_cache(maxsize=None)
def _ref_joint(n, k):
    z, _, Qs, pid, tips, observe = _problem(n)
    x, lp, margin = levelref.joint(_tree(), z["edge.length"], Qs[k], pid[k], tips, observe)
    assert np.all(margin > 1e-9), margin                                      # a condition on the inputs
    return x, lp, margin


def _length(z):
    return float(np.sum(z["edge.length"]))


def _rows_bar(what, got, want, length, longest=None):
    """|error| <= 1e-12 |want| + 1e-14 x tree length, the project's bar.  On a tree of length 1.2e5 that floor is 1.2e-9, which
    a row of one branch (its dwell times sum to t_b <= 3) could miss by six digits and pass; with ``longest`` the rows are
    also held to the same form with the longest branch in place of the tree length: what the project's bar is on a tree of one
    such branch.  The reference's own rows differ from ``exactref``'s by at most 0.03 of that tighter form on the small trees of
    tests/test_level_ref_cpu.py (which asserts it), so it is not spent on the reference"""
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    allow = 1e-12 * np.abs(want) + 1e-14 * length
    worst = float(np.max(err / allow))
    print(f"{what}: error / allowance {worst:.3g}")
    assert np.all(np.isfinite(got)) and worst <= 1.0, (what, worst)
    if longest is not None:
        worst = float(np.max(err / (1e-12 * np.abs(want) + 1e-14 * longest)))
        print(f"{what}: error / allowance with the longest branch as the floor's length {worst:.3g}")
        assert worst <= 1.0, (what, worst)


def _ll_bar(what, got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    worst = float(np.max(np.abs(got - want) / (1e-12 * np.maximum(1.0, np.abs(want)))))
    print(f"{what}: loglik error / allowance {worst:.3g}")
    assert np.all(np.isfinite(got)) and worst <= 1.0, (what, worst)


# ---- 1. loglik_models ----
@pytest.mark.parametrize("n", [2, 4, 5])
def test_loglik_models(n):
    """2 and 4 states: P in registers, ``ne_max`` = 65 535, five expm launches; 5 states: P in the workspace.  Tips in three
    launches, the cherries in two, in cross and in paired mode; the values are those of the other entry points bit for bit"""
    z, _, Qs, pid, tips, observe = _problem(n)
    K = len(Qs)
    want = np.stack([_ref_loglik(n, k) for k in range(K)])
    assert np.all(want < LOG_TINY)
    ll = api.loglik_models(z, Qs, pid, sites=tips, observe=observe)
    _ll_bar(f"loglik_models n={n} cross", ll, want)
    som = np.array([1, 0, 1], dtype=np.int32)
    ks = np.arange(K)
    llp = api.loglik_models(z, Qs, pid, sites=tips, observe=observe, site_of_model=som)
    assert llp.shape == (K,) and np.array_equal(llp, ll[ks, som])
    st, ll_st = api.expected_sumstat_models(z, Qs, pid, sites=tips, observe=observe)
    assert np.array_equal(ll_st, ll) and np.all(np.isfinite(st))
    root = int(_tree().root)
    an = api.ancestral_states_models(z, Qs, pid, sites=tips, observe=observe, nodes=[root, 1])
    assert np.array_equal(an.loglik, ll)
    anp = api.ancestral_states_models(z, Qs, pid, sites=tips, observe=observe, site_of_model=som, nodes=[root, 1])
    assert np.array_equal(anp.loglik, llp)
    assert np.array_equal(anp.node_post, an.node_post[ks, som]) and np.array_equal(anp.joint_states, an.joint_states[ks, som])


# ---- 2. expected_sumstat, the one-model call ----
@pytest.mark.parametrize("n,chunk", [(2, 50000), (4, 30000), (9, 5000)])
def test_expected_sumstat(n, chunk):
    """Totals, all 262 142 branch rows and all 262 143 posterior rows of model 0 (2 states: the per-launch edge cap is the grid's;
    4 states: the lane branch kernel; 9 states: ``ex_branch_wide_kernel<16>``).  The rows on both sides of edge row 65 535 are
    the same bits when the branch stage is cut elsewhere: ``expect_chunk`` = 40 000 moves no boundary at 4 and 9 states (the
    256 MB scratch already cuts at 32 768 and 6 472 edges), so a second value below those cuts is run too"""
    z, info, Qs, pid, tips, observe = _problem(n)
    lens, length = z["edge.length"], _length(z)
    E, NT = lens.size, lens.size + 1
    want = _ref(n, 0, True)
    stats, ll, br, post = api.expected_sumstat(z, Qs[0], pid[0], sites=tips, observe=observe, per_branch=True, nodes=True)
    assert br.shape == (2, E, n * n) and post.shape == (2, NT, n)
    _ll_bar(f"expected_sumstat n={n}", ll, want["loglik"])
    _rows_bar(f"expected_sumstat n={n} branch rows", br, want["branch"], length, longest=big.TABLE_LONG)
    _rows_bar(f"expected_sumstat n={n} totals", stats, want["stats"], length)
    worst = float(np.max(np.abs(post - want["post"])))
    print(f"expected_sumstat n={n}: node posteriors error / allowance {worst / 1e-13:.3g}")
    assert worst <= 1e-13
    assert np.all(br[:, info["zero"]] == 0.0) and np.count_nonzero(np.all(br == 0.0, axis=(0, 2))) == 3
    np.testing.assert_allclose(br[:, :, :n].sum(axis=2), np.broadcast_to(lens, (2, E)), rtol=1e-12, atol=1e-14 * length)
    assert np.all(np.abs(stats[:, :n].sum(axis=1) - length) <= 1e-12 * length)
    rows = [65534, 65535, 65536, 65537]
    try:
        for c in (40000, chunk):
            _, ll_c, br_c = api.expected_sumstat(z, Qs[0], pid[0], sites=tips, observe=observe, per_branch=True, expect_chunk=c)
            assert np.array_equal(br_c[:, rows], br[:, rows]) and np.array_equal(br_c, br) and np.array_equal(ll_c, ll)
    finally:
        _lib.set_debug_options()


# ---- 3. expected_sumstat_models ----
@pytest.mark.parametrize("n", [4, 9])
def test_expected_sumstat_models(n):
    z, _, Qs, pid, tips, observe = _problem(n)
    K, length = len(Qs), _length(z)
    st, ll = api.expected_sumstat_models(z, Qs, pid, sites=tips, observe=observe)
    assert st.shape == (K, 2, n * n) and ll.shape == (K, 2)
    _ll_bar(f"expected_sumstat_models n={n}", ll, np.stack([_ref(n, k, True)["loglik"] for k in range(K)]))
    _rows_bar(f"expected_sumstat_models n={n} totals", st, np.stack([_ref(n, k, True)["stats"] for k in range(K)]), length)
    assert np.array_equal(ll, api.loglik_models(z, Qs, pid, sites=tips, observe=observe))
    for k in range(K):
        st_one, ll_one = api.expected_sumstat(z, Qs[k], pid[k], sites=tips, observe=observe)
        assert np.array_equal(ll[k], ll_one)
        _rows_bar(f"expected_sumstat_models n={n} model {k} against expected_sumstat", st[k], st_one, length)


# ---- 4. expected_branch_stats_models ----
EDGE_SEL = [65536, 0, 65535, 65534, 262141, 65535]


@pytest.mark.parametrize("n", [4, 9])
def test_expected_branch_stats_models(n):
    """Five branch-stage launches of 65 535 selected edges at most; the selection straddles the first cut"""
    z, info, Qs, pid, tips, observe = _problem(n)
    K, length = len(Qs), _length(z)
    E = z["edge.length"].size
    br, ll = api.expected_branch_stats_models(z, Qs, pid, sites=tips, observe=observe)
    assert br.shape == (K, 2, E, n * n) and ll.shape == (K, 2)
    _ll_bar(f"expected_branch_stats_models n={n}", ll, np.stack([_ref(n, k, True)["loglik"] for k in range(K)]))
    for k in range(K):
        _rows_bar(f"expected_branch_stats_models n={n} model {k} rows", br[k], _ref(n, k, True)["branch"], length, longest=big.TABLE_LONG)
    assert np.all(br[:, :, info["zero"]] == 0.0)
    st, ll_tot = api.expected_sumstat_models(z, Qs, pid, sites=tips, observe=observe)
    assert np.array_equal(bc.sum_in_run_order(br), st) and np.array_equal(ll, ll_tot)
    sel, ll_sel = api.expected_branch_stats_models(z, Qs, pid, sites=tips, observe=observe, edges=EDGE_SEL)
    assert sel.shape == (K, 2, len(EDGE_SEL), n * n)
    assert np.array_equal(sel, br[:, :, EDGE_SEL]) and np.array_equal(ll_sel, ll)
    lab = np.random.default_rng(0xB17 + n).uniform(-1.0, 1.0, (n, n))
    got, ll_lab = api.expected_branch_stats_models(z, Qs, pid, sites=tips, observe=observe, labels=lab)
    assert got.shape == (K, 2, E, 1) and np.array_equal(ll_lab, ll)
    assert np.array_equal(got, bc.label_reduce(br, lab))


# ---- 5. ancestral_states_models ----
NODE_SEL = [65536, 65535, 1, 262143, 131073, 65537, 65535, 131072]           # both sides of row 65 535, the root, a repeat


@pytest.mark.parametrize("n", [4, 9])
def test_ancestral_states_models(n):
    """Marginals of all 262 143 nodes (five ``post`` launches; the 131 071 internal rows alone exceed one), the joint reconstruction
    through two launches of the max-product level of the cherries and up to five of a traceback level"""
    z, _, Qs, pid, tips, observe = _problem(n)
    K = len(Qs)
    NT = z["edge.length"].size + 1
    got = api.ancestral_states_models(z, Qs, pid, sites=tips, observe=observe)
    assert got.node_post.shape == (K, 2, NT, n) and got.joint_states.shape == (K, 2, NT)
    assert np.array_equal(got.loglik, api.loglik_models(z, Qs, pid, sites=tips, observe=observe))
    assert np.all(np.isfinite(got.joint_logp)) and np.all(got.joint_logp < LOG_TINY) and np.all(got.joint_logp <= got.loglik)
    obs = np.arange(1, n + 1) if observe is None else np.asarray(observe)
    T = tips.shape[1]
    for k in range(K):
        want = _ref(n, k, True)
        _ll_bar(f"ancestral_states_models n={n} model {k}", got.loglik[k], want["loglik"])
        worst = float(np.max(np.abs(got.node_post[k] - want["post"])))
        x, lp, margin = _ref_joint(n, k)
        worst_lp = float(np.max(np.abs(got.joint_logp[k] - lp) / np.abs(lp)))
        price = levelref.assignment_logp(_tree(), z["edge.length"], Qs[k], pid[k], tips, got.joint_states[k], observe)
        below = float(np.max((lp - price) / np.maximum(1.0, np.abs(lp))))
        differ = int(np.sum(got.joint_states[k] != x))
        print(f"ancestral_states_models n={n} model {k}: node posteriors error / allowance {worst / 1e-13:.3g}, joint_logp error "
              f"{worst_lp:.3g} (allowed 1e-12), the reference's price of the device's assignment below its maximum by {below:.3g} "
              f"(allowed 1e-10), smallest decision margin {margin.min():.3g}, states that differ {differ}")
        assert worst <= 1e-13 and worst_lp <= 1e-12 and below <= 1e-10 and differ == 0
        seen = obs[got.joint_states[k][:, :T] - 1]
        assert np.all((tips == 0) | (seen == tips))
    rows = np.asarray(NODE_SEL) - 1
    for som in (None, np.array([1, 0, 1], dtype=np.int32)[:K]):
        part = api.ancestral_states_models(z, Qs, pid, sites=tips, observe=observe, site_of_model=som, nodes=NODE_SEL)
        whole = got if som is None else [a[np.arange(K), som] for a in got[:4]]
        assert np.array_equal(part.loglik, whole[0]) and np.array_equal(part.joint_logp, whole[3])
        assert np.array_equal(part.node_post, whole[1][..., rows, :]) and np.array_equal(part.joint_states, whole[2][..., rows])


# ---- 6. 65 537 sites on the 6-tip tree ----
def _twin6(z, Q, pid, tips):
    st, ll = exactref.expected(z["edge"], z["edge.length"], Q, pid, tips)
    return st, ll


@pytest.mark.parametrize("n,K", [(2, 2), (9, 1)])
def test_sites_past_the_grid(n, K):
    """S = 65 537 = 65 535 + 2 sites, the last three the first three again: chunks of 65 535 and 2 sites in the many-model calls"""
    z = bc.tree6()
    length = _length(z)
    sets, index = big.many_sites(n)
    tips = sets[index]
    Qs, pid = bc.models(n, K, seed=3)
    want = [_twin6(z, Qs[k], pid[k], sets) for k in range(K)]
    want_st = np.stack([w[0][index] for w in want])
    want_ll = np.stack([w[1][index] for w in want])
    ll = api.loglik_models(z, Qs, pid, sites=tips)
    st, ll_st = api.expected_sumstat_models(z, Qs, pid, sites=tips)
    st_one, ll_one = api.expected_sumstat(z, Qs[0], pid[0], sites=tips)
    assert ll.shape == (K, big.PAST) and st.shape == (K, big.PAST, n * n) and st_one.shape == (big.PAST, n * n)
    _ll_bar(f"n={n} S=65537 loglik_models", ll, want_ll)
    _rows_bar(f"n={n} S=65537 expected_sumstat_models", st, want_st, length)
    _ll_bar(f"n={n} S=65537 expected_sumstat", ll_one, want_ll[0])
    _rows_bar(f"n={n} S=65537 expected_sumstat", st_one, want_st[0], length)
    assert np.array_equal(ll_st, ll)
    for a in (ll, st, ll_one[None], st_one[None]):
        assert np.array_equal(a[:, -3:], a[:, :3])


# ---- 7. 65 537 models on the 6-tip tree ----
@pytest.mark.parametrize("n", [2, 9])
def test_models_past_the_grid(n):
    """K = 65 537 paired models on three sites, the last three the first three again; at 9 states chunks of 65 535 and 2 models
    and one Pade launch per model.  The whole call is the call made in two halves bit for bit"""
    z = bc.tree6()
    length = _length(z)
    K = big.PAST
    Qs, pid = big.many_models(n)
    tips = bc.sites(n, 6, 3)
    som = bc.owner(K, 3)
    som[-3:] = som[:3]
    kw = dict(sites=tips, site_of_model=som)
    ll = api.loglik_models(z, Qs, pid, **kw)
    st, ll_st = api.expected_sumstat_models(z, Qs, pid, **kw)
    assert ll.shape == (K,) and st.shape == (K, n * n) and np.array_equal(ll_st, ll)
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(st))
    assert np.array_equal(ll[-3:], ll[:3]) and np.array_equal(st[-3:], st[:3])
    check = list(range(0, K, K // 16))[:16] + [K - 3, K - 2, K - 1]
    want = [_twin6(z, Qs[k], pid[k], tips[som[k]][None]) for k in check]
    _ll_bar(f"n={n} K=65537 loglik_models", ll[check], np.array([w[1][0] for w in want]))
    _rows_bar(f"n={n} K=65537 expected_sumstat_models", st[check], np.stack([w[0][0] for w in want]), length)
    h = 40000
    halves = [api.loglik_models(z, Qs[a:b], pid[a:b], sites=tips, site_of_model=som[a:b]) for a, b in ((0, h), (h, K))]
    assert np.array_equal(np.concatenate(halves), ll)
    halves = [api.expected_sumstat_models(z, Qs[a:b], pid[a:b], sites=tips, site_of_model=som[a:b]) for a, b in ((0, h), (h, K))]
    assert np.array_equal(np.concatenate([x[0] for x in halves]), st) and np.array_equal(np.concatenate([x[1] for x in halves]), ll)
