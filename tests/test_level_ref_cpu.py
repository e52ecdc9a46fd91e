"""The level-vectorised reference (tests/levelref.py) and the big inputs (tests/bigtreecases.py) of tests/test_gpu_launch_splits.py,
without a device: the reference against the per-node twins (``exactref.expected``, ``ancref.marginal``, ``ancref.joint``,
``ancref.assignment_logp``) on a 64-tip balanced tree of the same builder and on the shuffled 40-tip random tree, at 2, 4 and 9
states, with an ``observe`` map, missing tips and zero-length branches; the builder's properties at 2^17 tips; and the reference
alone on the inputs the GPU tests use, where the conditions those tests rely on are asserted for the committed seeds: every
log-likelihood finite and below log(1e-308), the dwell times summing to the tree length, every decision margin above 1e-9."""
import functools
import math

import numpy as np
import pytest

import ancref
import bigtreecases as big
import branchrowscases as bc
import exactref
import levelref


def _close(what, got, want, length):
    """1e-13 relative with a floor of 1e-14 x tree length"""
    err = np.abs(got - want)
    allow = 1e-13 * np.abs(want) + 1e-14 * length
    print(f"{what}: error / allowance {np.max(err / allow):.3g}")
    assert got.shape == want.shape and np.all(err <= allow), (what, float(np.max(err / allow)))


def _small(tree):
    return big.balanced(6)[0] if tree == "balanced64" else bc.tree40()


# ---- 1. against the per-node twins ----
@pytest.mark.parametrize("n", [2, 4, 9])
@pytest.mark.parametrize("tree", ["balanced64", "random40"])
def test_against_the_per_node_twins(tree, n):
    z = _small(tree)
    edge, lens = z["edge"], z["edge.length"]
    assert np.sum(lens == 0.0) == (3 if tree == "balanced64" else 1)
    T = int(z["Nnode"]) + 1
    observe = bc.parity(n) if n == 4 else None
    Qs, pid = bc.models(n, 2)
    tips = bc.sites(n, T, 3, observe)
    assert np.any(tips == 0)
    length = float(np.sum(lens))
    what = f"{tree} n={n}"
    for k in range(2):
        got = levelref.expected(edge, lens, Qs[k], pid[k], tips, observe)
        st, ll, br, post = exactref.expected(edge, lens, Qs[k], pid[k], tips, observe, per_branch=True, nodes=True)
        _close(f"{what} model {k} per-branch rows", got["branch"], br, length)
        # the GPU tests' tighter row bar, 1e-12 |want| + 1e-14 x the longest branch of the big tree: the two references use a
        # tenth of it at the most (measured: 0.03), so nine tenths are left for the device
        tight = float(np.max(np.abs(got["branch"] - br) / (1e-12 * np.abs(br) + 1e-14 * big.TABLE_LONG)))
        print(f"{what} model {k} per-branch rows: error over the GPU tests' tighter allowance {tight:.3g}")
        assert tight <= 0.1
        _close(f"{what} model {k} totals", got["stats"], st, length)
        _close(f"{what} model {k} loglik", got["loglik"], ll, length)
        _close(f"{what} model {k} node posteriors", got["post"], post, length)
        assert np.all(got["branch"][:, lens == 0.0] == 0.0)
        post_a, ll_a = ancref.marginal(edge, lens, Qs[k], pid[k], tips, observe)
        _close(f"{what} model {k} ancref.marginal", got["post"], post_a, length)
        _close(f"{what} model {k} ancref loglik", got["loglik"], ll_a, length)
        only = levelref.expected(edge, lens, Qs[k], pid[k], tips, observe, per_branch=False, nodes=False)
        assert np.array_equal(only["loglik"], got["loglik"]) and set(only) == {"loglik"}
        x, lp, margin = levelref.joint(edge, lens, Qs[k], pid[k], tips, observe)
        x_a, lp_a, margin_a = ancref.joint(edge, lens, Qs[k], pid[k], tips, observe)
        assert margin.shape == (3,) and float(margin.min()) == margin_a
        assert margin.min() > 1e-9 and margin_a > 1e-9, (what, margin, margin_a)   # a condition on the inputs
        assert np.array_equal(x, x_a) and np.array_equal(lp, lp_a)
        rs = np.random.default_rng(n + k)
        other = x.copy()
        free = np.setdiff1d(np.arange(T + 1, 2 * T), np.asarray(edge)[lens == 0.0].reshape(-1)) - 1
        other[:, free] = rs.integers(1, n + 1, (3, free.size))                 # any states away from the zero-length branches
        assert np.any(other != x)
        for a in (x, other):
            price = levelref.assignment_logp(edge, lens, Qs[k], pid[k], tips, a, observe)
            _close(f"{what} model {k} price", price, ancref.assignment_logp(edge, lens, Qs[k], pid[k], tips, a, observe), length)
            assert np.all(price <= lp + 1e-12 * np.abs(lp))                    # nothing beats the maximum
        np.testing.assert_allclose(levelref.assignment_logp(edge, lens, Qs[k], pid[k], tips, x, observe), lp, rtol=1e-12)
        other[1, 7] = 0
        assert levelref.assignment_logp(edge, lens, Qs[k], pid[k], tips, other, observe)[1] == -math.inf


def test_an_impossible_site_is_minus_infinity():
    """two tips in different states on a cherry of two zero-length edges"""
    z = bc.tree6()
    lens = z["edge.length"].copy()
    lens[[8, 9]] = 0.0                                                        # the edges into tips 5 and 6
    Qs, pid = bc.models(3, 1)
    tips = np.array([[1, 2, 3, 1, 2, 2], [1, 2, 3, 1, 2, 3]])
    with np.errstate(invalid="ignore", divide="ignore"):
        r = levelref.expected(z["edge"], lens, Qs[0], pid[0], tips, per_branch=False)
        x, lp, _ = levelref.joint(z["edge"], lens, Qs[0], pid[0], tips)
    assert np.isfinite(r["loglik"][0]) and r["loglik"][1] == -math.inf
    assert np.all(x[1] == 0) and lp[1] == -math.inf and np.all(x[0] > 0)


# ---- 2. the builder at 2^17 tips ----
def test_the_balanced_tree_of_131072_tips():
    z, info = big.balanced()
    edge, lens = z["edge"].astype(np.int64), z["edge.length"]
    T, E = 131072, 262142
    assert edge.shape == (E, 2) and lens.shape == (E,) and z["Nnode"] == T - 1 == 131071
    tr = levelref.Tree(edge)
    assert tr.root == T + 1 and info["root"] == T + 1
    assert [u.size for u in tr.up] == [1 << d for d in range(16, -1, -1)]     # 65 536 cherries: one past the cap
    assert [r.size for r in tr.down] == [2 << d for d in range(17)]
    assert tr.up[0].size == big.GRID_MAX + 1
    assert np.array_equal(np.sort(edge[:, 1]), np.delete(np.arange(1, 2 * T), T))   # every node but the root is a child once
    assert np.array_equal(np.bincount(edge[:, 0], minlength=2 * T)[T + 1:], np.full(T - 1, 2))
    assert not np.array_equal(edge[:, 1], np.sort(edge[:, 1])) and np.any(np.diff(edge[:, 0]) < 0)   # shuffled
    assert np.array_equal(np.sort(tr.edge[tr.down[-1], 1]), np.arange(1, T + 1))   # every tip at depth 17
    zero = np.flatnonzero(lens == 0.0)
    assert sorted(info["zero"]) == zero.tolist() and zero.size == 3
    tip_b, cherry_b, mid_b = info["zero"]
    assert edge[tip_b, 1] <= T and tr.height[edge[cherry_b, 1]] == 1 and tr.height[edge[mid_b, 1]] == 17 - 8
    assert np.unique(edge[zero].reshape(-1)).size == 6                        # no two of them on one node
    assert info["table"].size == 16 and np.unique(info["table"]).size == 16 and np.all(info["table"] > 0)
    assert info["table"].max() == 3.0 and np.all((np.sort(info["table"])[:15] >= 0.02) & (np.sort(info["table"])[:15] <= 0.6))
    assert np.all(np.isin(lens[lens > 0.0], info["table"])) and np.unique(lens).size == 17
    again, _ = big.balanced()
    assert np.array_equal(again["edge"], z["edge"]) and np.array_equal(again["edge.length"], lens)
    # the launches the GPU tests count on
    cap = big.GRID_MAX
    assert [min(cap, T - t0) for t0 in range(0, T, cap)] == [cap, cap, 2]      # tips
    assert -(-tr.up[0].size // cap) == 2 and tr.up[0].size - cap == 1          # the cherries: a second launch of one step
    assert -(-tr.down[-1].size // cap) == 3 and -(-tr.down[-2].size // cap) == 2
    assert -(-(E + 1) // cap) == 5 and -(-E // cap) == 5 and -(-(T - 1) // cap) == 3


def test_the_many_sites_and_many_models_inputs():
    for n in (2, 9):
        sets, index = big.many_sites(n)
        assert index.size == 65537 == big.GRID_MAX + 2 and np.array_equal(index[-3:], index[:3])
        assert sets.shape[1] == 6 and sets.min() == 0 and sets.max() == n
        assert np.unique(index).size > min(sets.shape[0], 3 ** 6) // 2
        Qs, pid = big.many_models(n)
        assert Qs.shape == (65537, n, n) and pid.shape == (65537, n)
        assert np.array_equal(Qs[-3:], Qs[:3]) and np.array_equal(pid[-3:], pid[:3])
        assert np.all(np.abs(Qs.sum(axis=2)) < 1e-12) and np.all(np.diagonal(Qs, axis1=1, axis2=2) < 0)


def test_the_plans_cut_where_the_gpu_tests_say():
    """The host plans' formulas restated on the sizes of tests/test_gpu_launch_splits.py: which caps are the grid's 65 535 there.
    ``ll_plan`` is ``test_many_models_host_cpu.plan`` (held to the header by that file's stand-alone program); the others are one
    line each: phm_expect_api.cpp's ``ne_max``, ``br_edges_per_launch`` and ``aw_plan``'s ``min``s"""
    from test_many_models_host_cpu import plan
    cap, scratch = big.GRID_MAX, 256 << 20
    T, E, NT = 131072, 262142, 262143
    for free_b in (64 << 30, 256 << 30):
        for n, launches in ((2, 5), (4, 5)):                                  # P in registers: the cap itself, five expm launches
            Kc, Sc, ne = plan(free_b, n, 0, 2, 3, 0, 0, 0, 0, T=T, E=E, NT=NT)
            assert (Kc, Sc, ne) == (64, 2, cap) and -(-E // ne) == launches
        Kc, Sc, ne = plan(free_b, 5, 0, 2, 3, 0, 0, 0, 0, T=T, E=E, NT=NT)      # the Pade workspace cuts sooner
        assert (Kc, Sc, ne) == (64, 2, 5242)
        Kc, Sc, ne = plan(free_b, 2, 0, 65537, 2, 0, 0, 0, 0)                   # the 6-tip tree: chunks of 65 535 and 2 sites
        assert (Kc, Sc) == (64, cap) and [min(Sc, 65537 - s0) for s0 in range(0, 65537, Sc)] == [cap, 2]
        Kc, Sc, ne = plan(free_b, 2, 1, 3, 65537, 0, 0, 0, 0)                   # 65 537 paired models: the lanes of the x dimension
        assert Kc % 64 == 0 and Kc >= 65600 and Sc == 1

    def ex_ne_max(n, Spm=64):                                                 # phm_expect_api.cpp, S = 2 sites padded to 64
        return max(1, min(E, cap, scratch // (8 * n * n * Spm)))

    assert [ex_ne_max(n) for n in (2, 4, 9)] == [cap, 32768, 6472]
    # edge rows 65 534 .. 65 537: cut apart by the default plan at 2 and 4 states, and by none of the expect_chunk values run there
    assert [65534 // ex_ne_max(n) != 65537 // ex_ne_max(n) for n in (2, 4, 9)] == [True, True, False]
    assert all(65534 // c == 65537 // c for c in (40000, 50000, 30000, 5000))
    assert min(ex_ne_max(4), 40000) == ex_ne_max(4) and min(ex_ne_max(9), 40000) == ex_ne_max(9)   # 40 000 moves nothing there

    def br_ne(n, evals):                                                      # br_edges_per_launch: K = 3 or 2 models x 2 sites
        return max(1, min(E, cap, scratch // (8 * n * n * evals)))

    assert br_ne(4, 6) == cap and br_ne(9, 4) == cap and -(-E // cap) == 5
    n_runs = -(-E // 16)
    assert n_runs == 16384 < cap                                              # the run caps of the scores drivers are NOT reached
    # aw_plan on the 6-tip tree at 9 states (16 lanes), its own footprint; the drivers' additions are of the same order
    n, NP, E6, T6, NT6 = 9, 16, 10, 6, 11
    per_model = 8 * (E6 * n * n + n * n + n) + 4 * E6 + 4 + T6                # paired: the model's tips
    per_eval = (8 * NP + 4) * NT6 + 8
    budget = (64 << 30) // 2 - 8 * 5 * n * n * E6
    assert min(budget // (per_model + per_eval), 65537, cap) == cap           # Kc_max: chunks of 65 535 and 2 models
    assert min(65537, cap) == cap and budget // (per_model + per_eval * cap) >= 1   # Sc_max: chunks of 65 535 and 2 sites


# ---- 3. the reference alone on the big inputs ----
@functools.lru_cache(maxsize=None)
def _tree():
    return levelref.Tree(big.balanced()[0]["edge"])


@pytest.mark.parametrize("n", [2, 5])
def test_the_reference_logliks_on_the_inputs_of_the_gpu_tests(n):
    z, _, Qs, pid, tips, observe = big.problem(n, 3)
    for k in range(3):
        ll = levelref.expected(_tree(), z["edge.length"], Qs[k], pid[k], tips, observe, per_branch=False, nodes=False)["loglik"]
        print(f"n={n} model {k}: loglik {ll}")
        assert np.all(np.isfinite(ll)) and np.all(ll < math.log(1e-308)), ll


@pytest.mark.parametrize("n,K,k", [(2, 3, 0), (4, 3, 0), (4, 3, 1), (4, 3, 2), (9, 2, 0), (9, 2, 1)])
def test_the_reference_on_the_inputs_of_the_gpu_tests(n, K, k):
    """what tests/test_gpu_launch_splits.py relies on, for the committed seeds: every model whose branch rows, posteriors or
    joint reconstruction (4 and 9 states) it compares"""
    z, info, Qs, pid, tips, observe = big.problem(n, K)
    lens = z["edge.length"]
    length = float(np.sum(lens))
    r = levelref.expected(_tree(), lens, Qs[k], pid[k], tips, observe)
    assert np.all(np.isfinite(r["loglik"])) and np.all(r["loglik"] < math.log(1e-308)), r["loglik"]
    dwell = r["stats"][:, :n].sum(axis=1)
    print(f"n={n} model {k}: loglik {r['loglik']}, dwell sum / tree length - 1: {dwell / length - 1.0}")
    assert np.all(np.abs(dwell - length) <= 1e-12 * length)
    assert np.all(np.isfinite(r["branch"])) and np.all(r["branch"][:, info["zero"]] == 0.0)
    assert np.all(np.abs(r["post"].sum(axis=2) - 1.0) <= 1e-12)
    if n == 2:
        return
    x, lp, margin = levelref.joint(_tree(), lens, Qs[k], pid[k], tips, observe)
    print(f"n={n} model {k}: joint logp {lp}, smallest decision margin per site {margin}")
    assert np.all(margin > 1e-9), margin
    assert np.all(np.isfinite(lp)) and np.all(lp < math.log(1e-308)) and np.all(lp <= r["loglik"])
    assert np.all(x >= 1) and np.all(x <= n)
