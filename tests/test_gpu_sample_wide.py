"""The exact sampler of histories over many rate matrices and sites at 9..64 states on the device
(phm_sample_histories_models_wide) against its Python twin (tests/samplemodelsref.py), through
``api.sample_histories``: the first and the last unpadded state count of every lane class of the tree passes and the codon model's
61; node states, counts and map offsets and states exactly, dwell times to 1e-12 of the tree length (section 19's bar), the
log-likelihood bit for bit with ``api.loglik_models``; chunks, devices, replica offsets and the optional outputs; an impossible
model, a model that leaves no state, a branch at mu t = 400; and the device's own statistics against the exact expectations.

Why exact: section 19's argument.  The device's P (Pade) and the twin's (scipy) differ in the last bits, so a draw flips only if a
uniform falls within about 1e-12 relative of a threshold.  Should one occur, that case's seed changes and section 24 records it; no
tolerance is added.  Seeds are ``1000 + n K + D`` throughout unless a case states its own."""
import numpy as np
import pytest

import exactref
import samplecases as sc
from phylomap_amd import _lib, api
from test_gpu_sample_models import check_against_twin
from test_sample_models_cpu import z_columns, z_nodes

pytestmark = pytest.mark.gpu

STATES = [9, 16, 17, 32, 33, 61, 64]


@pytest.fixture(scope="module", autouse=True)
def one_blas_thread():
    try:
        import threadpoolctl
    except ImportError:
        yield
        return
    with threadpoolctl.threadpool_limits(limits=1):
        yield


def random_Qs(K, n, seed, lo=0.05, hi=1.0):
    """section 23's rates: uniform in (lo, hi) * 4 / n, so that a state's total rate does not grow with n"""
    Qs = np.random.default_rng(seed).uniform(lo, hi, (K, n, n)) * 4.0 / n
    for Q in Qs:
        np.fill_diagonal(Q, 0.0)
        np.fill_diagonal(Q, -Q.sum(axis=1))
    return Qs


def parity(n):
    return tuple(1 + (i % 2) for i in range(n))


def simulated_tips(z, Q, pid, S, seed, observe=None, missing=0.1):
    tips, _ = api.simulate_histories(z, Q, pid, S, observe=observe, seed=seed)
    tips[np.random.default_rng(seed).random(tips.shape) < missing] = 0
    return tips


def per_model_pid(K, n, seed):
    p = np.random.default_rng(seed).uniform(0.2, 1.0, (K, n))
    return p / p.sum(axis=1, keepdims=True)


def maps_readd_to_statistics(stats, ll, m, n, E, tree_length):
    """every finite history: its dwell columns sum to the tree length, its maps' dwell per state are its dwell columns (both
    within 1e-12 of the tree length) and its maps' changes of state are its count columns exactly"""
    cols = n + n * (n - 1)
    st = stats.reshape(-1, cols)
    D = st.shape[0] // ll.size
    fin = np.repeat(np.isfinite(ll).reshape(-1), D)
    tol = 1e-12 * tree_length
    assert np.all(np.abs(st[fin, :n].sum(axis=1) - tree_length) <= tol)
    row = np.repeat(np.arange(m.off.size - 1), np.diff(m.off))
    hist, s0 = row // E, m.state.astype(np.int64) - 1
    acc = np.zeros((st.shape[0], cols))
    np.add.at(acc, (hist, s0), m.dwell)
    same = row[1:] == row[:-1]
    frm, to = s0[:-1][same], s0[1:][same]
    assert np.all(frm != to)
    np.add.at(acc, (hist[:-1][same], n + frm * (n - 1) + np.where(to > frm, to - 1, to)), 1.0)
    assert np.array_equal(acc[fin, n:], st[fin, n:])
    assert np.all(np.abs(acc[fin, :n] - st[fin, :n]) <= tol)
    assert np.all(acc[~fin] == 0.0)


def check(z, Qs, pid, sites, D, observe=None, som=None, seed=1, **opt):
    n, E = Qs.shape[1], z["edge"].shape[0]
    stats, ll, nodes, m = check_against_twin(z, Qs, pid, sites, D, observe=observe, som=som, seed=seed, **opt)
    maps_readd_to_statistics(stats, ll, m, n, E, float(z["edge.length"].sum()))
    return stats, ll, nodes, m


@pytest.mark.parametrize("n", STATES)
def test_one_full_tile(n):
    edge, lens = sc.tree()
    K, D = 1, 64
    Qs = random_Qs(K, n, 100 * n + K)
    pid = np.full(n, 1.0 / n)
    z = sc.as_z(edge, lens, np.ones(24, dtype=np.int32))
    sites = simulated_tips(z, Qs[0], pid, 1, 50 + n)
    check(z, Qs, pid, sites, D, seed=1000 + n * K + D)


@pytest.mark.parametrize("n", STATES)
def test_cross_shuffled_observe_and_a_short_second_tile(n):
    edge, lens = sc.tree(shuffle=True)
    assert lens.min() == 0.0
    K, S, D = 3, 2, 70                                                # the second tile of an evaluation has 6 valid lanes
    Qs = random_Qs(K, n, 100 * n + K)
    obs = parity(n)
    z = sc.as_z(edge, lens, np.ones(24, dtype=np.int32))
    sites = simulated_tips(z, Qs[0], np.full(n, 1.0 / n), S, 50 + n, observe=obs)
    check(z, Qs, per_model_pid(K, n, n + K), sites, D, observe=obs, seed=1000 + n * K + D)


@pytest.mark.parametrize("n", STATES)
def test_paired_three_draws(n):
    edge, lens = sc.tree()
    K, S, D = 5, 2, 3                                                 # every evaluation: one tile of 3 valid lanes
    Qs = random_Qs(K, n, 100 * n + K)
    pid = np.full(n, 1.0 / n)
    z = sc.as_z(edge, lens, np.ones(24, dtype=np.int32))
    sites = simulated_tips(z, Qs[0], pid, S, 50 + n)
    check(z, Qs, pid, sites, D, som=[(k + 1) % S for k in range(K)], seed=1000 + n * K + D)


def same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and
            np.array_equal(a[3].off, b[3].off) and np.array_equal(a[3].dwell, b[3].dwell) and np.array_equal(a[3].state, b[3].state))


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("n", [9, 33])
def test_chunks_devices_offsets_and_parts_change_no_bit(n, paired):
    edge, lens = sc.tree(shuffle=True)
    K, S, D, r = 3, 2, 70, 5
    Qs = random_Qs(K, n, 7 * n)
    z = sc.as_z(edge, lens, np.ones(24, dtype=np.int32))
    sites = simulated_tips(z, Qs[0], np.full(n, 1.0 / n), S, 60 + n)
    pid = per_model_pid(K, n, 3)
    som = [1, 0, 1] if paired else None

    def run(draws=D, nodes=True, maps=True, **opt):
        return api.sample_histories(z, Qs, pid, draws, sites=sites, site_of_model=som, nodes=nodes, maps=maps, seed=11, **opt)

    plain = run()
    try:
        assert same(run(expect_chunk=1), plain)
        assert same(run(devices=[0, 0]), plain)
    finally:
        _lib.set_debug_options()
    # replica_offset = r: draw d is draw d + r of the run with offset 0
    shifted = run(draws=D - r, replica_offset=r)
    E = edge.shape[0]
    assert np.array_equal(shifted[0], plain[0][..., r:, :]) and np.array_equal(shifted[1], plain[1])
    assert np.array_equal(shifted[2], plain[2][..., r:, :])
    keep = np.zeros(plain[0].shape[:-1], dtype=bool)
    keep[..., r:] = True
    rows = np.repeat(keep.reshape(-1), E)
    seg = np.repeat(rows, np.diff(plain[3].off))
    assert np.array_equal(np.diff(shifted[3].off), np.diff(plain[3].off)[rows])
    assert np.array_equal(shifted[3].dwell, plain[3].dwell[seg]) and np.array_equal(shifted[3].state, plain[3].state[seg])
    # the optional outputs leave the rest bit for bit
    bare = run(nodes=False, maps=False)
    assert len(bare) == 2 and np.array_equal(bare[0], plain[0]) and np.array_equal(bare[1], plain[1])
    only_nodes = run(maps=False)
    assert np.array_equal(only_nodes[0], plain[0]) and np.array_equal(only_nodes[2], plain[2])
    only_maps = run(nodes=False)
    assert np.array_equal(only_maps[0], plain[0]) and np.array_equal(only_maps[2].dwell, plain[3].dwell)
    assert np.array_equal(only_maps[2].off, plain[3].off) and np.array_equal(only_maps[2].state, plain[3].state)


def test_an_impossible_model_among_three():
    n, D = 9, 70
    edge, lens = sc.tree()
    Qs = random_Qs(3, n, 41)
    Qs[1, :4, 4:] = 0.0                                               # block-diagonal: states 1..4 and 5..9 never meet
    Qs[1, 4:, :4] = 0.0
    np.fill_diagonal(Qs[1], 0.0)
    np.fill_diagonal(Qs[1], -Qs[1].sum(axis=1))
    pid = np.full(n, 1.0 / n)
    z = sc.as_z(edge, lens, np.ones(24, dtype=np.int32))
    sites = simulated_tips(z, Qs[0], pid, 1, 8, missing=0.0)
    assert sites.min() <= 4 and sites.max() >= 5                      # tips in both blocks
    stats, ll, nodes, m = check(z, Qs, pid, sites, D, seed=31)
    assert ll[1, 0] == -np.inf and np.isfinite(ll[0, 0]) and np.isfinite(ll[2, 0])
    assert np.all(np.isnan(stats[1])) and np.all(nodes[1] == 0)
    cnt = m.counts().reshape(3, D, edge.shape[0])
    assert np.all(cnt[1] == 0) and np.all(cnt[[0, 2]] >= 1)


def test_a_model_that_leaves_no_state():
    n, D = 9, 64
    edge, lens = sc.tree()
    Qs = np.zeros((1, n, n))
    pid = np.full(n, 1.0 / n)
    z = sc.as_z(edge, lens, np.full(24, 4, dtype=np.int32))
    stats, ll, nodes, m = check(z, Qs, pid, z["states"][None], D, seed=32)
    E = edge.shape[0]
    assert np.all(m.counts() == 1) and np.all(m.state == 4) and np.all(nodes == 4)
    assert np.array_equal(m.dwell.reshape(D, E), np.tile(lens, (D, 1)))
    assert np.all(stats[0, 0, :, n:] == 0) and np.all(np.delete(stats[0, 0, :, :n], 3, axis=1) == 0)
    assert np.allclose(stats[0, 0, :, 3], lens.sum(), rtol=1e-14)


def test_a_branch_at_mu_t_400():
    n, D = 9, 64
    edge, lens = sc.tree()
    Qs = random_Qs(1, n, 43)
    mu = float(np.max(-np.diag(Qs[0])))
    b_long = 7
    lens = lens.copy()
    lens[b_long] = 400.0 / mu
    assert lens.max() == lens[b_long] and abs(mu * lens[b_long] - 400.0) < 1e-10
    pid = np.full(n, 1.0 / n)
    z = sc.as_z(edge, lens, np.ones(24, dtype=np.int32))
    sites = simulated_tips(z, Qs[0], pid, 1, 9)
    stats, ll, nodes, m = check(z, Qs, pid, sites, D, seed=77)
    seg = m.counts().reshape(D, edge.shape[0])[:, b_long]
    print(f"mu t = 400: segments on the long branch {seg.min()} .. {seg.max()}, mean {seg.mean():.1f}")
    # a row has at most N + 1 segments, N about Poisson(400); every state leaves at a rate of at least min(-q_ii), so at least that
    # share of the 400 events are changes of state (the mean over 64 rows has a standard deviation of about 2.5)
    assert 0.9 * 400.0 * float(np.min(-np.diag(Qs[0]))) / mu < seg.mean() < 1.1 * 400.0 and seg.max() > 256


def test_statistics_on_the_device():
    n, D = 17, 4096
    edge, lens = sc.tree()
    Q = sc.random_Q(n, 1) * 4.0 / n
    pid = np.full(n, 1.0 / n)
    tips = sc.tips_for(edge, lens, Q, 5, None, 0.1)
    z = sc.as_z(edge, lens, tips)
    stats, ll, nodes = api.sample_histories(z, Q[None], pid, D, nodes=True, seed=7 + n)
    want, ll_want, post = exactref.expected(edge, lens, Q, pid, tips[None], nodes=True)
    assert abs(ll[0, 0] - ll_want[0]) < 1e-11 * abs(ll_want[0])      # Pade against scipy: check_against_twin's bar
    zc = z_columns(stats[0, 0], want[0])
    zn = z_nodes(nodes[0, 0], post[0])
    print(f"n={n}: max |z| columns {zc.max():.2f}, nodes {zn.max():.2f}")
    assert zc.max() < 5.0 and zn.max() < 5.0
