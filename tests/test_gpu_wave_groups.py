"""The persistent kernels of the exact sampler and of the forward simulation under many models at the sizes where one wave item
covers SEVERAL branches, the last item of a tile is cut short and a wave takes a second item (sm_branch_kernel in its tile and
packed forms, simm_level_kernel; DESIGN.md sections 19, 20 and 22).  Every other exact test runs them with one branch per item
and one item per wave; tests/test_wave_groups_cpu.py asserts what each shape below reaches (tests/wavegroups.py).

Each call is held to its Python twin with the tolerances of the tests it extends -- states, counts, map offsets and map states
exactly, dwell sums and dwell times to 1e-12 of the tree length, ``loglik`` bit for bit with ``api.loglik_models`` -- and, bit for
bit in every output, to the same call cut into chunks small enough that every item is one branch and every wave takes one item."""
import numpy as np
import pytest

import samplecases as sc
import samplemodelsref as ref
import test_gpu_gibbs as tg
import wavegroups as wg
from phylomap_amd import _lib, api, synth
from test_gpu_sample_models import check_against_twin, models, pids
from test_gpu_simulate_models import _check, _models, _pids, _same

pytestmark = pytest.mark.gpu


def same_sample(a, b, maps=True):
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    if maps:
        assert np.array_equal(a[3].off, b[3].off) and np.array_equal(a[3].state, b[3].state) and np.array_equal(a[3].dwell, b[3].dwell)


@pytest.mark.parametrize("n,observe,missing,per_model,paired", [
    (3, None, 0.1, True, False),                           # register accumulators over the three branches of an item
    (4, sc.PARITY, 0.1, False, True),                      # hidden rates, one site per model
    (8, None, 0.0, True, False),                           # run-time n: one atomic per segment
])
def test_sample_histories_grouped(n, observe, missing, per_model, paired):
    """550 tiles x 46 edges: items of 3 branches, the sixteenth of one, 608 waves on a second item (10 evaluations x 3 470 draws;
    paired by site_of_model that takes 10 models, crossed 5 models x 2 sites)"""
    K, S = wg.SAMPLE_KS[paired]
    D = wg.SAMPLE_D
    edge, lens = sc.tree(shuffle=True)
    Qs = models(n, K, 300 * n + K, hidden=observe is not None)
    sites = np.stack([sc.tips_for(edge, lens, Qs[0], 80 + s, observe, missing) for s in range(S)])
    som = [(k + 1) % S for k in range(K)] if paired else None
    z = sc.as_z(edge, lens, sites[0])
    pid = pids(n, K, per_model, 2 * n + K)
    seed = 2000 + n
    plain = check_against_twin(z, Qs, pid, sites, D, observe=observe, som=som, seed=seed)
    assert np.all(np.isfinite(plain[1])) and plain[1].size == 10          # every evaluation is drawn: 550 tiles in one flush
    try:
        chunked = api.sample_histories(z, Qs, pid, D, sites=sites, observe=observe, site_of_model=som, nodes=True, maps=True,
                                       seed=seed, expect_chunk=wg.CHUNK_SAMPLE)
    finally:
        _lib.set_debug_options()
    same_sample(plain, chunked)


def test_long_branch_grouped():
    """test_long_branch's tree and models (mu t = 2 280, 22.8, 2.28 on one branch) at D = 160 000 draws: 7 500 tiles, items of 9
    and 1 branches, 15 000 items on 8 192 waves -- the two-pass series with its 2^512 rescaling inside a grouped walk and on a
    second trip.  No maps (model 0 alone would write about 10^9 segments)."""
    D = wg.LONG_D
    edge, lens = synth.random_tree(6, 0.3, 9)
    lens = lens.copy()
    lens[4] = 228.0
    fast = np.array([[-10.0, 10.0], [7.0, -7.0]])
    Qs = np.stack([fast, fast * 0.01, fast * 0.001])
    tips = sc.tips_for(edge, lens, Qs[1], 3)
    z = sc.as_z(edge, lens, tips)
    pid = [.5, .5]
    plain = api.sample_histories(z, Qs, pid, D, nodes=True, seed=77)
    try:
        chunked = api.sample_histories(z, Qs, pid, D, nodes=True, seed=77, expect_chunk=wg.CHUNK_SAMPLE)
    finally:
        _lib.set_debug_options()
    same_sample(plain, chunked, maps=False)
    stats, ll, nodes = plain
    assert stats.shape == (3, 1, D, 4) and np.array_equal(ll, api.loglik_models(z, Qs, pid))
    want = ref.sample_models(edge, lens, Qs, pid, tips[None], 64, seed=77)             # draws 0 .. 63 of every model
    assert np.array_equal(nodes[:, :, :64], want["nodes"])
    assert np.array_equal(stats[:, :, :64, 2:], want["stats"][..., 2:])
    tree_len = float(lens.sum())
    assert np.all(np.abs(stats[:, :, :64, :2] - want["stats"][..., :2]) <= 1e-12 * tree_len)
    assert np.all(np.abs(stats[..., :2].sum(axis=-1) - tree_len) <= 1e-12 * tree_len)
    assert stats[0, 0, :, 2:].sum(axis=-1).mean() > 1000                              # model 0 does walk its long branch


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("n", [3, 5])
def test_simulate_histories_models_grouped(n, shuffle):
    """774 tiles on the complete 32-tip tree: the level of 32 edges in items of 3, 3, ..., 2 edges, the levels above it in items
    of one; the models meet in mid-wave (16 500 histories each).  All histories against api.simulate_histories, 3 x 64 per model
    against the Python twin: the first 64, 64 in the middle and the last 64, which take in the waves shared with a neighbour."""
    K, R = wg.SIM_KR
    edge, lens = wg.complete_tree(shuffle=shuffle)
    z = {"edge": edge, "edge.length": lens, "Nnode": 31}
    Qs, pid = _models(n, K, 40 + n), _pids(n, K, True, 41 + n)
    seed, off = 500 + n, 4321
    rows = [(0, 64), (R // 2 - 32, 64), (R - 64, 64)]
    plain = _check(z, Qs, pid, R, seed, off=off, twin_rows=rows)
    try:
        chunked = api.simulate_histories_models(z, Qs, pid, R, nodes=True, maps=True, seed=seed, replica_offset=off,
                                                expect_chunk=wg.CHUNK_SIM)
    finally:
        _lib.set_debug_options()
    _same(plain, chunked)


@pytest.mark.parametrize("n", [3, 8])
def test_posterior_rates_grouped(n):
    """11 420 chains x 3 sites in the packed form: 537 tiles, items of 3 branches and a last one of one, 400 waves on a second
    item, 36 idle lanes in the last wave of every site.  Every recorded row goes back through sample_histories and loglik_models
    (all chains); the Python update is repeated for the first and the last 64 chains."""
    Cn = wg.GIBBS_CHAINS
    r = tg.run(n, Cn, True, False)
    assert r["sites"].shape[0] == wg.GIBBS_SITES
    tg.check_rows(r, chains=list(range(64)) + list(range(Cn - 64, Cn)))
    try:
        other = tg.run(n, Cn, True, False, expect_chunk=wg.CHUNK_GIBBS)
    finally:
        _lib.set_debug_options()
    for k in tg.KEYS:
        assert np.array_equal(r[k], other[k]), k
