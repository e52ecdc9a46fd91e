"""The MCMC stochastic maps for 5 to 64 states (mcmc_maps_wtiles_kernel, phm_mcmc_maps.hip) at every class of the sweep it replays
(tests/mcmcmapsclasses.py; tests/test_mcmc_maps_classes_cpu.py shows that the cases draw in every block of eight states and reach
all ten wt_branch_kernel instantiations): the maps of the public calls against the merged paths of the CPU oracle -- offsets and
states bit for bit, dwell within 4 L 2^-53 relative (mcmcmapsclasses.dwell_bar) -- against the Python twin bit for bit up to 17
states, against the statistics of the same call for every chain, and against each other under the engine option sets of a case."""
import numpy as np
import pytest

import mcmcmapsclasses as M
import wtilesclasses as W
from phylomap_amd import api
from test_gpu_mcmc_maps import _check_history
from test_gpu_parity import _same

pytestmark = pytest.mark.gpu

FN = {"plain": api.sumstatMCMC, "bigtree": api.sumstatMCMC_bigtree, "sparse": api.SPARSEsumstatMCMC, "ks": api.sumstatMCMCks_sweep}
ALL = M.all_cases()


def _call(case, its, run, maps=True, **opt):
    kw = dict(maps=True, map_iters=its) if maps else dict(mapping="tiles")
    return FN[case.variant](case.z, case.Q, case.pid, case.Omega, case.N, reduce=False, n_replicas=case.S, seed=case.seed, **kw,
                            **{**run, **opt})


def _same_maps(a, b, what):
    assert np.array_equal(a.off, b.off), what
    assert np.array_equal(a.state, b.state), what
    assert np.array_equal(a.dwell, b.dwell), what


def _against_oracle(case, m, its):
    """offsets and states of every row of the compared replicas bit for bit, dwell within the bar; the worst dwell error over the bar"""
    E, J = case.n_edge, len(its)
    bar, worst = M.dwell_bar(case.case), 0.0
    for r in case.replicas:
        maps = M.oracle_maps(case.case, r)
        for j, it in enumerate(its):
            off, dwell, state, _ = maps[it]
            k = (r * J + j) * E
            lo, hi = m.off[k], m.off[k + E]
            assert np.array_equal(m.off[k:k + E + 1] - lo, off), (r, it)
            assert np.array_equal(m.state[lo:hi] - 1, state), (r, it)
            worst = max(worst, float(np.max(np.abs(m.dwell[lo:hi] - dwell) / dwell)))
    return worst / bar


def _against_twin(case, m, its):
    r, J = case.S - 1, len(its)
    rows = M.twin_rows(case.case, r)
    for j, it in enumerate(its):
        _check_history(m, r * J + j, rows, it, case.n_edge)


def _every_chain(case, out, m, its):
    """the maps of all S chains against the statistics of the same call and the tree"""
    n, E, S, J = case.n, case.n_edge, case.S, len(its)
    assert m.n_hist == S * J and m.n_edge == E and out.shape[:2] == (S, case.N)
    row = np.repeat(np.arange(m.off.size - 1), np.diff(m.off))
    same = row[:-1] == row[1:]
    h, a, b = row[:-1][same] // E, m.state[:-1][same].astype(np.int64) - 1, m.state[1:][same].astype(np.int64) - 1
    assert m.state.min() >= 1 and m.state.max() <= n and np.all(np.diff(m.off) >= 1)
    assert np.all(a != b)                                                      # no state repeats within a row
    if case.ks:                                                                # n x n block, self pairs (virtual jumps) aside
        cnt = np.bincount(h * n * n + a * n + b, minlength=S * J * n * n).reshape(S, J, n, n)
        want = out[:, its, n:n + n * n].reshape(S, J, n, n).copy()
        want[:, :, np.arange(n), np.arange(n)] = 0.0
    else:
        col = a * (n - 1) + np.where(b > a, b - 1, b)
        cnt = np.bincount(h * case.ncnt + col, minlength=S * J * case.ncnt).reshape(S, J, case.ncnt)
        want = out[:, its, n:n + case.ncnt]
    assert np.array_equal(cnt.astype(np.float64), want)
    dw = np.zeros((S * J, n))
    np.add.at(dw, (row // E, m.state.astype(np.int64) - 1), m.dwell)
    assert np.max(np.abs(dw.reshape(S, J, n) - out[:, its, :n])) <= 1e-12 * case.length
    rs = np.zeros(S * J * E)
    np.add.at(rs, row, m.dwell)
    np.testing.assert_allclose(rs.reshape(S * J, E), np.broadcast_to(case.z["edge.length"], (S * J, E)), rtol=1e-10)
    edge, T = np.asarray(case.z["edge"]), len(case.z["states"])
    tip_rows = edge[:, 1] <= T
    last, obs = m.node_states()[:, tip_rows, 1], np.asarray(case.z["states"])[edge[tip_rows, 1] - 1][None, :]
    assert np.all((last - obs) % 2 == 0) if case.ks else np.all(last == obs)


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_maps_of_every_class_against_the_oracle_the_twin_and_the_statistics(case):
    """map_iters = [0, 2, N - 1] under every engine option set of the case, then every iteration under the first"""
    its = M.map_iters(case.N)
    first, ratios = None, []
    for run in case.runs:
        out, m = _call(case, its, run)
        if first is None:
            first = m
            assert np.array_equal(out, _call(case, its, run, maps=False))
            for r in case.replicas:                                            # the new cases' statistics have no other test
                want, rc = W.oracle_rows(case.case, r)
                assert rc == 0
                _same(out[r], want, case.n, "tiles", ks=case.ks)
            _every_chain(case, out, m, its)
            ratios.append(_against_oracle(case, m, its))
            if case.twin:
                _against_twin(case, m, its)
        else:
            _same_maps(m, first, run)
    every = list(range(case.N))
    out, m = _call(case, None, case.runs[0])
    _every_chain(case, out, m, every)
    ratios.append(_against_oracle(case, m, every))
    if case.twin:
        _against_twin(case, m, every)
    # the recorded iterations' rows among all: the two calls made the same maps for every chain
    k = ((np.arange(case.S)[:, None, None] * case.N + np.asarray(its)[None, :, None]) * case.n_edge + np.arange(case.n_edge)).ravel()
    lens = np.diff(m.off)[k]
    assert np.array_equal(lens, np.diff(first.off))
    idx = np.repeat(m.off[k] - first.off[:-1], lens) + np.arange(first.off[-1])
    assert np.array_equal(m.state[idx], first.state) and np.array_equal(m.dwell[idx], first.dwell)
    print(f"{case.name}: worst dwell error over the bar {max(ratios):.3g} (L = {M.longest_branch(case.case)})")
    assert max(ratios) <= 1.0


LONG = [c for c in ALL if c.long_branch]


@pytest.mark.parametrize("case", LONG, ids=[c.name for c in LONG])
def test_long_branch_recovery_gives_the_default_maps(case):
    """cap_tail = 0.9 provisions slots too small for the 100-segment branch: the engine recovers and replays"""
    its = M.map_iters(case.N)
    base = _call(case, its, case.runs[0])
    got = _call(case, its, case.runs[0], cap_tail=0.9)
    n = case.n
    assert np.array_equal(got[0][..., n:], base[0][..., n:])
    _same_maps(got[1], base[1], "cap_tail")


def test_devices_and_replica_offset_give_the_one_call_maps_at_33_states():
    case = M.by_name("dense33")
    its, run = M.map_iters(case.N), case.runs[0]
    E, J, S = case.n_edge, 3, case.S
    out, base = _call(case, its, run)
    o2, m2 = _call(case, its, run, devices=[0, 0])
    assert np.array_equal(o2, out)
    _same_maps(m2, base, "devices")
    o3, m3 = FN[case.variant](case.z, case.Q, case.pid, case.Omega, case.N, maps=True, map_iters=its, reduce=False, n_replicas=S - 64,
                              replica_offset=64, seed=case.seed, **run)
    assert np.array_equal(o3, out[64:])
    k = 64 * J * E
    assert np.array_equal(m3.off, base.off[k:] - base.off[k])
    assert np.array_equal(m3.state, base.state[base.off[k]:]) and np.array_equal(m3.dwell, base.dwell[base.off[k]:])
