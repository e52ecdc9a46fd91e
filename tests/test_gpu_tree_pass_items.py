"""The tree passes of the (tile, branch) mapping with one launch per tree level (phm_tiles.hip): wave-uniform items in the pruning,
root, node-draw and reduction kernels, and ONE node-draw item per (tile, internal node) that draws both children -- a tip edge with
given states only stores its end states (makePLrcpp* src/phylomap.cpp:503-529, sampleinternalnodes* :618-657, updatenodestates
:460-475).  The cluster kernels (few tiles) keep the per-edge text: the two forms and the automatic choice must agree bit for bit,
and with the oracle.

Per-replica tip states (tips_per_replica) CAN be requested with this mapping through _lib.Engine(states=..., tips_per_replica=True):
one case below."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from phylomap_amd import _lib, api, synth
from test_gpu_one_chain import _ladder, _orders, _same, _tree_from_edges

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "phm_tiles.h")) as _f:      # workgroups of a node-draw launch, four waves each
    TILES_PERSISTENT_WGS = int(re.search(r"constexpr int TILES_PERSISTENT_WGS = (\d+);", _f.read()).group(1))
_ORACLE_VARIANT = {_lib.PHM_MCMC_BIGTREE: O.BIGTREE, _lib.PHM_MCMC_KS: O.KS}


def _node_level_sizes(z):
    """Internal nodes per depth level (root: level 0) from the edge table: the differences of the level offsets of the node draws.
    (The engine does not hand its own offsets to Python; tests/native/node_order_check.cpp checks those against the same definition.)"""
    edge = np.asarray(z["edge"])
    T = edge.shape[0] // 2 + 1
    parent = {int(c): int(p) for p, c in edge}
    depth = {T + 1: 0}

    def d(v):
        path = []
        while v not in depth:
            path.append(v); v = parent[v]
        base = depth[v]
        for k, w in enumerate(reversed(path)):
            depth[w] = base + k + 1
        return depth[path[0]] if path else base

    return np.bincount([d(v) for v in range(T + 1, 2 * T)])


def _three(z, Q, pid, Omega, N, S, variant=_lib.PHM_MCMC_BIGTREE, seed=19, **kw):
    """level_groups 1 (a launch per level: the kernels under test), 2 (cluster kernels), 0 (automatic): statistics, the last replica's
    state, launches; all three bit for bit the same, replicas {0, 63, 64, last} equal to the oracle."""
    n = Q.shape[0]
    out = {}
    for lg in (1, 2, 0):
        eng = _lib.Engine(z, Q, pid, Omega, N, variant=variant, seed=seed, n_replicas=S, mapping="tiles", level_groups=lg, **kw)
        eng.run(N); eng.sync()
        out[lg] = (eng.stats(0, N), eng.dump(S - 1), eng.info().last_run_launches)
        eng.close()
    for lg in (2, 0):
        np.testing.assert_array_equal(out[lg][0], out[1][0])
        for k in ("seg_count", "node_states", "PL"):
            np.testing.assert_array_equal(out[lg][1][k], out[1][1][k])
    nen, nodelist, root = _orders(z)
    sites = kw.get("states")
    for r in sorted({0, 63, 64, S - 1}):
        if r >= S:
            continue
        zr = z if sites is None else dict(z, states=sites[r])
        want, rc = O.maketreelistMCMC(zr, Q, pid, np.eye(n) + Q / Omega, Omega, nen, nodelist, root, N, variant=_ORACLE_VARIANT[variant],
                                      seed=seed, replica=r)
        assert rc == 0
        _same(out[1][0][r], want, n, ks=variant == _lib.PHM_MCMC_KS)
    return out


def _n3_problem():
    Q = synth.dense_Q(3, 0.02, 0.3, seed=3)
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    pid = np.full(3, 1.0 / 3)
    return synth.make_tree(37, Q, Omega, 41, pid), Q, pid, Omega


@pytest.mark.parametrize("case,S", [("two_tips", 5), ("two_tips", 70), ("three_tips", 5), ("three_tips", 70), ("c1", 5), ("c1", 70),
                                    ("n3", 70), ("n3", 130)])
def test_per_level_kernels_equal_clusters_and_oracle(case, S):
    """2 tips: one node, no internal child; 3 tips; the 100-tip C1 tree (n = 2); 37 tips at n = 3.  S = 5 and 70: the last tile is
    ragged and the items of a level are no multiple of the four waves of a workgroup."""
    if case == "n3":
        z, Q, pid, Omega = _n3_problem()
    else:
        z, Q, pid, Omega = synth.config_problem({"two_tips": 2, "three_tips": 2, "c1": 1}[case], n_tips={"two_tips": 2, "three_tips": 3, "c1": None}[case])
    out = _three(z, Q, pid, Omega, 4, S)
    sizes = _node_level_sizes(z)
    assert int(sizes.sum()) == len(z["states"]) - 1
    # per sweep: a launch per height level, the root draw, a launch per depth level (as many as height levels), the branch kernel and
    # two reductions -- the node items keep the launch count of the edge items
    assert out[1][2] == 4 * (2 * len(sizes) + 4), (out[1][2], len(sizes))


def test_ladder_one_node_per_level_one_tip_and_one_internal_child():
    """300-tip caterpillar: 299 levels of ONE node each, every node with one tip and one internal child (the last one: two tips)."""
    Q = synth.config_Q(2)
    n = Q.shape[0]
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    pid = np.full(n, 1.0 / n)
    edge, lens = _ladder(300, 0.5, 3)
    z = _tree_from_edges(edge, lens, Q, pid, 11)
    assert list(_node_level_sizes(z)) == [1] * 299
    _three(z, Q, pid, Omega, 3, 70, seed=8)


def test_ladder_hidden_rates_sweep_draws_the_tips():
    """The hidden-rates sweep on the ladder: tips are drawn against their parity mask, so a tip side of a node item reads its segment
    count and draws like an internal child (without a node-state store)."""
    Q = synth.make2sQ(.1, .1, .2, .2, 10)
    n = Q.shape[0]
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    pid = np.full(n, 1.0 / n)
    edge, lens = _ladder(300, 0.5, 3)
    z = _tree_from_edges(edge, lens, Q, pid, 11)
    out = _three(z, Q, pid, Omega, 3, 70, variant=_lib.PHM_MCMC_KS, seed=8)
    got = api.sumstatMCMCks_sweep(z, Q, pid, Omega, 3, seed=8, n_replicas=70, mapping="tiles", level_groups=1)      # the driver's own entry point
    np.testing.assert_array_equal(got, out[1][0])


def test_random_tree_hidden_rates_sweep_every_pair_of_child_kinds():
    """Hidden rates on a random 45-tip tree: nodes with two internal children, with one on either side, and with two drawn tips."""
    Q = synth.make2sQ(.1, .1, .2, .2, 10)
    n = Q.shape[0]
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    pid = np.full(n, 1.0 / n)
    z = synth.make_tree(45, Q, Omega, 77, pid)
    edge = np.asarray(z["edge"])
    kinds = {tuple(int(c) > 45 for c in edge[edge[:, 0] == v, 1]) for v in range(46, 90)}
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}, kinds
    _three(z, Q, pid, Omega, 3, 70, variant=_lib.PHM_MCMC_KS, seed=8)


def test_per_replica_tip_states():
    """tips_per_replica: a tip side reads its state from the tile's [tip][64] rows instead of the shared vector."""
    z, Q, pid, Omega = synth.config_problem(2, n_tips=60)
    S = 70
    sites = np.random.default_rng(5).integers(1, Q.shape[0] + 1, size=(S, 60)).astype(np.int32)
    _three(z, Q, pid, Omega, 3, S, tips_per_replica=True, states=sites)


def test_c2_many_tiles_persistent_waves_take_several_items():
    """The C2 tree (1 000 tips) at 66 tiles: the automatic choice is one launch per level there, and the widest level holds more
    (tile, node) items than the 8 192 persistent waves of a node-draw launch, so a wave of the persistent loop draws more than one
    item."""
    z, Q, pid, Omega = synth.config_problem(2)
    S = 4224
    tiles = (S + 63) // 64
    widest = int(_node_level_sizes(z).max())
    while widest * tiles <= TILES_PERSISTENT_WGS * 4:      # (does not happen on this tree: kept so that the case keeps its point)
        S += 64 * 8; tiles = (S + 63) // 64
    assert widest * tiles > TILES_PERSISTENT_WGS * 4, (widest, tiles)
    out = _three(z, Q, pid, Omega, 3, S)
    assert out[0][2] == out[1][2] > 3 * 20, (out[0][2], out[1][2])      # automatic = per level: dozens of launches per sweep, not a handful of tiers


def test_seg_read_counts_segments_before_and_after_every_sweep():
    """phm_info.seg_read after k sweeps = sum over the sweeps of (segments held before + segments held after), valid replicas only
    (S = 70: the second tile holds six).  The reduction kernel that counts them takes wave-uniform items now."""
    z, Q, pid, Omega = synth.config_problem(1)
    S, N = 70, 3
    E = np.asarray(z["edge"]).shape[0]
    eng = _lib.Engine(z, Q, pid, Omega, N, variant=_lib.PHM_MCMC_BIGTREE, seed=4, n_replicas=S, mapping="tiles", level_groups=1)
    held = S * sum(len(m) for m in z["maps"])
    want = 0
    for k in range(N):
        eng.run(1); eng.sync()
        after = sum(int(eng.dump(r)["seg_count"][:E].sum()) for r in range(S))
        want += held + after
        held = after
        assert eng.info().seg_read == want, (k, eng.info().seg_read, want)
    eng.close()
