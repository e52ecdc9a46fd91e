"""Sweep parts of the (tile, branch) mapping with one launch per tree level (phm_engine_run): contiguous groups
of tiles run their sweeps on streams of their own, part 0 on the caller's.  Tiles do not read each other's state and every random
number is addressed, so any number of parts must give the bits of one part: statistics per replica and reduced, the read + written
segment counter, no recovery.  And one part must give what the commit before the parts gave (tests/golden/sweep_parts/parent.npz,
recorded from a build of that commit by tests/golden/sweep_parts/make_golden.py): the segment counter now comes from rows the
branch kernel writes per group of branches, not from a second walk over the segment counts.

Five tiles (320 replicas): parts of unequal size (3 + 2; 2 + 2 + 1) and, at four parts, parts of one tile; 300 replicas: the last
tile is ragged and sits in the last part."""
import functools
import os

import numpy as np
import pytest

import sweeppartscases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_parts", "parent.npz")


@functools.lru_cache(maxsize=None)
def _one_part(name, S, reduce):
    stats, seg, rec, launches = C.sweep(name, S, reduce, sweep_parts=1)
    stats.setflags(write=False); seg.setflags(write=False)
    return stats, seg, rec, tuple(launches)


def _same_as_one_part(name, S, parts, effective, **debug):
    for reduce in (True, False):
        want, want_seg, want_rec, want_launches = _one_part(name, S, reduce)
        got, got_seg, got_rec, got_launches = C.sweep(name, S, reduce, sweep_parts=parts, **debug)
        assert want_rec == 0 and got_rec == 0
        assert want.shape == got.shape
        assert np.array_equal(got, want), (name, S, parts, reduce)
        assert np.array_equal(got_seg, want_seg), (got_seg, want_seg)
        # every part makes the launches of a sweep over its own tiles: the run really went through the parts
        assert tuple(got_launches) == tuple(effective * k for k in want_launches), (got_launches, want_launches)


@pytest.mark.parametrize("parts", [2, 3, 4])
@pytest.mark.parametrize("name,S", [("n4", 320), ("n4", 300), ("n2", 320), ("n2", 300)])
def test_forced_parts_equal_one_part(name, S, parts):
    _same_as_one_part(name, S, parts, parts)


@pytest.mark.parametrize("parts", [2, 4])
def test_forced_parts_equal_one_part_hidden_rates(parts):
    """The KS sweep: tips drawn against their parity mask, n x n counters, the root-state column."""
    _same_as_one_part("ks", 300, parts, parts)


def test_groups_of_two_branches_in_four_parts():
    """C2 tree at 66 tiles: a wave of the branch kernel walks two branches and writes one segment row for both, which the reduction
    sums (n_groups = n_edge / 2 rows per tile); parts of 17, 17, 16 and 16 tiles.  The recorded parent run of this case
    (test_one_part_equals_the_recorded_parent_run[c2-...]) pins the counter itself."""
    want, want_seg, want_rec, want_launches = _one_part("c2", 4224, True)
    got, got_seg, got_rec, got_launches = C.sweep("c2", 4224, True, sweep_parts=4)
    assert want_rec == 0 and got_rec == 0
    assert np.array_equal(got, want) and np.array_equal(got_seg, want_seg)
    assert tuple(got_launches) == tuple(4 * k for k in want_launches)


def test_capacity_recovery_replays_through_the_parts():
    """Slots provisioned far too small on purpose (cap_tail = 0.9 at six times the uniformization rate, as
    tests/test_gpu_parity.py::test_capacity_overflow_is_recovered_like_an_unbounded_list): the overflow flag raised by ANY part
    must reach the one sync, and the rebuilt engine replays through the parts again.  Four tiles in three parts against one part."""
    kw = dict(omega_scale=6.0, cap_tail=0.9)
    want, want_seg, want_rec, _ = C.sweep("n4", 200, False, sweep_parts=1, **kw)
    got, got_seg, got_rec, _ = C.sweep("n4", 200, False, sweep_parts=3, **kw)
    assert want_rec >= 1 and got_rec == want_rec, (want_rec, got_rec)
    assert np.array_equal(got, want)
    assert np.array_equal(got_seg, want_seg)


def test_fewer_tiles_than_parts():
    """Four parts forced on two tiles: two parts of one tile each."""
    _same_as_one_part("n4", 128, 4, 2)
    _same_as_one_part("n4", 64, 4, 1)


def test_cluster_kernels_keep_one_part():
    """The cluster kernels (the automatic choice on a tree this small) take no parts: same launches, same bits as one launch per level."""
    want, want_seg, _, _ = _one_part("n4", 300, True)
    a = C.sweep("n4", 300, True, level_groups=2, sweep_parts=1)
    b = C.sweep("n4", 300, True, level_groups=2, sweep_parts=4)
    assert a[3] == b[3]
    for got in (a, b):
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want_seg) and got[2] == 0


@pytest.mark.parametrize("name,S,lg,reduce", C.GOLDEN_CASES)
def test_one_part_equals_the_recorded_parent_run(name, S, lg, reduce):
    with np.load(GOLDEN) as g:
        k = C.golden_key(name, S, lg, reduce)
        want, want_seg = g[k + "_stats"], g[k + "_seg"]
    if lg == 1:
        got, got_seg, rec, _ = _one_part(name, S, reduce)
    else:
        got, got_seg, rec, _ = C.sweep(name, S, reduce, level_groups=lg, sweep_parts=1)
    assert rec == 0
    assert got.shape == want.shape
    assert np.array_equal(got, want)
    assert np.array_equal(got_seg, want_seg), (got_seg, want_seg)
