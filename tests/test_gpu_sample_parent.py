"""The exact samplers of histories and the wide ancestral pass against the commit before they shared their branch draw, tile
driver and wide device state (DESIGN.md sections 19a, 19b and 23a: phm_sample_branch.h, phm_sample_host.{h,cpp},
phm_ancestral_wide_host.{h,cpp}): phm_sample_histories_models_wide at 9, 17, 33 and 64 states, phm_ancestral_models_wide at 33 and
phm_sample_histories_models with maps at 2, 4 and 8.  That change moved code only, every sum and product in its place, so every
output must be the recorded one byte for byte, NaN and -inf included (tests/golden/sample_paths/parent.npz, recorded from a build
of that commit by tests/golden/sample_paths/make_golden.py; the cases are tests/samplepathcases.py)."""
import os

import numpy as np
import pytest

import samplepathcases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_paths", "parent.npz")


def test_the_golden_file_holds_exactly_these_cases():
    with np.load(GOLDEN) as g:
        assert {k.split(".")[0] for k in g.files} == set(C.CASES)
    assert os.path.getsize(GOLDEN) < (1 << 20)


@pytest.mark.parametrize("name", list(C.CASES))
def test_equals_the_recorded_parent_run(name):
    out = C.raw(name)
    if "map_off" in out:
        # a branch with two or more changes of state: the wide kernel staged B in LDS and both kernels drew a state from it
        assert np.isfinite(out["loglik"]).any() and C.most_changes_on_a_branch(out) >= 2
    got = C.pin(name, out)
    with np.load(GOLDEN) as g:
        want = {k: g[k] for k in g.files if k.split(".")[0] == name}
    assert sorted(got) == sorted(want)
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k


def test_the_case_without_maps_has_the_statistics_of_the_case_with_them():
    """wide_n9_cross_nomaps returns no rows to count changes in: it is on the pinned path because its statistics are those of
    wide_n9_cross_chunk0, whose maps show a branch with two or more changes"""
    with np.load(GOLDEN) as g:
        for k in ("stats", "loglik", "nodes"):
            assert g[f"wide_n9_cross_nomaps.{k}"].tobytes() == g[f"wide_n9_cross_chunk0.{k}"].tobytes()
