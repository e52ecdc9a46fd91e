"""The one-model-per-lane kernels (2 to 8 states) against the commit before their shared device pieces (DESIGN.md section 17c:
state-count dispatch, lane prologue, rescale, mu_k and the cell of B_k, grids in phm_ll_device.h; the gibbs drivers' shared host
pieces in phm_gibbs_host.h): phm_loglik_models, phm_expected_stats_models, phm_ancestral_models, phm_sample_histories_models and
phm_gibbs_rates at every state count that tests/test_gpu_many_models_parent.py does not reach.  That change moved code only, so
every output must be the recorded one byte for byte, NaN and -inf included (tests/golden/lane_kernels/parent.npz, recorded from a
build of that commit by tests/golden/lane_kernels/make_golden.py; the cases are tests/lanekernelcases.py)."""
import os

import numpy as np
import pytest

import lanekernelcases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lane_kernels", "parent.npz")


def test_the_golden_file_holds_exactly_these_cases():
    with np.load(GOLDEN) as g:
        assert {k.split(".")[0] for k in g.files} == set(C.CASES)
    assert os.path.getsize(GOLDEN) < (1 << 20)


def test_the_cases_cover_what_the_kernels_branch_on():
    assert C.TREE_N == (2, 4, 6, 7, 8) and C.GIBBS_N == (2, 4, 5, 8)
    for n in C.TREE_N:
        Qs, _ = C.models(n, C.K)
        assert C.K > 64 and C.K % 64 and not Qs[7].any()
        tips = C.sites(n, C.S)
        assert (tips == 0).any() and tips[-1, 3] == n and n not in C.observe(n)


@pytest.mark.parametrize("name", list(C.CASES))
def test_equals_the_recorded_parent_run(name):
    got = C.run(name)
    with np.load(GOLDEN) as g:
        want = {k: g[k] for k in g.files if k.split(".")[0] == name}
    assert sorted(got) == sorted(want)
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k
