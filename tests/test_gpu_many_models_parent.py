"""The many-model entry points against the commit before their shared host core (chunk plan, device state,
model and tip staging, P and the tips / up / root launches in phm_loglik_host.cpp; the ExDown schedule in phm_expect_host.h):
phm_loglik_models, phm_expected_stats_models, phm_ancestral_models, phm_ancestral_models_wide, phm_sample_histories_models,
phm_gibbs_rates and, for the shared ExDown builder, phm_expected_stats.  That change moved host code only, so every output must be
the recorded one byte for byte, NaN and -inf included (tests/golden/many_models/parent.npz, recorded from a build of that commit
by tests/golden/many_models/make_golden.py; the cases are tests/manymodelscases.py)."""
import os

import numpy as np
import pytest

import manymodelscases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "many_models", "parent.npz")


def test_the_golden_file_holds_exactly_these_cases():
    with np.load(GOLDEN) as g:
        assert {k.split(".")[0] for k in g.files} == set(C.CASES)
    assert os.path.getsize(GOLDEN) < (1 << 20)


@pytest.mark.parametrize("name", list(C.CASES))
def test_equals_the_recorded_parent_run(name):
    got = C.run(name)
    with np.load(GOLDEN) as g:
        want = {k: g[k] for k in g.files if k.split(".")[0] == name}
    assert sorted(got) == sorted(want)
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k
