"""The producers of character histories against the commit before their shared device pieces (the map-row sink of phm_maps.h, the
statistics lanes of phm_history.h, the branch walk of phm_sim_walk.h) and the shared host front end of the two simulators
(phm_sim_host.h): phm_simulate_histories / _maps, phm_simulate_histories_models, phm_sample_histories_models, phm_gibbs_rates,
phm_maketreelistEXP / _maps and phm_maketreelistMCMC_maps.  That change moved code only, so every output must be the recorded one
byte for byte, dtype and shape included (tests/golden/history_producers/parent.npz, recorded from a build of that commit by
tests/golden/history_producers/make_golden.py; the cases are tests/historycases.py)."""
import os

import numpy as np
import pytest

import historycases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "history_producers", "parent.npz")


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
