"""The Python binding layer against the parent's records (tests/golden/api_calls/parent.json, tests/apicallcases.py): every
argument that reaches the C ABI -- scalars, option bytes, tree counts, and dtype, size and bytes of every array -- and shape,
strides, dtype and place of every returned array, compared for equality.  No GPU needed: the recorder's proxy answers the
calls."""
import ctypes
import gc
import json
import os
import weakref

import numpy as np

import pytest

import apicallcases as A
from phylomap_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_calls", "parent.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_and_the_cases_name_the_same_calls(golden):
    assert sorted(golden["cases"]) == sorted(A.CASES) and sorted(golden["refusals"]) == sorted(A.REFUSALS)
    symbols = {c[0] for rec in golden["cases"].values() for c in rec["calls"]}
    assert "phm_ancestral_models_wide" in {c[0] for c in golden["cases"]["ancestral_wide"]["calls"]}
    left_out = {"phm_version", "phm_struct_size", "phm_device_count", "phm_last_error", "phm_status_string", "phm_tree_orders",
                "phm_last_kernel_ms", "phm_sparse_kernel_source", "phm_qupdate_apply", "phm_engine_set_model", "phm_engine_run",
                "phm_engine_sync", "phm_engine_info", "phm_engine_destroy", "phm_engine_reduced_stats_device",
                "phm_engine_time_pruning", "phm_engine_phase_ms"}        # not asked for: host-only, or Python that did not change
    assert symbols == set(_lib.EXPORTS) - left_out


@pytest.mark.parametrize("name", sorted(A.CASES))
def test_call_reaches_the_c_abi_as_the_parent_made_it(golden, name):
    saved = (_lib._p, _lib.load())
    got = json.loads(json.dumps(A.run(name)))
    assert (_lib._p, _lib._lib) == saved                                  # the recorder put both back
    want = golden["cases"][name]
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]
    for k, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert len(g[1]) == len(w[1]), (g[0], k)
        for i, (ga, wa) in enumerate(zip(g[1], w[1])):
            assert ga == wa, f"call {k} {g[0]}, argument {i}"
    assert got["result"] == want["result"]


@pytest.mark.parametrize("name", sorted(A.REFUSALS))
def test_refusal_has_the_parents_type_and_message(golden, name):
    assert A.refusal(name) == golden["refusals"][name]


def test_argtypes_are_element_for_element_the_parents(golden):
    got = json.loads(json.dumps(A.argtypes()))
    assert sorted(got) == sorted(golden["argtypes"])
    for name, want in golden["argtypes"].items():
        assert got[name] == want, name


def test_a_pointer_keeps_its_array_and_a_tree_object_its_arrays():
    """what api.py's argument tuples rely on: _lib._p's pointer holds the array; the tree structs do not, their objects do"""
    a = np.arange(4.0)
    w = weakref.ref(a)
    ptr = _lib._p(a, ctypes.c_double)
    del a
    gc.collect()
    assert w() is not None and ptr[3] == 3.0
    del ptr
    gc.collect()
    assert w() is None
    pt = _lib.PlainTree(A.Z6, A.SITES6)
    assert pt.edge is not None and pt.states.base is None and (pt.T, pt.E, pt.NT) == (6, 10, 11)
