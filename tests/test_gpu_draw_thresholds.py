"""The packed form of the (tile, branch) kernel draws segment states from integer thresholds (phm_draw_tab.h, tiles_branch_kernel<NS, KS,
false> of phm_tiles.hip): chain rows 1 .. TILES_TTAB from LDS (no step draws from row 0), rows up to
DRAW_TAB_ROWS - 1 from the table in global memory, anything else by the arithmetic draw.  Cases built like those of tests/tilesclasses.py -- 12 tips, two tiles with 6 live
lanes in the second, 3 sweeps, groups 1 and 3 -- whose branches carry caller-supplied paths of 17, 18, 48 and 2 segments in turn: the
first draw of a branch of m segments reads chain row m - 2, so sweep 1 starts on

    row TILES_TTAB     = 15   the last row in LDS,
    row TILES_TTAB + 1 = 16   the first row from the global table,
    row 46                    the deepest row a caller's path can put first in the packed form,

and walks down through every row below.  NOT reachable by construction, and why: rows DRAW_TAB_ROWS - 1 = 63 and DRAW_TAB_ROWS = 64
(the last tabulated and the first arithmetic row) need 65 and 66 segments on a branch, and from 49 caller-supplied (or expected)
segments on the engine picks the LONG form, which keeps the arithmetic draw; in the packed form only a lane that outgrows 64 segments
by chance reads them (the general path, same draw function): on the GPU the global-table rows 47 to 63 and the arithmetic draw inside
draw_state_far are covered only by test_gpu_parity.py::test_tiles_mapping_general_loop_when_a_lane_outgrows_64_segments_unexpectedly,
which holds its counts to the oracle bit for bit.  The histories are compared with the maps replay for the plain sweeps only (the
replay's twin is set up for them as in tests/test_gpu_tiles_classes.py); bigtree, bf and ks are held to the oracle.  An entry with a zero total (the fallback bit) is one the sampler never
requests: the node states at both ends of a branch are drawn from the pruning pass given its m segments, so the end state is
reachable from every state the walk can be in; tests/test_draw_thresholds_cpu.py covers that bit.  The 4-state matrix has four
structural zeros (thresholds no word and every word satisfies).

Asserted: counts bit for bit, dwell sums to test_gpu_parity._same's bar against the CPU oracle, no recovery; the sampled histories of
the plain sweeps equal to the maps replay's twin (which draws arithmetically) through test_gpu_mcmc_maps._check_history; the table the
device built, read back through the engine's test aid, byte for byte the one the host compiler makes of the same header."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rateupdatecases as RC
import tilesclasses as T
from phylomap_amd import _lib, api, synth
from test_gpu_mcmc_maps import _check_history, _twin
from test_gpu_tiles_classes import _API, _against_oracle, _run, _same_across_groups

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phylomap_amd", "csrc")


def _constant(header, name):
    m = re.search(rf"constexpr int {name} = (\d+);", open(os.path.join(CSRC, header)).read())
    assert m, name
    return int(m.group(1))


TTAB, ROWS = _constant("phm_tiles.h", "TILES_TTAB"), _constant("phm_draw_tab.h", "DRAW_TAB_ROWS")
PACKED_MAX = int(T.LONG_SEGMENTS)                                         # 48 segments: the most before the engine picks LONG
SEGMENTS = (TTAB + 2, TTAB + 3, PACKED_MAX, 2)                            # first draw on rows TTAB, TTAB + 1, PACKED_MAX - 2; and the usual 2
assert TTAB + 3 <= PACKED_MAX < ROWS + 1                                  # the R edges lie beyond the packed form (docstring)

SWEEPS = (("plain", 2), ("plain", 3), ("plain", 4), ("bigtree", 2), ("bigtree", 3), ("bigtree", 4), ("bf", 2), ("bf", 3), ("bf", 4), ("ks", 4))


@functools.lru_cache(maxsize=None)
def _case(variant, n):
    Q = T.model(n, variant)
    pid = np.full(n, 1.0 / n)
    z = synth.make_tree(12, Q, T.omega_of(Q), 5200 + 10 * n + len(variant), pid)
    if variant == "ks":
        z = RC.parity_tips(z)
    maps, names = [], []
    for b, (m, mn) in enumerate(zip(z["maps"], z["mapnames"])):
        path = synth.initial_path(float(np.sum(m)), int(mn[-1]), SEGMENTS[b % len(SEGMENTS)])
        maps.append(path[0]); names.append(path[1])
    z = dict(z, maps=maps, mapnames=names)
    case = T.Case(f"thr_{variant}{n}", "branches of 17, 18, 48 and 2 caller-supplied segments", Q, pid, z, variant, 70, 1900 + n, groups=(1, 3),
                  runs=(1, 2))
    assert not case.long and sorted({len(m) for m in maps}) == sorted(SEGMENTS)
    return case


@pytest.mark.parametrize("variant,n", SWEEPS, ids=lambda v: str(v))
def test_sweeps_from_the_threshold_rows_equal_the_oracle(variant, n):
    case = _case(variant, n)
    runs = {g: _run(case, g) for g in case.groups}
    for run in runs.values():
        _against_oracle(case, run)                                        # counts bit for bit, dwell sums to _same's bar, recoveries 0
        _same_across_groups(case, run.stats, runs[case.groups[0]].stats)


@pytest.mark.parametrize("n", [2, 3, 4])
def test_histories_equal_the_maps_replay(n):
    """the replay kernel (phm_mcmc_maps.hip) and its Python twin keep the arithmetic draw: the same segments, states and dwell times"""
    case = _case("plain", n)
    its, E = [0, 2], case.E
    for g in case.groups:
        kw = dict(seed=case.seed, n_replicas=case.S, reduce=False, branch_group=g)
        out, m = _API["plain"](case.z, case.Q, case.pid, case.Omega, case.N, maps=True, map_iters=its, **kw)
        assert m.n_hist == case.S * len(its) and m.n_edge == E
        np.testing.assert_array_equal(out, _API["plain"](case.z, case.Q, case.pid, case.Omega, case.N, mapping="tiles", **kw))
        for r in case.replicas:
            tout, rows = _twin(case.z, case.Q, case.Omega, case.pid, case.N, case.seed, r, "plain", its)
            for j in range(len(its)):
                _check_history(m, r * len(its) + j, rows, j, E)
            np.testing.assert_array_equal(out[r][:, n:], np.array(tout)[:, n:])


@pytest.fixture(scope="module")
def host_tables(tmp_path_factory):
    """the table of every state count as the host compiler builds it from the header: tests/native/draw_thresholds_check.cpp in its
    printing mode, -ffp-contract=off like the library"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("draw_tab")
    exe = str(d / "draw_thresholds_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "native", "draw_thresholds_check.cpp"),
                           "-o", exe])

    def table(B, rows):
        path = d / f"model{B.shape[0]}.txt"
        path.write_text(f"{B.shape[0]}\n" + " ".join(float(v).hex() for v in B.ravel()) + "\n")
        out = subprocess.run([exe, str(path), str(rows)], capture_output=True, text=True, check=True).stdout
        words = [int(w, 16) for line in out.splitlines() if re.fullmatch(r"[0-9a-f]{8}( [0-9a-f]{8}){3}", line) for w in line.split()]
        return np.array(words, dtype=np.uint32)
    return table


@pytest.mark.parametrize("n", [2, 3, 4])
def test_device_built_table_equals_the_host_built_one(n, host_tables):
    case = _case("bigtree", n)
    L = _lib.load()
    fn = L.phm_engine_debug_draw_table
    fn.restype, fn.argtypes = ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    eng = _lib.Engine(case.z, case.Q, case.pid, case.Omega, case.N, variant=_lib.PHM_MCMC_BIGTREE, seed=case.seed, n_replicas=case.S, mapping="tiles")
    try:
        rows = ctypes.c_int32(0)
        _lib.check(fn(eng.h, None, 0, ctypes.byref(rows)))
        assert rows.value == ROWS                                         # slots of 48-segment paths: the chain tables are longer than the table
        got = np.zeros(rows.value * n * n * 4, dtype=np.uint32)
        _lib.check(fn(eng.h, got.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), got.size, ctypes.byref(rows)))
    finally:
        eng.close()
    want = host_tables(np.asarray(case.B), rows.value)
    assert got.size == want.size
    np.testing.assert_array_equal(got, want)
    last = got.reshape(-1, 4)[:, 3]
    assert np.all(last[n * n:] <= n - 1)                                  # no fallback bit past row 0 under these models
    if n == 4:                                                            # the four structural zeros of row 0 cannot be tabulated
        assert int(np.sum(last[:16] == 0x80000000)) == 4
