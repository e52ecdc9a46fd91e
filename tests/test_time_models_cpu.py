"""The expectations through time under many rate matrices without a device (phm_expected_through_time_models, DESIGN.md section
28): where the symbol is declared and bound, every refusal of the entry point before its first device call by status and message,
the pure host pieces (the checks of bounds and points, the plan of crossings and sub-branches, the items of a launch) in a
stand-alone program under AddressSanitizer and UBSan, the twin ``timeref_models`` against ``timeref`` at one model, and
``ancestral.average_over_models``.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

import branchrowscases as bc
import timeref
import timeref_models
from phylomap_amd import _lib, ancestral, api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "phm_expected_through_time_models"


def test_symbol_is_declared_apart_and_bound_to_the_prototype():
    L = _lib.load()
    assert hasattr(L, NAME) and _lib.EXT5_EXPORTS == [NAME]
    assert NAME not in _lib.EXPORTS + _lib.EXT_EXPORTS + _lib.EXT2_EXPORTS + _lib.EXT3_EXPORTS + _lib.EXT4_EXPORTS
    assert _lib.EXT4_EXPORTS == ["phm_expected_branch_stats_models"]
    assert L.phm_version() == 300
    i32, i64, pi, pd = C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_double)
    totals = list(L.phm_expected_stats_models.argtypes)
    single = list(L.phm_expected_through_time.argtypes)
    # the first nine arguments are phm_expected_stats_models', the rest phm_expected_through_time's after its options
    assert list(getattr(L, NAME).argtypes) == totals[:9] + [i32, pd, pd, pd, i64, pi, pd, pd, pd] == totals[:9] + single[6:]
    inc = os.path.join(ROOT, "include")
    for name in ("phylomap_hip.h", "phylomap_hip_ext.h", "phylomap_hip_ext2.h", "phylomap_hip_ext3.h", "phylomap_hip_ext4.h"):
        assert NAME not in open(os.path.join(inc, name)).read()
    ext5 = open(os.path.join(inc, "phylomap_hip_ext5.h")).read()
    assert re.findall(r"\b(phm_[A-Za-z0-9_]+)\s*\(", ext5) == [NAME] and '#include "phylomap_hip_ext4.h"' in ext5
    proto = re.search(NAME + r"\s*\(([^;]*)\)\s*;", ext5).group(1)
    kinds = [re.sub(r"\s*\w+$", "", a.strip().replace("const ", "")) for a in proto.split(",")]   # each argument's type
    assert kinds == ["phm_tree*", "int32_t", "int32_t", "double*", "double*", "int32_t", "int32_t*", "int32_t*", "phm_options*",
                     "int32_t", "double*", "double*", "double*", "int64_t", "int32_t*", "double*", "double*", "double*"]
    assert NAME in api.expected_through_time_models.__doc__
    mk = open(os.path.join(ROOT, "Makefile")).read()
    for f in ("phm_time_models.hip", "phm_time_models_api.cpp", "include/phylomap_hip_ext5.h"):
        assert f in mk


def _raw(z, Qs, pid, S=2, bounds=None, n_bounds=None, points=None, n_points=None, som=None, occ=True, bins=True, post=True, ll=True,
         tree=True, q=True, p=True):
    """one call of the entry point with the tree's tips tiled S times -> (status, message)"""
    Qs = np.asarray(Qs, dtype=np.float64)
    K, n = Qs.shape[0], Qs.shape[1]
    Qf = np.ascontiguousarray(Qs.transpose(0, 2, 1))
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    pt = _lib.PlainTree(z, np.tile(z["states"], (S, 1)))
    o = _lib.make_options(n_replicas=S, tips_per_replica=True)
    bnd = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.float64)
    nb = (0 if bnd is None else bnd.size) if n_bounds is None else n_bounds
    pe = pp = None
    if points is not None:
        pe, pp = np.ascontiguousarray(points[0], dtype=np.int32), np.ascontiguousarray(points[1], dtype=np.float64)
    npt = (0 if pe is None else pe.size) if n_points is None else n_points
    sm = None if som is None else np.ascontiguousarray(som, dtype=np.int32)
    ev = K * S
    o_occ = np.zeros(n * max(nb, 1) * ev) if occ else None
    o_bin = np.zeros(n * n * max(nb, 1) * ev) if bins else None
    o_post = np.zeros(n * max(npt, 1) * ev) if post else None
    o_ll = np.zeros(ev) if ll else None
    L = _lib.load()
    status = getattr(L, NAME)(C.byref(pt.c) if tree else None, n, K, _lib._p(Qf, C.c_double) if q else None,
                              _lib._p(pid, C.c_double) if p else None, pid.size // n, None, _lib._p(sm, C.c_int32), C.byref(o), nb,
                              _lib._p(bnd, C.c_double), _lib._p(o_occ, C.c_double), _lib._p(o_bin, C.c_double), npt,
                              _lib._p(pe, C.c_int32), _lib._p(pp, C.c_double), _lib._p(o_post, C.c_double), _lib._p(o_ll, C.c_double))
    return status, L.phm_last_error().decode()


def _random_Q(n, rs):
    Q = rs.uniform(0.05, 1.0, (n, n)) * 4.0 / n
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q


def test_refusals_need_no_device():
    L = _lib.load()
    T = 16
    edge, lens = synth.random_tree(T, 0.5, 3)
    z = {"edge": edge, "edge.length": lens, "Nnode": T - 1, "states": np.ones(T, dtype=np.int32)}
    E = edge.shape[0]
    rs = np.random.default_rng(3)
    bounds = [0.0, 0.2, 0.7]
    points = ([0, 3, E - 1], [0.0, 0.5 * lens[3], lens[E - 1]])
    for n in (4, 9):                                                           # both routes share every check
        Qs = np.stack([_random_Q(n, rs) for _ in range(3)])
        pid = np.ones(n)
        ok = dict(bounds=bounds, points=points)
        for missing in ("tree", "q", "p"):
            st, msg = _raw(z, Qs, pid, **ok, **{missing: False})
            assert st == 1 and msg.startswith(NAME + ": NULL argument"), (missing, st, msg)
        st, msg = _raw(z, Qs, pid, **ok, occ=False, bins=False, post=False, ll=False)
        assert st == 1 and msg == NAME + ": no output requested (occupancy, bin_stats, point_post and loglik are all NULL)", msg
        bad = Qs.copy()
        bad[2, 0, 3], bad[2, 0, 1] = -0.05, bad[2, 0, 1] + 0.05                # ll_validate's checks, under this name where it names one
        st, msg = _raw(z, bad, pid, **ok)
        assert st == 1 and msg.startswith("model 2")
        st, msg = _raw(z, Qs, np.ones(2 * n), **ok)                            # n_pid = 2 with 3 models
        assert st == 1 and msg.startswith(NAME + ": n_pid")
        for s in (-1, 2):                                                      # a site outside 0..S-1: the model is named
            st, msg = _raw(z, Qs, pid, **ok, som=[0, s, 1])
            assert st == 1 and msg == NAME + ": site_of_model[1] must be in 0..S-1", msg
        # the counts: phm_expected_through_time's checks in its words
        st, msg = _raw(z, Qs, pid, points=points, n_bounds=-1)
        assert st == 1 and msg == NAME + ": bounds must hold n_bounds >= 0 values", msg
        st, msg = _raw(z, Qs, pid, points=points, n_bounds=2)                  # no array behind the count
        assert st == 1 and msg == NAME + ": bounds must hold n_bounds >= 0 values", msg
        st, msg = _raw(z, Qs, pid, points=points, bins=False)
        assert st == 1 and msg == NAME + ": occupancy needs n_bounds >= 1", msg
        st, msg = _raw(z, Qs, pid, bounds=[0.3], points=points)
        assert st == 1 and msg == NAME + ": bin_stats needs n_bounds >= 2", msg
        st, msg = _raw(z, Qs, pid, bounds=bounds, n_points=2, post=False)
        assert st == 1 and msg == NAME + ": point_edge and point_pos must hold n_points >= 0 values", msg
        st, msg = _raw(z, Qs, pid, bounds=bounds, points=points, n_points=-1)
        assert st == 1 and msg == NAME + ": point_edge and point_pos must hold n_points >= 0 values", msg
        st, msg = _raw(z, Qs, pid, bounds=bounds)
        assert st == 1 and msg == NAME + ": point_post needs n_points >= 1", msg
        # a bad bound: the 0-based index is named
        for v in (-0.1, np.nan, np.inf):
            st, msg = _raw(z, Qs, pid, bounds=[0.0, v, 0.7], points=points)
            assert st == 1 and msg == NAME + ": bounds[1] must be finite and >= 0", msg
        for b in ([0.0, 0.2, 0.2], [0.0, 0.7, 0.2]):
            st, msg = _raw(z, Qs, pid, bounds=b, points=points)
            assert st == 1 and msg == NAME + ": bounds[2] is not above bounds[1] (bounds must increase strictly)", msg
        # a bad point: the 0-based point is named
        for e in (-1, E):
            st, msg = _raw(z, Qs, pid, bounds=bounds, points=([0, e, 1], [0.0, 0.0, 0.0]))
            assert st == 1 and msg == NAME + f": point 1: edge row {e} is not in 0..n_edge-1", msg
        for pos in (-0.01, 1.0001 * lens[5], np.nan):
            st, msg = _raw(z, Qs, pid, bounds=bounds, points=([0, 1, 5], [0.0, 0.0, pos]))
            assert st == 1 and msg.startswith(NAME + ": point 2: position ") and msg.endswith(" is not in [0, t_b] of edge row 5"), msg
        fast = Qs.copy()
        fast[1] *= 1e7                                                         # mu t_b above 1e6 on the longer branches
        mu = float(np.max(-np.diag(fast[1])))
        over = mu * lens > 1e6
        first = int(np.argmax(over))
        assert over[first] and not np.all(over)
        st, msg = _raw(z, fast, pid, **ok)
        assert st == 2 and msg == NAME + f": model 1, edge row {first + 1}: max(-q_ii) * t_b above 1e6", msg
        if L.phm_device_count() == 0:                                          # a valid call gets as far as the device
            assert _raw(z, Qs, pid, **ok)[0] == 3
            assert _raw(z, Qs, pid, **ok, ll=False)[0] == 3                    # any output may be NULL as long as one is not
            assert _raw(z, Qs, pid, ll=True, occ=False, bins=False, post=False)[0] == 3
            assert _raw(z, Qs, pid, **ok, som=[1, 0, 1])[0] == 3
    for n in (1, 65):
        st, msg = _raw(z, np.zeros((1, n, n)), np.ones(n), bounds=bounds, points=points)
        assert st == 1 and msg.startswith(NAME + ": ") and "2..64" in msg, msg


def test_host_pieces_under_sanitizers(tmp_path):
    """tests/native/time_models_host_check.cpp: the checks, the plan on a hand-made tree and the launch sizes of
    phm_time_models_host.h, host code only, under AddressSanitizer and UBSan; it checks itself"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    exe = str(tmp_path / "time_models_host_check")
    csrc = os.path.join(ROOT, "phylomap_amd", "csrc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "native", "time_models_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.splitlines()[-1] == "ok"


def test_the_twin_of_one_model_is_timeref():
    z = bc.tree6()
    n, T = 3, 6
    Qs, pid = bc.models(n, 2)
    tips = bc.sites(n, T, S=3)
    el = np.asarray(z["edge.length"])
    E = el.size
    d = timeref.depths(z["edge"], el)
    bounds = np.array([0.0, 0.3 * d.max(), d.max(), 1.5 * d.max()])
    points = (np.concatenate([np.arange(E)] * 2), np.concatenate([np.zeros(E), 0.4 * el]))
    want = timeref.through_time(z["edge"], el, Qs[1], pid[1], tips, bounds=bounds, points=points)
    got = timeref_models.through_time_models(z["edge"], el, Qs[1:2], pid[1:2], tips, bounds=bounds, points=points)
    assert sorted(got) == sorted(want) == ["bins", "loglik", "occupancy", "points"]
    for key in want:
        assert got[key].shape == (1,) + want[key].shape and np.array_equal(got[key][0], want[key]), key
    # two models, a prior shared or per model, and the paired order: each slice is timeref's on that model and site
    both = timeref_models.through_time_models(z["edge"], el, Qs, pid, tips, bounds=bounds, points=points)
    assert both["occupancy"].shape == (2, 3, 4, n) and both["bins"].shape == (2, 3, 3, n * n) and both["points"].shape == (2, 3, 2 * E, n)
    assert np.array_equal(both["bins"][1], want["bins"])
    paired = timeref_models.through_time_models(z["edge"], el, Qs, pid, tips, bounds=bounds, points=points, site_of_model=[2, 0])
    assert paired["loglik"].shape == (2,) and paired["occupancy"].shape == (2, 4, n)
    for k, s in enumerate((2, 0)):                                             # numpy's products over 1 site and over 3 round apart
        for key in both:
            np.testing.assert_allclose(paired[key][k], both[key][k, s], rtol=1e-13, atol=1e-15, err_msg=f"{key} {k}")
    shared = timeref_models.through_time_models(z["edge"], el, Qs, pid[1], tips, bounds=bounds)
    assert np.array_equal(shared["occupancy"][1], want["occupancy"]) and "points" not in shared


def test_average_over_models_on_hand_made_arrays():
    values = np.array([[[1.0, 2.0], [3.0, 4.0]],
                       [[np.nan, np.nan], [np.nan, np.nan]],
                       [[5.0, 6.0], [7.0, 8.0]]])                               # [K = 3, 2, 2], an impossible model in the middle
    got = ancestral.average_over_models(values, [1.0, 0.0, 3.0])
    assert np.array_equal(got, np.array([[4.0, 5.0], [6.0, 7.0]]))              # 0.25 * first + 0.75 * last, exact in binary
    uniform = ancestral.average_over_models(values[[0, 2]], None)
    assert np.array_equal(uniform, np.array([[3.0, 4.0], [5.0, 6.0]]))
    assert np.array_equal(ancestral.average_over_models(values[[0, 2]]), uniform)
    w = ancestral.akaike_weights([-10.0, -np.inf, -10.0], 2)
    assert np.array_equal(ancestral.average_over_models(values, w), uniform)
    assert np.array_equal(ancestral.average_over_models(values, w), ancestral.model_average(values, w))
    for bad in ([1.0, 2.0], [1.0, -1.0, 1.0], [0.0, 0.0, 0.0]):
        try:
            ancestral.average_over_models(values, bad)
        except ValueError:
            pass
        else:
            raise AssertionError("weights of the wrong length, negative or all zero must be refused")
    assert "expected_through_time_models" in ancestral.average_over_models.__doc__
