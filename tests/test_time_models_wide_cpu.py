"""The batched expectations through time at 9..64 states without a device (phm_expected_through_time_models_wide, DESIGN.md
section 29): where the symbol is declared and bound, every refusal of the entry point before its first device call by status and
message, the Python side (``batched``, ``labels``) and the new pure host pieces (the restated form rule against
``sw_form_terms``, the launch sizes) in a stand-alone program under AddressSanitizer and UBSan.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from phylomap_amd import _lib, api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "phm_expected_through_time_models_wide"
PARENT = "phm_expected_through_time_models"


def test_symbol_is_declared_apart_and_bound_to_the_prototype():
    L = _lib.load()
    assert hasattr(L, NAME) and _lib.EXT6_EXPORTS == [NAME]
    assert NAME not in (_lib.EXPORTS + _lib.EXT_EXPORTS + _lib.EXT2_EXPORTS + _lib.EXT3_EXPORTS + _lib.EXT4_EXPORTS + _lib.EXT5_EXPORTS)
    assert _lib.EXT5_EXPORTS == [PARENT]
    assert L.phm_version() == 300
    i32, pd = C.c_int32, C.POINTER(C.c_double)
    parent = list(getattr(L, PARENT).argtypes)
    assert len(parent) == 18
    # the parent's eighteen arguments one for one, n_labels and labels after bounds
    assert list(getattr(L, NAME).argtypes) == parent[:11] + [i32, pd] + parent[11:]
    inc = os.path.join(ROOT, "include")
    for name in ("phylomap_hip.h", "phylomap_hip_ext.h", "phylomap_hip_ext2.h", "phylomap_hip_ext3.h", "phylomap_hip_ext4.h"):
        assert NAME not in open(os.path.join(inc, name)).read()
    ext5 = open(os.path.join(inc, "phylomap_hip_ext5.h")).read()
    assert re.findall(r"\b(phm_[A-Za-z0-9_]+)\s*\(", ext5) == [PARENT]           # named in its comment, not declared there
    ext6 = open(os.path.join(inc, "phylomap_hip_ext6.h")).read()
    assert re.findall(r"\b(phm_[A-Za-z0-9_]+)\s*\(", ext6) == [NAME] and '#include "phylomap_hip_ext5.h"' in ext6
    assert ext6.count("#include") == 1
    proto = re.search(NAME + r"\s*\(([^;]*)\)\s*;", ext6).group(1)
    kinds = [re.sub(r"\s*\w+$", "", a.strip().replace("const ", "")) for a in proto.split(",")]   # each argument's type
    assert kinds == ["phm_tree*", "int32_t", "int32_t", "double*", "double*", "int32_t", "int32_t*", "int32_t*", "phm_options*",
                     "int32_t", "double*", "int32_t", "double*", "double*", "double*", "int64_t", "int32_t*", "double*", "double*",
                     "double*"]
    names = [re.search(r"(\w+)$", a.strip()).group(1) for a in proto.split(",")]
    assert names[9:13] == ["n_bounds", "bounds", "n_labels", "labels"]
    ctype = {"phm_tree*": _lib.Tree, "phm_options*": _lib.Options, "double*": C.c_double, "int32_t*": C.c_int32}
    want = [C.POINTER(ctype[k]) if k.endswith("*") else {"int32_t": C.c_int32, "int64_t": C.c_int64}[k] for k in kinds]
    assert list(getattr(L, NAME).argtypes) == want
    doc = api.expected_through_time_models.__doc__
    assert NAME in doc and "bit for bit" in doc and "batched" in doc
    mk = open(os.path.join(ROOT, "Makefile")).read()
    for f in ("phm_time_models_wide.hip", "phm_time_models_wide_api.cpp", "include/phylomap_hip_ext6.h"):
        assert f in mk
    for f in ("phm_time_models_wide.hip", "phm_time_models_wide.h", "phm_time_models_wide_api.cpp"):
        assert os.path.exists(os.path.join(ROOT, "phylomap_amd", "csrc", f))


def _raw(z, Qs, pid, S=2, bounds=None, n_bounds=None, points=None, n_points=None, som=None, occ=True, bins=True, post=True, ll=True,
         tree=True, q=True, p=True, labels=None, n_labels=None):
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
    lab = None if labels is None else np.ascontiguousarray(np.asarray(labels, dtype=np.float64).transpose(0, 2, 1))
    nl = (0 if lab is None else lab.shape[0]) if n_labels is None else n_labels
    ev = K * S
    o_occ = np.zeros(n * max(nb, 1) * ev) if occ else None
    o_bin = np.zeros(n * n * max(nb, 1) * ev) if bins else None
    o_post = np.zeros(n * max(npt, 1) * ev) if post else None
    o_ll = np.zeros(ev) if ll else None
    L = _lib.load()
    status = getattr(L, NAME)(C.byref(pt.c) if tree else None, n, K, _lib._p(Qf, C.c_double) if q else None,
                              _lib._p(pid, C.c_double) if p else None, pid.size // n, None, _lib._p(sm, C.c_int32), C.byref(o), nb,
                              _lib._p(bnd, C.c_double), nl, _lib._p(lab, C.c_double), _lib._p(o_occ, C.c_double),
                              _lib._p(o_bin, C.c_double), npt, _lib._p(pe, C.c_int32), _lib._p(pp, C.c_double),
                              _lib._p(o_post, C.c_double), _lib._p(o_ll, C.c_double))
    return status, L.phm_last_error().decode()


def _random_Q(n, rs):
    Q = rs.uniform(0.05, 1.0, (n, n)) * 4.0 / n
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q


def _tree16():
    T = 16
    edge, lens = synth.random_tree(T, 0.5, 3)
    return {"edge": edge, "edge.length": lens, "Nnode": T - 1, "states": np.ones(T, dtype=np.int32)}


def test_refusals_need_no_device():
    L = _lib.load()
    z = _tree16()
    lens = z["edge.length"]
    E = z["edge"].shape[0]
    rs = np.random.default_rng(3)
    bounds = [0.0, 0.2, 0.7]
    points = ([0, 3, E - 1], [0.0, 0.5 * lens[3], lens[E - 1]])
    n = 9
    Qs = np.stack([_random_Q(n, rs) for _ in range(3)])
    pid = np.ones(n)
    ok = dict(bounds=bounds, points=points)
    # section 28's refusals, message for message under the new name
    for missing in ("tree", "q", "p"):
        st, msg = _raw(z, Qs, pid, **ok, **{missing: False})
        assert st == 1 and msg == NAME + ": NULL argument (x, Q and pid are required)", (missing, st, msg)
    st, msg = _raw(z, Qs, pid, **ok, occ=False, bins=False, post=False, ll=False)
    assert st == 1 and msg == NAME + ": no output requested (occupancy, bin_stats, point_post and loglik are all NULL)", msg
    bad = Qs.copy()
    bad[2, 0, 3], bad[2, 0, 1] = -0.05, bad[2, 0, 1] + 0.05                    # ll_validate's checks, under this name where it names one
    st, msg = _raw(z, bad, pid, **ok)
    assert st == 1 and msg.startswith("model 2")
    st, msg = _raw(z, Qs, np.ones(2 * n), **ok)                                # n_pid = 2 with 3 models
    assert st == 1 and msg.startswith(NAME + ": n_pid")
    for s in (-1, 2):
        st, msg = _raw(z, Qs, pid, **ok, som=[0, s, 1])
        assert st == 1 and msg == NAME + ": site_of_model[1] must be in 0..S-1", msg
    st, msg = _raw(z, Qs, pid, points=points, n_bounds=-1)
    assert st == 1 and msg == NAME + ": bounds must hold n_bounds >= 0 values", msg
    st, msg = _raw(z, Qs, pid, points=points, n_bounds=2)
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
    for v in (-0.1, np.nan, np.inf):
        st, msg = _raw(z, Qs, pid, bounds=[0.0, v, 0.7], points=points)
        assert st == 1 and msg == NAME + ": bounds[1] must be finite and >= 0", msg
    for b in ([0.0, 0.2, 0.2], [0.0, 0.7, 0.2]):
        st, msg = _raw(z, Qs, pid, bounds=b, points=points)
        assert st == 1 and msg == NAME + ": bounds[2] is not above bounds[1] (bounds must increase strictly)", msg
    for e in (-1, E):
        st, msg = _raw(z, Qs, pid, bounds=bounds, points=([0, e, 1], [0.0, 0.0, 0.0]))
        assert st == 1 and msg == NAME + f": point 1: edge row {e} is not in 0..n_edge-1", msg
    for pos in (-0.01, 1.0001 * lens[5], np.nan):
        st, msg = _raw(z, Qs, pid, bounds=bounds, points=([0, 1, 5], [0.0, 0.0, pos]))
        assert st == 1 and msg.startswith(NAME + ": point 2: position ") and msg.endswith(" is not in [0, t_b] of edge row 5"), msg
    fast = Qs.copy()
    fast[1] *= 1e7                                                             # mu t_b above 1e6 on the longer branches
    mu = float(np.max(-np.diag(fast[1])))
    over = mu * lens > 1e6
    first = int(np.argmax(over))
    assert over[first] and not np.all(over)
    st, msg = _raw(z, fast, pid, **ok)
    assert st == 2 and msg == NAME + f": model 1, edge row {first + 1}: max(-q_ii) * t_b above 1e6", msg
    # section 27's label checks in its words
    labels = rs.uniform(0.0, 1.0, (2, n, n))
    for nl in (0, -1):
        st, msg = _raw(z, Qs, pid, **ok, labels=labels, n_labels=nl)
        assert st == 1 and msg == NAME + ": n_labels must be >= 1 when labels is given", msg
    st, msg = _raw(z, Qs, pid, **ok, labels=labels, n_labels=65536)
    assert st == 1 and msg == NAME + ": n_labels must be at most 65535", msg
    for v in (np.nan, np.inf):
        bad_lab = labels.copy()
        bad_lab[1, 2, 3] = v
        st, msg = _raw(z, Qs, pid, **ok, labels=bad_lab)
        assert st == 1 and msg == NAME + ": label 1 has a non-finite weight", msg
    st, msg = _raw(z, Qs, pid, bounds=bounds, points=points, labels=labels, bins=False)
    assert st == 1 and msg == NAME + ": labels need bin_stats", msg
    # the state counts it serves: the other _wide entry points' words
    for m in (4, 8, 65, 1):
        st, msg = _raw(z, np.stack([_random_Q(m, rs)]), np.ones(m), **ok)
        assert st == 2 and msg == NAME + ": 9..64 states only: 2..8 states go to " + PARENT, (m, st, msg)
    if L.phm_device_count() == 0:                                              # a valid call gets as far as the device
        assert _raw(z, Qs, pid, **ok)[0] == 3
        assert _raw(z, Qs, pid, **ok, ll=False)[0] == 3                        # any output may be NULL as long as one is not
        assert _raw(z, Qs, pid, ll=True, occ=False, bins=False, post=False)[0] == 3
        assert _raw(z, Qs, pid, **ok, som=[1, 0, 1])[0] == 3
        assert _raw(z, Qs, pid, **ok, labels=labels)[0] == 3
        Q64 = np.stack([_random_Q(64, rs)])
        assert _raw(z, Q64, np.ones(64), **ok)[0] == 3


class _Recorder:
    """stands in for the loaded library: records which entry point a call of ``api`` reaches and with how many arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, len(args)))
            return 0
        return fn


def test_the_default_call_is_unchanged_and_labels_need_the_batched_route(monkeypatch):
    z = _tree16()
    rs = np.random.default_rng(5)
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(_lib, "set_debug_options", lambda **kw: None)
    for n in (4, 9, 20):
        Qs = np.stack([_random_Q(n, rs) for _ in range(2)])
        kw = dict(bounds=[0.0, 0.3, 0.6], points=([0, 1], [0.0, 0.0]))
        rec.calls.clear()
        got = api.expected_through_time_models(z, Qs, np.ones(n), **kw)
        also = api.expected_through_time_models(z, Qs, np.ones(n), batched=False, **kw)
        assert rec.calls == [(PARENT, 18)] * 2                                  # exactly the C call it made
        assert got.bins.shape == also.bins.shape == (2, 1, 2, n * n)
        rec.calls.clear()
        got = api.expected_through_time_models(z, Qs, np.ones(n), batched=True, **kw)
        assert rec.calls == [(PARENT, 18) if n <= 8 else (NAME, 20)]            # at 2..8 states batched changes nothing
        labels = rs.uniform(0.0, 1.0, (3, n, n))
        rec.calls.clear()
        if n <= 8:
            for batched in (False, True):
                with pytest.raises(ValueError, match="2..8 states"):
                    api.expected_through_time_models(z, Qs, np.ones(n), labels=labels, batched=batched, **kw)
            assert rec.calls == []
        else:
            with pytest.raises(ValueError, match="batched=True"):
                api.expected_through_time_models(z, Qs, np.ones(n), labels=labels, **kw)
            with pytest.raises(ValueError, match=r"\[L, n, n\]"):
                api.expected_through_time_models(z, Qs, np.ones(n), labels=labels[:, :-1], batched=True, **kw)
            assert rec.calls == []
            got = api.expected_through_time_models(z, Qs, np.ones(n), labels=labels, batched=True, **kw)
            one = api.expected_through_time_models(z, Qs, np.ones(n), labels=labels[0], batched=True, site_of_model=[0, 0], **kw)
            assert rec.calls == [(NAME, 20)] * 2
            assert got.bins.shape == (2, 1, 2, 3) and one.bins.shape == (2, 2, 1) and got.occupancy.shape == (2, 1, 3, n)


def test_host_pieces_under_sanitizers(tmp_path):
    """tests/native/time_models_wide_host_check.cpp: the restated form rule against sw_form_terms and the launch sizes, host code
    only, under AddressSanitizer and UBSan; it checks itself"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    exe = str(tmp_path / "time_models_wide_host_check")
    csrc = os.path.join(ROOT, "phylomap_amd", "csrc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "native", "time_models_wide_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.splitlines()[-1] == "ok"
