"""Stochastic maps of the MCMC samplers without a device: the twin (tests/mcmcmapsref.py) against pyref and
the oracle, the spec's invariants on the twin's maps, the argument checks of phm_maketreelistMCMC_maps (all before any device
call), and the R layer (shim/phylomap_mcmc_maps_shim.cpp, shim/R/phylomap_mcmc_maps.R)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mcmcmapsref
import oracle_lib as O
import pyref
from phylomap_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {"plain": O.PLAIN, "bigtree": O.BIGTREE, "sparse": O.SPARSE, "ks": O.KS, "bf": O.BF}


def _model(n, variant):
    if variant == "ks":
        Q = synth.make2sQ(0.3, 0.2, 0.4, 0.3, 2.0) if n == 4 else synth.make2sQ(0.3, 0.2, [0.4, 0.3], [0.3, 0.2], [2.0, 0.5])
    elif variant == "sparse":
        Q = synth.tridiagonal_Q(n, 0.2)
    else:
        Q = synth.dense_Q(n, 0.05, 0.25, seed=0x3D00 + n)
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    return Q, Omega


def _case(n, variant, T=7, seed=0x3D1):
    Q, Omega = _model(n, variant)
    z = synth.make_tree(T, Q, Omega, seed + n, init_segments=max(2, n if variant == "sparse" else 2))
    nen, nodelist, root = _lib.tree_orders(z)
    pid = np.arange(1.0, n + 1.0) / (n * (n + 1) / 2)
    return z, Q, Omega, pid, [int(v) for v in nen], [int(v) for v in nodelist], int(root)


def _cases():
    out = []
    for v in ("plain", "bigtree", "sparse", "bf"):
        for n in (2, 3, 4, 5, 7):
            out.append((n, v))
    out += [(4, "ks"), (6, "ks")]
    return out


@pytest.mark.parametrize("n,variant", _cases())
def test_twin_statistics_equal_pyref(n, variant):
    z, Q, Omega, pid, nen, nodelist, root = _case(n, variant)
    N, seed = 4, 7 + n
    a = (z, Q.tolist(), pid.tolist(), Omega, N, nen, nodelist, root, seed, 3)
    out, rows = mcmcmapsref.sumstatMCMC(*a, variant=variant)
    assert np.array_equal(np.array(out), np.array(pyref.sumstatMCMC(*a, variant=variant)))
    assert len(rows) == N * len(z["edge"])


@pytest.mark.parametrize("n,variant", [(2, "plain"), (4, "bigtree"), (3, "sparse"), (4, "ks"), (5, "bf"), (7, "plain")])
def test_twin_last_iteration_matches_the_oracle_paths(n, variant):
    z, Q, Omega, pid, nen, nodelist, root = _case(n, variant)
    N, seed = 3, 21 + n
    _, rows = mcmcmapsref.sumstatMCMC(z, Q.tolist(), pid.tolist(), Omega, N, nen, nodelist, root, seed, 0, variant=variant,
                                      map_iters=[N - 1])
    B = np.eye(n) + Q / Omega
    _, rc, db = O.maketreelistMCMC(z, Q, pid, B, Omega, nen, nodelist, root, N, variant=VARIANTS[variant], seed=seed, dump=True)
    assert rc == 0
    for b in range(len(z["edge"])):
        m = int(db.seg_count[b])
        d, s = np.asarray(db.seg_dwell[b, :m]), np.asarray(db.seg_state[b, :m])
        nd, ns = [d[0]], [s[0]]                                  # the final path with its virtual jumps, merged again
        for x, y in zip(d[1:], s[1:]):
            if y == ns[-1]:
                nd[-1] += x
            else:
                nd.append(x); ns.append(y)
        want = rows[(0, b)]
        assert [st for _, st in want] == [int(v) for v in ns], b           # both 0-based
        np.testing.assert_allclose([x for x, _ in want], nd, rtol=0, atol=1e-14)


@pytest.mark.parametrize("n,variant", [(2, "plain"), (3, "bigtree"), (4, "sparse"), (4, "ks"), (6, "ks"), (5, "bf"), (7, "plain")])
def test_twin_maps_satisfy_the_spec(n, variant):
    z, Q, Omega, pid, nen, nodelist, root = _case(n, variant, T=9)
    N, seed = 5, 33 + n
    its = [1, 4]
    S = 2
    chains = [mcmcmapsref.sumstatMCMC(z, Q.tolist(), pid.tolist(), Omega, N, nen, nodelist, root, seed, r, variant=variant,
                                      map_iters=its) for r in range(S)]
    E, T = len(z["edge"]), len(z["states"])
    off, dwell, state = mcmcmapsref.pack([c[1] for c in chains], len(its), E)
    assert off.size == S * len(its) * E + 1
    ks = variant in ("ks", "bf")
    edge = np.asarray(z["edge"])
    for s in range(S):
        out = np.array(chains[s][0])
        for j, it in enumerate(its):
            h = s * len(its) + j
            cnt = np.zeros((n, n))
            last_into, first_of = {}, {}
            for b in range(E):
                k = h * E + b
                st = state[off[k]:off[k + 1]] - 1
                dw = dwell[off[k]:off[k + 1]]
                assert st.size >= 1 and np.all(st[1:] != st[:-1])
                assert np.all(dw >= 0.0)
                np.testing.assert_allclose(dw.sum(), float(z["edge.length"][b]), rtol=1e-12)
                for a, c in zip(st[:-1], st[1:]):
                    cnt[a, c] += 1
                child = int(edge[b, 1])
                if child <= T:
                    obs = int(z["states"][child - 1]) - 1
                    assert (st[-1] % 2 == obs % 2) if variant == "ks" else st[-1] == obs
                else:
                    last_into[child] = st[-1]
                if st.size > 1:
                    first_of.setdefault(int(edge[b, 0]), []).append(st[0])
            for v, firsts in first_of.items():
                if v in last_into:
                    assert all(f == last_into[v] for f in firsts)
            if ks:
                want = out[it, n:n + n * n].reshape(n, n).copy()
                np.fill_diagonal(want, 0.0)
                assert np.array_equal(cnt, want)
            else:
                got = np.array([cnt[a, c] for a in range(n) for c in range(n) if a != c])
                assert np.array_equal(got, out[it, n:n + n * (n - 1)])


def _call(off, cap=0, dwell=None, state=None, iters=None, n_iters=0, mapping="auto", variant=_lib.PHM_MCMC, N=4):
    L = _lib.load()
    Q = synth.config_Q(2)
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    z = synth.make_tree(8, Q, Omega, 0x3E)
    ft = _lib.FlatTree(z)
    Qf = np.asfortranarray(Q)
    B = np.asfortranarray(np.eye(4) + Q / Omega)
    pid = np.full(4, 0.25)
    nen, nodelist, root = _lib.tree_orders(z)
    o = _lib.make_options(mapping=mapping, n_replicas=2)
    out = np.zeros((2, 12, N))
    it = None if iters is None else np.ascontiguousarray(iters, dtype=np.int32)
    return L.phm_maketreelistMCMC_maps(int(variant), C.byref(ft.c), 4, _lib._p(Qf, C.c_double), _lib._p(pid, C.c_double),
                                       _lib._p(B, C.c_double), float(Omega), _lib._p(nen, C.c_int32), _lib._p(nodelist, C.c_int32),
                                       int(root), N, None if it is None else _lib._p(it, C.c_int32), int(n_iters), C.byref(o),
                                       _lib._p(out, C.c_double), None if off is None else _lib._p(off, C.c_int64), int(cap),
                                       None if dwell is None else _lib._p(dwell, C.c_double),
                                       None if state is None else _lib._p(state, C.c_int32))


def test_mcmc_map_arguments_are_checked_before_the_device():
    L = _lib.load()
    E = 14
    off = np.zeros(2 * 4 * E + 1, dtype=np.int64)
    assert _call(None) == 1
    assert "map_off is NULL" in L.phm_last_error().decode()
    for bad in ([2, 1], [1, 1], [0, 4], [-1, 2]):                            # unsorted, duplicate, out of range
        assert _call(off, iters=bad, n_iters=2) == 1, bad
        assert "map_iters" in L.phm_last_error().decode()
    assert _call(off, iters=None, n_iters=3) == 1                             # NULL map_iters needs n_map_iters = 0
    assert _call(off, iters=[0], n_iters=0) == 1
    for mapping in ("replicas", "branches"):
        assert _call(off, mapping=mapping) == 2
        assert "PHM_MAP_TILES" in L.phm_last_error().decode()
    for v in (_lib.PHM_MCMC_MT, _lib.PHM_MCMC_KSMT, 17):
        assert _call(off, variant=v) == 2
    good = np.arange(2 * 2 * E + 1, dtype=np.int64)                           # filling: the offsets are checked too
    dwell, state = np.zeros(100), np.zeros(100, dtype=np.int32)
    assert _call(good, cap=10, dwell=dwell, state=state, iters=[1, 3], n_iters=2) == 1
    assert "map_cap" in L.phm_last_error().decode()
    assert _call(good, cap=100, dwell=dwell, state=None, iters=[1, 3], n_iters=2) == 1


def test_mcmc_maps_symbol_is_exported():
    L = _lib.load()
    assert hasattr(L, "phm_maketreelistMCMC_maps") and "phm_maketreelistMCMC_maps" in _lib.EXPORTS


def test_mcmc_maps_r_wrapper_names_the_exported_call_symbol():
    src = open(os.path.join(ROOT, "shim", "phylomap_mcmc_maps_shim.cpp")).read()
    exported = set(re.findall(r"RcppExport SEXP (\w+)\(", src))
    assert exported == {"phylomap_hip_mcmc_maps"}
    rfile = open(os.path.join(ROOT, "shim", "R", "phylomap_mcmc_maps.R")).read()
    assert set(re.findall(r"\.Call\('(\w+)'", rfile)) == exported
    assert re.search(r"^sumstatMCMCmaps <- function\(z, Q, pid, Omega, N, map_iters = NULL, variant = \"plain\"\)", rfile, re.M)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_mcmc_maps_shim_compiles_against_the_mock():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "tests", "mock_rcpp"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "shim", "phylomap_mcmc_maps_shim.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
