"""ctypes front end to oracle/_ref/libphm_ref.so: the reference's own src/phylomap.cpp built on the stand-in Rcpp / Armadillo
headers (oracle/ref/, oracle/ref_build.sh).  TEST INFRASTRUCTURE ONLY.  The library exists only where the reference tree was
present at build time; ``available()`` says so, and every test that needs it skips itself otherwise.

Argument layouts follow tests/oracle_lib.py, so that one set of inputs drives both sides."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import oracle_lib as O
from oracle_lib import FlatTree, Tree, _ptr

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(_ROOT, "oracle", "_ref", "libphm_ref.so")

OK, EXC_SAMPLE, EXC_INDEX, EXC_OTHER = 0, 1, 2, 3          # status of a call: a C++ exception of the reference comes back as a code
SKIP_REASON = "oracle/_ref/libphm_ref.so is absent (the reference tree was not present when build() ran)"

_lib = None


def available() -> bool:
    return os.path.exists(_SO)


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(_SO)
        L.ref_rcout_lines.restype = C.c_long
        _lib = L
    return _lib


def rcout_lines() -> int:
    """How many lines the reference has sent to Rcout so far (its "newunifSample problem" message)."""
    return int(lib().ref_rcout_lines())


def mcmc_cols(n, variant, dic=False):
    if variant in (O.PLAIN, O.BIGTREE, O.SPARSE):
        return n + n * (n - 1)
    k = n // 2 - 1 if variant in (O.KS, O.KSMT) else 0
    return n + n * n + 2 + 3 * k + 1 + (1 if dic else 0)


def maketreelistMCMC(z, Q, pid, B, Omega, nen, nodelist, root, N, variant=O.PLAIN, seed=1, prior=None, dic=False):
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    ft = FlatTree(z)
    Qc, Bc = np.asfortranarray(Q), np.asfortranarray(np.asarray(B, dtype=np.float64))
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    nen = np.ascontiguousarray(nen, dtype=np.int32)
    nodelist = np.ascontiguousarray(nodelist, dtype=np.int32)
    cols = mcmc_cols(n, variant, dic)
    out = np.zeros((N, cols), order="F")
    pr = None if prior is None else np.ascontiguousarray(prior, dtype=np.float64)
    rc = lib().ref_maketreelistMCMC(int(variant) + (16 if dic else 0), C.byref(ft.c), n, _ptr(Qc, C.c_double), _ptr(pid, C.c_double),
                                    _ptr(Bc, C.c_double), C.c_double(Omega), _ptr(nen, C.c_int32), _ptr(nodelist, C.c_int32),
                                    int(root), int(N), None if pr is None else _ptr(pr, C.c_double), 0 if pr is None else pr.size,
                                    C.c_uint32(seed & 0xFFFFFFFF), _ptr(out, C.c_double), cols)
    return out, rc


def maketreelistMCMCmt(treelist, Q, pid, B, Omega, nen_m, nodelist_m, roots, N, prior, variant=O.MT, seed=1):
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    fts = [FlatTree(z) for z in treelist]
    arr = (C.POINTER(Tree) * len(fts))(*[C.pointer(ft.c) for ft in fts])
    Qc, Bc = np.asfortranarray(Q), np.asfortranarray(np.asarray(B, dtype=np.float64))
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    nen_m = np.ascontiguousarray(nen_m, dtype=np.int32)
    nodelist_m = np.ascontiguousarray(nodelist_m, dtype=np.int32)
    roots = np.ascontiguousarray(roots, dtype=np.int32)
    pr = np.ascontiguousarray(prior, dtype=np.float64)
    cols = mcmc_cols(n, variant)
    out = np.zeros((N, cols), order="F")
    rc = lib().ref_maketreelistMCMCmt(int(variant), arr, len(fts), n, _ptr(Qc, C.c_double), _ptr(pid, C.c_double), _ptr(Bc, C.c_double),
                                      C.c_double(Omega), _ptr(nen_m, C.c_int32), _ptr(nodelist_m, C.c_int32), _ptr(roots, C.c_int32),
                                      int(N), _ptr(pr, C.c_double), pr.size, C.c_uint32(seed & 0xFFFFFFFF), _ptr(out, C.c_double), cols)
    return out, rc


def maketreelistEXP(z, Q, pid, nen, nodelist, root, N, lefts, rights, d, seed=1):
    Q = np.asarray(Q, dtype=np.float64)
    n = Q.shape[0]
    ft = FlatTree(z)
    Qc = np.asfortranarray(Q)
    Lc, Rc, Dc = (np.asfortranarray(np.asarray(a, dtype=np.float64)) for a in (lefts, rights, d))
    pid = np.ascontiguousarray(pid, dtype=np.float64)
    nen = np.ascontiguousarray(nen, dtype=np.int32)
    nodelist = np.ascontiguousarray(nodelist, dtype=np.int32)
    cols = n + n * (n - 1)
    out = np.zeros((N, cols), order="F")
    rc = lib().ref_maketreelistEXP(C.byref(ft.c), n, _ptr(Qc, C.c_double), _ptr(pid, C.c_double), _ptr(nen, C.c_int32),
                                   _ptr(nodelist, C.c_int32), int(root), int(N), _ptr(Lc, C.c_double), _ptr(Rc, C.c_double),
                                   _ptr(Dc, C.c_double), C.c_uint32(seed & 0xFFFFFFFF), _ptr(out, C.c_double), cols)
    return out, rc


def shortener(d, s, n, bf=False):
    d = np.ascontiguousarray(d, dtype=np.float64).copy()
    s = np.ascontiguousarray(s, dtype=np.int32).copy()
    row = np.zeros(n + n * n if bf else n + n * (n - 1))
    m = C.c_int(0)
    rc = lib().ref_shortener(_ptr(d, C.c_double), _ptr(s, C.c_int32), len(d), n, int(bf), _ptr(row, C.c_double), C.byref(m))
    return d[:m.value], s[:m.value], row, rc


def matTospmat(B):
    B = np.ascontiguousarray(B, dtype=np.float64)
    out = np.zeros_like(B)
    rc = lib().ref_matTospmat(_ptr(B, C.c_double), B.shape[0], _ptr(out, C.c_double))
    return out, rc


def makePL(z, n, B, nen, seg_count, kind):
    """kind: 0 makePLrcpp, 1 makePLrcpp_bigtree, 2 SPARSEmakePLrcpp, 3 makePLnormalized."""
    ft = FlatTree(z)
    Bc = np.ascontiguousarray(B, dtype=np.float64)
    nen = np.ascontiguousarray(nen, dtype=np.int32)
    sc = np.ascontiguousarray(seg_count, dtype=np.int32)
    PL = np.zeros((2 * ft.T - 1, n))
    rc = lib().ref_makePL(int(kind), C.byref(ft.c), n, _ptr(Bc, C.c_double), _ptr(nen, C.c_int32), _ptr(sc, C.c_int32), _ptr(PL, C.c_double))
    return PL, rc


def makePLexp(z, n, P, nen):
    ft = FlatTree(z)
    P = np.ascontiguousarray(P, dtype=np.float64)
    nen = np.ascontiguousarray(nen, dtype=np.int32)
    PL = np.zeros((2 * ft.T - 1, n))
    rc = lib().ref_makePLexp(C.byref(ft.c), n, _ptr(P, C.c_double), _ptr(nen, C.c_int32), _ptr(PL, C.c_double))
    return PL, rc


def matexp(L, R, dvals, t):
    L = np.ascontiguousarray(L, dtype=np.float64)
    R = np.ascontiguousarray(R, dtype=np.float64)
    dv = np.ascontiguousarray(dvals, dtype=np.float64)
    n = L.shape[0]
    P = np.zeros((n, n))
    rc = lib().ref_matexp(_ptr(L, C.c_double), _ptr(R, C.c_double), _ptr(dv, C.c_double), n, C.c_double(t), _ptr(P, C.c_double))
    return P, rc


def sampleOnce(w, u):
    w = np.ascontiguousarray(w, dtype=np.float64)
    idx = C.c_int(-1)
    rc = lib().ref_sampleOnce(_ptr(w, C.c_double), w.size, C.c_double(u), C.byref(idx))
    return idx.value, rc


def sample(p, seed):
    """set.seed(seed); sample(0:(n-1), 1, TRUE, p) -> (index, status)."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    idx = C.c_int(-1)
    rc = lib().ref_sample(_ptr(p, C.c_double), p.size, C.c_uint32(seed), C.byref(idx))
    return idx.value, rc


def runif_rexp(seed, nu, ne, rate):
    u, e = np.zeros(nu), np.zeros(ne)
    rc = lib().ref_runif_rexp(C.c_uint32(seed), nu, ne, C.c_double(rate), _ptr(u, C.c_double), _ptr(e, C.c_double))
    return u, e, rc
