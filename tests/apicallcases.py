"""What the Python layer hands to the C ABI, call by call, without a device: the recorder and the cases that
tests/golden/api_calls/parent.json pins (recorded by tests/golden/api_calls/make_golden.py from the commit before the binding
layer got its shared helpers, compared by tests/test_api_calls_cpu.py).  Shared by the recorder script and the test so that
both make the same calls.

``Recorder`` replaces ``_lib._p`` by a wrapper that also remembers each array under its data address, and the cached library
``_lib._lib`` by a proxy: the host-only symbols in ``PASS`` go to the real library, every other call is recorded and answers 0
(phm_set_debug_options is recorded and passed on).  Per positional argument, in ABI order, a record holds: a scalar's value;
the bytes of a ``byref`` Options / DebugOptions; of a Tree (or an array of them) the three counts and each of the six pointers
resolved by address; of a Model its scalars and three pointers; of a pointer the dtype, byte count and SHA-256 of the memory
behind it.  The ``dwell`` and ``state`` buffers after an int64 offsets array come from ``np.empty``: dtype and byte count only.
An offsets array with capacity 0 is a sizing call: the proxy writes ``off[i] = 2 * i`` so that the filling call's sizes are
pinned too.  A pointer that did not go through ``_lib._p`` is an error, and so is one whose array is gone when the call is
made: the recorder holds weak references only, so whatever keeps an array alive until its call is the code under test.

Two results of the Python layer depend on the machine's LAPACK / vector math in their last bits (the eigendecomposition that
``sumstatEXP`` computes without ``eig=``, the default starts of ``posterior_rates``): a case names those arguments in
``loose`` and only dtype and byte count are recorded for them; the cases with ``eig=`` and ``theta0=`` pin the same arguments'
bytes.  Every other input is exact arithmetic on fixed numbers or a fixed-seed integer generator.  Checked on one machine by
switching kernels: with ``NPY_DISABLE_CPU_FEATURES`` naming the AVX-512 groups the bytes of the default starts change (numpy's
``exp``), with ``OPENBLAS_CORETYPE=Haswell`` or ``Nehalem`` those of lefts, rights and d do, and with both set every record
of the golden file still compares equal.

Of every returned array the shape, strides, dtype and the offset of its data inside the buffer handed to C (named by the
call and argument it was first seen in) are recorded; an array C never saw by its bytes.  Tuples, dicts and named tuples are
keyed by position or name."""
import ctypes as C
import hashlib
import weakref

import numpy as np

import manymodelscases as mm
from phylomap_amd import _lib, api, ratemodel, synth

PASS = ("phm_tree_orders", "phm_last_error", "phm_struct_size", "phm_status_string", "phm_version")


def _addr(ptr):
    return C.cast(ptr, C.c_void_p).value


class Recorder:
    def __init__(self, loose=None):
        self.loose = loose or {}                 # {symbol: argument positions recorded without their bytes}
        self.seen = {}                           # data address -> [weak reference to the array that owns the memory,
                                                 # (call, argument) first resolved in, dtype, byte count]
        self.calls = []

    def __enter__(self):
        self.real = _lib.load()
        self.saved = (_lib._p, _lib._lib)
        real_p = self.saved[0]

        def p(a, t):
            if a is not None:
                owner = a
                while isinstance(owner.base, np.ndarray):    # a view such as tips.reshape(-1) may go; its memory's owner may not
                    owner = owner.base
                ent = self.seen.get(a.ctypes.data)
                if ent is None or ent[0]() is not owner or ent[2:] != [a.dtype, a.nbytes]:
                    self.seen[a.ctypes.data] = [weakref.ref(owner), None, a.dtype, a.nbytes]
            return real_p(a, t)

        _lib._p, _lib._lib = p, _Proxy(self)
        return self

    def __exit__(self, *exc):
        _lib._p, _lib._lib = self.saved
        return False

    # ---- arguments ----------------------------------------------------------------------------------------------------------
    def _resolve(self, ptr, where, data=True):
        if not ptr:
            return None
        ent = self.seen.get(_addr(ptr))
        assert ent is not None, f"{where}: a pointer that did not go through _lib._p"
        assert ent[0]() is not None, f"{where}: the array behind this pointer was freed before the call"
        if ent[1] is None:
            ent[1] = where
        rec = {"dtype": ent[2].str, "nbytes": int(ent[3])}
        if data:
            rec["sha256"] = hashlib.sha256(C.string_at(_addr(ptr), ent[3])).hexdigest()
        return rec

    def _tree(self, t, where):
        return {"counts": [t.n_tips, t.n_node, t.n_edge],
                "pointers": [self._resolve(getattr(t, f), where) for f in ("edge", "edge_length", "states", "map_off", "maps", "mapnames")]}

    def _arg(self, a, where):
        if a is None or isinstance(a, (int, float)):
            return a
        if isinstance(a, np.generic):
            return a.item()
        obj = getattr(a, "_obj", a)              # byref(x) -> x
        if isinstance(obj, (_lib.Options, _lib.DebugOptions)):
            return {"struct": type(obj).__name__, "bytes": bytes(obj).hex()}
        if isinstance(obj, _lib.Tree):
            return self._tree(obj, where)
        if isinstance(obj, C.Array) and obj._type_ is _lib.Tree:
            return [self._tree(t, where) for t in obj]
        if isinstance(obj, _lib.Model):
            return {"model": [obj.n_states, obj.Omega, obj.variant], "pointers": [self._resolve(getattr(obj, f), where) for f in ("Q", "pid", "B")]}
        if isinstance(obj, C._Pointer):
            return self._resolve(obj, where)
        if isinstance(obj, C.c_void_p) and obj is a:
            return {"handle": obj.value}
        return {"out": type(obj).__name__}     # byref of a scalar or struct the library fills

    def record(self, name, args):
        k = len(self.calls)
        loose = self.loose.get(name, ())
        recs, i = [], 0
        while i < len(args):
            a = args[i]
            ent = self.seen.get(_addr(a)) if isinstance(a, C._Pointer) and a else None
            if ent is not None and ent[2] == np.int64:                     # the maps tail: offsets, capacity, dwell, state
                off, cap = np.ctypeslib.as_array(a, (ent[3] // 8,)), args[i + 1]
                recs += [self._resolve(a, (k, i)), cap] + [self._resolve(b, (k, i + 2 + j), data=False) for j, b in enumerate(args[i + 2:i + 4])]
                if cap == 0:
                    off[:] = 2 * np.arange(off.size)
                i += 4
                continue
            recs.append(self._resolve(a, (k, i), data=False) if i in loose else self._arg(a, (k, i)))
            i += 1
        self.calls.append([name, recs])

    # ---- results ------------------------------------------------------------------------------------------------------------
    def result(self, r):
        if isinstance(r, np.ndarray):
            rec = {"shape": list(r.shape), "strides": list(r.strides), "dtype": r.dtype.str}
            lo = r.ctypes.data
            for base, (ref, where, _, nbytes) in self.seen.items():
                if ref() is not None and where is not None and base <= lo and lo + max(r.nbytes, 1) <= base + max(nbytes, 1) and nbytes:
                    return dict(rec, offset=lo - base, buffer=list(where))
            return dict(rec, sha256=hashlib.sha256(np.ascontiguousarray(r).tobytes()).hexdigest())
        if isinstance(r, tuple) and hasattr(r, "_fields"):
            return {f: self.result(v) for f, v in zip(r._fields, r)}
        if isinstance(r, (tuple, list)):
            return [self.result(v) for v in r]
        if isinstance(r, dict):
            return {k: self.result(v) for k, v in r.items()}
        if isinstance(r, (_lib.Options, _lib.DebugOptions)):
            return {"struct": type(r).__name__, "bytes": bytes(r).hex()}
        if r is None or isinstance(r, (bool, int, float, str)):
            return r
        if isinstance(r, np.generic):
            return r.item()
        if hasattr(r, "off") and hasattr(r, "dwell"):                      # maps.Maps
            return {"off": self.result(r.off), "dwell": self.result(r.dwell), "state": self.result(r.state), "n_edge": r.n_edge}
        return {"object": type(r).__name__}


class _Proxy:
    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        real = getattr(self._rec.real, name)
        if name in PASS:
            return real

        def call(*args):
            self._rec.record(name, args)
            return real(*args) if name == "phm_set_debug_options" else 0

        return call


def argtypes():
    """{symbol: [names of the argtypes (None: never set), name of the restype]} of the loaded library"""
    L = _lib.load()
    fns = {name: getattr(L, name) for name in _lib.EXPORTS}
    return {name: [None if f.argtypes is None else [t.__name__ for t in f.argtypes], getattr(f.restype, "__name__", None)]
            for name, f in fns.items()}


def record(fn, loose=None):
    """{"calls": [[symbol, [argument records]], ...], "result": ...} of one case"""
    try:
        with Recorder(loose) as r:
            return {"calls": r.calls, "result": r.result(fn())}
    finally:
        _lib.set_debug_options()                 # the cases' debug keywords reached the real library


# ---- the inputs: fixed numbers only ------------------------------------------------------------------------------------------
Z6 = mm.z_of(np.array([1, 2, 0, 3, 1, 2], dtype=np.int32))
SITES6 = np.array([[1, 2, 0, 3, 1, 2], [2, 2, 1, 0, 3, 1], [3, 1, 1, 2, 0, 2]], dtype=np.int32)
OBS3 = [1, 2, 1]
PTS = ([0, 4, 9], [0.0, 0.45, 0.125])


def Q_of(n, scale=1.0):
    """a fixed non-symmetric rate matrix in exact binary fractions"""
    Q = np.array([[((3 * i + 5 * j) % 7 + 1) / 16.0 for j in range(n)] for i in range(n)]) * scale
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q


def Qs_of(n, k):
    return np.stack([Q_of(n, 1.0 + 0.25 * m) for m in range(k)])


def pid_of(n, k=None):
    return (np.arange(1, n + 1) / 8.0) if k is None else np.stack([np.arange(1, n + 1) / 8.0 + m / 4.0 for m in range(k)])


def z8(n, states=None, seed=11):
    """synth.make_tree(8, ...) with fixed tips; the branch lengths rounded to 1e-6 (they come from a logarithm) and the initial
    paths rebuilt from the rounded lengths, so that every byte is the same on every machine"""
    st = np.array([1, 2, 1, 2, 2, 1, 1, 2], dtype=np.int32) if states is None else np.asarray(states, dtype=np.int32)
    z = synth.make_tree(8, Q_of(n), 2.0, seed, states=st)
    lens = np.round(z["edge.length"], 6)
    return dict(z, **{"edge.length": lens, "maps": [synth.initial_path(float(t), int(mn[-1]))[0] for t, mn in zip(lens, z["mapnames"])]})


Q4 = synth.make2sQ(0.125, 0.25, 0.5, 0.375, 2.0)                          # hidden rates, k = 1: 4 states
OMEGA = 2.0
SITES8 = np.array([[1, 2, 1, 2, 2, 1, 1, 2], [2, 2, 1, 1, 2, 1, 2, 1]], dtype=np.int32)
EIG3 = (np.array([[1.0, 0.5, 0.25], [1.0, -0.5, 0.125], [1.0, 0.25, -0.75]]), np.array([[0.5, 0.25, 0.25], [1.0, -1.0, 0.0], [0.5, 0.5, -1.0]]),
        np.diag([0.0, -0.75, -1.5]))


def _cases():
    out = {}

    def case(name, fn, loose=None):
        assert name not in out
        out[name] = (fn, loose)

    sweeps = [("mcmc", api.sumstatMCMC, 2), ("bigtree", api.sumstatMCMC_bigtree, 3), ("sparse", api.SPARSEsumstatMCMC, 3),
              ("ks_sweep", api.sumstatMCMCks_sweep, 4), ("bf_sweep", api.sumstatMCMCbf_sweep, 2)]
    for tag, fn, n in sweeps:
        Q = Q4 if n == 4 else Q_of(n)
        base = lambda fn=fn, n=n, Q=Q, **kw: fn(z8(n), Q, pid_of(n), OMEGA, 3, seed=5, **kw)
        case(f"{tag}_one_chain", base)
        case(f"{tag}_replicas", lambda base=base: base(n_replicas=2))
        case(f"{tag}_reduce", lambda base=base: base(n_replicas=2, reduce=True))
        case(f"{tag}_sites", lambda base=base: base(sites=SITES8))
        case(f"{tag}_maps_all", lambda base=base: base(n_replicas=2, maps=True))
        case(f"{tag}_maps_iters", lambda base=base: base(n_replicas=2, maps=True, map_iters=[0, 2]))
    prior2, prior8 = [1.0, 2.0, 1.5, 0.5], [1.0, 2.0, 1.5, 0.5, 2.0, 1.0, 3.0, 0.25]
    case("bf", lambda: api.sumstatMCMCbf(z8(2), Q_of(2), pid_of(2), OMEGA, 3, prior2, seed=6))
    case("ks", lambda: api.sumstatMCMCks(z8(4), Q4, pid_of(4), OMEGA, 3, prior8, seed=6))
    case("dic2s", lambda: api.sumstatMCMC2sDICt(z8(2), Q_of(2), pid_of(2), OMEGA, 3, prior2, seed=6))
    case("ksdic", lambda: api.sumstatMCMCksDICt(z8(4), Q4, pid_of(4), OMEGA, 3, prior8, seed=6))
    case("mt", lambda: api.sumstatMCMCmt([z8(2), z8(2, seed=12), z8(2, seed=13)], Q_of(2), pid_of(2), OMEGA, 3, prior2, seed=6))
    case("ksmt", lambda: api.sumstatMCMCksmt([z8(4), z8(4, seed=12)], Q4, pid_of(4), OMEGA, 3, prior8, seed=6))

    Qsym = np.array([[-0.75, 0.5, 0.25], [0.5, -0.625, 0.125], [0.25, 0.125, -0.375]])      # a real spectrum
    case("exp_plain", lambda: api.sumstatEXP(z8(3), Qsym, pid_of(3), 4, seed=3), loose={"phm_maketreelistEXP": (8, 9, 10)})
    case("exp_eig", lambda: api.sumstatEXP(z8(3), Q_of(3), pid_of(3), 4, eig=EIG3, seed=3))
    case("exp_maps", lambda: api.sumstatEXP(z8(3), Q_of(3), pid_of(3), 4, eig=EIG3, maps=True, seed=3))
    for mfma in (False, True):
        case(f"expm_eigen_mfma{int(mfma)}", lambda m=mfma: api.expm_eigen(*EIG3, [0.25, 0.5, 2.0], device=0, mfma=m))
        case(f"expm_pade_mfma{int(mfma)}", lambda m=mfma: api.expm_pade(Q_of(3), [0.25, 0.5, 2.0], mfma=m))

    case("simulate", lambda: api.simulate_histories(Z6, Q_of(3), pid_of(3), 5, seed=9))
    case("simulate_observe", lambda: api.simulate_histories(Z6, Q_of(3), pid_of(3), 5, observe=OBS3, replica_offset=4))
    case("simulate_nodes", lambda: api.simulate_histories(Z6, Q_of(3), pid_of(3), 5, nodes=True))
    case("simulate_maps", lambda: api.simulate_histories(Z6, Q_of(3), pid_of(3), 5, nodes=True, maps=True))
    sm = api.simulate_histories_models
    case("simulate_models_2d", lambda: sm(Z6, Q_of(3), pid_of(3), 4, seed=9))
    case("simulate_models_3d", lambda: sm(Z6, Qs_of(3, 5), pid_of(3), 4, observe=OBS3))
    case("simulate_models_pid_per_model", lambda: sm(Z6, Qs_of(3, 5), pid_of(3, 5), 4))
    case("simulate_models_nodes", lambda: sm(Z6, Qs_of(3, 5), pid_of(3, 5), 4, nodes=True))
    case("simulate_models_maps", lambda: sm(Z6, Qs_of(3, 5), pid_of(3), 4, nodes=True, maps=True))

    es = api.expected_sumstat
    case("expected_replicas", lambda: es(Z6, Q_of(3), pid_of(3), n_replicas=3))
    case("expected_sites", lambda: es(Z6, Q_of(3), pid_of(3), sites=SITES6, observe=OBS3))
    case("expected_per_branch", lambda: es(Z6, Q_of(3), pid_of(3), sites=SITES6, per_branch=True))
    case("expected_nodes", lambda: es(Z6, Q_of(3), pid_of(3), sites=SITES6, per_branch=True, nodes=True, devices=2))
    et = api.expected_through_time
    case("time_no_bounds", lambda: et(Z6, Q_of(3), pid_of(3), sites=SITES6))
    case("time_one_bound", lambda: et(Z6, Q_of(3), pid_of(3), bounds=[0.25], sites=SITES6))
    case("time_three_bounds", lambda: et(Z6, Q_of(3), pid_of(3), bounds=[0.0, 0.25, 0.75], observe=OBS3))
    case("time_points", lambda: et(Z6, Q_of(3), pid_of(3), bounds=[0.0, 0.5], points=PTS, sites=SITES6))

    som = [2, 0, 1, 1, 0]
    many = [("loglik", api.loglik_models, {}), ("expected", api.expected_sumstat_models, {}),
            ("sample", lambda z, Qs, pid, **kw: api.sample_histories(z, Qs, pid, 3, **kw), {"seed": 8}),
            ("sample_nodes_maps", lambda z, Qs, pid, **kw: api.sample_histories(z, Qs, pid, 3, nodes=True, maps=True, **kw), {}),
            ("ancestral", api.ancestral_states_models, {})]
    for tag, fn, kw in many:
        for mode, s in (("cross", None), ("paired", som)):
            for ptag, pid in (("shared", pid_of(3)), ("per_model", pid_of(3, 5))):
                case(f"{tag}_{mode}_pid_{ptag}", lambda fn=fn, s=s, pid=pid, kw=kw: fn(Z6, Qs_of(3, 5), pid, sites=SITES6, observe=OBS3, site_of_model=s, **kw))
    case("loglik_one_matrix_no_sites", lambda: api.loglik_models(Z6, Q_of(3), pid_of(3)))
    anc = api.ancestral_states_models
    case("ancestral_node_subset", lambda: anc(Z6, Qs_of(3, 5), pid_of(3), sites=SITES6, nodes=mm.NODE_SEL))
    case("ancestral_no_marginal", lambda: anc(Z6, Qs_of(3, 5), pid_of(3), sites=SITES6, marginal=False))
    case("ancestral_no_joint", lambda: anc(Z6, Qs_of(3, 5), pid_of(3), sites=SITES6, site_of_model=som, joint=False))
    case("ancestral_wide", lambda: anc(Z6, Qs_of(9, 2), pid_of(9), sites=SITES6, nodes=mm.NODE_SEL))

    m3 = ratemodel.sym(3)
    pr = api.posterior_rates
    th_joint = (np.arange(4 * m3.p).reshape(4, m3.p) + 1) / 16.0
    th_site = (np.arange(6 * m3.p).reshape(6, m3.p) + 1) / 16.0
    prior_p = np.array([[1.5, 2.0], [1.0, 0.5], [2.0, 1.0]])
    loose = {"phm_gibbs_rates": (5,)}
    case("gibbs_joint_default_theta0", lambda: pr(Z6, m3, pid_of(3), [1.5, 2.0], 5, sites=SITES6[:2], seed=7), loose=loose)
    case("gibbs_per_site_default_theta0", lambda: pr(Z6, m3, pid_of(3), prior_p, 5, chains=2, sites=SITES6, per_site=True, thin=2), loose=loose)
    case("gibbs_joint_theta0", lambda: pr(Z6, m3, pid_of(3), prior_p, 5, sites=SITES6[:2], observe=OBS3, theta0=th_joint, theta_max=20.0))
    case("gibbs_per_site_theta0", lambda: pr(Z6, m3, pid_of(3, 6), np.tile(prior_p, (6, 1, 1)), 5, chains=2, sites=SITES6, per_site=True,
                                             theta0=th_site, theta_max=20.0))
    case("gibbs_no_stats", lambda: pr(Z6, m3, pid_of(3, 4), prior_p, 4, theta0=th_joint, theta_max=20.0, stats=False))

    case("options_devices_int", lambda: _lib.make_options(seed=3, n_replicas=4, devices=2))
    case("options_devices_list", lambda: _lib.make_options(mapping="tiles", rescale=True, recover=False, devices=[1, 0]))
    case("options_debug", lambda: _lib.make_options(seed=(1 << 40) + 5, cap_tail=0.5, expect_chunk=2))

    def engine(z, n, Q, variant, reduce, **kw):
        e = _lib.Engine(z, Q, pid_of(n), OMEGA, 6, variant=variant, n_replicas=2, reduce=reduce, seed=4, **kw)
        return {"cols": e.cols, "S": e.S, "stats": e.stats(1, 3), "dump": e.dump(replica=1, seg_cap=16)}

    case("engine_one_tree", lambda: engine(z8(3), 3, Q_of(3), _lib.PHM_MCMC, False))
    case("engine_one_tree_reduced", lambda: engine(z8(4), 4, Q4, _lib.PHM_MCMC_KS, True, B=np.eye(4) + Q4 / OMEGA))
    case("engine_tree_list", lambda: engine([z8(2), z8(2, seed=12)], 2, Q_of(2), _lib.PHM_MCMC_MT, False))
    case("engine_states", lambda: engine(z8(2), 2, Q_of(2), _lib.PHM_MCMC_BF, True, states=SITES8, tips_per_replica=True))
    return out


CASES = _cases()


def run(name):
    fn, loose = CASES[name]
    return record(fn, loose)


# ---- one refusal per shared helper: the parent's messages ---------------------------------------------------------------------
REFUSALS = {
    "Qs_rank": lambda: api.loglik_models(Z6, np.zeros((2, 2, 3, 3)), pid_of(3)),
    "Qs_not_square": lambda: api.sample_histories(Z6, np.zeros((2, 3, 4)), pid_of(3), 2),
    "pid_length": lambda: api.expected_sumstat_models(Z6, Qs_of(3, 5), pid_of(4)),
    "pid_rows": lambda: api.simulate_histories_models(Z6, Qs_of(3, 5), pid_of(3, 2), 2),
    "pid_rows_chains": lambda: api.posterior_rates(Z6, ratemodel.sym(3), pid_of(3, 3), [1.5, 2.0], 3),
    "site_of_model_length": lambda: api.ancestral_states_models(Z6, Qs_of(3, 5), pid_of(3), sites=SITES6, site_of_model=[0, 1]),
    "observe_length": lambda: api.expected_sumstat(Z6, Q_of(3), pid_of(3), observe=[1, 2]),
    "observe_length_simulate": lambda: api.simulate_histories(Z6, Q_of(3), pid_of(3), 2, observe=[1, 2, 1, 2]),
    "tip_columns": lambda: api.loglik_models(Z6, Qs_of(3, 5), pid_of(3), sites=SITES8),
}


def refusal(name):
    """[exception type, message] of one refused call; nothing may reach the library"""
    with Recorder() as r:
        try:
            REFUSALS[name]()
        except Exception as e:
            assert not [c for c in r.calls if c[0] != "phm_set_debug_options"], r.calls
            return [type(e).__name__, str(e)]
    raise AssertionError(f"{name}: the call was not refused")
