"""The seeded grid of cases on which the oracle's R-stream mode is pinned against the reference's own C++ (tests/ref_lib.py), and
the runners of both sides.  Shared by tests/test_reference_pin_cpu.py and tests/golden/make_ref_golden.py.

A case is a dict: ``driver`` (one of DRIVERS), ``n``, ``Q``, ``pid``, ``Omega``, ``B``, ``N``, ``seed``, ``prior`` (or None), and
either ``z`` (one tree with ``nen`` / ``nodelist`` / ``root``) or ``trees`` (a list, with ``nen_m`` / ``nodelist_m`` / ``roots``).
``expect`` names what both sides must report: "ok", "zero_prob" or "unif_cap" (tests/test_reference_pin_cpu.py::compare)."""
from __future__ import annotations

import numpy as np

import oracle_lib as O
from phylomap_amd import api, synth, treeorder

DRIVERS = ("mcmc", "bigtree", "sparse", "exp", "bf", "ks", "mt", "ksmt", "bfdic", "ksdic")
_VARIANT = {"mcmc": O.PLAIN, "bigtree": O.BIGTREE, "sparse": O.SPARSE, "bf": O.BF, "ks": O.KS, "mt": O.MT, "ksmt": O.KSMT,
            "bfdic": O.BF, "ksdic": O.KS}


# ---- rate matrices --------------------------------------------------------------------------------------------------------------
def dense_rates(n, seed):
    """Asymmetric dense Q (every B entry positive): the MCMC drivers."""
    if n == 2:
        return np.array([[-0.1, 0.1], [0.15, -0.15]])
    return synth.dense_Q(n, 0.01, 0.05, seed=0xC0FFEE + seed)


def symmetric_rates(n, seed):
    """Symmetric dense Q (real spectrum, as matexp needs): the EXP driver."""
    Q = dense_rates(n, seed)
    if n > 2:
        Q = (Q + Q.T) / 2
        np.fill_diagonal(Q, 0.0)
        np.fill_diagonal(Q, -Q.sum(axis=1))
    return Q


def hidden_rates(n):
    k = n // 2 - 1
    return synth.make2sQ(0.1, 0.12, [0.2 + 0.01 * i for i in range(k)], [0.25 - 0.01 * i for i in range(k)], [3.0 + i for i in range(k)])


# ---- trees ----------------------------------------------------------------------------------------------------------------------
def build_tree(tips, Q, Omega, seed, segs=2, shuffled=False, zero_middle=False, tip_states=None):
    """synth.make_tree with per-branch initial paths: ``segs`` an int, or a list cycled over the branches (a 1 is applied to
    internal branches only; a tip branch gets 2 instead, so that every observed state stays reachable).  ``zero_middle``: three
    segments per branch, the middle one of length zero.  ``shuffled``: the edge rows (and everything stored per row) permuted."""
    z = synth.make_tree(tips, Q, Omega, seed, states=tip_states)
    edge, lens, states = np.asarray(z["edge"]), np.asarray(z["edge.length"]), np.asarray(z["states"])
    E = edge.shape[0]
    maps, names = [], []
    for r in range(E):
        child = int(edge[r, 1])
        end = int(states[child - 1]) if child <= tips else 1
        if zero_middle:
            maps.append(np.array([lens[r] / 2, 0.0, lens[r] / 2]))
            names.append(np.array([1, 2, end], dtype=np.int32))
            continue
        m = segs if isinstance(segs, int) else segs[r % len(segs)]
        if m == 1 and child <= tips:
            m = 2
        a, b = synth.initial_path(float(lens[r]), end, m)
        maps.append(a)
        names.append(b)
    z["maps"], z["mapnames"] = maps, names
    if shuffled:
        perm = np.random.default_rng(seed).permutation(E)
        z["edge"] = edge[perm]
        z["edge.length"] = lens[perm]
        z["maps"] = [maps[i] for i in perm]
        z["mapnames"] = [names[i] for i in perm]
        z["node.states"] = np.asarray(z["node.states"])[perm]
    return z


def _orders(case):
    z = case["z"]
    case["nen"], case["nodelist"], case["root"] = treeorder.pruningwiseedgeorder(z), treeorder.makenodelist(z), treeorder.myreorder(z)
    return case


def _one(name, driver, Q, z, N, seed, Omega, prior=None, B=None, expect="ok", record=False):
    n = Q.shape[0]
    return _orders({"name": name, "driver": driver, "n": n, "Q": Q, "pid": np.full(n, 1.0 / n), "Omega": float(Omega),
                    "B": np.eye(n) + Q / Omega if B is None else B, "z": z, "N": int(N), "seed": int(seed), "prior": prior,
                    "expect": expect, "record": record})


def _many(name, driver, Q, trees, N, seed, Omega, prior, record=False):
    n = Q.shape[0]
    return {"name": name, "driver": driver, "n": n, "Q": Q, "pid": np.full(n, 1.0 / n), "Omega": float(Omega), "B": np.eye(n) + Q / Omega,
            "trees": trees, "nen_m": np.array([treeorder.pruningwiseedgeorder(z) for z in trees], dtype=np.int32),
            "nodelist_m": np.array([treeorder.makenodelist(z) for z in trees], dtype=np.int32).reshape(len(trees), -1),
            "roots": np.array([treeorder.myreorder(z) for z in trees], dtype=np.int32), "N": int(N), "seed": int(seed),
            "prior": prior, "expect": "ok", "record": record}


# tree configurations of the fixed-Q grid: (tag, tips, segs, shuffled, zero_middle, omega_at_max, N for n <= 4, N for n > 4)
_CONFIGS = (
    ("t2", 2, 3, False, False, False, 40, 40),
    ("t3mix", 3, [2, 1, 3, 9], True, False, False, 7, 7),
    ("t16mix", 16, [3, 2, 9, 1, 140, 2], True, False, False, 120, 60),
    ("t60", 60, 2, False, False, False, 300, 100),
    ("t16zero", 16, 3, False, True, False, 25, 25),
    ("t16omega", 16, 3, False, False, True, 50, 50),
    ("t16one", 16, 3, True, False, True, 1, 1),
)
_RECORDED = {"mcmc_n2_t16mix", "mcmc_n3_t3mix", "bigtree_n4_t16zero", "sparse_n4_t16omega", "mcmc_n20_t2", "bigtree_n5_t16mix",
             "sparse_n8_t16one", "sparse_n4_threshold", "exp_n2_t16", "exp_n4_t3", "exp_n20_t2", "exp_n3_cap", "bf_t16mix_lt1", "bf_t3mix_ge1",
             "ks_n4_t16", "ks_n6_t2", "mt_3x12", "ksmt_n4_3x12", "bfdic_t16", "ksdic_n4_t16", "mcmc_n2_zero_prob"}


def cases():
    """The whole grid, in a fixed order."""
    out = []
    seed = 0
    # the three fixed-Q MCMC drivers
    for n in (2, 3, 4, 5, 8, 20):
        for driver in ("mcmc", "bigtree", "sparse"):
            for tag, tips, segs, shuffled, zero, at_max, n_small, n_big in _CONFIGS:
                seed += 1
                Q = dense_rates(n, n)
                top = float(np.max(np.abs(np.diag(Q))))
                Omega = top if at_max else 1.25 * top
                z = build_tree(tips, Q, 1.25 * top, 1000 + seed, segs, shuffled, zero)
                out.append(_one(f"{driver}_n{n}_{tag}", driver, Q, z, n_small if n <= 4 else n_big, seed, Omega))
    # SPARSE: entries of B at and around the 1e-7 threshold of matTospmat (exactly 1e-7 and below are dropped, the next double is kept)
    Q = dense_rates(4, 4)
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    B = np.eye(4) + Q / Omega
    B[0, 2], B[1, 2], B[2, 0], B[3, 1] = 1e-7, np.nextafter(1e-7, 1.0), 0.9e-7, 1.1e-7
    out.append(_one("sparse_n4_threshold", "sparse", Q, build_tree(16, Q, Omega, 77, 3), 80, 77, Omega, B=B))
    # EXP: short and long branches, so that 0 jumps, 1 jump (equal and different ends) and many jumps all occur
    for n in (2, 3, 4, 5, 8, 20):
        for tag, tips, shuffled, N in (("t2", 2, False, 60), ("t3", 3, True, 40), ("t16", 16, True, 120), ("t60", 60, False, 60 if n > 4 else 200)):
            seed += 1
            Q = symmetric_rates(n, n)
            Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
            out.append(_one(f"exp_n{n}_{tag}", "exp", Q, build_tree(tips, Q, Omega, 2000 + seed, 2, shuffled), N, seed, Omega))
    # EXP: the 300-jump cap of newunifSample (rate x time of several hundred on every branch)
    Q = symmetric_rates(3, 3)
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))
    z = build_tree(3, Q, Omega, 88, 2)
    z["edge.length"] = np.asarray(z["edge.length"]) * 0 + 400.0 / float(np.max(np.abs(np.diag(Q))))
    out.append(_one("exp_n3_cap", "exp", Q, z, 3, 88, Omega, expect="unif_cap"))
    # bf (two states, rate updates): priors that take Rf_rgamma through shape < 1 and through shape >= 1
    Q2 = dense_rates(2, 2)
    for ptag, prior in (("lt1", [0.3, 10.0, 0.2, 5.0]), ("ge1", [1.0, 10.0, 2.0, 10.0])):
        for tag, tips, segs, shuffled, zero, at_max, n_small, _ in _CONFIGS:
            seed += 1
            Omega = 0.5 if not at_max else 0.15       # max |q_ii|: a zero on the diagonal of B, and proposals above Omega
            z = build_tree(tips, Q2, 0.5, 3000 + seed, segs, shuffled, zero)
            out.append(_one(f"bf_{tag}_{ptag}", "bf", Q2, z, n_small, seed, Omega, prior=prior))
    # ks (hidden rates, parity-only tips, rate updates)
    for n in (4, 6, 8, 20):
        for tag, tips, segs, shuffled, N in (("t2", 2, 3, False, 5), ("t16", 16, [3, 2, 9, 1, 140, 2], True, 100), ("t60", 60, 2, False, 60)):
            seed += 1
            Q = hidden_rates(n)
            Omega = 1.5 * float(np.max(np.abs(np.diag(Q))))
            z = build_tree(tips, Q, Omega, 4000 + seed, segs, shuffled)
            if n == 20 and tips == 2:
                N = 40       # long enough to meet an exactly tied 20-state draw: test_tie_order_beyond_sixteen_states_is_the_librarys
            out.append(_one(f"ks_n{n}_{tag}", "ks", Q, z, N, seed, Omega, prior=[1.0, 10.0, 2.0, 10.0, 20.0, 2.0]))
    # the multi-tree drivers
    for count, tips, N in ((1, 2, 3), (3, 12, 150), (5, 16, 60)):
        seed += 1
        trees = synth.make_treelist(count, tips, Q2, 0.5, 5000 + seed, init_segments=3)
        out.append(_many(f"mt_{count}x{tips}", "mt", Q2, trees, N, seed, 0.5, [1.0, 10.0, 2.0, 10.0]))
        for n in (4, 6, 8):
            seed += 1
            Q = hidden_rates(n)
            Omega = 1.5 * float(np.max(np.abs(np.diag(Q))))
            trees = synth.make_treelist(count, tips, Q, Omega, 6000 + seed, init_segments=3)
            out.append(_many(f"ksmt_n{n}_{count}x{tips}", "ksmt", Q, trees, N, seed, Omega, [1.0, 10.0, 2.0, 10.0, 2.0, 10.0, 20.0, 2.0]))
    # the DIC pair (sweep + log p(y | Q) by expmat + updates)
    for tag, tips, N in (("t2", 2, 4), ("t16", 16, 60)):
        seed += 1
        out.append(_one(f"bfdic_{tag}", "bfdic", Q2, build_tree(tips, Q2, 0.5, 7000 + seed, 3), N, seed, 0.5, prior=[1.0, 10.0, 2.0, 10.0]))
        for n in (4, 6):
            seed += 1
            Q = hidden_rates(n)
            Omega = 1.5 * float(np.max(np.abs(np.diag(Q))))
            out.append(_one(f"ksdic_n{n}_{tag}", "ksdic", Q, build_tree(tips, Q, Omega, 7000 + seed, 3), N, seed, Omega,
                            prior=[1.0, 10.0, 2.0, 10.0, 20.0, 2.0]))
    # impossible tip data: two sibling tips in different states on one-segment paths (B^0 = I cannot connect them)
    z = build_tree(2, Q2, 0.5, 99, 2, tip_states=[1, 2])
    z["maps"] = [np.array([float(t)]) for t in z["edge.length"]]
    z["mapnames"] = [np.array([int(s)], dtype=np.int32) for s in (z["states"][int(c) - 1] for c in np.asarray(z["edge"])[:, 1])]
    out.append(_one("mcmc_n2_zero_prob", "mcmc", Q2, z, 2, 99, 0.5, expect="zero_prob"))
    for c in out:
        c["record"] = c["name"] in _RECORDED
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names) and _RECORDED <= set(names), sorted(_RECORDED - set(names))
    return out


# ---- columns --------------------------------------------------------------------------------------------------------------------
def real_columns(driver, n):
    """Indices of the real-valued columns (dwell sums, recorded rates and kappas, the DIC log-likelihood); the rest are
    integer-valued (transition counts, root state, tree index)."""
    cols = list(range(n))
    if driver in ("bf", "mt", "bfdic"):
        cols += [n + n * n, n + n * n + 1]
    if driver in ("ks", "ksmt", "ksdic"):
        cols += list(range(n + n * n, n + n * n + 2 + 3 * (n // 2 - 1)))
    return cols


def loglik_column(driver, n):
    """The DIC drivers' last column, log p(y | Q): the one place where the two sides use different logarithms (libm / orc_log)."""
    if driver == "bfdic":
        return n + n * n + 3
    if driver == "ksdic":
        return n + n * n + 2 + 3 * (n // 2 - 1) + 1
    return None


# ---- runners --------------------------------------------------------------------------------------------------------------------
def run_oracle(c, faithful_search=False):
    d, dic = c["driver"], c["driver"] in ("bfdic", "ksdic")
    if d == "exp":
        lefts, rights, dm = api.eigen_decompose(c["Q"])
        return O.maketreelistEXP(c["z"], c["Q"], c["pid"], c["nen"], c["nodelist"], c["root"], c["N"], lefts, rights, dm, seed=c["seed"],
                                 rstream=True, recompute=True, faithful_search=faithful_search)
    if d in ("mt", "ksmt"):
        return O.maketreelistMCMCmt(c["trees"], c["Q"], c["pid"], c["B"], c["Omega"], c["nen_m"], c["nodelist_m"], c["roots"], c["N"],
                                    c["prior"], variant=_VARIANT[d], seed=c["seed"], rstream=True, faithful_search=faithful_search)
    return O.maketreelistMCMC(c["z"], c["Q"], c["pid"], c["B"], c["Omega"], c["nen"], c["nodelist"], c["root"], c["N"], variant=_VARIANT[d],
                              seed=c["seed"], prior=c["prior"], rstream=True, dic=dic, faithful_search=faithful_search)


def run_reference(c):
    import ref_lib as R
    d, dic = c["driver"], c["driver"] in ("bfdic", "ksdic")
    if d == "exp":
        lefts, rights, dm = api.eigen_decompose(c["Q"])
        return R.maketreelistEXP(c["z"], c["Q"], c["pid"], c["nen"], c["nodelist"], c["root"], c["N"], lefts, rights, dm, seed=c["seed"])
    if d in ("mt", "ksmt"):
        return R.maketreelistMCMCmt(c["trees"], c["Q"], c["pid"], c["B"], c["Omega"], c["nen_m"], c["nodelist_m"], c["roots"], c["N"],
                                    c["prior"], variant=_VARIANT[d], seed=c["seed"])
    return R.maketreelistMCMC(c["z"], c["Q"], c["pid"], c["B"], c["Omega"], c["nen"], c["nodelist"], c["root"], c["N"], variant=_VARIANT[d],
                              seed=c["seed"], prior=c["prior"], dic=dic)


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
def _pack_tree(z, prefix):
    lens = np.array([len(m) for m in z["maps"]], dtype=np.int32)
    return {prefix + "edge": np.asarray(z["edge"], dtype=np.int32), prefix + "edge_length": np.asarray(z["edge.length"], dtype=np.float64),
            prefix + "states": np.asarray(z["states"], dtype=np.int32), prefix + "map_len": lens,
            prefix + "maps": np.concatenate([np.asarray(m, dtype=np.float64) for m in z["maps"]]),
            prefix + "mapnames": np.concatenate([np.asarray(m, dtype=np.int32) for m in z["mapnames"]]).astype(np.int32)}


def _unpack_tree(d, prefix):
    off = np.concatenate([[0], np.cumsum(d[prefix + "map_len"])])
    E = d[prefix + "edge"].shape[0]
    return {"edge": d[prefix + "edge"], "Nnode": int(d[prefix + "states"].size - 1), "edge.length": d[prefix + "edge_length"],
            "states": d[prefix + "states"], "maps": [d[prefix + "maps"][off[i]:off[i + 1]] for i in range(E)],
            "mapnames": [d[prefix + "mapnames"][off[i]:off[i + 1]] for i in range(E)], "node.states": np.ones((E, 2), dtype=np.int32)}


def pack_case(c, ref_out, ref_rc):
    """Everything a recorded test needs: the inputs as arrays and the reference's output matrix and status."""
    d = {"driver": np.array(c["driver"]), "expect": np.array(c["expect"]), "Q": c["Q"], "pid": c["pid"], "Omega": np.float64(c["Omega"]),
         "B": c["B"], "N": np.int32(c["N"]), "seed": np.int64(c["seed"]),
         "prior": np.asarray([] if c["prior"] is None else c["prior"], dtype=np.float64),
         "ref_out": np.ascontiguousarray(ref_out), "ref_rc": np.int32(ref_rc)}
    if "trees" in c:
        d["treecount"] = np.int32(len(c["trees"]))
        for j, z in enumerate(c["trees"]):
            d.update(_pack_tree(z, f"t{j}_"))
        d.update(nen_m=c["nen_m"], nodelist_m=c["nodelist_m"], roots=c["roots"])
    else:
        d.update(_pack_tree(c["z"], "t0_"))
        d.update(nen=c["nen"], nodelist=c["nodelist"], root=np.int32(c["root"]))
    return d


def unpack_case(d, name):
    n = d["Q"].shape[0]
    c = {"name": name, "driver": str(d["driver"]), "expect": str(d["expect"]), "n": n, "Q": d["Q"], "pid": d["pid"], "Omega": float(d["Omega"]),
         "B": d["B"], "N": int(d["N"]), "seed": int(d["seed"]), "prior": (list(d["prior"]) if d["prior"].size else None)}
    if "treecount" in d:
        c["trees"] = [_unpack_tree(d, f"t{j}_") for j in range(int(d["treecount"]))]
        c.update(nen_m=d["nen_m"], nodelist_m=d["nodelist_m"], roots=d["roots"])
    else:
        c["z"] = _unpack_tree(d, "t0_")
        c.update(nen=d["nen"], nodelist=d["nodelist"], root=int(d["root"]))
    return c
