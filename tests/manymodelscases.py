"""The small many-model calls whose outputs tests/golden/many_models/parent.npz pins bit for bit (recorded by
tests/golden/many_models/make_golden.py from the commit before the shared host core of DESIGN.md section 17, compared by
tests/test_gpu_many_models_parent.py).  Shared by the recorder and the test so that both make the same calls.

The tree is a fixed unbalanced 6-tip tree with unequal branch lengths: height levels of 2, 1, 1 and 1 nodes, depth levels of
1, 2, 1 and 1.  K = 70 models are one full wave and a ragged one; expect_chunk = 2 gives two chunks of models, chunks of 2 + 1
sites and two edges per Pade launch at 5 states.  The tips of the last site hold a state that ``observe`` never shows, and
model 7 has every rate zero (P = I)."""
import hashlib

import numpy as np

from phylomap_amd import api, ratemodel

EDGE = np.array([[7, 8], [8, 1], [8, 2], [7, 9], [9, 3], [9, 10], [10, 4], [10, 11], [11, 5], [11, 6]], dtype=np.int32)
LENS = np.array([0.31, 0.12, 0.47, 0.08, 0.9, 0.23, 0.55, 0.17, 0.05, 0.64])
T, NT = 6, 11
K, S = 70, 3
NODE_SEL = [9, 2, 11, 7, 4]                             # a subset, not ascending: internal nodes, tips and the root
OBSERVE = {3: [1, 2, 1], 5: [1, 2, 1, 2, 4], 9: None}  # 3 states: nothing shows as 3; 5 states: nothing shows as 3 or 5
WHOLE = 32 << 10                                        # bytes: larger arrays are pinned by the SHA-256 of their bytes


def z_of(states=None):
    return {"edge": EDGE, "edge.length": LENS, "Nnode": T - 1, "states": np.ones(T, dtype=np.int32) if states is None else states}


def models(n, k, zero=True):
    """k non-symmetric rate matrices and a root prior per model"""
    rs = np.random.default_rng(100 + n)
    Qs = rs.uniform(0.05, 1.0, (k, n, n))
    for Q in Qs:
        np.fill_diagonal(Q, 0.0)
        np.fill_diagonal(Q, -Q.sum(axis=1))
    if zero and k > 7:
        Qs[7] = 0.0
    pid = rs.uniform(0.5, 1.5, (k, n))
    return Qs, pid


def sites(n, s, impossible=True):
    """s tip sets in what ``observe`` can show, a few tips missing; the last one impossible when asked"""
    rs = np.random.default_rng(200 + n)
    seen = sorted(set(OBSERVE[n])) if OBSERVE[n] else list(range(1, n + 1))
    tips = rs.choice(seen, (s, T)).astype(np.int32)
    tips[rs.random(tips.shape) < 0.15] = 0
    if impossible:
        tips[s - 1, 3] = 3
    return tips


def owner(k, s):
    """a shuffled site_of_model that names every site"""
    return np.random.default_rng(300 + k).permutation(np.arange(k) % s).astype(np.int32)


def _opt(chunk):
    return {"expect_chunk": chunk} if chunk else {}


def _loglik(n, paired, chunk):
    Qs, pid = models(n, K)
    som = owner(K, S) if paired else None
    return {"loglik": api.loglik_models(z_of(), Qs, pid, sites=sites(n, S), observe=OBSERVE[n], site_of_model=som, **_opt(chunk))}


def _expected(n, paired, chunk):
    Qs, pid = models(n, K)
    som = owner(K, S) if paired else None
    st, ll = api.expected_sumstat_models(z_of(), Qs, pid, sites=sites(n, S), observe=OBSERVE[n], site_of_model=som, **_opt(chunk))
    return {"stats": st, "loglik": ll}


def _ancestral(n, k, paired, chunk):
    Qs, pid = models(n, k)
    som = owner(k, S) if paired else None
    r = api.ancestral_states_models(z_of(), Qs, pid, sites=sites(n, S), observe=OBSERVE[n], site_of_model=som, nodes=NODE_SEL,
                                    **_opt(chunk))
    return {"loglik": r.loglik, "node_post": r.node_post, "joint_states": r.joint_states, "joint_logp": r.joint_logp}


def _sample(n, chunk):
    Qs, pid = models(n, K, zero=False)
    st, ll, nodes = api.sample_histories(z_of(), Qs, pid, 70, sites=sites(n, 2, impossible=False), observe=OBSERVE[n], nodes=True,
                                         seed=1234, **_opt(chunk))
    return {"stats": st, "loglik": ll, "nodes": nodes}


def _gibbs(joint):
    m = ratemodel.sym(3)
    rs = np.random.default_rng(400)
    th0 = rs.uniform(0.1, 1.5, (70, m.p))
    r = api.posterior_rates(z_of(), m, np.full(3, 1.0 / 3), np.tile([1.5, 2.0], (m.p, 1)), 4, chains=70 if joint else 35,
                            sites=sites(3, 2, impossible=False), observe=OBSERVE[3], per_site=not joint, theta0=th0, theta_max=20.0,
                            thin=2, seed=77)
    return {k: r[k] for k in ("theta", "loglik", "stats", "rejected", "status")}


def _single():
    Qs, pid = models(3, 1)
    st, ll, post = api.expected_sumstat(z_of(), Qs[0], pid[0], sites=sites(3, 70, impossible=False), observe=OBSERVE[3], nodes=True)
    return {"stats": st, "loglik": ll, "nodes": post}


def _cases():
    out = []
    for n in (3, 5):
        for paired in (False, True):
            for chunk in (0, 2):
                tag = f"n{n}_{'paired' if paired else 'cross'}_chunk{chunk}"
                out.append((f"loglik_{tag}", lambda n=n, p=paired, c=chunk: _loglik(n, p, c)))
                out.append((f"expected_{tag}", lambda n=n, p=paired, c=chunk: _expected(n, p, c)))
                out.append((f"ancestral_{tag}", lambda n=n, p=paired, c=chunk: _ancestral(n, K, p, c)))
        for chunk in (0, 2):
            out.append((f"sample_n{n}_chunk{chunk}", lambda n=n, c=chunk: _sample(n, c)))
    for paired in (False, True):
        for chunk in (0, 2):
            out.append((f"ancestral_wide_{'paired' if paired else 'cross'}_chunk{chunk}", lambda p=paired, c=chunk: _ancestral(9, 3, p, c)))
    out.append(("gibbs_joint", lambda: _gibbs(True)))
    out.append(("gibbs_per_site", lambda: _gibbs(False)))
    out.append(("expected_sumstat_single", _single))
    return out


CASES = dict(_cases())


def pinned(a):
    """what the golden file holds of an output array: the array itself, or, above WHOLE bytes, its shape and the SHA-256 of its
    bytes (equal digests: equal bytes, NaN and -inf included); compared as bytes either way"""
    a = np.ascontiguousarray(a)
    if a.nbytes <= WHOLE:
        return a
    return np.concatenate([np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8),
                           np.frombuffer(np.array(a.shape, dtype=np.int64).tobytes(), dtype=np.uint8)])


def run(name):
    """{golden key: pinned array} of one case"""
    return {f"{name}.{k}": pinned(v) for k, v in CASES[name]().items()}
