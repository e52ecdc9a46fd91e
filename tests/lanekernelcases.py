"""The small one-model-per-lane calls (2 to 8 states) whose outputs tests/golden/lane_kernels/parent.npz pins bit for bit
(recorded by tests/golden/lane_kernels/make_golden.py from the commit before the lane kernels got their shared device pieces,
phm_ll_device.h of DESIGN.md section 17c; compared by tests/test_gpu_lane_kernels_parent.py).  Shared by the recorder and the test so
that both make the same calls.  tests/manymodelscases.py pins 3 and 5 states; these are the other template instantiations of
every lane kernel, and the rate sampler at 2, 4, 5 and 8.

Tree, models, owner and pinned are manymodelscases': the 6-tip tree, K = 70 models (one full wave and a ragged one, model 7
with every rate zero), 3 sites; expect_chunk = 2 gives two chunks of models, chunks of 2 + 1 sites and several launches per
level.  ``observe`` folds the last state onto the first, so no tip shows as state n; a few tips are missing, and one tip of
the last site claims state n, which makes that site impossible under every model."""
import numpy as np

from phylomap_amd import api, ratemodel

from manymodelscases import K, NODE_SEL, S, T, models, owner, pinned, z_of

CHUNK = 2
TREE_N = (2, 4, 6, 7, 8)
GIBBS_N = (2, 4, 5, 8)


def observe(n):
    """state i shows as i, but state n shows as 1"""
    return list(range(1, n)) + [1]


def sites(n, s, impossible=True):
    """s tip sets in what ``observe`` can show (1 .. n-1), a few tips missing; the last one impossible when asked"""
    rs = np.random.default_rng(500 + n)
    tips = rs.integers(1, n, (s, T)).astype(np.int32)
    tips[rs.random(tips.shape) < 0.15] = 0
    tips[0, 1] = tips[s - 1, 0] = 0                     # missing tips at every n, whatever the draw above gave
    if impossible:
        tips[s - 1, 3] = n
    return tips


def _args(n, paired):
    Qs, pid = models(n, K)
    kw = {"sites": sites(n, S), "observe": observe(n), "site_of_model": owner(K, S) if paired else None, "expect_chunk": CHUNK}
    return (z_of(), Qs, pid), kw


def _loglik(n, paired):
    a, kw = _args(n, paired)
    return {"loglik": api.loglik_models(*a, **kw)}


def _expected(n, paired):
    a, kw = _args(n, paired)
    st, ll = api.expected_sumstat_models(*a, **kw)
    return {"stats": st, "loglik": ll}


def _ancestral(n, paired):
    a, kw = _args(n, paired)
    r = api.ancestral_states_models(*a, nodes=NODE_SEL, **kw)
    return {"loglik": r.loglik, "node_post": r.node_post, "joint_states": r.joint_states, "joint_logp": r.joint_logp}


def _sample(n):
    Qs, pid = models(n, K, zero=False)
    st, ll, nodes = api.sample_histories(z_of(), Qs, pid, 70, sites=sites(n, 2, impossible=False), observe=observe(n), nodes=True,
                                         seed=4321, expect_chunk=CHUNK)
    return {"stats": st, "loglik": ll, "nodes": nodes}


def _gibbs(n, joint):
    m = ratemodel.sym(n)
    th0 = np.random.default_rng(600 + n).uniform(0.1, 1.5, (70, m.p))
    r = api.posterior_rates(z_of(), m, np.full(n, 1.0 / n), np.tile([1.5, 2.0], (m.p, 1)), 4, chains=70 if joint else 35,
                            sites=sites(n, 2, impossible=False), observe=observe(n), per_site=not joint, theta0=th0, theta_max=20.0,
                            thin=2, seed=78)
    return {k: r[k] for k in ("theta", "loglik", "stats", "rejected", "status")}


def _cases():
    out = []
    for n in TREE_N:
        for paired in (False, True):
            tag = f"n{n}_{'paired' if paired else 'cross'}"
            out.append((f"loglik_{tag}", lambda n=n, p=paired: _loglik(n, p)))
            out.append((f"expected_{tag}", lambda n=n, p=paired: _expected(n, p)))
            out.append((f"ancestral_{tag}", lambda n=n, p=paired: _ancestral(n, p)))
        out.append((f"sample_n{n}", lambda n=n: _sample(n)))
    for n in GIBBS_N:
        out.append((f"gibbs_joint_n{n}", lambda n=n: _gibbs(n, True)))
        out.append((f"gibbs_per_site_n{n}", lambda n=n: _gibbs(n, False)))
    return out


CASES = dict(_cases())


def run(name):
    """{golden key: pinned array} of one case"""
    return {f"{name}.{k}": pinned(v) for k, v in CASES[name]().items()}
