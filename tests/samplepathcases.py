"""The small calls of the exact samplers and of the wide ancestral pass whose outputs tests/golden/sample_paths/parent.npz pins bit
for bit (recorded by tests/golden/sample_paths/make_golden.py from the commit before the two samplers got their one branch draw,
tile driver and wide device state -- DESIGN.md sections 19a, 19b and 23a --, compared by tests/test_gpu_sample_parent.py).  Shared
by the recorder and the test so that both make the same calls.  TEST INFRASTRUCTURE ONLY.

They cover what tests/golden/many_models and tests/golden/history_producers do not: the wide sampler at one state count per lane
class of the tree passes and at the LDS maximum, the wide ancestral pass at 33 states, and the narrow sampler with maps at 2, 4
(compile-time forms) and 8 states (run-time form) on this tree.  The tree is manymodelscases' 6-tip unbalanced one.  D = 70 draws:
the second tile of an evaluation has 6 live lanes.  Every input is built from integer-seeded generators and element-wise
arithmetic; no linear-algebra call and no simulation enters the recorded bytes.

Wide models (K = 3): 0 an ordinary one, 1 block-diagonal (states 1 .. n/2 and the rest never meet), 2 every rate zero.  Sites
(S = 2): 0 shows one state of the first block (possible under all three), 1 shows states of both blocks, so that it is impossible
under models 1 and 2.  Paired, the models own sites 1, 1 and 0: one impossible evaluation, two finite ones."""
import numpy as np

from manymodelscases import EDGE, LENS, NODE_SEL, T, pinned, z_of
from phylomap_amd import api

D = 70
WIDE_NS = (9, 17, 33, 64)                               # lane classes 16, 32, 64 of the tree passes, and the LDS maximum
NARROW_NS = (2, 4, 8)
WIDE_OWNER = np.array([1, 1, 0], dtype=np.int32)
NARROW_K = 70                                           # one full wave of models and a ragged one; model 7 has every rate zero
LONG = int(np.argmax(LENS))                             # the branch that the deep case stretches to mu t = 400


def wide_models(n):
    rs = np.random.default_rng(1100 + n)
    Qs = rs.uniform(0.05, 1.0, (3, n, n)) * (4.0 / n)
    h = n // 2
    Qs[1, :h, h:] = 0.0
    Qs[1, h:, :h] = 0.0
    Qs[2] = 0.0
    for Q in Qs:
        np.fill_diagonal(Q, 0.0)
        np.fill_diagonal(Q, -Q.sum(axis=1))
    return Qs, rs.uniform(0.5, 1.5, (3, n))


def wide_sites(n):
    rs = np.random.default_rng(1200 + n)
    tips = np.empty((2, T), dtype=np.int32)
    tips[0] = 2
    tips[0, 2] = 0                                      # a missing tip
    tips[1] = rs.integers(1, n + 1, T)
    tips[1, 0], tips[1, 1], tips[1, 4] = 1, n, 0        # both blocks, and a missing tip
    return tips


def narrow_models(n):
    rs = np.random.default_rng(1300 + n)
    Qs = rs.uniform(0.05, 1.0, (NARROW_K, n, n))
    Qs[7] = 0.0
    for Q in Qs:
        np.fill_diagonal(Q, 0.0)
        np.fill_diagonal(Q, -Q.sum(axis=1))
    return Qs, rs.uniform(0.5, 1.5, (NARROW_K, n))


def narrow_sites(n):
    rs = np.random.default_rng(1400 + n)
    tips = rs.integers(1, n + 1, (2, T)).astype(np.int32)
    tips[rs.random(tips.shape) < 0.15] = 0
    tips[1, 0], tips[1, 1] = 1, 2                       # two states: impossible under the model without rates
    return tips


def _opt(chunk):
    return {"expect_chunk": chunk} if chunk else {}


def _out(r, maps):
    out = {"stats": r[0], "loglik": r[1], "nodes": r[2]}
    if maps:
        out.update({"map_off": r[3].off, "map_dwell": r[3].dwell, "map_state": r[3].state})
    return out


def _wide(n, paired, chunk, maps=True, deep=False):
    Qs, pid = wide_models(n)
    lens = LENS.copy()
    if deep:
        lens[LONG] = 400.0 / float(np.max(-np.diag(Qs[0])))
    z = dict(z_of(), **{"edge.length": lens})
    r = api.sample_histories(z, Qs, pid, D, sites=wide_sites(n), site_of_model=WIDE_OWNER if paired else None, nodes=True, maps=maps,
                             seed=5000 + n, **_opt(chunk))
    return _out(r, maps)


def _narrow(n, chunk):
    Qs, pid = narrow_models(n)
    r = api.sample_histories(z_of(), Qs, pid, D, sites=narrow_sites(n), nodes=True, maps=True, seed=6000 + n, **_opt(chunk))
    return _out(r, True)


def _ancestral(paired, chunk):
    Qs, pid = wide_models(33)
    r = api.ancestral_states_models(z_of(), Qs, pid, sites=wide_sites(33), site_of_model=WIDE_OWNER if paired else None, nodes=NODE_SEL,
                                    **_opt(chunk))
    return {"loglik": r.loglik, "node_post": r.node_post, "joint_states": r.joint_states, "joint_logp": r.joint_logp}


def _cases():
    out = []
    for n in WIDE_NS:
        for paired in (False, True):
            for chunk in (0, 1):
                out.append((f"wide_n{n}_{'paired' if paired else 'cross'}_chunk{chunk}", lambda n=n, p=paired, c=chunk: _wide(n, p, c)))
    out.append(("wide_n9_cross_nomaps", lambda: _wide(9, False, 0, maps=False)))
    out.append(("wide_n9_deep", lambda: _wide(9, False, 0, deep=True)))
    for paired in (False, True):
        for chunk in (0, 2):
            out.append((f"ancestral_n33_{'paired' if paired else 'cross'}_chunk{chunk}", lambda p=paired, c=chunk: _ancestral(p, c)))
    for n in NARROW_NS:
        for chunk in (0, 2):
            out.append((f"narrow_n{n}_chunk{chunk}", lambda n=n, c=chunk: _narrow(n, c)))
    return out


CASES = dict(_cases())
E = EDGE.shape[0]


def most_changes_on_a_branch(out):
    """the largest number of changes of state that a history of the case has on one branch (segments of the map row - 1)"""
    return int(np.max(np.diff(out["map_off"]))) - 1


def raw(name):
    return CASES[name]()


def pin(name, out):
    """{golden key: pinned array} of one case's outputs"""
    return {f"{name}.{k}": pinned(v) for k, v in out.items()}


def run(name):
    return pin(name, raw(name))
