"""The rate-updating drivers beyond six states, on every mapping, against the oracle ("Dispatch classes under
a changing model").  sumstatMCMCks / sumstatMCMCksDICt / sumstatMCMCksmt are the product paths that hand a live chain a new model
after every sweep (phm_engine_set_model -> upload_model), and upload_model re-decides per model what a 5 .. 64 state engine runs:
band kernels, LDS transition slots, ELLPACK rows, the running-sum and mask tables.  The cases (tests/rateupdatecases.py; pinned
to those rules by tests/test_rate_updates_cpu.py) sit on either side of every such decision, and two of them cross one under the
running chain.

The bar is tests/test_gpu_parity.py::_same(ks=True): bit for bit on the replica mapping; elsewhere counts and root state exact,
dwell sums within 1e-10, derived columns (rates, log-likelihood) within 1e-9, all relative."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import rateupdatecases as RC
from phylomap_amd import _lib, api
from test_gpu_parity import _same

pytestmark = pytest.mark.gpu

N, SEED, PRIOR = RC.N_ITERS, RC.SEED, RC.PRIOR


def _rel(got, want):
    """largest relative difference (0 where both are 0)"""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    den = np.where(want == 0, 1.0, np.abs(want))
    return float(np.max(np.abs(got - want) / den)) if got.size else 0.0


def _bar(got, want, n, mapping, label):
    """print the figures, then the bar"""
    ncnt = n * n
    print(f"[rate-updates] {label} {mapping}: dwell {_rel(got[..., :n], want[..., :n]):.3e} "
          f"derived {_rel(got[..., n + ncnt:], want[..., n + ncnt:]):.3e} "
          f"counts {'equal' if np.array_equal(got[..., n:n + ncnt], want[..., n:n + ncnt]) else 'DIFFER'}")
    _same(got, want, n, mapping, ks=True)


@functools.lru_cache(maxsize=None)
def _gpu_rows(name, S, mapping, devices=None):
    """one run of sumstatMCMCks per (case, chains, mapping), shared by the direct and the inductive comparison"""
    p = RC.problem(name)
    opt = {} if devices is None else {"devices": list(devices)}
    got = api.sumstatMCMCks(p.z, p.Q, p.pid, p.Omega, N, PRIOR, seed=SEED, n_replicas=S, mapping=mapping, **opt)
    assert got.shape == (N, p.cols)
    got.setflags(write=False)
    return got


# ---- a. one chain, every case on every mapping, against the oracle's own updating run ---------------------------------------
@pytest.mark.parametrize("mapping", RC.MAPPINGS)
@pytest.mark.parametrize("name", list(RC.CASES))
def test_one_chain_under_a_changing_wide_model_matches_the_oracle(name, mapping):
    p = RC.problem(name)
    want, rc = RC.oracle_run(name)
    assert rc == 0
    got = _gpu_rows(name, 1, mapping)
    _bar(got, want, p.n, mapping, name)
    assert len(np.unique(got[:, p.n + p.ncnt])) >= 3                      # l01 moves


# ---- b. the inductive check ---------------------------------------------------------------------------------------------------
def _inductive(name, S, mapping, devices=None):
    """Q_0 is given; Q_{i+1} is what the oracle's updates make of (Q_i, the GPU's row i); the oracle then runs every replica under
    Q_0 .. Q_{N-1} and the rows are summed.  Induction over i: row i of the GPU was swept under Q_i if its parameter columns are
    record_Q(Q_i) bit for bit (host arithmetic on the identical row; tests/test_host_cpu.py pins phm_qupdate_apply to
    orc_qupdate_apply) -- and then its counts must be the oracle's exactly and its dwell sums the oracle's to rounding."""
    p = RC.problem(name)
    n, ncnt = p.n, p.ncnt
    got = _gpu_rows(name, S, mapping, devices)
    Qs = RC.schedule_from_rows(O.KS, p.Q, p.Omega, PRIOR, got, SEED)
    want = RC.summed_schedule_rows(name, Qs, S)
    print(f"[rate-updates] inductive {name} S={S} {mapping}{' two shards' if devices else ''}: dwell {_rel(got[:, :n], want[:, :n]):.3e} "
          f"parameters {_rel(got[:, n + ncnt:-1], want[:, n + ncnt:-1]):.3e}")
    for i in range(N):
        np.testing.assert_array_equal(got[i, n + ncnt:-1], RC.param_columns(Qs[i]), err_msg=f"parameter columns of iteration {i}")
    np.testing.assert_array_equal(got[:, n + ncnt:-1], want[:, n + ncnt:-1])
    np.testing.assert_array_equal(got[:, n:n + ncnt], want[:, n:n + ncnt])
    np.testing.assert_array_equal(got[:, -1], want[:, -1])
    np.testing.assert_allclose(got[:, :n], want[:, :n], rtol=1e-10, atol=0)
    np.testing.assert_allclose(got[:, :n].sum(1), S * p.length, rtol=1e-11)
    assert len({q.tobytes() for q in Qs}) >= N - 2                        # the models do change


@pytest.mark.parametrize("mapping", RC.MAPPINGS)
@pytest.mark.parametrize("S", RC.MULTI_S)
@pytest.mark.parametrize("name", RC.MULTI_NS)
def test_sites_sharing_a_changing_model_match_the_oracle_inductively(name, S, mapping):
    _inductive(name, S, mapping)


def test_sites_on_two_shards_match_the_oracle_inductively():
    """devices = [0, 0]: 64 + 6 sites on two engines of one device, their reduced rows added on the host before the update"""
    _inductive("n26", 70, "tiles", devices=(0, 0))


@pytest.mark.parametrize("mapping", ["branches", "tiles"])
@pytest.mark.parametrize("name", list(RC.CASES))
def test_one_chain_matches_the_oracle_inductively(name, mapping):
    """the direct comparison above needs every discrete draw to survive a rate rounded differently; this one does not"""
    _inductive(name, 1, mapping)


# ---- c. recovery replays wide models -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapping", ["branches", "tiles"])
@pytest.mark.parametrize("name", RC.RECOVERY)
def test_capacity_recovery_replays_the_models_of_a_wide_chain(name, mapping):
    """cap_tail = 0.9 provisions about the expected segment count per branch: the slots overflow, the engine is rebuilt with doubled
    slots and the sweeps so far are replayed -- each under the model it ran under the first time"""
    p = RC.problem(name)
    want, rc, Om = RC.recovery_oracle(name)
    assert rc == 0
    with pytest.raises(_lib.PhmError) as e:
        api.sumstatMCMCks(p.z, p.Q, p.pid, Om, N, PRIOR, seed=SEED, mapping=mapping, cap_tail=0.9, recover=False)
    assert e.value.status == 6
    got = api.sumstatMCMCks(p.z, p.Q, p.pid, Om, N, PRIOR, seed=SEED, mapping=mapping, cap_tail=0.9)
    _bar(got, want, p.n, mapping, f"recovery {name}")


# ---- d. lists of trees ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapping", ["replicas", "branches"])
@pytest.mark.parametrize("n", RC.LIST_NS)
def test_lists_of_trees_under_a_changing_wide_model(n, mapping):
    """sumstatMCMCksmt: the list engine (replicas) bit for bit; an engine per tree (branches) at the bar of
    tests/test_gpu_parity.py::test_multi_tree_drivers_with_an_engine_per_tree"""
    trees, Q, pid, Omega = RC.list_problem(n)[:4]
    seed = 11
    want, rc = RC.list_oracle(n, seed)
    assert rc == 0
    got = api.sumstatMCMCksmt(trees, Q, pid, Omega, N, RC.PRIOR_MT, seed=seed, mapping=mapping)
    assert got.shape == want.shape
    print(f"[rate-updates] list n={n} {mapping}: dwell {_rel(got[:, :n], want[:, :n]):.3e} parameters {_rel(got[:, n + n * n:-1], want[:, n + n * n:-1]):.3e}")
    if mapping == "replicas":
        np.testing.assert_array_equal(got, want)
        return
    np.testing.assert_array_equal(got[:, n:n + n * n], want[:, n:n + n * n])
    np.testing.assert_array_equal(got[:, -1], want[:, -1])
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)


# ---- e. the DIC pass --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapping", RC.MAPPINGS)
@pytest.mark.parametrize("name", RC.DIC_NS)
def test_dic_driver_beyond_four_states(name, mapping):
    p = RC.problem(name)
    want, rc = RC.oracle_run(name, True)
    assert rc == 0
    got = api.sumstatMCMCksDICt(p.z, p.Q, p.pid, p.Omega, N, PRIOR, seed=SEED, mapping=mapping)
    _bar(got, want, p.n, mapping, f"dic {name}")
    np.testing.assert_allclose(got[0, -1], RC.scaled_loglik(p.z, p.Q, p.pid, masks=True), rtol=1e-11)


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("shape", RC.DIC_SHAPES)
def test_dic_pass_on_a_wide_level_and_on_many_levels(shape, n):
    """launch_exp_pl_loglik (phm_exp.hip): complete4096 has a height level of 2 048 nodes, more than one run kernel's block, so
    exp_pl_level_kernel runs; ladder200 has 199 levels, more than one run kernel takes, so further run kernels follow the first.
    The first log p(y | Q) is also held to an independent scipy expm pass with log scale factors (an unscaled one underflows)."""
    z, Q, pid, Omega, prior, _ = RC.dic_shape_problem(shape, n)
    want, rc = RC.dic_shape_oracle(shape, n)
    assert rc == 0
    fn = api.sumstatMCMC2sDICt if n == 2 else api.sumstatMCMCksDICt
    got = fn(z, Q, pid, Omega, RC.DIC_SHAPE_ITERS, prior, seed=RC.DIC_SHAPE_SEED, mapping="branches")
    _bar(got, want, n, "branches", f"dic {shape} n={n}")
    np.testing.assert_allclose(got[0, -1], RC.scaled_loglik(z, Q, pid, masks=n == 4), rtol=1e-11)
