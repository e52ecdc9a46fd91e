"""What tests/test_gpu_rate_updates_wide.py relies on, checked without a GPU: the oracle's schedule entry reproduces its updating
drivers bit for bit, and every case of tests/rateupdatecases.py is the input it was chosen to be -- the oracle accepts it, it takes
the branch of upload_model (phm_engine.cpp) it is named for, its rates move, and its paths fit the replica mapping's scratch."""
import numpy as np
import pytest

import oracle_lib as O
import rateupdatecases as RC
from phylomap_amd import synth


def _ks4():
    Q = synth.make2sQ(.1, .1, .2, .2, 10)
    pid = np.full(4, .25)
    z = synth.make_tree(30, Q, 1.0, 16, pid)
    z["states"] = ((z["states"] - 1) % 2 + 1).astype(np.int32)
    return z, Q, pid, 25.0, RC.PRIOR, O.KS


def _bf2():
    Q = np.array([[-.1, .1], [.1, -.1]])
    pid = np.array([.5, .5])
    return synth.make_tree(40, Q, 0.5, 15, pid), Q, pid, 10.0, (.55, 1, .56, 1.01), O.BF


def _case(name):
    p = RC.problem(name)
    return p.z, p.Q, p.pid, p.Omega, RC.PRIOR, O.KS


@pytest.mark.parametrize("which", ["ks4", "n8", "n34", "bf2"])
def test_schedule_of_the_recorded_models_reproduces_the_updating_driver(which):
    """In the counter-based mode the updates draw on streams of their own (hs_u: replica word 0xFFFFFFFF, entity 0xFFFFFF00 | id),
    so a run that is handed the models instead of drawing them makes every draw of the chain exactly as before: the schedule
    built by orc_qupdate_apply from the updating run's own rows gives that run back, every column, bit for bit."""
    z, Q, pid, Omega, prior, variant = {"ks4": _ks4, "bf2": _bf2}.get(which, lambda: _case(which))()
    n, N, seed = Q.shape[0], RC.N_ITERS, 7 + (5 << 32)                  # both words of the Philox key in use
    nen, nodelist, root = RC.orders(z)
    want, rc = O.maketreelistMCMC(z, Q, pid, np.eye(n) + Q / Omega, Omega, nen, nodelist, root, N, variant=variant, seed=seed, prior=prior)
    assert rc == 0
    Qs = RC.schedule_from_rows(variant, Q, Omega, prior, want, seed)
    assert len({q.tobytes() for q in Qs}) >= N - 2                        # the models do change
    got, rc = O.maketreelistMCMC_schedule(z, Qs, pid, Omega, nen, nodelist, root, variant=variant, seed=seed)
    assert rc == 0
    np.testing.assert_array_equal(got, want)
    if variant == O.KS:                                                   # record_Q writes the scheduled Q's columns
        for i in range(N):
            np.testing.assert_array_equal(got[i, n + n * n:-1], RC.param_columns(Qs[i]))
    # another replica follows the same models on draws of its own
    other, rc = O.maketreelistMCMC_schedule(z, Qs, pid, Omega, nen, nodelist, root, variant=variant, seed=seed, replica=1)
    assert rc == 0 and not np.array_equal(other[:, :n], want[:, :n])
    np.testing.assert_array_equal(other[:, n + n * n:-1], want[:, n + n * n:-1])


def test_schedule_entry_under_sanitizers(tmp_path):
    """tests/native/oracle_schedule_check.c and oracle/phm_oracle.c, built with the host compiler under AddressSanitizer and UBSan
    and run on their own: the same bit-for-bit reproduction on a tree made in C, and the refusals"""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "no host C compiler"
    exe = str(tmp_path / "oracle_schedule_check")
    subprocess.check_call([cc, "-std=c11", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(root, "oracle"), os.path.join(root, "tests", "native", "oracle_schedule_check.c"),
                           os.path.join(root, "oracle", "phm_oracle.c"), "-o", exe, "-lm"])
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok"), run.stdout


def test_schedule_of_one_model_is_the_fixed_model_sweep_and_bad_calls_are_refused():
    z, Q, pid, Omega, _, _ = _case("n8")
    n, N = 8, 6
    nen, nodelist, root = RC.orders(z)
    fixed, rc = O.maketreelistMCMC(z, Q, pid, np.eye(n) + Q / Omega, Omega, nen, nodelist, root, N, variant=O.KS, seed=3, replica=2)
    assert rc == 0
    got, rc = O.maketreelistMCMC_schedule(z, np.stack([Q] * N), pid, Omega, nen, nodelist, root, seed=3, replica=2)
    assert rc == 0
    np.testing.assert_array_equal(got, fixed)
    # the chain state carries over: the second half of a run under (Q, Q') is not a fresh run under Q'
    Q2 = RC.oracle_schedule("n8")[5]
    both, rc = O.maketreelistMCMC_schedule(z, np.stack([Q] * 3 + [Q2] * 3), pid, Omega, nen, nodelist, root, seed=3, replica=2)
    assert rc == 0
    np.testing.assert_array_equal(both[:3], fixed[:3])
    assert not np.array_equal(both[3:, :n], fixed[3:, :n])
    np.testing.assert_allclose(both[:, :n].sum(1), z["edge.length"].sum(), rtol=1e-12)
    # PLAIN has no parameter columns to write; the sequential modes share one stream between sweep and updates
    _, rc = O.maketreelistMCMC_schedule(z, np.stack([Q] * N), pid, Omega, nen, nodelist, root, variant=O.PLAIN)
    assert rc == O.ERR_BAD_INPUT
    import ctypes as C
    ft = O.FlatTree(z)
    rng, _ = O.make_rng(3, rstream=True)
    Qs, out = np.ascontiguousarray(np.stack([Q] * N)), np.zeros((N, n + n * n + 2 + 3 * 3 + 1), order="F")
    B = np.asfortranarray(np.eye(n) + Q / Omega)
    rc = O.lib().orc_maketreelistMCMC_schedule(C.byref(ft.c), n, O._ptr(Qs, C.c_double), O._ptr(pid, C.c_double), O._ptr(B, C.c_double),
                                               C.c_double(Omega), O._ptr(np.ascontiguousarray(nen, dtype=np.int32), C.c_int32),
                                               O._ptr(np.ascontiguousarray(nodelist, dtype=np.int32), C.c_int32), int(root), N, O.KS, 0,
                                               C.byref(rng), O._ptr(out, C.c_double), None)
    assert rc == O.ERR_BAD_INPUT


@pytest.mark.parametrize("name", list(RC.CASES))
def test_case_is_the_input_it_was_chosen_to_be(name):
    p = RC.problem(name)
    rows, rc = RC.oracle_run(name)
    assert rc == 0 and rows.shape == (RC.N_ITERS, p.cols)
    Qs = RC.oracle_schedule(name)
    n, k = p.n, p.k
    par = rows[:, n + p.ncnt:-1]
    # dispatch classes: (band, LDS slots, ELLPACK width) from the host's rules, at the start and once the kappas are in place
    first, later = RC.EXPECTED[name]
    assert RC.classes(Qs[0], p.Omega) == first
    assert RC.classes(Qs[-1], p.Omega) == later
    hb = RC.half_bandwidth(np.eye(n) + Qs[-1] / p.Omega)
    assert hb == 2 and (later[0] == 2) == (n <= RC.WT_BAND_NMAX)
    assert (later[1] > 0) == (4 * n - 4 <= RC.WT_MAX_SLOTS) and later[1] in (0, 4 * n - 4)
    assert (later[2] == 4) == (3 * 4 <= n)
    if p.widen:                         # every rk, lk is 0 in row 0 and some are positive by row 2: the band widens under a live chain
        assert np.all(par[0, 2:2 + 2 * k] == 0.0) and RC.half_bandwidth(np.eye(n) + Qs[0] / p.Omega) == 1
        assert np.any(par[2, 2:2 + 2 * k] > 0.0) and RC.classes(Qs[2], p.Omega)[0] == 2
        assert first[1] == 2 * n and first[2] == 2
    else:
        assert all(RC.classes(Q, p.Omega) == first for Q in Qs)
    # the rates move: at least half of the 2 + 3k parameters take 3 or more values
    assert par.shape[1] == 2 + 3 * k
    assert sum(len(np.unique(par[:, c])) >= 3 for c in range(par.shape[1])) * 2 >= par.shape[1]
    assert np.all(np.abs(np.diagonal(Qs, axis1=1, axis2=2)) <= p.Omega)
    # the replica mapping keeps one branch of a chain in 128 LDS slots at n > 4
    assert RC.longest_branch(name) < RC.WIDE_SEG_CAP
    np.testing.assert_allclose(rows[:, :n].sum(1), p.length, rtol=1e-12)


@pytest.mark.parametrize("name", RC.MULTI_NS)
def test_summed_schedule_rows_are_sums_over_replicas(name):
    """the reference of the multi-site runs, on the oracle's own models: replica 0's row is the single chain, the parameter
    columns are plain values, everything else adds up"""
    p, Qs = RC.problem(name), RC.oracle_schedule(name)
    one = RC.summed_schedule_rows(name, Qs, 1)
    np.testing.assert_array_equal(one, RC.oracle_run(name)[0])
    three = RC.summed_schedule_rows(name, Qs, 3)
    np.testing.assert_array_equal(three[:, p.n + p.ncnt:-1], one[:, p.n + p.ncnt:-1])
    np.testing.assert_allclose(three[:, :p.n].sum(1), 3 * p.length, rtol=1e-12)
    assert np.all(three[:, p.n:p.n + p.ncnt].sum(1) > one[:, p.n:p.n + p.ncnt].sum(1))


@pytest.mark.parametrize("name", RC.RECOVERY)
def test_recovery_cases(name):
    p = RC.problem(name)
    rows, rc, Om = RC.recovery_oracle(name)
    assert rc == 0 and Om > p.Omega
    par = rows[:, p.n + p.ncnt:-1]
    assert sum(len(np.unique(par[:, c])) >= 3 for c in range(par.shape[1])) * 2 >= par.shape[1]      # models to replay
    # more virtual jumps than the case's own run: the slots that cap_tail = 0.9 provisions are outgrown
    own = RC.oracle_run(name)[0]
    assert rows[:, p.n:p.n + p.ncnt].sum() > 1.5 * own[:, p.n:p.n + p.ncnt].sum()


@pytest.mark.parametrize("n", RC.LIST_NS)
def test_list_of_trees_cases(n):
    rows, rc = RC.list_oracle(n, 11)
    assert rc == 0 and rows.shape == (RC.N_ITERS, n + n * n + 2 + 3 * (n // 2 - 1) + 1)
    assert len(np.unique(rows[:, -1])) >= 3                                # several trees of the list get drawn
    assert len(np.unique(rows[:, n + n * n])) >= 3                         # l01 moves
    _, Q, _, Omega = RC.list_problem(n)[:4]
    assert RC.classes(Q, Omega) == ((2, 44, 4) if n == 12 else (0, 0, 4))


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("shape", RC.DIC_SHAPES)
def test_dic_tree_shapes_reach_the_level_kernel_and_a_second_run(shape, n):
    z, Q, pid, Omega, prior, variant = RC.dic_shape_problem(shape, n)
    sizes = RC.height_level_sizes(z["edge"])
    assert sum(sizes) == z["Nnode"]
    if shape == "complete4096":
        assert sizes == [2048 >> i for i in range(12)] and sizes[0] > RC.EXP_RUN_BLOCK >= sizes[1]
    else:
        assert len(sizes) == 199 > 3 * RC.EXP_RUN_LEVELS and max(sizes) == 1      # four run kernels
    assert len(np.unique(z["states"])) == 2
    rows, rc = RC.dic_shape_oracle(shape, n)
    assert rc == 0 and np.all(np.isfinite(rows[:, -1])) and len(np.unique(rows[:, -1])) >= 3      # the models change under the pass
    # the independent pass the GPU test pins the first log-likelihood to agrees with the oracle's Pade route
    np.testing.assert_allclose(rows[0, -1], RC.scaled_loglik(z, Q, pid, masks=n == 4), rtol=1e-11)
    if shape == "complete4096":                                                     # an unscaled pass would not do here
        assert rows[0, -1] < np.log(np.finfo(float).tiny)
