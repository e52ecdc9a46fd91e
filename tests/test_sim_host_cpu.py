"""The table builder of the two forward simulators' shared host front end (phylomap_amd/csrc/phm_sim_host.h: model_tables) without
a device.  A stand-alone program (tests/native/sim_host_check.cpp) is built with hipcc and AddressSanitizer + UBSan on the host
side, run on its own, and its output compared with a direct transcription of the loops the two ``*_validate`` functions had before
they shared this code: jump weights row-major with the diagonal zeroed, row totals summed left to right, 1 / (-q_ii), and the
refusal of a row that leaves its state and has no target."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def generator(n, which):
    """row-major; the program builds the same matrix column-major"""
    Q = [[0.0] * n for _ in range(n)]
    for i in range(n):
        s = 0.0
        for j in range(n):
            if j != i:
                Q[i][j] = (1 + (7 * i + 3 * j + which) % 5) / 8.0
                s += Q[i][j]
        Q[i][i] = -s
    return Q


def tables(name, Q, who=""):
    """the loops of sim_validate / simm_validate (after check_generator, which these matrices pass)"""
    n = len(Q)
    qoff, qtot, inv = [], [], []
    for i in range(n):
        row = list(Q[i])
        qii = row[i]
        row[i] = 0.0
        off = row[0]
        for j in range(1, n):
            off += row[j]
        if qii < 0.0 and not off > 0.0:
            return [f"{name} n={n} status=1", f"refused: {who}Q: row {i + 1} leaves its state but has no target"]
        qoff += row
        qtot.append(off)
        inv.append(1.0 / (-qii) if qii < 0.0 else 0.0)
    fmt = lambda what, v: what + "".join(" %.17g" % x for x in v)
    return [f"{name} n={n} status=0", fmt("qoff", qoff), fmt("qtot", qtot), fmt("inv_rate", inv)]


def expected_output():
    lines = tables("plain", generator(2, 0)) + tables("plain", generator(5, 1))
    Q = generator(5, 2)
    Q[2] = [0.0] * 5
    absorbing = tables("absorbing", Q)
    assert absorbing[3].split()[3] == "0" and absorbing[2].split()[3] == "0"          # inv_rate and total of state 3
    lines += absorbing
    Q = [[-1e-14, 0.0], [100.0, -100.0]]
    lines += tables("no_target", Q) + tables("no_target_model", Q, "model 2: ")
    for k in range(3):
        single, batch = tables("single", generator(5, 10 + k)), tables("batch", generator(5, 10 + k), f"model {k}: ")
        assert single[1:] == batch[1:]
        lines += single + batch
    return lines + ["ok"]


def test_model_tables_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    exe = str(tmp_path / "sim_host_check")
    csrc = os.path.join(ROOT, "phylomap_amd", "csrc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", csrc, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "sim_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    got, want = run.stdout.splitlines(), expected_output()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
