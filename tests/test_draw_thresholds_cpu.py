"""The integer form of the branch kernel's categorical draw (phm_draw_tab.h): for every chain row 0 .. 40 and
every pair (end state, previous state) the 16-byte entry of thresholds gives the index sample_cat gives, at the words 0, 1, 2^32 - 2,
2^32 - 1, T_j - 1 .. T_j + 2 and 1 000 random ones, and carries the fallback bit exactly where sample_cat raises DERR_ZERO_PROB.
Checked by a stand-alone program (tests/native/draw_thresholds_check.cpp: the header, and sample_cat / u01 restated for the host),
built with the host compiler under -ffp-contract=off, AddressSanitizer and UBSan and run on its own.  Models, 2 to 4 states: C3's
B = I + Q / Omega (four structural zeros: thresholds that no word satisfies and thresholds that every word satisfies both occur), the
nearly periodic 2-state chain of tilesclasses.case_c_slow, the 3-state matrix of the parity tests, a dense random B and a B with a
zero column (total = 0 entries) at every state count."""
import os
import re
import shutil
import subprocess

import numpy as np

from phylomap_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _models():
    out = []
    Q = synth.config_Q(3)
    Omega = 1.25 * float(np.max(np.abs(np.diag(Q))))                       # synth.config_problem(3)
    out.append(("C3", np.eye(4) + Q / Omega))
    Qs = np.array([[-1.0, 1.0], [1.0, -1.0]])
    out.append(("periodic2", np.eye(2) + Qs / 1.02))                       # tilesclasses.case_c_slow
    Q3 = np.array([[-.3, .2, .1], [.05, -.15, .1], [.2, .2, -.4]])         # tilesclasses.Q3
    out.append(("parity3", np.eye(3) + Q3 / (1.25 * 0.4)))
    rng = np.random.default_rng(20251)
    for n in (2, 3, 4):
        B = rng.random((n, n)) + 0.01
        out.append((f"dense{n}", B / B.sum(axis=1, keepdims=True)))
        Z = rng.random((n, n)) + 0.01
        Z[:, 0] = 0.0
        out.append((f"zerocol{n}", Z / Z.sum(axis=1, keepdims=True)))
    return out


def test_threshold_entries_equal_sample_cat_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "draw_thresholds_check")
    csrc = os.path.join(ROOT, "phylomap_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, os.path.join(ROOT, "tests", "native", "draw_thresholds_check.cpp"), "-o", exe])
    models = _models()
    path = tmp_path / "models.txt"
    with open(path, "w") as f:
        for _, B in models:
            f.write(f"{B.shape[0]}\n" + " ".join(float(v).hex() for v in B.ravel()) + "\n")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok"), run.stdout
    rows = [dict(zip(("model", "states", "draws", "none", "every", "fallback", "bad"), map(int, re.findall(r"-?\d+", line))))
            for line in run.stdout.splitlines() if line.startswith("model ")]
    assert len(rows) == len(models)
    for (name, B), r in zip(models, rows):
        n = B.shape[0]
        assert r["states"] == n and r["bad"] == 0, (name, r)
        entries = 41 * n * n
        # B >= 0: the total of entry (kk, cs, s) is zero exactly where no path of kk + 1 steps leads from s to cs (C3: the four
        # structural zeros at row 0; a zero column: end state 0 at every row)
        reach, step, unreachable = np.eye(n, dtype=bool), B > 0, 0
        for _ in range(41):
            reach = (reach.astype(int) @ step.astype(int)) > 0
            unreachable += int(np.sum(~reach))
        assert r["fallback"] == unreachable, (name, r)
        assert (unreachable == 41 * n) if name.startswith("zerocol") else (unreachable == (4 if name == "C3" else 0)), (name, unreachable)
        # every entry without the bit was compared at the 4 fixed words, its thresholds' neighbours and 1 000 random words
        assert r["draws"] >= (entries - r["fallback"]) * 1004, (name, r)
    c3 = rows[0]
    assert c3["none"] > 0 and c3["every"] > 0, c3      # both edge cases occur in the flagship's own model
