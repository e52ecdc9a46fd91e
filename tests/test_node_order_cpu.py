"""The depth-level order over internal nodes (phm_sched.h node_depth_levels) that the node draws of the (tile, branch) mapping walk,
an item per internal node: checked by a stand-alone program (tests/native/node_order_check.cpp) on the 2-tip tree, a ladder, a
balanced tree and a random 1 000-tip tree -- every internal node exactly once, a node's parent one level earlier, the level offsets
tiling the order.  The program and phm_sched.cpp are built with the host compiler under AddressSanitizer and UBSan and run on
their own."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_node_depth_levels_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "node_order_check")
    csrc = os.path.join(ROOT, "phylomap_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "native", "node_order_check.cpp"), os.path.join(csrc, "phm_sched.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok"), run.stdout
