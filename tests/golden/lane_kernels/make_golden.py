"""Records tests/golden/lane_kernels/parent.npz: the outputs of the small lane-kernel calls of tests/lanekernelcases.py.

Run it on a GPU against a build of the commit BEFORE the lane kernels got their shared device pieces (its phylomap_amd/csrc has
no phm_ll_device.h), with that build's package first on the path and this repository's tests/ for the cases:

    PYTHONPATH=<checkout of the parent commit>:<this repository>/tests python tests/golden/lane_kernels/make_golden.py OUT.npz

Never regenerate it from the code under test: tests/test_gpu_lane_kernels_parent.py compares the current build against these
bytes."""
import os
import sys

import numpy as np

import lanekernelcases as C
import phylomap_amd

if __name__ == "__main__":
    csrc = os.path.join(os.path.dirname(os.path.abspath(phylomap_amd.__file__)), "csrc")
    assert not os.path.exists(os.path.join(csrc, "phm_ll_device.h")), "this build already has the shared lane pieces: record from its parent"
    out = {}
    for name in C.CASES:
        out.update(C.run(name))
    np.savez_compressed(sys.argv[1], **out)
    print("wrote", sys.argv[1], len(out), "arrays,", os.path.getsize(sys.argv[1]), "bytes")
