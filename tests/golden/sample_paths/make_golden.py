"""Records tests/golden/sample_paths/parent.npz: the outputs of the small sampler and wide ancestral calls of
tests/samplepathcases.py.

Run it on a GPU against a build of the commit BEFORE the two exact samplers got their one branch draw, tile driver and wide device
state (its phylomap_amd/csrc has no phm_sample_branch.h), with that build's package first on the path and this repository's tests/
for the cases:

    PYTHONPATH=<checkout of the parent commit>:<this repository>/tests python tests/golden/sample_paths/make_golden.py OUT.npz

Never regenerate it from the code under test: tests/test_gpu_sample_parent.py compares the current build against these bytes."""
import os
import sys

import numpy as np

import samplepathcases as C
import phylomap_amd

if __name__ == "__main__":
    csrc = os.path.join(os.path.dirname(os.path.abspath(phylomap_amd.__file__)), "csrc")
    assert not os.path.exists(os.path.join(csrc, "phm_sample_branch.h")), "this build already has the shared pieces: record from its parent"
    out = {}
    for name in C.CASES:
        got = C.raw(name)
        if "map_off" in got:
            print(name, "most changes of state on one branch:", C.most_changes_on_a_branch(got), flush=True)
        out.update(C.pin(name, got))
    np.savez_compressed(sys.argv[1], **out)
    print("wrote", sys.argv[1], len(out), "arrays,", os.path.getsize(sys.argv[1]), "bytes")
