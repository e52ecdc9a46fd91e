"""Records tests/golden/sweep_parts/parent.npz: statistics and seg_read of the small (tile, branch) sweeps of
tests/sweeppartscases.py.

Run it on a GPU against a build of the commit BEFORE the sweep parts and the segment rows of the branch kernel (its
tiles_chunk_kernel still walks mcount), with that build's package first on the path and this repository's tests/ for the cases:

    PYTHONPATH=<checkout of the parent commit>:<this repository>/tests python tests/golden/sweep_parts/make_golden.py OUT.npz

Never regenerate it from the code under test: tests/test_gpu_sweep_parts.py::test_one_part_equals_the_recorded_parent_run compares
the current build against these numbers."""
import sys

import numpy as np

import sweeppartscases as C
from phylomap_amd import _lib

if __name__ == "__main__":
    assert "sweep_parts" not in dict(_lib.DebugOptions._fields_), "this build already has the sweep parts: record from its parent"
    out = {}
    for name, S, lg, reduce in C.GOLDEN_CASES:
        stats, seg, rec, _ = C.sweep(name, S, reduce, level_groups=lg)
        assert rec == 0
        k = C.golden_key(name, S, lg, reduce)
        out[k + "_stats"], out[k + "_seg"] = stats, seg
    np.savez_compressed(sys.argv[1], **out)
    print("wrote", sys.argv[1], len(out), "arrays")
