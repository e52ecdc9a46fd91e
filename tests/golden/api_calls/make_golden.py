"""Records tests/golden/api_calls/parent.json: what the calls of tests/apicallcases.py hand to the C ABI and return, and the
messages of the refused ones; also the ``argtypes`` and ``restype`` that ``_lib.load()`` sets, by type name.

Run it against a build of the commit BEFORE the binding layer got its shared helpers (its phylomap_amd/api.py still has
``_expect_args(z, Q, pid, ...)``), with that build's package first on the path and this repository's tests/ for the cases; no
GPU is needed, the recorder's proxy answers every call:

    PYTHONPATH=<checkout of the parent commit>:<this repository>/tests python tests/golden/api_calls/make_golden.py OUT.json

Never regenerate it from the code under test: tests/test_api_calls_cpu.py compares the current layer against these records."""
import inspect
import json
import os
import sys

import apicallcases as A
from phylomap_amd import api

if __name__ == "__main__":
    old = getattr(api, "_expect_args", None)
    assert old is not None and list(inspect.signature(old).parameters)[:3] == ["z", "Q", "pid"], \
        "this api.py already has the shared helpers: record from its parent"
    out = {"cases": {name: A.run(name) for name in A.CASES}, "refusals": {name: A.refusal(name) for name in A.REFUSALS},
           "argtypes": A.argtypes()}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", sys.argv[1], len(out["cases"]), "cases,", len(out["refusals"]), "refusals,", os.path.getsize(sys.argv[1]), "bytes")
