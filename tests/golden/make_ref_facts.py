#!/usr/bin/env python3
"""Generate tests/golden/ref_facts.json with the REFERENCE's own CPU code.

Runs only where oracle/_ref/libpfac_ref.so was built (the reference sources are present): for every small
workload of tests/conftest.py, the reference's trie (sizes, SHA-256 of its edge list) and the digests of its
scalar and OpenMP matchers' results.  test_oracle_golden.py::test_restatement_equals_reference_code compares the
restatement with these facts where the reference cannot be built, and with the reference itself where it can.

    python tests/golden/make_ref_facts.py
"""

import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import binding as ob                       # noqa: E402
from tests.conftest import make_workloads              # noqa: E402
from tests.test_oracle_golden import reference_facts   # noqa: E402


def main():
    assert ob.have_reference(), "build oracle/_ref first: make -C oracle ref"
    out = {"_doc": "facts of the reference's own trie builder and CPU matchers (oracle/_ref) on the workloads of tests/conftest.py; "
                   "see make_ref_facts.py", "workloads": {}}
    for name, w in make_workloads(tempfile.mkdtemp()).items():
        o = ob.Oracle(w.pattern_file)
        out["workloads"][name] = reference_facts(w, o)
        o.close()
        print(name, out["workloads"][name]["num_states"], "states", out["workloads"][name]["results"]["dense_omp0"][1], "matches")
    path = os.path.join(ROOT, "tests", "golden", "ref_facts.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
