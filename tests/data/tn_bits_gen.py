"""Writes tests/data/tn_bits_parent.json: SHA-256 of every input and raw output buffer of the cases of
tests/test_tn_bits_gpu.py, built and run by that module's own functions.  Run it on an MI355X in a checkout of the commit
BEFORE the TN bodies' shared pieces were factored out (with this file and the test module copied in) - never from the
code under test:

    python tests/data/tn_bits_gen.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import test_tn_bits_gpu as T                                  # noqa: E402


def main():
    table = {}
    for name, build in T.CASES.items():
        ins, outs = build()
        table[name] = {"in": T.digests(ins), "out": T.digests(outs)}
        print(name, len(outs), "outputs")
    with open(T.TABLE, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
