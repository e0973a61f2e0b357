#!/usr/bin/env python
"""Writes tests/golden/count_chain.json: for every scenario of tests/count_chain_cases.py the launches per kernel and the
SHA-256 of the counts and of the window totals, as the library that is loaded produces them.

The fixture pins the launch chain of the count launcher across a change of its host code, so it is generated on the library
of the commit BEFORE the change (build that commit, or name its library in PHAMERS_AB_LIB with
PHK_ALLOW_DIAGNOSTIC_BUILD=1), never on the code under test.  Every scenario runs twice, on two contexts; the file is
written only if the two runs agree.

    python tools/gen_golden_count_chain.py [out.json]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from phamers_amd import _lib                 # noqa: E402
from tests import count_chain_cases as cases  # noqa: E402


def one_run():
    ctx = _lib.Context(_lib.default_device())
    try:
        sc = cases.Scenarios(ctx)
        return {name: sc.run(name) for name in cases.Scenarios.NAMES}
    finally:
        ctx.close()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "count_chain.json")
    a, b = one_run(), one_run()
    for name in cases.Scenarios.NAMES:
        print(name, json.dumps(a[name]["launches"]))
        if a[name] != b[name]:
            print("the two runs differ in %r:\n%s\n%s" % (name, a[name], b[name]))
            return 1
    with open(out, "w") as f:
        json.dump({"scenarios": a}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
