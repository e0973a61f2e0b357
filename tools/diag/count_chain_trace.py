#!/usr/bin/env python
"""Runs every scenario of tests/count_chain_cases.py once, in their order, in one process -- the program to put under a kernel
trace (rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/diag/count_chain_trace.py): the profile's family
names do not tell a 512-thread instance from a 1024-thread one, the trace's dispatches do.  With --reduce CSV it prints the
trace's dispatch sequence instead, one line each: full kernel name, grid, workgroup, LDS bytes (profiles/count_driver/)."""
import csv
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)


def reduce(path):
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        print("%s grid=%s workgroup=%s lds=%s" % (r["Kernel_Name"], r["Grid_Size_X"], r["Workgroup_Size_X"], r["LDS_Block_Size"]))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--reduce":
        return reduce(sys.argv[2])
    from phamers_amd import _lib
    from tests import count_chain_cases as cases
    ctx = _lib.Context(_lib.default_device())
    sc = cases.Scenarios(ctx)
    for name in cases.Scenarios.NAMES:
        sc.call(name)
    ctx.sync()
    ctx.close()


if __name__ == "__main__":
    main()
