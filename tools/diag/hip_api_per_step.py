#!/usr/bin/env python
"""Per-step HIP API calls from one rocprofv3 trace of tools/diag/score_driver_ab.py --trace-steps N:

    rocprofv3 --hip-runtime-trace --output-format csv -d DIR -- python tools/diag/score_driver_ab.py --config 1 --trace-steps 20
    python tools/diag/hip_api_per_step.py DIR 20

The traced program waits for the device before and after its N steps and nowhere inside them, so the block of calls between
two consecutive hipStreamSynchronize that holds the most launches is those N steps; its calls per function, divided by N.
One JSON line: the whole trace's number of calls, the block's, and the per-step figures."""
import collections
import csv
import glob
import json
import sys


def main():
    d, steps = sys.argv[1], int(sys.argv[2])
    rows = []
    for f in glob.glob(d + "/**/*hip_api_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), r["Function"]))
    rows.sort()
    syncs = [i for i, r in enumerate(rows) if r[1] == "hipStreamSynchronize"]
    launches, a, b = max((sum(1 for r in rows[a + 1:b] if "Launch" in r[1]), a, b) for a, b in zip(syncs, syncs[1:]))
    per = collections.Counter(r[1] for r in rows[a + 1:b])
    print(json.dumps({"api_calls_total": len(rows), "window_calls": b - a - 1,
                      "per_step": {k: v / steps for k, v in sorted(per.items())}}))


if __name__ == "__main__":
    main()
