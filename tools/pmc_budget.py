"""The training tile kernel's counters per run of a directory of rocprofv3
--pmc passes (one sub-directory per run, e.g. one per GSVC_KNOB_TILE_ABLATE
value of ``tools/pmc_workloads.py train50k --knob TILE_ABLATE=V``): per run
the mean of the kernel's last 50 dispatches of every counter, one JSON line
each (profiles/tile_valu/).

    python tools/pmc_budget.py OUT_DIR [kernel-name substring]
"""
from __future__ import annotations

import collections
import csv
import glob
import json
import os
import sys


def run_counters(d: str, kern: str, last: int = 50):
    c = collections.defaultdict(list)
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if kern in r["Kernel_Name"]:
                c[r["Counter_Name"]].append(float(r["Counter_Value"]))
    return {k: round(sum(v[-last:]) / len(v[-last:])) for k, v in sorted(c.items())}


def main():
    root = sys.argv[1]
    kern = sys.argv[2] if len(sys.argv) > 2 else "train_tile_band"
    for d in sorted(glob.glob(os.path.join(root, "*", ""))):
        e = run_counters(d, kern)
        if e:
            print(json.dumps({"run": os.path.basename(d.rstrip("/")), **e}))


if __name__ == "__main__":
    main()
