#!/usr/bin/env python
"""Per-launch counter sums of the k_bake instance of two option arms. <root>/<arm>/<pass>/**/*counter_collection.csv
are rocprofv3 --pmc outputs of `tools/ab_options.py --steps 1 --arm ...`, one pass per directory (the sq1, sq2, sq3
and grbm counter sets of tools/gpu_session.sh, no tracing in the same run). Writes <root>/pmc_summary.json.

  python tools/arm_counters.py profiles/wave_locked lock0 lock1
"""
import csv, glob, json, os, sys
from collections import defaultdict
root = sys.argv[1]
arms = sys.argv[2:] or ["lock0", "lock1"]
out = {}
for arm in arms:
    tot = defaultdict(float); n = defaultdict(int); name = None
    for step in ("sq1", "sq2", "sq3", "grbm"):
        for p in glob.glob(os.path.join(root, arm, step, "**", "*counter_collection.csv"), recursive=True):
            seen = set()
            for r in csv.DictReader(open(p)):
                if "k_bake" not in r["Kernel_Name"]:
                    continue
                name = r["Kernel_Name"]
                key = (step, r["Counter_Name"])
                tot[key] += float(r["Counter_Value"])
                seen.add(r.get("Dispatch_Id"))
            for k in [k for k in tot if k[0] == step]:
                n[k] = len(seen)
    out[arm] = {"kernel": name, "per_launch": {f"{s}/{c}": tot[s, c] / max(n[s, c], 1) for s, c in sorted(tot)},
                "launches": {f"{s}/{c}": n[s, c] for s, c in sorted(n)}}
json.dump(out, open(os.path.join(root, "pmc_summary.json"), "w"), indent=1)
print(json.dumps(out, indent=1))
