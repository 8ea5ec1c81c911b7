#!/usr/bin/env python3
"""The reference's controller study on the MI355X (kinova_src/scripts/kinova_compare_robust_controller.m and ..._summary.m): per model
uncertainty level, `samples` rollouts of T seconds under ARMOUR's robust input and under Giusti and Althoff's, the same starts, references
and plants for both; v recomputed at every 10 ms node; the median over samples of each joint's max |v|.  Writes
profiles/althoff_study.json: levels, controllers, per_joint_median_max_v [levels][controllers][joints], the medians of the rollouts' own
max |v| monitor, status counts and wall seconds per level.

    python tools/althoff_study.py [--out profiles/althoff_study.json] [--samples 100] [--T 2.5] [--levels 0,0.05,0.1,0.15,0.2,0.25,0.3] [--seed 0]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "althoff_study.json"))
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--T", type=float, default=2.5)
    ap.add_argument("--levels", default="0,0.05,0.1,0.15,0.2,0.25,0.3")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from armour_amd.tracking import compare_robust_controller
    levels = tuple(float(x) for x in a.levels.split(","))
    controllers = ("robust", "althoff")
    out = compare_robust_controller(levels=levels, samples=a.samples, seed=a.seed, T=a.T, controllers=controllers)
    doc = dict(what="compare_robust_controller, Kinova, T = %g s, dt = 1e-3, %d samples per level, seed %d, true plant 1.01 x nominal; v at every "
                    "10th node (%d per rollout); N m" % (a.T, a.samples, a.seed, out["result"][0][0].trace.shape[1]),
               levels=list(levels), controllers=list(controllers),
               per_joint_median_max_v=out["per_joint_median_max_v"].tolist(),
               median_max_v_every_node=out["median_max_v"].tolist(),
               status_counts=[[{int(s): int((st == s).sum()) for s in np.unique(st)} for st in per_level] for per_level in out["status"]],
               device_ms=[[r.device_ms for r in runs] for runs in out["result"]],
               wall_s_per_level=out["wall_s"].tolist())
    for li, level in enumerate(levels):
        print(json.dumps(dict(level=level, wall_s=doc["wall_s_per_level"][li], status=doc["status_counts"][li],
                              median_max_v={c: [round(x, 4) for x in doc["per_joint_median_max_v"][li][ci]] for ci, c in enumerate(controllers)})), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
