"""The batched workspace RRT* (armour_ws_tree_plan) measured; writes profiles/ws_tree_bench.json (or --out) and prints ONE JSON line.

    python tools/ws_tree_bench.py [--max-iterations 1000] [--max-nodes 1024] [--seed 7] [--reps 10] [--skip-cap] [--out FILE]

* `batch`: the 107 reference worlds (scenes.reference_worlds; start and goal POINTS = the end effector of the start and of the goal
  configuration, O padded with scenes.FAR_BOX, every world with the seed --seed, the sampling box ws_planner.workspace_box, the planner's
  default step / edge_step / rewire_radius / goal_rate / goal_tol) in ONE launch: device ms = the entry's event time, median of --reps calls
  after a warm-up; call_ms = the median host time of the same calls (uploads, launch, the paths back); the status counts, path costs,
  rewire counts and tree sizes per world; the host twin's wall time on the same inputs (armour_ws_tree_plan_host, one call, one core), whether
  every output of the two is the same bit for bit, and `digest` = the SHA-256 of the device's outputs (two builds of the library that
  print the same digest computed the same trees: the node-storage A/B of DESIGN.md 4.12f);
* `one_world`: the same for hard_7_window alone (W = 1: one block, so one compute unit -- the planner's stated limit);
* `at_the_cap`: the batch once more with --cap-iterations / ARMOUR_WS_MAX_NODES nodes, i.e. the longest scans the kernel can be asked for.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATUS = ("partial", "reached", "start_blocked")
FIELDS = ("status", "iterations", "count", "rewires", "chain_kept", "path_cost", "goal_dist", "nodes", "parent", "node_cost")


def same_bits(a, b):
    return all(np.ascontiguousarray(getattr(a, k)).tobytes() == np.ascontiguousarray(getattr(b, k)).tobytes() for k in FIELDS) and all(
        (p is None and q is None) or (p is not None and q is not None and p.tobytes() == q.tobytes()) for p, q in zip(a.paths, b.paths))


def digest(r):
    h = hashlib.sha256()
    for k in FIELDS:
        h.update(np.ascontiguousarray(getattr(r, k)).tobytes())
    for p in r.paths:
        h.update(b"-" if p is None else p.tobytes())
    return h.hexdigest()


def measure(obs, starts, goals, seeds, box, options, reps):
    from armour_amd.ws_planner import plan_workspace_trees
    plan = lambda **kw: plan_workspace_trees(obs, starts, goals, seeds, box[0], box[1], **options, **kw)
    plan()                                                                           # warm-up
    runs, call = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        runs.append(plan())
        call.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(r.ms for r in runs)
    dev = plan(trees=True)
    t0 = time.perf_counter()
    host = plan(trees=True, host=True)
    host_ms = (time.perf_counter() - t0) * 1e3
    return dict(worlds=int(obs.shape[0]), obstacles_per_world=int(obs.shape[1]), device_ms=round(ms[len(ms) // 2], 4), device_ms_min=round(ms[0], 4),
                call_ms=round(sorted(call)[len(call) // 2], 3), host_twin_wall_ms=round(host_ms, 2), device_equals_host=bool(same_bits(dev, host)),
                digest=digest(dev), host_margin_min=float(host.margin.min()), status_counts={STATUS[s]: int((dev.status == s).sum()) for s in range(3)},
                iterations=[int(i) for i in dev.iterations], tree_sizes=[int(c) for c in dev.count], rewires=[int(c) for c in dev.rewires],
                path_cost=[round(float(c), 6) for c in dev.path_cost], goal_dist=[round(float(c), 6) for c in dev.goal_dist],
                path_points=[0 if p is None else int(len(p)) for p in dev.paths])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-iterations", type=int, default=1000)
    ap.add_argument("--max-nodes", type=int, default=1024)
    ap.add_argument("--cap-iterations", type=int, default=4500)
    ap.add_argument("--skip-cap", action="store_true")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ws_tree_bench.json"))
    a = ap.parse_args()
    from armour_amd import _lib, ik, scenes
    from armour_amd.planner import kinova_robot
    from armour_amd.ws_planner import EDGE_STEP, GOAL_RATE, GOAL_TOL, REWIRE_RADIUS, STEP, workspace_box
    robot = kinova_robot()
    ws = scenes.reference_worlds()
    names = [name for name, _ in ws]
    O = max(p["obstacles"].shape[0] for _, p in ws)
    obs = np.stack([scenes.pad_obstacles(p["obstacles"], O) for _, p in ws])
    starts = ik.end_effector(robot, np.stack([p["q0"] for _, p in ws]))
    goals = ik.end_effector(robot, np.stack([p["goal"] for _, p in ws]))
    seeds = np.full(len(ws), a.seed, dtype=np.uint64)
    box = workspace_box(robot)
    options = dict(max_iterations=a.max_iterations, max_nodes=a.max_nodes)
    out = dict(tool="ws_tree_bench", robot="kinova_gen3_no_gripper", library=os.path.basename(_lib.LIB_PATH), seed=a.seed, reps=a.reps, step=STEP, edge_step=EDGE_STEP,
               rewire_radius=REWIRE_RADIUS, goal_rate=GOAL_RATE, goal_tol=GOAL_TOL, box=[list(box[0]), list(box[1])], **options)
    out["batch"] = dict(measure(obs, starts, goals, seeds, box, options, a.reps), names=names)
    w = names.index("hard_7_window")
    out["one_world"] = dict(measure(obs[w:w + 1], starts[w:w + 1], goals[w:w + 1], seeds[w:w + 1], box, options, a.reps), name=names[w])
    cap = dict(max_iterations=a.cap_iterations, max_nodes=_lib.WS_MAX_NODES)
    full = None if a.skip_cap else measure(obs, starts, goals, seeds, box, cap, max(a.reps // 3, 1))
    if full is not None:
        out["at_the_cap"] = dict(cap, **{k: full[k] for k in ("device_ms", "device_ms_min", "call_ms", "host_twin_wall_ms", "device_equals_host", "digest", "status_counts")},
                                 tree_size_max=int(max(full["tree_sizes"])), rewires_sum=int(sum(full["rewires"])))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
