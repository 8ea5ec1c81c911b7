"""The path shortener (armour_path_shortcut) measured; writes profiles/shortcut_bench.json (or --out) and prints ONE JSON line.

    python tools/shortcut_bench.py [--step 0.5] [--edge-step 0.05] [--max-iterations 2000] [--max-nodes 2048] [--seed 7] [--reps 10] [--out FILE]

The 107 reference worlds (scenes.reference_worlds, each from its start to its goal, O padded with scenes.FAR_BOX, every world with the seed
--seed) are planned once with the batched tree planner under tools/tree_bench.py's settings; the found paths are then shortened in ONE
launch, with passes 1 and 2: device ms = the entry's event time, median of --reps calls after a warm-up; call_ms = the median host time of
the same calls; the host twin's wall time on the same inputs (armour_path_shortcut_host, one call), with whether both gave the same
statuses, passes and paths; points and wrapped length before and after, per world and summed.

--moving: a run of its own that leaves profiles/shortcut_bench.json alone and writes the key `shortcut` of profiles/tree_moving_bench.json
(or --out; the file's other keys are kept), passes = 2, all in this process: the static paths by the static entry and by
armour_path_shortcut_moving at zero velocity on the same window (the like-for-like cost of the window rule; `ratio_v0` = static ms /
moving ms); and the paths that armour_tree_plan_moving finds with every obstacle in linear motion (tools/tree_bench.py's seeded velocities
and window) shortened against the moving obstacles.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(robot, obs, paths, edge_step, passes, reps, **motion):
    from armour_amd.tree_planner import shortcut_paths
    shortcut_paths(robot, obs, paths, edge_step=edge_step, passes=passes, **motion)              # warm-up
    runs, call = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        runs.append(shortcut_paths(robot, obs, paths, edge_step=edge_step, passes=passes, **motion))
        call.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(r.ms for r in runs)
    dev = runs[-1]
    t0 = time.perf_counter()
    host = shortcut_paths(robot, obs, paths, edge_step=edge_step, passes=passes, host=True, **motion)
    host_ms = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(dev.status, host.status) and np.array_equal(dev.passes_done, host.passes_done) and np.array_equal(dev.first_bad, host.first_bad) and
                all((a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b)) for a, b in zip(dev.paths, host.paths)))
    points_out = [0 if p is None else int(len(p)) for p in dev.paths]
    return dict(passes=passes, device_ms=round(ms[len(ms) // 2], 4), device_ms_min=round(ms[0], 4), call_ms=round(sorted(call)[len(call) // 2], 3),
                host_twin_wall_ms=round(host_ms, 2), device_equals_host=same, host_margin_min=float(host.margin.min()),
                invalid=int((dev.status != 0).sum()), points_in_sum=int(sum(len(p) for p in paths)), points_out_sum=int(sum(points_out)),
                length_in_sum=float(dev.length_in.sum()), length_out_sum=float(dev.length_out.sum()),
                length_ratio=float(dev.length_out.sum() / dev.length_in.sum()), points_out=points_out,
                length_in=[round(float(x), 6) for x in dev.length_in], length_out=[round(float(x), 6) for x in dev.length_out], passes_done=[int(x) for x in dev.passes_done])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=float, default=0.5)
    ap.add_argument("--edge-step", type=float, default=0.05)
    ap.add_argument("--max-iterations", type=int, default=2000)
    ap.add_argument("--max-nodes", type=int, default=2048)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--moving", action="store_true")
    ap.add_argument("--moving-seed", type=int, default=2)
    ap.add_argument("--moving-speed", type=float, nargs=2, default=[0.05, 0.2])
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "tree_moving_bench.json" if a.moving else "shortcut_bench.json")
    from armour_amd import scenes
    from armour_amd.planner import kinova_robot
    from armour_amd.tree_planner import plan_trees
    robot = kinova_robot()
    ws = scenes.reference_worlds()
    O = max(p["obstacles"].shape[0] for _, p in ws)
    obs = np.stack([scenes.pad_obstacles(p["obstacles"], O) for _, p in ws])
    options = dict(step=a.step, edge_step=a.edge_step, max_iterations=a.max_iterations, max_nodes=a.max_nodes)
    plan_trees(robot, obs, np.stack([p["q0"] for _, p in ws]), np.stack([p["goal"] for _, p in ws]), np.full(len(ws), a.seed, dtype=np.uint64), **options)   # warm-up
    plans = plan_trees(robot, obs, np.stack([p["q0"] for _, p in ws]), np.stack([p["goal"] for _, p in ws]), np.full(len(ws), a.seed, dtype=np.uint64), **options)
    found = [w for w, p in enumerate(plans.paths) if p is not None]
    paths = [plans.paths[w] for w in found]
    out = dict(tool="shortcut_bench", robot="kinova_gen3_no_gripper", seed=a.seed, reps=a.reps, **options, worlds=len(ws), found=len(found),
               obstacles_per_world=int(O), tree_plan_device_ms=round(plans.ms, 4), names=[ws[w][0] for w in found], points_in=[int(len(p)) for p in paths])
    if a.moving:
        from armour_amd.planner import default_params
        from tree_bench import seeded_velocities, write_key
        window = dict(t_from=0.0, t_to=float(default_params(1).duration))
        lo, hi = a.moving_speed
        vel = seeded_velocities(ws, O, a.moving_seed, lo, hi)
        starts, goals, seeds = np.stack([p["q0"] for _, p in ws]), np.stack([p["goal"] for _, p in ws]), np.full(len(ws), a.seed, dtype=np.uint64)
        moved = plan_trees(robot, obs, starts, goals, seeds, velocity=vel, **window, **options)
        mfound = [w for w, p in enumerate(moved.paths) if p is not None]
        keep = ("device_ms", "device_ms_min", "call_ms", "host_twin_wall_ms", "device_equals_host", "host_margin_min", "invalid", "points_in_sum", "points_out_sum",
                "length_ratio")
        res = dict(static=measure(robot, obs[found], paths, a.edge_step, 2, a.reps),
                   moving_v0=measure(robot, obs[found], paths, a.edge_step, 2, a.reps, velocity=np.zeros_like(vel[found]), **window),
                   moving=measure(robot, obs[mfound], [moved.paths[w] for w in mfound], a.edge_step, 2, a.reps, velocity=vel[mfound], **window))
        mv = dict(tool="shortcut_bench --moving", seed=a.seed, reps=a.reps, **options, worlds=len(ws), obstacles_per_world=int(O), passes=2,
                  window=[window["t_from"], window["t_to"]], moving_seed=a.moving_seed, speed=[lo, hi], found_static=len(found), found_moving=len(mfound),
                  **{k: {f: r[f] for f in keep} for k, r in res.items()})
        mv["ratio_v0"] = round(res["static"]["device_ms"] / res["moving_v0"]["device_ms"], 4)
        mv["v0_equals_static"] = bool(res["static"]["points_out"] == res["moving_v0"]["points_out"] and res["static"]["length_out"] == res["moving_v0"]["length_out"])
        write_key(a.out, "shortcut", mv)
        print(json.dumps(mv))
        return
    out["passes_1"] = measure(robot, obs[found], paths, a.edge_step, 1, a.reps)
    out["passes_2"] = measure(robot, obs[found], paths, a.edge_step, 2, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
