"""The batched tree planner (armour_tree_plan) measured; writes profiles/tree_bench.json (or --out) and prints ONE JSON line.

    python tools/tree_bench.py [--step 0.5] [--edge-step 0.05] [--max-iterations 2000] [--max-nodes 2048] [--seed 7] [--reps 10] [--out FILE]

* `batch`: the 107 reference worlds (scenes.reference_worlds, each from its start to its goal, O padded with scenes.FAR_BOX, every world
  with the seed --seed) in ONE launch: device ms = the entry's event time, median of --reps calls after a warm-up; call_ms = the median
  host time of the same calls (uploads, launch, the paths back); the status counts, the iterations and tree sizes per world; and the host
  twin's wall time on the same inputs (armour_tree_plan_host, one call), with whether both gave the same statuses, iterations and paths;
* `one_world`: the same for hard_7_window alone (W = 1: one block, so one compute unit -- the planner's stated limit).
* --moving: a run of its own that leaves profiles/tree_bench.json alone and writes the key `tree` of profiles/tree_moving_bench.json (or
  --out; the file's other keys are kept): the batch above by the static entry, by armour_tree_plan_moving at zero velocity on the same
  window (the like-for-like cost of the window rule: same worlds, same trees; `ratio_v0` = static ms / moving ms) and with every obstacle
  in linear motion (seeded velocities, --moving-seed, speeds --moving-speed LO HI in m/s, as tools/trial_bench.py --moving draws them) on
  the window [0, the plan's duration], all in this process, with the share of worlds found and whether device and host twin agree.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATUS = ("not_found", "found", "start_blocked", "goal_blocked", "tree_full")


def seeded_velocities(ws, O, seed, lo, hi):
    """[W, O, 3]: world i's obstacles get random directions and speeds lo .. hi m/s from the stream (seed, i); the padding stands still"""
    vel = np.zeros((len(ws), O, 3))
    for i, (_, p) in enumerate(ws):
        rng = np.random.default_rng([seed, i])
        v = rng.normal(size=(np.asarray(p["obstacles"]).reshape(-1, 12).shape[0], 3))
        vel[i, :v.shape[0]] = v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.uniform(lo, hi, (v.shape[0], 1))
    return vel


def write_key(path, key, value):
    """profiles/tree_moving_bench.json is shared by this tool, tools/shortcut_bench.py and the comparison with the parent commit: one key each"""
    out = {}
    if os.path.exists(path):
        with open(path) as f:
            out = json.load(f)
    out[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def measure(robot, obs, starts, goals, seeds, options, reps):
    from armour_amd.tree_planner import plan_trees
    plan_trees(robot, obs, starts, goals, seeds, **options)                         # warm-up
    runs, call = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        runs.append(plan_trees(robot, obs, starts, goals, seeds, **options))
        call.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(r.ms for r in runs)
    dev = plan_trees(robot, obs, starts, goals, seeds, trees=True, **options)
    t0 = time.perf_counter()
    host = plan_trees(robot, obs, starts, goals, seeds, host=True, **options)
    host_ms = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(dev.status, host.status) and np.array_equal(dev.iterations, host.iterations) and
                all((a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b)) for a, b in zip(dev.paths, host.paths)))
    return dict(worlds=int(obs.shape[0]), obstacles_per_world=int(obs.shape[1]), device_ms=round(ms[len(ms) // 2], 4), device_ms_min=round(ms[0], 4),
                call_ms=round(sorted(call)[len(call) // 2], 3), host_twin_wall_ms=round(host_ms, 2), device_equals_host=same,
                host_margin_min=float(host.margin.min()), status_counts={STATUS[s]: int((dev.status == s).sum()) for s in range(5)},
                iterations=[int(i) for i in dev.iterations], tree_sizes=[[int(c[0]), int(c[1])] for c in dev.count],
                path_points=[0 if p is None else int(len(p)) for p in dev.paths])


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
    a.out = a.out or os.path.join(ROOT, "profiles", "tree_moving_bench.json" if a.moving else "tree_bench.json")
    from armour_amd import scenes
    from armour_amd.planner import kinova_robot
    robot = kinova_robot()
    ws = scenes.reference_worlds()
    names = [name for name, _ in ws]
    O = max(p["obstacles"].shape[0] for _, p in ws)
    obs = np.stack([scenes.pad_obstacles(p["obstacles"], O) for _, p in ws])
    starts = np.stack([p["q0"] for _, p in ws])
    goals = np.stack([p["goal"] for _, p in ws])
    seeds = np.full(len(ws), a.seed, dtype=np.uint64)
    options = dict(step=a.step, edge_step=a.edge_step, max_iterations=a.max_iterations, max_nodes=a.max_nodes)
    if a.moving:
        from armour_amd.planner import default_params
        window = dict(t_from=0.0, t_to=float(default_params(1).duration))
        lo, hi = a.moving_speed
        keep = ("device_ms", "device_ms_min", "call_ms", "host_twin_wall_ms", "device_equals_host", "host_margin_min", "status_counts")
        legs = dict(static={}, moving_v0=dict(window, velocity=np.zeros(obs.shape[:2] + (3,))),
                    moving=dict(window, velocity=seeded_velocities(ws, O, a.moving_seed, lo, hi)))
        res = {k: measure(robot, obs, starts, goals, seeds, dict(options, **kw), a.reps) for k, kw in legs.items()}
        out = dict(tool="tree_bench --moving", seed=a.seed, reps=a.reps, **options, worlds=len(ws), obstacles_per_world=int(O), window=[window["t_from"], window["t_to"]],
                   moving_seed=a.moving_seed, speed=[lo, hi], **{k: {f: r[f] for f in keep} for k, r in res.items()})
        out["ratio_v0"] = round(res["static"]["device_ms"] / res["moving_v0"]["device_ms"], 4)
        out["v0_equals_static"] = bool(res["static"]["iterations"] == res["moving_v0"]["iterations"] and res["static"]["path_points"] == res["moving_v0"]["path_points"])
        out["found_share"] = {k: round(r["status_counts"]["found"] / len(ws), 4) for k, r in res.items()}
        write_key(a.out, "tree", out)
        print(json.dumps(out))
        return
    out = dict(tool="tree_bench", robot="kinova_gen3_no_gripper", seed=a.seed, reps=a.reps, **options)
    out["batch"] = dict(measure(robot, obs, starts, goals, seeds, options, a.reps), names=names)
    w = names.index("hard_7_window")
    out["one_world"] = dict(measure(robot, obs[w:w + 1], starts[w:w + 1], goals[w:w + 1], seeds[w:w + 1], options, a.reps), name=names[w])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
