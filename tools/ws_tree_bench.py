"""The batched workspace RRT* (armour_ws_tree_plan) measured; writes profiles/ws_tree_bench.json (or --out) and prints ONE JSON line.

    python tools/ws_tree_bench.py [--max-iterations 1000] [--max-nodes 1024] [--seed 7] [--reps 10] [--skip-cap] [--skip-host] [--instalments 10] [--out FILE]
    python tools/ws_tree_bench.py --ab PARENT_LIBRARY [--rounds 3] [--out profiles/ws_trees_bench.json]
    python tools/ws_tree_bench.py --moving [--moving-seed 2] [--moving-speed 0.05 0.2] [--out profiles/ws_tree_moving_bench.json]

* `batch`: the 107 reference worlds (scenes.reference_worlds; start and goal POINTS = the end effector of the start and of the goal
  configuration, O padded with scenes.FAR_BOX, every world with the seed --seed, the sampling box ws_planner.workspace_box, the planner's
  default step / edge_step / rewire_radius / goal_rate / goal_tol) in ONE launch: device ms = the entry's event time, median of --reps calls
  after a warm-up; call_ms = the median host time of the same calls (uploads, launch, the paths back); the status counts, path costs,
  rewire counts and tree sizes per world; the host twin's wall time on the same inputs (armour_ws_tree_plan_host, one call, one core), whether
  every output of the two is the same bit for bit, and `digest` = the SHA-256 of the device's outputs (two builds of the library that
  print the same digest computed the same trees: the node-storage A/B of DESIGN.md 4.12f);
* `one_world`: the same for hard_7_window alone (W = 1: one block, so one compute unit -- the planner's stated limit);
* `at_the_cap`: the batch once more with --cap-iterations / ARMOUR_WS_MAX_NODES nodes, i.e. the longest scans the kernel can be asked for.
* `instalments` (--instalments K, default 10; 0: none, as for a library without armour_ws_trees_*): the batch once more on resident trees
  (ws_planner.WorkspaceTrees), every world grown by --max-iterations / K iterations K times; per instalment the median device ms and whole
  call ms over --reps fresh handles, their sums beside the one plan's, the create and first-grow (upload) cost, and whether the digest of
  the last grow's outputs with the trees read back equals the batch's digest.
--skip-host leaves the host twin out (device_equals_host is null then).
--ab: the plan entry of PARENT_LIBRARY (a libarmour_hip.so of the parent commit) against this tree's, on one device in one visit: a fresh
  process of this tool per run with the library chosen by ARMOUR_HIP_LIB, parent, new, parent, new, ... for --rounds rounds; per shape the
  device ms of every run, the medians, the parent's own spread (max - min over its rounds), whether the new median lies within it, and
  whether the digests are equal; the last new run's `instalments` row.  Written to --out (default profiles/ws_trees_bench.json).
--moving: a run of its own that writes profiles/ws_tree_moving_bench.json (or --out): the batch by the static entry, by
  armour_ws_tree_plan_moving at zero velocity on the window [0, 1] (the like-for-like cost of the window rule: same worlds, same trees;
  `ratio_v0` = static ms / moving ms, `v0_equals_static` = the digests are equal) and with every obstacle in linear motion (velocities from
  the stream (--moving-seed, world), speeds --moving-speed LO HI in m/s, as tools/tree_bench.py --moving draws them) on the same window;
  with --ab-static PARENT_LIBRARY also the static batch and one world of the parent commit's library against this one's, alternating in
  fresh processes for --rounds rounds (the key `static_against_parent`).
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

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


def measure(obs, starts, goals, seeds, box, options, reps, with_host=True):
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
    host = plan(trees=True, host=True) if with_host else None
    host_ms = (time.perf_counter() - t0) * 1e3
    return dict(worlds=int(obs.shape[0]), obstacles_per_world=int(obs.shape[1]), device_ms=round(ms[len(ms) // 2], 4), device_ms_min=round(ms[0], 4),
                call_ms=round(sorted(call)[len(call) // 2], 3), host_twin_wall_ms=round(host_ms, 2) if with_host else None,
                device_equals_host=bool(same_bits(dev, host)) if with_host else None,
                digest=digest(dev), host_margin_min=float(host.margin.min()) if with_host else None, status_counts={STATUS[s]: int((dev.status == s).sum()) for s in range(3)},
                iterations=[int(i) for i in dev.iterations], tree_sizes=[int(c) for c in dev.count], rewires=[int(c) for c in dev.rewires],
                path_cost=[round(float(c), 6) for c in dev.path_cost], goal_dist=[round(float(c), 6) for c in dev.goal_dist],
                path_points=[0 if p is None else int(len(p)) for p in dev.paths])


def moving(a, obs, starts, goals, seeds, box, options, ws):
    """--moving: see the module text"""
    from tree_bench import seeded_velocities
    lo, hi = a.moving_speed
    window = dict(t_from=0.0, t_to=1.0)
    legs = dict(static={}, moving_v0=dict(window, velocity=np.zeros(obs.shape[:2] + (3,))),
                moving=dict(window, velocity=seeded_velocities(ws, obs.shape[1], a.moving_seed, lo, hi)))
    keep = ("device_ms", "device_ms_min", "call_ms", "device_equals_host", "host_margin_min", "digest", "status_counts")
    res = {k: measure(obs, starts, goals, seeds, box, dict(options, **kw), a.reps, not a.skip_host) for k, kw in legs.items()}
    out = dict(tool="ws_tree_bench --moving", seed=a.seed, reps=a.reps, **options, worlds=int(obs.shape[0]), obstacles_per_world=int(obs.shape[1]), window=[0.0, 1.0],
               moving_seed=a.moving_seed, speed=[lo, hi], **{k: {f: r[f] for f in keep} for k, r in res.items()})
    out["ratio_v0"] = round(res["static"]["device_ms"] / res["moving_v0"]["device_ms"], 4)
    out["v0_equals_static"] = bool(res["static"]["digest"] == res["moving_v0"]["digest"])
    out["worlds_planned_differently_moving"] = int(sum(x != y for x, y in zip(res["static"]["tree_sizes"], res["moving"]["tree_sizes"])))
    if a.ab_static:
        a.ab, a.instalments = a.ab_static, 0
        rows = ab(a, write=False)
        out["static_against_parent"] = {k: rows[k] for k in ("batch", "one_world")}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def instalments(obs, starts, goals, seeds, box, options, reps, K, plan_row):
    """The batch on resident trees: K grows of max_iterations / K iterations each, on `reps` fresh handles"""
    from armour_amd import _lib
    from armour_amd.ws_planner import WorkspaceTrees
    n, W = options["max_iterations"] // K, obs.shape[0]
    everyone = np.arange(W)
    dev_ms, call_ms, create_ms = [], [], []
    for rep in range(reps + 1):                                                      # (the first handle is the warm-up)
        t0 = time.perf_counter()
        trees = WorkspaceTrees(obs, goals, seeds, box[0], box[1], max_nodes=options["max_nodes"])
        create_ms.append((time.perf_counter() - t0) * 1e3)
        d, c = [], []
        for k in range(K):
            t0 = time.perf_counter()
            res = trees.grow(everyone, starts, n)
            c.append((time.perf_counter() - t0) * 1e3)
            d.append(res.ms)
        if rep:
            dev_ms.append(d)
            call_ms.append(c)
        if rep == reps:
            t = trees.read(everyone)
            grown = _lib.Result(**{k: getattr(res, k) for k in ("status", "iterations", "count", "rewires", "chain_kept", "path_cost", "goal_dist", "paths")},
                                nodes=t.nodes, parent=t.parent, node_cost=t.node_cost)
        trees.close()
    med = lambda rows: [round(float(np.median([r[k] for r in rows])), 4) for k in range(K)]
    d, c = med(dev_ms), med(call_ms)
    return dict(instalments=K, iterations_per_instalment=n, handles=reps, device_ms=d, call_ms=c, device_ms_sum=round(sum(d), 4), call_ms_sum=round(sum(c), 3),
                first_call_ms_with_upload=c[0], create_ms=round(float(np.median(create_ms[1:])), 3), one_plan_device_ms=plan_row["device_ms"],
                one_plan_call_ms=plan_row["call_ms"], digest=digest(grown), equals_one_plan=bool(digest(grown) == plan_row["digest"]),
                expected_ms_per_instalment="iterations_per_instalment x 6.7 us + one launch (arithmetic from DESIGN.md 4.12f, not a measurement)")


SHAPES = ("batch", "one_world", "at_the_cap")


def ab(a, write=True):
    """--ab: parent, new, parent, new, ... in fresh processes; see the module text"""
    runs = {"parent": [], "new": []}
    with tempfile.TemporaryDirectory() as tmp:
        for rnd in range(a.rounds):
            for side in ("parent", "new"):
                out = os.path.join(tmp, "%s_%d.json" % (side, rnd))
                env = dict(os.environ)
                env.pop("ARMOUR_HIP_LIB", None)
                if side == "parent":
                    env["ARMOUR_HIP_LIB"] = os.path.abspath(a.ab)
                cmd = [sys.executable, os.path.abspath(__file__), "--skip-host", "--out", out, "--max-iterations", str(a.max_iterations), "--max-nodes", str(a.max_nodes),
                       "--cap-iterations", str(a.cap_iterations), "--seed", str(a.seed), "--reps", str(a.reps),
                       "--instalments", str(a.instalments if side == "new" and rnd == a.rounds - 1 else 0)] + (["--skip-cap"] if a.skip_cap else [])
                subprocess.run(cmd, env=env, check=True, stdout=subprocess.DEVNULL, timeout=600)
                runs[side].append(json.load(open(out)))
    rows = {}
    for shape in (s for s in SHAPES if s in runs["new"][0]):
        p, n = [r[shape]["device_ms"] for r in runs["parent"]], [r[shape]["device_ms"] for r in runs["new"]]
        pm, nm, spread = float(np.median(p)), float(np.median(n)), max(p) - min(p)
        digests = {r[shape]["digest"] for side in runs for r in runs[side]}
        rows[shape] = dict(parent_device_ms=p, new_device_ms=n, parent_median=pm, new_median=nm, parent_spread=round(spread, 4), new_over_parent=round(nm / pm, 4),
                           within_parent_spread=bool(nm <= pm + spread), digests_equal=len(digests) == 1, digest=runs["new"][-1][shape]["digest"],
                           parent_call_ms=[r[shape]["call_ms"] for r in runs["parent"]], new_call_ms=[r[shape]["call_ms"] for r in runs["new"]])
    if not write:
        return rows
    last = runs["new"][-1]
    out = dict(tool="ws_tree_bench --ab", what="armour_ws_tree_plan of the parent commit's library against this one on one MI355X in one visit: parent, new, parent, new, "
               "...; a fresh process per run, the library chosen by ARMOUR_HIP_LIB.  device ms = the median of `reps` launches per run; parent_spread = max - min of "
               "the parent's runs; within_parent_spread: the new median is not above the parent's median by more than that spread.",
               rounds=a.rounds, **{k: last[k] for k in ("robot", "seed", "reps", "max_iterations", "max_nodes", "step", "edge_step", "rewire_radius", "goal_rate", "goal_tol")},
               cap=dict(max_iterations=a.cap_iterations), plan_entry=rows, instalments=last.get("instalments"))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-iterations", type=int, default=1000)
    ap.add_argument("--max-nodes", type=int, default=1024)
    ap.add_argument("--cap-iterations", type=int, default=4500)
    ap.add_argument("--skip-cap", action="store_true")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--instalments", type=int, default=10)
    ap.add_argument("--ab")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--moving", action="store_true")
    ap.add_argument("--moving-seed", type=int, default=2)
    ap.add_argument("--moving-speed", type=float, nargs=2, default=[0.05, 0.2])
    ap.add_argument("--ab-static")
    ap.add_argument("--out")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "ws_tree_moving_bench.json" if a.moving else "ws_trees_bench.json" if a.ab else "ws_tree_bench.json")
    if a.ab:
        return ab(a)
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
    if a.moving:
        return moving(a, obs, starts, goals, seeds, box, options, ws)
    out["batch"] = dict(measure(obs, starts, goals, seeds, box, options, a.reps, not a.skip_host), names=names)
    w = names.index("hard_7_window")
    out["one_world"] = dict(measure(obs[w:w + 1], starts[w:w + 1], goals[w:w + 1], seeds[w:w + 1], box, options, a.reps, not a.skip_host), name=names[w])
    if a.instalments > 0:
        out["instalments"] = instalments(obs, starts, goals, seeds, box, options, a.reps, a.instalments, out["batch"])
    cap = dict(max_iterations=a.cap_iterations, max_nodes=_lib.WS_MAX_NODES)
    full = None if a.skip_cap else measure(obs, starts, goals, seeds, box, cap, max(a.reps // 3, 1), not a.skip_host)
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
