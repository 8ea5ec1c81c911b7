"""Whole planning trials (armour_amd.trials.run_trials) and the path audit (armour_path_audit) measured; writes profiles/trial_bench.json
and prints ONE JSON line.

    python tools/trial_bench.py [--T 128] [--max-iterations 400] [--steps 0.01 0.05] [--reps 10] [--kernel-stats] [--hlp straight|roadmap-field [--batched]|tree [--tree-shortcut P] [--tree-mode seed]|workspace]

* the 107 reference worlds end to end: outcomes, iterations, build / solve ms per batch iteration, audit ms, and -- re-auditing every
  executed piece -- the undecided pieces at each of --steps (with and without the controller's ultimate bound as tube);
* audit throughput: (piece, sub-interval) items per second of the trial's own executed pieces at W = 1 (world 0's) and W = 107 (all),
  kernel ms = the median `ms` of armour_path_audit over --reps launches, verdict mode and clearance mode;
* --hlp roadmap-field: the same worlds once more with the roadmap's cost-to-go fields as the high-level planner (armour_amd.roadmap.field_hlps
  on uniform_roadmap(--roadmap-nodes, --roadmap-radius, 16, seed 0)): `hlp_outcomes` holds the outcome counts under both HLPs, the roadmap run's
  check / field ms, the worlds whose outcome differs and `ms_per_batch` (the waypoint queries' hlp_ms next to build, solve and audit ms);
  with --batched the waypoints of an iteration come from one Roadmap.descend_many call.  Everything else in the file is the straight-line
  run's, as before;
* --hlp tree: the same worlds once more with the batched tree planner as the high-level planner (armour_amd.tree_planner.tree_hlps: a fresh
  RRT-Connect per world and iteration, all live worlds in one armour_tree_plan call; --tree-seed, --tree-iterations, --tree-nodes):
  `hlp_outcomes_tree` holds the outcome counts beside the straight-line run's, the worlds whose outcome differs and `ms_per_batch` (hlp_ms next
  to build, solve and audit ms).  One run, one seed.  A `hlp_outcomes` section that profiles/trial_bench.json already holds (a roadmap-field
  run) is kept, so that the three planners' rows stand side by side.  With --tree-shortcut P (every found path shortened with P passes of
  armour_path_shortcut) and / or --tree-mode seed (the last path is offered first; a tree grows only when it fails) the run goes under
  `hlp_outcomes_tree_seed` instead, with the number of reused paths and hard_2_wall's outcome by name, and the `hlp_outcomes_tree` row that
  the file already holds is kept for comparison;
* --hlp workspace: the same worlds once more with the reference's own high-level planner, the end-effector RRT* (armour_amd.ws_planner.
  workspace_hlps: a fresh workspace tree per world and iteration, all live worlds in one armour_ws_tree_plan call and one armour_ik call;
  --tree-seed, --ws-iterations, --ws-nodes, --ws-lookahead in metres, --ws-buffer; --ws-mode keep: ONE resident tree per world, grown by
  --ws-iterations at every call and bounded by --ws-nodes over the whole trial -- that run adds the row
  `hlp_outcomes_workspace_keep["<iterations>_per_call"]` to the saved profile, beside the 'new' row, and measures nothing else again):
  `hlp_outcomes_workspace` holds the outcome counts beside
  the straight-line run's, the worlds whose outcome differs, how many waypoints fell back to the goal configuration and `ms_per_batch`.  The
  sections of the other planners that profiles/trial_bench.json already holds are kept;
* --moving: a run of its own that writes profiles/trial_moving_bench.json and leaves profiles/trial_bench.json alone: the same worlds with every
  obstacle in linear motion (seeded velocities, --moving-seed, speeds --moving-speed LO HI in m/s; run_trials(velocities=...)) under the
  straight-line planner, under armour_amd.roadmap.moving_field_hlps (device_roadmap(--roadmap-nodes, --roadmap-radius, 16, seed 0): one
  check_moving, one field and one descend_many per iteration) and under armour_amd.tree_planner.moving_tree_hlps (the --tree-* options; no
  roadmap: at most three launches per iteration) and -- the row `moving_workspace`, run when named in --moving-planners -- under
  armour_amd.ws_planner.moving_workspace_hlps (the --ws-* options, mode 'new': one armour_ws_tree_plan_moving and one armour_ik_moving call per
  iteration): outcome counts of each, `struck_at_rest` among them, the pieces by kind and verdict, and
  hlp / build / solve / audit ms per batch iteration.  --moving-planners runs some of the four rows and keeps the file's others.
  Records, not pass criteria;
* --moving --spacetime: the same moving worlds under armour_amd.roadmap.spacetime_hlps (one plan_slices per iteration: --spacetime-K slices of
  --spacetime-dt seconds) at each of --spacetime-speeds rad/s, written to profiles/trial_spacetime_bench.json: the record layout of --moving per
  speed, and the share of waypoint queries for which the search found a path within its slices.  Records, not pass criteria;
* --kernel-stats: a `rocprofv3 --kernel-trace --stats` summary of the audit kernel in profiles/trial_kernel_stats.csv, taken in a run of
  its own: a fresh child process under a time limit that only repeats the W = 107 audit.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def executed_pieces(res):
    """Every executed piece of a run_trials result as the arrays armour_path_audit takes (world = index into res["worlds"])."""
    rows = [(w, r["piece"]) for w, wr in enumerate(res["worlds"]) for r in wr["records"]]
    world = np.array([w for w, _ in rows], dtype=np.int32)
    cols = [np.stack([p[c] for _, p in rows]) for c in range(4)]
    return world, cols, np.array([p[4] for _, p in rows]), np.array([p[5] for _, p in rows])


def throughput(robot, obs, world, cols, ta, tb, k_range, D, step, reps, clearance):
    from armour_amd.path_audit import audit, audit_items
    items = int(audit_items(robot, *cols, k_range, D, ta, tb, step=step).sum())
    audit(robot, obs, world, *cols, k_range, D, ta, tb, step=step, clearance=clearance)       # warm-up
    ms = sorted(audit(robot, obs, world, *cols, k_range, D, ta, tb, step=step, clearance=clearance).ms for _ in range(reps))
    kms = ms[len(ms) // 2]
    return dict(pieces=int(world.size), items=items, kernel_ms=round(kms, 4), kernel_ms_min=round(ms[0], 4), items_per_s=round(items / (kms * 1e-3)))


def child(path, reps):
    """The profiled run: nothing but the saved W = 107 audit, `reps` times."""
    from armour_amd.path_audit import audit
    from armour_amd.planner import kinova_robot
    d = np.load(path)
    for _ in range(reps):
        audit(kinova_robot(), d["obs"], d["world"], d["q0"], d["qd0"], d["qdd0"], d["k"], d["k_range"], float(d["D"]), d["ta"], d["tb"], step=float(d["step"]))


def kernel_stats(saved, reps, out_csv):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "trial", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", saved, "--reps", str(reps)]
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        if run.returncode != 0:
            return dict(error=run.stderr[-400:])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return dict(error="no kernel_stats.csv written")
        rows = list(csv.reader(open(files[0])))
        os.makedirs(os.path.dirname(out_csv), exist_ok=True)
        with open(out_csv, "w", newline="") as f:
            csv.writer(f).writerows(rows)
        hit = [dict(zip(rows[0], r)) for r in rows[1:] if "path_audit_kernel" in r[0]]
        return hit[0] if hit else dict(error="path_audit_kernel not in the trace")


def roadmap_field_trials(robot, ws, straight, a):
    """The worlds once more under field_hlps; outcome counts under both HLPs and the worlds that end differently."""
    import time
    from armour_amd.roadmap import Roadmap, field_hlps, uniform_roadmap
    from armour_amd.trials import OUTCOMES, run_trials
    n = robot.num_factors
    cont = np.array(robot.continuous[:n]).astype(bool)
    nodes, edges = uniform_roadmap(a.roadmap_nodes, a.roadmap_radius, 16, 0, np.array(robot.state_limits_lb[:n]), np.array(robot.state_limits_ub[:n]), cont)
    rm = Roadmap(robot, nodes, edges, continuous=cont.astype(np.uint8))
    t0 = time.perf_counter()
    make = field_hlps(rm, ws, batched=a.batched)
    setup_ms = (time.perf_counter() - t0) * 1e3
    res = run_trials(ws, hlp=make, T=a.T, max_iterations=a.max_iterations, audit_step=a.steps[0])
    rm.close()
    per_batch = lambda key: dict(mean=float(np.mean([b[key] for b in res["batches"]])), max=float(np.max([b[key] for b in res["batches"]])))
    count = lambda r: {o: sum(1 for w in r["worlds"] if w["outcome"] == o) for o in OUTCOMES}
    return dict(roadmap=dict(N=int(nodes.shape[0]), E=int(edges.shape[0]), radius=a.roadmap_radius, check_and_field_wall_ms=setup_ms),
                straight=count(straight), roadmap_field=count(res), roadmap_field_summary=res["summary"], batched=bool(a.batched),
                ms_per_batch={key: per_batch(key) for key in ("hlp_ms", "build_ms", "solve_ms", "audit_ms")}, first_batch=res["batches"][0],
                changed={w["name"]: [s["outcome"], w["outcome"]] for s, w in zip(straight["worlds"], res["worlds"]) if s["outcome"] != w["outcome"]})


def moving_trials(robot, ws, a):
    """The worlds with moving obstacles under the straight-line planner and under moving_field_hlps: outcomes, pieces by kind and verdict, ms per batch."""
    from armour_amd.roadmap import Roadmap, device_roadmap, moving_field_hlps
    from armour_amd.trials import OUTCOMES, STRUCK_OUTCOME, run_trials
    n = robot.num_factors
    cont = np.array(robot.continuous[:n]).astype(bool)
    lo, hi = a.moving_speed
    vel = []
    for i, (_, p) in enumerate(ws):
        rng = np.random.default_rng([a.moving_seed, i])
        v = rng.normal(size=(np.asarray(p["obstacles"]).reshape(-1, 12).shape[0], 3))
        vel.append(v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.uniform(lo, hi, (v.shape[0], 1)))
    out = dict(tool="trial_bench --moving", T=a.T, worlds=len(ws), max_iterations=a.max_iterations, seed=a.moving_seed, speed=[lo, hi])
    rm = None
    if "moving_field" in a.moving_planners:
        nodes, edges = device_roadmap(robot, a.roadmap_nodes, a.roadmap_radius, 16, 0, np.array(robot.state_limits_lb[:n]), np.array(robot.state_limits_ub[:n]), cont)
        rm = Roadmap(robot, nodes, edges, continuous=cont.astype(np.uint8))
        out["roadmap"] = dict(N=int(nodes.shape[0]), E=int(edges.shape[0]), radius=a.roadmap_radius)
    from armour_amd.tree_planner import moving_tree_hlps
    from armour_amd.ws_planner import moving_workspace_hlps
    planners = dict(moving_workspace=lambda: moving_workspace_hlps(ws, robot, vel, seed=a.tree_seed, lookahead=a.ws_lookahead, max_iterations=a.ws_iterations,
                                                                   max_nodes=a.ws_nodes, buffer=a.ws_buffer),
                    straight=lambda: "straight", moving_field=lambda: moving_field_hlps(rm, ws, vel),
                    moving_tree=lambda: moving_tree_hlps(ws, robot, vel, seed=a.tree_seed, shortcut=a.tree_shortcut, mode=a.tree_mode, max_iterations=a.tree_iterations,
                                                         max_nodes=a.tree_nodes))
    if "moving_workspace" in a.moving_planners:
        out["workspace"] = dict(seed=a.tree_seed, lookahead_m=a.ws_lookahead, max_iterations=a.ws_iterations, max_nodes=a.ws_nodes, buffer=a.ws_buffer, mode="new")
    if "moving_tree" in a.moving_planners:
        out["tree"] = dict(seed=a.tree_seed, shortcut=a.tree_shortcut, mode=a.tree_mode, max_iterations=a.tree_iterations, max_nodes=a.tree_nodes)
    for key in a.moving_planners:
        hlp = planners[key]()
        res = run_trials(ws, hlp=hlp, T=a.T, max_iterations=a.max_iterations, audit_step=a.steps[0], velocities=vel)
        recs = [r for w in res["worlds"] for r in w["records"]]
        per_batch = lambda k: dict(mean=float(np.mean([b[k] for b in res["batches"]])), max=float(np.max([b[k] for b in res["batches"]])))
        extra = dict(fallbacks=int(sum(h.fallbacks for h in hlp.hlps.values())), calls=int(sum(h.calls for h in hlp.hlps.values()))) if key == "moving_workspace" else {}
        out[key] = dict(**extra, outcomes={o: sum(1 for w in res["worlds"] if w["outcome"] == o) for o in OUTCOMES + (STRUCK_OUTCOME,)}, summary=res["summary"],
                        pieces={kind: {str(v): sum(1 for r in recs if r["executed"] == kind and r["audit_verdict"] == v) for v in (0, 1, 2)}
                                for kind in ("plan", "brake", "stay")},
                        ms_per_batch={k: per_batch(k) for k in ("hlp_ms", "build_ms", "solve_ms", "audit_ms")}, first_batch=res["batches"][0])
    if rm is not None:
        rm.close()
    return out


def spacetime_trials(robot, ws, a):
    """--moving --spacetime: the moving worlds under armour_amd.roadmap.spacetime_hlps at each of --spacetime-speeds (the velocities, the roadmap
    and the record layout of moving_trials; --spacetime-dt, --spacetime-K).  The outcomes are records, not pass criteria."""
    from armour_amd.roadmap import Roadmap, device_roadmap, spacetime_hlps
    from armour_amd.trials import OUTCOMES, STRUCK_OUTCOME, run_trials
    n = robot.num_factors
    cont = np.array(robot.continuous[:n]).astype(bool)
    lo, hi = a.moving_speed
    vel = []
    for i, (_, p) in enumerate(ws):
        rng = np.random.default_rng([a.moving_seed, i])
        v = rng.normal(size=(np.asarray(p["obstacles"]).reshape(-1, 12).shape[0], 3))
        vel.append(v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.uniform(lo, hi, (v.shape[0], 1)))
    nodes, edges = device_roadmap(robot, a.roadmap_nodes, a.roadmap_radius, 16, 0, np.array(robot.state_limits_lb[:n]), np.array(robot.state_limits_ub[:n]), cont)
    rm = Roadmap(robot, nodes, edges, continuous=cont.astype(np.uint8))
    out = dict(tool="trial_bench --moving --spacetime", T=a.T, worlds=len(ws), max_iterations=a.max_iterations, seed=a.moving_seed, speed=[lo, hi],
               dt=a.spacetime_dt, K=a.spacetime_K, roadmap=dict(N=int(nodes.shape[0]), E=int(edges.shape[0]), radius=a.roadmap_radius))
    for speed in a.spacetime_speeds:
        make = spacetime_hlps(rm, ws, vel, speed, dt=a.spacetime_dt, K=a.spacetime_K)
        found = []
        inner = make.get_waypoints

        def counting(indices, qs, lookaheads, inner=inner, make=make, found=found):
            wps = inner(indices, qs, lookaheads)
            found.append((sum(make.last_plans[i]["path"] is not None for i in indices), len(indices)))
            return wps

        make.get_waypoints = counting
        res = run_trials(ws, hlp=make, T=a.T, max_iterations=a.max_iterations, audit_step=a.steps[0], velocities=vel)
        recs = [r for w in res["worlds"] for r in w["records"]]
        per_batch = lambda k: dict(mean=float(np.mean([b[k] for b in res["batches"]])), max=float(np.max([b[k] for b in res["batches"]])))
        out["speed_%g" % speed] = dict(outcomes={o: sum(1 for w in res["worlds"] if w["outcome"] == o) for o in OUTCOMES + (STRUCK_OUTCOME,)}, summary=res["summary"],
                                       pieces={kind: {str(v): sum(1 for r in recs if r["executed"] == kind and r["audit_verdict"] == v) for v in (0, 1, 2)}
                                               for kind in ("plan", "brake", "stay")},
                                       paths_found_share=float(sum(f for f, _ in found)) / max(1, sum(q for _, q in found)),
                                       ms_per_batch={k: per_batch(k) for k in ("hlp_ms", "build_ms", "solve_ms", "audit_ms")}, first_batch=res["batches"][0])
    rm.close()
    return out


def tree_trials(robot, ws, straight, a):
    """The worlds once more under tree_hlps; outcome counts under both HLPs and the worlds that end differently."""
    from armour_amd.tree_planner import tree_hlps
    from armour_amd.trials import OUTCOMES, run_trials
    options = dict(step=0.5, edge_step=0.05, max_iterations=a.tree_iterations, max_nodes=a.tree_nodes)
    make = tree_hlps(ws, robot, seed=a.tree_seed, shortcut=a.tree_shortcut, mode=a.tree_mode, **options)
    res = run_trials(ws, hlp=make, T=a.T, max_iterations=a.max_iterations, audit_step=a.steps[0])
    per_batch = lambda key: dict(mean=float(np.mean([b[key] for b in res["batches"]])), max=float(np.max([b[key] for b in res["batches"]])))
    count = lambda r: {o: sum(1 for w in r["worlds"] if w["outcome"] == o) for o in OUTCOMES}
    extra = {}
    if a.tree_shortcut or a.tree_mode != "new":
        extra = dict(shortcut=a.tree_shortcut, mode=a.tree_mode, hlp_calls=int(sum(h.calls for h in make.hlps.values())),
                     paths_reused=int(sum(h.reused for h in make.hlps.values())),
                     hard_scenarios={w["name"]: w["outcome"] for w in res["worlds"][100:]})
    return dict(tree=dict(options, seed=a.tree_seed, **extra), straight=count(straight), tree_outcomes=count(res), tree_summary=res["summary"],
                ms_per_batch={key: per_batch(key) for key in ("hlp_ms", "build_ms", "solve_ms", "audit_ms")}, first_batch=res["batches"][0],
                changed={w["name"]: [s["outcome"], w["outcome"]] for s, w in zip(straight["worlds"], res["worlds"]) if s["outcome"] != w["outcome"]})


def workspace_trials(robot, ws, straight, a):
    """The worlds once more under workspace_hlps; outcome counts under both HLPs and the worlds that end differently."""
    from armour_amd.trials import OUTCOMES, run_trials
    from armour_amd.ws_planner import EDGE_STEP, GOAL_RATE, GOAL_TOL, REWIRE_RADIUS, STEP, workspace_hlps
    options = dict(max_iterations=a.ws_iterations, max_nodes=a.ws_nodes, buffer=a.ws_buffer)
    make = workspace_hlps(ws, robot, seed=a.tree_seed, lookahead=a.ws_lookahead, mode=a.ws_mode, **options)
    res = run_trials(ws, hlp=make, T=a.T, max_iterations=a.max_iterations, audit_step=a.steps[0])
    per_batch = lambda key: dict(mean=float(np.mean([b[key] for b in res["batches"]])), max=float(np.max([b[key] for b in res["batches"]])))
    count = lambda r: {o: sum(1 for w in r["worlds"] if w["outcome"] == o) for o in OUTCOMES}
    calls, fallbacks = int(sum(h.calls for h in make.hlps.values())), int(sum(h.fallbacks for h in make.hlps.values()))
    if a.ws_mode == "keep":
        options = dict(options, mode="keep", iterations_per_call=a.ws_iterations, tree_sizes_at_the_end=dict(
            mean=float(np.mean([h.count for h in make.hlps.values()])), max=int(max(h.count for h in make.hlps.values())),
            full=int(sum(h.count >= a.ws_nodes for h in make.hlps.values()))))
        make.close()
    return dict(workspace=dict(options, seed=a.tree_seed, lookahead_m=a.ws_lookahead, step=STEP, edge_step=EDGE_STEP, rewire_radius=REWIRE_RADIUS, goal_rate=GOAL_RATE,
                               goal_tol=GOAL_TOL, hlp_calls=calls, goal_configuration_fallbacks=fallbacks),
                straight=count(straight), workspace_outcomes=count(res), workspace_summary=res["summary"],
                hard_scenarios={w["name"]: w["outcome"] for w in res["worlds"][100:]},
                ms_per_batch={key: per_batch(key) for key in ("hlp_ms", "build_ms", "solve_ms", "audit_ms")}, first_batch=res["batches"][0],
                changed={w["name"]: [s["outcome"], w["outcome"]] for s, w in zip(straight["worlds"], res["worlds"]) if s["outcome"] != w["outcome"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--max-iterations", type=int, default=400)
    ap.add_argument("--steps", type=float, nargs="+", default=[0.01, 0.05])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--hlp", choices=["straight", "roadmap-field", "tree", "workspace"], default="straight")
    ap.add_argument("--ws-iterations", type=int, default=1000)
    ap.add_argument("--ws-nodes", type=int, default=1024)
    ap.add_argument("--ws-lookahead", type=float, default=0.1)
    ap.add_argument("--ws-buffer", type=float, default=0.0)
    ap.add_argument("--ws-mode", choices=["new", "keep"], default="new")
    ap.add_argument("--tree-seed", type=int, default=0)
    ap.add_argument("--tree-iterations", type=int, default=2000)
    ap.add_argument("--tree-nodes", type=int, default=2048)
    ap.add_argument("--tree-shortcut", type=int, default=0)
    ap.add_argument("--tree-mode", choices=["new", "seed"], default="new")
    ap.add_argument("--roadmap-nodes", type=int, default=20000)
    ap.add_argument("--roadmap-radius", type=float, default=1.5)
    ap.add_argument("--batched", action="store_true")
    ap.add_argument("--moving", action="store_true")
    ap.add_argument("--moving-seed", type=int, default=2)
    ap.add_argument("--moving-speed", type=float, nargs=2, default=[0.05, 0.2])
    ap.add_argument("--moving-planners", nargs="+", choices=["straight", "moving_field", "moving_tree", "moving_workspace"],
                    default=["straight", "moving_field", "moving_tree"])
    ap.add_argument("--spacetime", action="store_true")
    ap.add_argument("--spacetime-speeds", type=float, nargs="+", default=[0.5, 1.0, 2.0])
    ap.add_argument("--spacetime-dt", type=float, default=0.25)
    ap.add_argument("--spacetime-K", type=int, default=32)
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    from armour_amd import scenes
    from armour_amd.path_audit import audit
    from armour_amd.planner import kinova_robot
    from armour_amd.tracking import ultimate_bound
    from armour_amd.trials import run_trials
    robot = kinova_robot()
    ws = scenes.reference_worlds()
    if a.moving:
        out = spacetime_trials(robot, ws, a) if a.spacetime else moving_trials(robot, ws, a)
        path = os.path.join(ROOT, "profiles", "trial_spacetime_bench.json" if a.spacetime else "trial_moving_bench.json")
        if not a.spacetime and os.path.exists(path):      # the rows of the planners that this run left out are kept
            with open(path) as f:
                out = dict(json.load(f), **out)
        with open(path, "w") as f:
            json.dump(out, f, indent=1, default=float)
            f.write("\n")
        print(json.dumps(out, default=float))
        return
    res = run_trials(ws, T=a.T, max_iterations=a.max_iterations, audit_step=a.steps[0])
    s = res["summary"]
    its = np.array([w["iterations"] for w in res["worlds"]])
    bt = res["batches"]
    out = dict(tool="trial_bench", robot="kinova_gen3_no_gripper", T=a.T, worlds=len(ws), max_iterations=a.max_iterations, summary=s,
               outcomes_saved_scenes={o: sum(1 for w in res["worlds"][:100] if w["outcome"] == o) for o in ("goal", "collision", "stuck", "iteration_limit")},
               outcomes_hard_scenarios={w["name"]: w["outcome"] for w in res["worlds"][100:]},
               iterations=dict(mean=float(its.mean()), max=int(its.max()), min=int(its.min())),
               build_ms_per_batch=dict(mean=float(np.mean([b["build_ms"] for b in bt])), max=float(np.max([b["build_ms"] for b in bt]))),
               solve_ms_per_batch=dict(mean=float(np.mean([b["solve_ms"] for b in bt])), max=float(np.max([b["solve_ms"] for b in bt]))),
               audit_ms_per_batch=dict(mean=float(np.mean([b["audit_ms"] for b in bt])), max=float(np.max([b["audit_ms"] for b in bt]))),
               first_batch=bt[0], min_clearance=float(min(r["clearance"] for w in res["worlds"] for r in w["records"])))
    if a.hlp == "roadmap-field":
        out["hlp_outcomes"] = roadmap_field_trials(robot, ws, res, a)
    saved_json = os.path.join(ROOT, "profiles", "trial_bench.json")
    if a.hlp == "tree":
        variant = a.tree_shortcut or a.tree_mode != "new"
        out["hlp_outcomes_tree_seed" if variant else "hlp_outcomes_tree"] = tree_trials(robot, ws, res, a)
    if a.hlp == "workspace" and a.ws_mode == "keep":
        # one row of a finished profile: the 'keep' run at this many iterations per call goes beside the 'new' row, and nothing else of the
        # saved file is measured again
        saved = json.load(open(saved_json))
        row = workspace_trials(robot, ws, res, a)
        row["new_mode_row"] = {k: saved["hlp_outcomes_workspace"][k] for k in ("workspace_outcomes", "hard_scenarios") if k in saved.get("hlp_outcomes_workspace", {})}
        if "ms_per_batch" in saved.get("hlp_outcomes_workspace", {}):
            row["new_mode_row"]["hlp_ms_mean"] = saved["hlp_outcomes_workspace"]["ms_per_batch"]["hlp_ms"]["mean"]
        saved.setdefault("hlp_outcomes_workspace_keep", {})["%d_per_call" % a.ws_iterations] = row
        with open(saved_json, "w") as f:
            json.dump(saved, f, indent=1, default=float)
            f.write("\n")
        print(json.dumps(dict(hlp_outcomes_workspace_keep=saved["hlp_outcomes_workspace_keep"]), default=float))
        return
    if a.hlp == "workspace":
        out["hlp_outcomes_workspace"] = workspace_trials(robot, ws, res, a)
    if a.hlp in ("tree", "workspace") and os.path.exists(saved_json):
        saved = json.load(open(saved_json))
        for key in ("hlp_outcomes", "hlp_outcomes_tree", "hlp_outcomes_tree_seed", "hlp_outcomes_workspace", "hlp_outcomes_workspace_keep"):
            if key not in out and saved.get(key) is not None:
                out[key] = saved[key]
    k_range, D = res["k_range"], res["duration"]
    O = max(w["obstacles"].shape[0] for w in res["worlds"])
    obs = np.stack([scenes.pad_obstacles(w["obstacles"], O) for w in res["worlds"]])
    world, cols, ta, tb = executed_pieces(res)
    qe = ultimate_bound(robot)[1]
    out["undecided"] = {}
    for step in a.steps:
        for tag, tube in (("no_tube", None), ("ultimate_bound_tube", np.full(robot.num_factors, qe))):
            v = audit(robot, obs, world, *cols, k_range, D, ta, tb, tube=tube, step=step).verdict
            out["undecided"]["step_%g/%s" % (step, tag)] = dict(pieces=int(v.size), free=int((v == 0).sum()), hit=int((v == 1).sum()), undecided=int((v == 2).sum()),
                                                                undecided_share=round(float((v == 2).mean()), 4))
    out["ultimate_bound_position"] = qe
    out["throughput"] = {}
    one = world == 0
    for step in a.steps:
        for mode, cl in (("verdict", False), ("clearance", True)):
            out["throughput"]["step_%g/%s" % (step, mode)] = {
                "W=107": throughput(robot, obs, world, cols, ta, tb, k_range, D, step, a.reps, cl),
                "W=1": throughput(robot, obs[:1], world[one], [c[one] for c in cols], ta[one], tb[one], k_range, D, step, a.reps, cl)}
    if a.kernel_stats:
        with tempfile.TemporaryDirectory() as tmp:
            saved = os.path.join(tmp, "pieces.npz")
            np.savez(saved, obs=obs, world=world, q0=cols[0], qd0=cols[1], qdd0=cols[2], k=cols[3], k_range=k_range, D=D, ta=ta, tb=tb, step=a.steps[0])
            out["kernel_stats"] = kernel_stats(saved, a.reps, os.path.join(ROOT, "profiles", "trial_kernel_stats.csv"))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(saved_json, "w") as f:
        json.dump(out, f, indent=1, default=float)
        f.write("\n")
    print(json.dumps(out, default=float))


if __name__ == "__main__":
    main()
