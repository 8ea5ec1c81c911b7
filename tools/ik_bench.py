"""The batched inverse kinematics (armour_ik) measured; writes profiles/ik_bench.json (or --out) and prints ONE JSON line.

    python tools/ik_bench.py [--seed 7] [--reps 10] [--out FILE]
    python tools/ik_bench.py --moving [--moving-seed 2] [--moving-speed 0.05 0.2] [--ab-static PARENT_LIBRARY] [--rounds 3] [--out profiles/ik_moving_bench.json]

* `batch_S32` / `batch_S256`: the 107 reference worlds (scenes.reference_worlds; target = the end effector of the world's goal configuration,
  q_ref = its start, O padded with scenes.FAR_BOX, world w with the seed --seed + w, the entry's default lambda, e_max, tol and
  max_iterations) in ONE launch with 32 and with 256 seeds per target: device ms = the entry's event time, median of --reps calls after a
  warm-up; call_ms = the median host time of the same calls (uploads, launch, the results back); the status counts, the share of
  converged items and their iteration statistics; the host twin's wall time on the same inputs (armour_ik_host, one call on one core), and
  how the device's answer compares to it (discrete outcomes equal or not, the largest |dq| and |derr|);
* `one_target_S256`: the same for hard_7_window alone (N = 1: one block, so one compute unit -- the stated limit).
* --moving: a run of its own that writes profiles/ik_moving_bench.json (or --out): per S the batch by the static entry, by armour_ik_moving at
  zero velocity on the window [0, 1] (the like-for-like cost of the window rule; `ratio_v0` = static ms / moving ms, `v0_equals_static`)
  and with every obstacle in linear motion (velocities from the stream (--moving-seed, world), speeds --moving-speed LO HI in m/s, as
  tools/tree_bench.py --moving draws them) on the same window; with --ab-static PARENT_LIBRARY also the static shapes of the parent
  commit's library (chosen by ARMOUR_HIP_LIB) against this one's, alternating in fresh processes for --rounds rounds: per shape the device ms
  of every run, the medians, the parent's own spread and whether the new median lies within it (the key `static_against_parent`).
"""
import argparse
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

STATUS = ("none_converged", "found", "all_blocked")


def measure(robot, targets, q_ref, obs, seeds, S, reps, **motion):
    from armour_amd import ik
    solve_ik = lambda *x, **kw: ik.solve_ik(*x, **kw, **motion)
    world = np.arange(len(targets))
    solve_ik(robot, targets, q_ref, obs, world, seeds, S=S)                          # warm-up
    runs, call = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        runs.append(solve_ik(robot, targets, q_ref, obs, world, seeds, S=S))
        call.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(r.ms for r in runs)
    dev = solve_ik(robot, targets, q_ref, obs, world, seeds, S=S, details=True)
    t0 = time.perf_counter()
    host = solve_ik(robot, targets, q_ref, obs, world, seeds, S=S, host=True, details=True)
    host_ms = (time.perf_counter() - t0) * 1e3
    conv = (dev.flags & 1) == 1
    its = dev.iterations[conv]
    same = (dev.iterations == host.iterations) & (dev.flags == host.flags)
    return dict(targets=int(len(targets)), seeds_per_target=int(S), obstacles_per_world=int(obs.shape[1]), device_ms=round(ms[len(ms) // 2], 4),
                device_ms_min=round(ms[0], 4), call_ms=round(sorted(call)[len(call) // 2], 3), host_twin_wall_ms=round(host_ms, 2),
                status_counts={STATUS[s]: int((dev.status == s).sum()) for s in range(3)}, picks_of_seed_0=int((dev.best == 0).sum()),
                items=int(conv.size), items_converged=int(conv.sum()), items_free=int(((dev.flags & 2) == 2).sum()),
                iterations_median=float(np.median(its)), iterations_p95=float(np.percentile(its, 95)), iterations_max=int(its.max()),
                host_margin_min=float(host.margin.min()), status_and_best_equal_host=bool(np.array_equal(dev.status, host.status) and np.array_equal(dev.best, host.best)),
                items_with_other_flags_or_iterations=int((~same).sum()), max_abs_dq_against_host=float(np.abs(dev.q_all - host.q_all)[same].max()),
                max_abs_derr_against_host=float(np.abs(dev.err - host.err)[same].max()))


def ab_static(a):
    """the static shapes of the parent's library against this one's: parent, new, parent, new, ... in fresh processes"""
    runs = {"parent": [], "new": []}
    with tempfile.TemporaryDirectory() as tmp:
        for rnd in range(a.rounds):
            for side in ("parent", "new"):
                out = os.path.join(tmp, "%s_%d.json" % (side, rnd))
                env = dict(os.environ)
                env.pop("ARMOUR_HIP_LIB", None)
                if side == "parent":
                    env["ARMOUR_HIP_LIB"] = os.path.abspath(a.ab_static)
                subprocess.run([sys.executable, os.path.abspath(__file__), "--out", out, "--seed", str(a.seed), "--reps", str(a.reps)], env=env, check=True,
                               stdout=subprocess.DEVNULL, timeout=600)
                runs[side].append(json.load(open(out)))
    rows = {}
    for shape in ("batch_S32", "batch_S256", "one_target_S256"):
        p, n = [r[shape]["device_ms"] for r in runs["parent"]], [r[shape]["device_ms"] for r in runs["new"]]
        pm, nm, spread = float(np.median(p)), float(np.median(n)), max(p) - min(p)
        same = all(r[shape][k] == runs["parent"][0][shape][k] for side in runs for r in runs[side] for k in ("status_counts", "items_converged", "items_free", "picks_of_seed_0"))
        rows[shape] = dict(parent_device_ms=p, new_device_ms=n, parent_median=pm, new_median=nm, parent_spread=round(spread, 4), new_over_parent=round(nm / pm, 4),
                           within_parent_spread=bool(nm <= pm + spread), counts_equal=bool(same))
    return rows


def moving(a, robot, ws, targets, starts, obs, seeds):
    """--moving: see the module text"""
    from tree_bench import seeded_velocities
    lo, hi = a.moving_speed
    window = dict(t_from=0.0, t_to=1.0)
    legs = dict(static={}, moving_v0=dict(window, velocity=np.zeros(obs.shape[:2] + (3,))),
                moving=dict(window, velocity=seeded_velocities(ws, obs.shape[1], a.moving_seed, lo, hi)))
    keep = ("device_ms", "device_ms_min", "call_ms", "status_counts", "items_converged", "items_free", "picks_of_seed_0", "host_margin_min", "status_and_best_equal_host",
            "items_with_other_flags_or_iterations", "max_abs_dq_against_host")
    out = dict(tool="ik_bench --moving", seed=a.seed, reps=a.reps, targets=int(len(targets)), obstacles_per_world=int(obs.shape[1]), window=[0.0, 1.0],
               moving_seed=a.moving_seed, speed=[lo, hi])
    for S in (32, 256):
        res = {k: measure(robot, targets, starts, obs, seeds, S, a.reps, **kw) for k, kw in legs.items()}
        row = {k: {f: r[f] for f in keep} for k, r in res.items()}
        row["ratio_v0"] = round(res["static"]["device_ms"] / res["moving_v0"]["device_ms"], 4)
        row["v0_equals_static"] = bool(all(res["static"][f] == res["moving_v0"][f] for f in ("status_counts", "items_converged", "items_free", "picks_of_seed_0")))
        out[f"batch_S{S}"] = row
    if a.ab_static:
        out["static_against_parent"] = ab_static(a)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--moving", action="store_true")
    ap.add_argument("--moving-seed", type=int, default=2)
    ap.add_argument("--moving-speed", type=float, nargs=2, default=[0.05, 0.2])
    ap.add_argument("--ab-static")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "ik_moving_bench.json" if a.moving else "ik_bench.json")
    from armour_amd import scenes
    from armour_amd.ik import end_effector
    from armour_amd.planner import kinova_robot
    robot = kinova_robot()
    ws = scenes.reference_worlds()
    names = [name for name, _ in ws]
    O = max(p["obstacles"].shape[0] for _, p in ws)
    obs = np.stack([scenes.pad_obstacles(p["obstacles"], O) for _, p in ws])
    starts = np.stack([p["q0"] for _, p in ws])
    targets = end_effector(robot, np.stack([p["goal"] for _, p in ws]))
    seeds = np.arange(len(ws), dtype=np.uint64) + np.uint64(a.seed)
    if a.moving:
        return moving(a, robot, ws, targets, starts, obs, seeds)
    out = dict(tool="ik_bench", robot="kinova_gen3_no_gripper", seed=a.seed, reps=a.reps, lam=0.05, e_max=0.1, tol=1e-9, max_iterations=200)
    for S in (32, 256):
        out[f"batch_S{S}"] = measure(robot, targets, starts, obs, seeds, S, a.reps)
    w = names.index("hard_7_window")
    out["one_target_S256"] = dict(measure(robot, targets[w:w + 1], starts[w:w + 1], obs[w:w + 1], seeds[w:w + 1], 256, a.reps), name=names[w])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
