"""The batched inverse kinematics (armour_ik) measured; writes profiles/ik_bench.json (or --out) and prints ONE JSON line.

    python tools/ik_bench.py [--seed 7] [--reps 10] [--out FILE]

* `batch_S32` / `batch_S256`: the 107 reference worlds (scenes.reference_worlds; target = the end effector of the world's goal configuration,
  q_ref = its start, O padded with scenes.FAR_BOX, world w with the seed --seed + w, the entry's default lambda, e_max, tol and
  max_iterations) in ONE launch with 32 and with 256 seeds per target: device ms = the entry's event time, median of --reps calls after a
  warm-up; call_ms = the median host time of the same calls (uploads, launch, the results back); the status counts, the share of
  converged items and their iteration statistics; the host twin's wall time on the same inputs (armour_ik_host, one call on one core), and
  how the device's answer compares to it (discrete outcomes equal or not, the largest |dq| and |derr|);
* `one_target_S256`: the same for hard_7_window alone (N = 1: one block, so one compute unit -- the stated limit).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATUS = ("none_converged", "found", "all_blocked")


def measure(robot, targets, q_ref, obs, seeds, S, reps):
    from armour_amd.ik import solve_ik
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ik_bench.json"))
    a = ap.parse_args()
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
