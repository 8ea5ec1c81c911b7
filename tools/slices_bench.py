"""The time-sliced roadmap check against K launches of the window check, the earliest-arrival search, and plan_slices as a whole; prints ONE
JSON line and writes it to profiles/roadmap_slices_bench.json (or --out).

    python tools/slices_bench.py [--nodes 20000] [--radius 0.3] [--graph-radius 1.5] [--k-max 16] [--edge-step 0.05] [--reps 10]
                                 [--ks 8 32 64] [--dt 0.25] [--speed 1.0] [--moving-seed 2] [--moving-speed 0.05 0.2] [--out FILE]

Roadmaps and worlds: those of tools/roadmap_bench.py (uniform_roadmap on the Kinova without gripper at --radius and --graph-radius; the 107
reference worlds, O padded), every obstacle in linear motion with the seeded velocities of tools/trial_bench.py --moving.  Per roadmap and K:

  * check_slices: the device ms of ONE armour_roadmap_check_slices over K slices of --dt seconds from world time 0 (median and minimum of
    --reps calls after a warm-up, nothing read back), and the host time of the whole call;
  * check_moving_x_K: the sum over the same K windows of the device ms of armour_roadmap_check_moving, in the same process (per window the
    median of --reps launches after a warm-up; masks read back as that entry always does) -- the yardstick; `ratio` = that sum / the sliced ms;
  * same_bits: the sliced masks equal the K window checks' (read back once, outside the timing);
  * free_share: the share of (node, slice) and (edge, slice) bits that are set;
  * arrival: kernel ms (median), sweeps (max, mean) and the worlds that reach their goal, for the worlds' own starts and goals joined as
    plan_slices joins them at --speed;
  * plan_slices: the median host time of the whole call (knn + check_slices + arrival + the polylines)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(xs):
    return float(np.median(xs))


def measure(robot, nodes, edges, cont, obs, vel, starts, goals, a):
    from armour_amd.roadmap import Roadmap
    rm = Roadmap(robot, nodes, edges, continuous=cont, edge_step=a.edge_step)
    W = obs.shape[0]
    t0 = np.zeros(W)
    out = dict(N=rm.N, E=rm.E, edge_samples=rm.edge_samples, O=int(obs.shape[1]), W=W)
    for K in a.ks:
        rm.check_slices(obs, vel, t0, a.dt, K, tables=False)                      # warm-up (module load, buffers)
        ms, call = [], []
        for _ in range(a.reps):
            t = time.perf_counter()
            ms.append(rm.check_slices(obs, vel, t0, a.dt, K, tables=False)["ms"])
            call.append((time.perf_counter() - t) * 1e3)
        s = rm.check_slices(obs, vel, t0, a.dt, K)
        times = s["slice_times"]
        windows, same = [], True
        for k in range(K):
            rm.check_moving(obs, vel, times[:, k], times[:, k + 1])                # warm-up
            runs = [rm.check_moving(obs, vel, times[:, k], times[:, k + 1]) for _ in range(a.reps)]
            windows.append(median([r["ms"] for r in runs]))
            bit = lambda m: ((m >> np.uint64(k)) & np.uint64(1)).astype(bool)
            same = same and np.array_equal(bit(s["node_slices"]), runs[-1]["node_free"]) and np.array_equal(bit(s["edge_slices"]), runs[-1]["edge_free"])
        bits = lambda m: float(sum(int(((m >> np.uint64(k)) & np.uint64(1)).sum()) for k in range(K))) / max(1, m.size * K)
        row = dict(check_slices_ms=round(median(ms), 4), check_slices_ms_min=round(min(ms), 4), check_slices_call_ms=round(median(call), 3),
                   check_moving_x_K_ms=round(float(sum(windows)), 4), check_moving_window_ms=round(median(windows), 4), same_bits=bool(same),
                   node_free_share=round(bits(s["node_slices"]), 4), edge_free_share=round(bits(s["edge_slices"]), 4))
        row["ratio"] = round(row["check_moving_x_K_ms"] / row["check_slices_ms"], 3)
        del s
        rm.plan_slices(starts, goals, obs, vel, t0, a.dt, K, a.speed)               # warm-up (the rows' upload)
        whole, kernel, sweeps, reached = [], [], None, 0
        for _ in range(a.reps):
            t = time.perf_counter()
            plans = rm.plan_slices(starts, goals, obs, vel, t0, a.dt, K, a.speed)
            whole.append((time.perf_counter() - t) * 1e3)
            kernel.append(rm.last_arrival["ms"])
            sweeps, reached = rm.last_arrival["sweeps"], sum(p["path"] is not None for p in plans)
        row["arrival"] = dict(kernel_ms=round(median(kernel), 4), sweeps_max=int(sweeps.max()), sweeps_mean=round(float(sweeps.mean()), 2), worlds_reached=int(reached),
                              check_slices_ms_with_extras=round(float(rm.last_slices["ms"]), 4))
        row["plan_slices_call_ms"] = round(median(whole), 3)
        out["K=%d" % K] = row
    rm.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=20000)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--graph-radius", type=float, default=1.5)
    ap.add_argument("--k-max", type=int, default=16)
    ap.add_argument("--edge-step", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ks", type=int, nargs="+", default=[8, 32, 64])
    ap.add_argument("--dt", type=float, default=0.25)
    ap.add_argument("--speed", type=float, default=1.0)
    ap.add_argument("--moving-seed", type=int, default=2)
    ap.add_argument("--moving-speed", type=float, nargs=2, default=[0.05, 0.2])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roadmap_slices_bench.json"))
    a = ap.parse_args()
    from armour_amd.planner import kinova_robot
    from armour_amd.roadmap import uniform_roadmap
    from armour_amd.scenes import as_batch, reference_worlds
    robot = kinova_robot()
    n = robot.num_factors
    cont = np.array(robot.continuous[:n]).astype(bool)
    lb, ub = np.array(robot.state_limits_lb[:n]), np.array(robot.state_limits_ub[:n])
    worlds = reference_worlds()
    obs = np.ascontiguousarray(as_batch(worlds)["obstacles"])
    lo, hi = a.moving_speed
    vel = np.zeros(obs.shape[:2] + (3,))
    for i, (_, p) in enumerate(worlds):                                             # tools/trial_bench.py --moving: world i's stream is (seed, i)
        rng = np.random.default_rng([a.moving_seed, i])
        v = rng.normal(size=(np.asarray(p["obstacles"]).reshape(-1, 12).shape[0], 3))
        vel[i, :v.shape[0]] = v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.uniform(lo, hi, (v.shape[0], 1))
    starts = np.stack([np.asarray(p["q0"], dtype=np.float64) for _, p in worlds])
    goals = np.stack([np.asarray(p["goal"], dtype=np.float64) for _, p in worlds])
    res = dict(tool="slices_bench", robot="kinova_gen3_no_gripper", worlds=obs.shape[0], edge_step=a.edge_step, dt=a.dt, speed=a.speed, reps=a.reps,
               moving_seed=a.moving_seed, moving_speed=[lo, hi])
    for key, radius in (("radius_%g" % a.radius, a.radius), ("radius_%g" % a.graph_radius, a.graph_radius)):
        nodes, edges = uniform_roadmap(a.nodes, radius, a.k_max, 0, lb, ub, cont)
        res[key] = measure(robot, nodes, edges, cont.astype(np.uint8), obs, vel, starts, goals, a)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
