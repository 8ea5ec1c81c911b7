"""Throughput and decisiveness of the self-collision checks (armour_self_check, armour_roadmap_check_self, armour_path_audit_self);
writes profiles/self_bench.json and prints it as ONE JSON line.

    python tools/self_bench.py [--configs 20000] [--nodes 20000] [--graph-radius 1.5] [--k-max 16] [--edge-step 0.05] [--audit-step 0.01]
                               [--reps 10] [--trial-worlds 107] [--T 128] [--out profiles/self_bench.json]

Robot: the Kinova without gripper.  Rows:
  configurations  items/s of armour_self_check on `configs` uniform configurations (an item = one configuration; a lane = (item, first link));
  roadmap         items/s of armour_roadmap_check_self on the --graph-radius roadmap of tools/roadmap_bench.py (items = nodes + edge
                  sub-segments), next to the world check's checks/s on the same roadmap and one world in the same run -- the yardstick;
  audit           items/s of armour_path_audit_self at --audit-step on random pieces (items = (piece, sub-interval));
  undecided       the share of roadmap edges and of pieces that are neither proved self-free nor shown to collide at a sample, without and with
                  calibrate_shrink on the reference's 214 start and goal configurations, at several steps;
  trials          outcome counts of the first --trial-worlds reference worlds under run_trials(self_check="record") (0: skipped)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(call, reps):
    call()
    ms = sorted(call() for _ in range(reps))
    return ms[len(ms) // 2]


def random_pieces(rng, lb, ub, P):
    n = lb.size
    q0 = lb + (ub - lb) * rng.random((P, n))
    return q0, rng.uniform(-0.6, 0.6, (P, n)), rng.uniform(-1.5, 1.5, (P, n)), rng.uniform(-1, 1, (P, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, default=20000)
    ap.add_argument("--nodes", type=int, default=20000)
    ap.add_argument("--graph-radius", type=float, default=1.5)
    ap.add_argument("--k-max", type=int, default=16)
    ap.add_argument("--edge-step", type=float, default=0.05)
    ap.add_argument("--audit-step", type=float, default=0.01)
    ap.add_argument("--pieces", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trial-worlds", type=int, default=107)
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "self_bench.json"))
    a = ap.parse_args()
    from armour_amd import scenes, self_check
    from armour_amd.path_audit import audit_items, audit_self
    from armour_amd.planner import default_params, kinova_robot
    from armour_amd.roadmap import Roadmap, uniform_roadmap
    robot = kinova_robot()
    n = robot.num_factors
    cont = np.array(robot.continuous[:n]).astype(bool)
    lb = np.where(cont, -np.pi, np.array(robot.state_limits_lb[:n]))
    ub = np.where(cont, np.pi, np.array(robot.state_limits_ub[:n]))
    rng = np.random.default_rng(0)
    worlds = scenes.reference_worlds()
    ref = np.stack([p["q0"] for _, p in worlds] + [p["goal"] for _, p in worlds])
    shrink = self_check.calibrate_shrink(robot, ref)
    res = dict(tool="self_bench", robot="kinova_gen3_no_gripper",
               calibrated_shrink={"%d,%d" % (i, j): round(float(shrink[i, j]), 5) for i, j in zip(*np.nonzero(shrink))},
               reference_configurations=dict(count=int(ref.shape[0]), overlapping=int((~self_check.check(robot, ref).free).sum()),
                                             overlapping_calibrated=int((~self_check.check(robot, ref, shrink=shrink).free).sum())))
    # configurations
    Q = lb + (ub - lb) * rng.random((a.configs, n))
    row = {}
    for key, cl in (("verdict", False), ("clearance", True)):
        ms = median_ms(lambda: self_check.check(robot, Q, clearance=cl).ms, a.reps)
        row[key] = dict(kernel_ms=round(ms, 4), items_per_s=round(a.configs / (ms * 1e-3)))
    row["colliding_share"] = round(float((~self_check.check(robot, Q).free).mean()), 4)
    res["configurations"] = dict(items=a.configs, **row)
    # roadmap, and the world check on the same roadmap as the yardstick
    nodes, edges = uniform_roadmap(a.nodes, a.graph_radius, a.k_max, 0, np.array(robot.state_limits_lb[:n]), np.array(robot.state_limits_ub[:n]), cont)
    obs = np.ascontiguousarray(scenes.as_batch(worlds)["obstacles"])
    rm = Roadmap(robot, nodes, edges, continuous=cont.astype(np.uint8), edge_step=a.edge_step)
    items = rm.N + rm.edge_samples
    ms_self = median_ms(lambda: rm.check_self()["ms"], a.reps)
    ms_world = median_ms(lambda: rm.check(obs[:1])["ms"], a.reps)
    res["roadmap"] = dict(N=rm.N, E=rm.E, edge_samples=rm.edge_samples, items=items, edge_step=a.edge_step, kernel_ms=round(ms_self, 4),
                          items_per_s=round(items / (ms_self * 1e-3)),
                          world_check_W1=dict(kernel_ms=round(ms_world, 4), checks_per_s=round(items / (ms_world * 1e-3)), O=int(obs.shape[1])))
    rm.close()
    # audit
    k_range, D = np.array(default_params(a.T).k_range[:n]), float(default_params(a.T).duration)
    pcs = random_pieces(rng, lb, ub, a.pieces)
    S = int(audit_items(robot, *pcs, k_range, D, 0.0, 0.5 * D, step=a.audit_step).sum())
    row = {}
    for key, cl in (("verdict", False), ("clearance", True)):
        ms = median_ms(lambda: audit_self(robot, *pcs, k_range, D, 0.0, 0.5 * D, step=a.audit_step, clearance=cl).ms, a.reps)
        row[key] = dict(kernel_ms=round(ms, 4), items_per_s=round(S / (ms * 1e-3)))
    res["audit"] = dict(pieces=a.pieces, items=S, step=a.audit_step, **row)
    # the undecided share: edges of a small roadmap and the pieces above, by step, without and with the calibrated shrink
    en, ee = uniform_roadmap(2000, a.graph_radius, a.k_max, 1, np.array(robot.state_limits_lb[:n]), np.array(robot.state_limits_ub[:n]), cont)
    und = dict(edges={}, pieces={})
    for name, sh in (("no_shrink", None), ("calibrated", shrink)):
        for step in (0.05, 0.02, 0.01):
            r2 = Roadmap(robot, en, ee, continuous=cont.astype(np.uint8), edge_step=step)
            m = r2.check_self(shrink=sh)
            r2.close()
            # an edge that is not self-free with 50 self-free samples on it counts as undecided
            bad = np.flatnonzero(~m["edge_free"])
            t = np.linspace(0, 1, 50)[None, :, None]
            d = en[ee[bad, 1]] - en[ee[bad, 0]]
            d = np.where(cont, d - 2 * np.pi * np.floor((d + np.pi) / (2 * np.pi)), d)
            dense = self_check.check(robot, (en[ee[bad, 0]][:, None, :] + t * d[:, None, :]).reshape(-1, n), shrink=sh).free.reshape(len(bad), 50).all(1)
            und["edges"]["%s_step_%g" % (name, step)] = dict(edges=int(len(ee)), self_free=int(m["edge_free"].sum()), undecided=int(dense.sum()),
                                                             undecided_share=round(float(dense.sum()) / max(1, len(ee)), 4))
        for step in (0.02, 0.01, 0.005):
            v = audit_self(robot, *pcs, k_range, D, 0.0, 0.5 * D, step=step, shrink=sh).verdict
            und["pieces"]["%s_step_%g" % (name, step)] = dict(pieces=a.pieces, verdicts=np.bincount(v, minlength=3).tolist(),
                                                              undecided_share=round(float((v == 2).mean()), 4))
    res["undecided"] = und
    # whole trials
    if a.trial_worlds > 0:
        from armour_amd.trials import run_trials
        out = run_trials(worlds[:a.trial_worlds], T=a.T, self_check="record", self_shrink=shrink)
        s = out["summary"]
        res["trials"] = dict(worlds=s["worlds"], T=a.T, **{k: s[k] for k in ("goal", "collision", "stuck", "iteration_limit", "pieces", "undecided_pieces",
                                                                             "self_hit_pieces", "self_undecided_pieces")})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
