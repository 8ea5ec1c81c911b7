"""Throughput of the roadmap check (armour_roadmap_check) and of the host search (armour_roadmap_plan); prints ONE JSON line.

    python tools/roadmap_bench.py [--nodes 20000] [--radius 0.3] [--k-max 16] [--edge-step 0.05] [--reps 10] [--graph-radius 1.5] [--out FILE]

Roadmap: armour_amd.roadmap.uniform_roadmap on the Kinova without gripper.  Worlds: the 107 reference worlds (scenes.reference_worlds,
O padded with scenes.FAR_BOX), all at once (W = 107) and the first alone (W = 1).  Per row: work items (nodes + edge sub-segments) x W,
kernel ms (median of `reps` launches, the ms of armour_roadmap_check), checks/s = items x W / kernel time, and the upper bound on
plane tests per launch (items x W x links x O x 15; the early exit at the first colliding pair does fewer).  With 7 joints a radius of
0.3 joins almost no pair of 20 000 uniform samples, so a second roadmap with --graph-radius is measured as well; its plan_ms is the
median host time of armour_roadmap_plan between random free start / goal nodes of world 0.

`field` (per roadmap): armour_roadmap_field for all worlds towards their own goals (W = 107) and for the first alone (W = 1) -- kernel ms
= the median `ms` of `reps` calls after a warm-up, call_ms = the median host time of the same calls (the seed search for W goals, the
uploads, the launch, the copy of cost and next back, and the wrapper's output arrays), sweeps, the share of nodes reached -- and the host
median of armour_roadmap_descend over the same 20 start / goal pairs plan_ms is taken on, in the same run (one field per pair's goal, then
the timed descend).  break_even_queries = field call_ms per world / (plan_ms - descend_ms): the queries per world after which the field has
paid for itself, by the whole call (null when descend is not faster); break_even_queries_kernel counts the launch alone.  With --out the line is also written to that file (profiles/roadmap_field_bench.json holds a run on the MI355X).

--knn measures the nearest-neighbour search instead (armour_roadmap_knn and what is built on it) and writes profiles/roadmap_knn_bench.json
(or --out): `build` -- roadmap.device_roadmap against roadmap.uniform_roadmap at --nodes (radius --graph-radius, --k-max), wall ms of
each, the search's device ms, and whether the edges are equal; `build_large` -- device_roadmap alone at --large-nodes; `descend` --
Roadmap.descend_many for the reference worlds (one start per world, --reps calls after a warm-up, median wall ms) against the loop of
Roadmap.descend over the same starts, and the search alone at that shape (Roadmap.knn, device ms); `trial` -- trials.run_trials on the
reference worlds for --trial-iterations iterations under field_hlps with and without batched: hlp / build / solve / audit ms per batch
iteration (mean) and the first iteration's (all worlds live)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure_field(rm, nodes, obs, goals, pairs, plan_ms, reps):
    """The `field` section: the launch at W = all and W = 1, and descend on the pairs plan() was timed on."""
    out = {}
    for W in (obs.shape[0], 1):
        rm.check(obs[:W])
        rm.field(goals[:W])                                 # warm-up (the CSR upload, buffers)
        runs, call = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            runs.append(rm.field(goals[:W]))
            call.append((time.perf_counter() - t0) * 1e3)
        ms = sorted(r["ms"] for r in runs)
        f = runs[-1]
        out["W=%d" % W] = dict(kernel_ms=round(ms[len(ms) // 2], 4), kernel_ms_min=round(ms[0], 4), call_ms=round(sorted(call)[len(call) // 2], 3),
                               sweeps_max=int(f["sweeps"].max()),
                               sweeps_mean=round(float(f["sweeps"].mean()), 2), reached_share=round(float(f["reached"].sum()) / max(1, W * rm.N), 4))
    rm.check(obs[:1])
    descend_ms, found, same = [], 0, 0
    for a, b, planned in pairs:
        rm.field(nodes[b])
        t0 = time.perf_counter()
        p, _ = rm.descend(0, nodes[a], connect_k=8)
        descend_ms.append((time.perf_counter() - t0) * 1e3)
        found += p is not None
        same += (p is not None) == planned
    if descend_ms:
        d = float(np.median(descend_ms))
        gain = plan_ms - d
        per_world = out["W=%d" % obs.shape[0]]["kernel_ms"] / obs.shape[0]
        call_per_world = out["W=%d" % obs.shape[0]]["call_ms"] / obs.shape[0]
        out.update(descend_ms=round(d, 4), descends_found=f"{found}/{len(descend_ms)}", found_as_plan=f"{same}/{len(descend_ms)}",
                   field_ms_per_world=round(per_world, 4), field_call_ms_per_world=round(call_per_world, 4),
                   break_even_queries=round(call_per_world / gain, 2) if gain > 0 else None,
                   break_even_queries_kernel=round(per_world / gain, 2) if gain > 0 else None)
    return out


def measure(robot, nodes, edges, cont, obs, goals, edge_step, reps):
    from armour_amd.roadmap import Roadmap
    rm = Roadmap(robot, nodes, edges, continuous=cont, edge_step=edge_step)
    J, O = robot.num_joints, obs.shape[1]
    rows = {}
    for W in (obs.shape[0], 1):
        rm.check(obs[:W])                                   # warm-up (module load, buffers)
        ms = sorted(rm.check(obs[:W])["ms"] for _ in range(reps))
        kms = ms[len(ms) // 2]
        items = (rm.N + rm.edge_samples) * W
        rows["W=%d" % W] = dict(kernel_ms=round(kms, 4), kernel_ms_min=round(ms[0], 4), items=items,
                                checks_per_s=round(items / (kms * 1e-3)), plane_tests_max=items * J * O * 15)
    v = rm.check(obs)
    free = np.flatnonzero(v["node_free"][0])
    rng = np.random.default_rng(0)
    plan_ms, found, pairs = [], 0, []
    for _ in range(20 if free.size >= 2 else 0):
        a, b = rng.choice(free, 2, replace=False)
        t0 = time.perf_counter()
        p = rm.plan(0, nodes[a], nodes[b], connect_k=8)
        plan_ms.append((time.perf_counter() - t0) * 1e3)
        found += p is not None
        pairs.append((a, b, p is not None))
    out = dict(N=rm.N, E=rm.E, edge_samples=rm.edge_samples, O=O, links=J, **rows)
    if plan_ms:
        out.update(plan_ms=round(float(np.median(plan_ms)), 3), plans_found=f"{found}/{len(plan_ms)}")
    out["field"] = measure_field(rm, nodes, obs, goals, pairs, float(np.median(plan_ms)) if plan_ms else 0.0, reps)
    rm.close()
    return out


def measure_knn(robot, cont, lb, ub, worlds, obs, goals, a):
    from armour_amd.roadmap import Roadmap, device_roadmap, field_hlps, uniform_roadmap
    from armour_amd.trials import run_trials
    res = {}
    wall = lambda f: (lambda t0, r: (r, (time.perf_counter() - t0) * 1e3))(time.perf_counter(), f())
    # the build: device against host at --nodes, device alone at --large-nodes
    device_roadmap(robot, 2048, a.graph_radius, a.k_max, 1, lb, ub, cont)                      # warm-up (module load)
    (n1, e1), dev_ms = wall(lambda: device_roadmap(robot, a.nodes, a.graph_radius, a.k_max, 0, lb, ub, cont))
    (n0, e0), host_ms = wall(lambda: uniform_roadmap(a.nodes, a.graph_radius, a.k_max, 0, lb, ub, cont))
    bare = Roadmap(robot, n1, np.zeros((0, 2), dtype=np.int32), continuous=cont.astype(np.uint8))
    ex = np.arange(a.nodes, dtype=np.int32)
    search = []
    for _ in range(a.reps):
        bare.knn(n1, a.k_max, radius=a.graph_radius, exclude=ex)
        search.append(bare.knn_ms)
    bare.close()
    res["build"] = dict(N=a.nodes, radius=a.graph_radius, k_max=a.k_max, E=int(e1.shape[0]), device_wall_ms=round(dev_ms, 2), host_wall_ms=round(host_ms, 2),
                        search_device_ms=round(float(np.median(search)), 3), same_edges=bool(np.array_equal(e0, e1) and np.array_equal(n0, n1)))
    (n2, e2), large_ms = wall(lambda: device_roadmap(robot, a.large_nodes, a.radius, a.k_max, 0, lb, ub, cont))
    bare = Roadmap(robot, n2, np.zeros((0, 2), dtype=np.int32), continuous=cont.astype(np.uint8))
    bare.knn(n2, a.k_max, radius=a.radius, exclude=np.arange(a.large_nodes, dtype=np.int32))
    res["build_large"] = dict(N=a.large_nodes, radius=a.radius, k_max=a.k_max, E=int(e2.shape[0]), device_wall_ms=round(large_ms, 2), search_device_ms=round(bare.knn_ms, 3))
    bare.close()
    # descend: one start per world, batched against the loop
    rm = Roadmap(robot, n1, e1, continuous=cont.astype(np.uint8), edge_step=a.edge_step)
    W = obs.shape[0]
    rm.check(obs)
    rm.field(goals)
    starts = np.stack([np.asarray(p["q0"], dtype=np.float64) for _, p in worlds])
    idx = np.arange(W, dtype=np.int32)
    rm.descend_many(idx, starts)
    many, loop, knn_ms, join_ms = [], [], [], []
    for _ in range(a.reps):
        got, ms = wall(lambda: rm.descend_many(idx, starts))
        many.append(ms)
        ref, ms = wall(lambda: [rm.descend(int(w), starts[w]) for w in idx])
        loop.append(ms)
        rm.knn(starts, 8, worlds=idx)
        knn_ms.append(rm.knn_ms)
        join_ms.append(rm.connect_many(idx, starts, targets=goals)["ms"])
    same = all((p is None and r is None) or (p is not None and r is not None and np.array_equal(p, r)) for (p, _), (r, _) in zip(got, ref))
    res["descend"] = dict(Q=W, N=rm.N, E=rm.E, descend_many_wall_ms=round(float(np.median(many)), 3), descend_loop_wall_ms=round(float(np.median(loop)), 3),
                          knn_device_ms=round(float(np.median(knn_ms)), 4), connect_batch_device_ms=round(float(np.median(join_ms)), 4),
                          paths=sum(1 for p, _ in got if p is not None), same_paths=bool(same))
    # a trial's iterations under both factories
    res["trial"] = {}
    for batched in (False, True):
        make = field_hlps(rm, worlds, batched=batched)
        out = run_trials(worlds, hlp=make, T=a.T, max_iterations=a.trial_iterations)
        bt = out["batches"]
        res["trial"]["batched" if batched else "loop"] = dict(
            batches=len(bt), first_batch={k: round(float(v), 3) for k, v in bt[0].items()},
            **{key + "_mean": round(float(np.mean([b[key] for b in bt])), 3) for key in ("hlp_ms", "build_ms", "solve_ms", "audit_ms")},
            hlp_ms_per_live_world=round(float(sum(b["hlp_ms"] for b in bt) / sum(b["live"] for b in bt)), 4))
    rm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=20000)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--graph-radius", type=float, default=1.5)
    ap.add_argument("--k-max", type=int, default=16)
    ap.add_argument("--edge-step", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--knn", action="store_true")
    ap.add_argument("--large-nodes", type=int, default=200000)
    ap.add_argument("--trial-iterations", type=int, default=20)
    ap.add_argument("--T", type=int, default=128)
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
    goals = np.stack([np.asarray(p["goal"], dtype=np.float64) for _, p in worlds])
    res = dict(tool="roadmap_bench", robot="kinova_gen3_no_gripper", worlds=obs.shape[0], edge_step=a.edge_step)
    if a.knn:
        res.update(mode="knn", **measure_knn(robot, cont, lb, ub, worlds, obs, goals, a))
        a.out = a.out or os.path.join(ROOT, "profiles", "roadmap_knn_bench.json")
    for key, radius in [] if a.knn else (("radius_%g" % a.radius, a.radius), ("radius_%g" % a.graph_radius, a.graph_radius)):
        nodes, edges = uniform_roadmap(a.nodes, radius, a.k_max, 0, lb, ub, cont)
        res[key] = measure(robot, nodes, edges, cont.astype(np.uint8), obs, goals, a.edge_step, a.reps)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
