"""Moving obstacles measured (armour_set_problems_moving, armour_path_audit_moving); writes profiles/moving_bench.json.

  python tools/moving_bench.py [--parent-lib PATH] [--rounds 3] [--out profiles/moving_bench.json]
  python tools/moving_bench.py --roadmap [--parent-lib PATH] [--rounds 3] [--out profiles/moving_roadmap_bench.json]

  static build    wall ms of set_parameters and the device ms of its kernels, B = 1 and B = 128, O = 20, T = 100; with --parent-lib (a libarmour_hip.so
                  of the parent commit) the parent's library and this one alternate, a fresh process per run (the library is chosen by
                  ARMOUR_HIP_LIB): parent, new, parent, new, ...; the parent's spread = max - min over its rounds.
  moving build    set_parameters_moving of the same worlds (velocities of 0.2 .. 1.0 m/s), in the runs of this library; its excess over the static
                  build next to the obstacle bytes uploaded and the d column stored.
  evaluation      us per fused evaluation at B = 128 on the moving tables (d read) against the static ones (d recomputed from the centres):
                  device events around 40 asynchronous evaluations on one stream, after 5 warm-up calls.
  audit           items/s of armour_path_audit_moving against armour_path_audit on the same random pieces over the reference's worlds (median
                  device ms of 10 launches, verdict and clearance mode, steps 0.01 and 0.002).

--roadmap measures the roadmap's window rule instead (armour_roadmap_check_moving) and writes profiles/moving_roadmap_bench.json:
  static check    kernel ms (median of 10 launches) of armour_roadmap_check on the two roadmaps tools/roadmap_bench.py measures (20 000 nodes, radius
                  0.3 and 1.5, edge step 0.05; the edges by roadmap.device_roadmap, which equal uniform_roadmap's) against the 107 reference worlds
                  and the first alone; with --parent-lib the parent's library and this one alternate as above, and the parent's spread is taken the
                  same way.
  moving check    the same launches of armour_roadmap_check_moving on the window [0, 1] at zero velocity and at 0.2 .. 1.0 m/s, in checks/s beside
                  the static column of the same process, with the free nodes and edges each form finds.

Every run needs the GPU; without one the tool fails."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, O = 100, 20
SHAPES = (1, 128)


def _velocity(seed, shape):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=shape + (3,))
    return v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.uniform(0.2, 1.0, shape + (1,))


def _median(x):
    return float(np.median(np.asarray(x, dtype=np.float64)))


def worker_build(moving, reps=7):
    """Per batch size: wall and device ms of `reps` builds after 2 warm-up builds (static; and moving where the library has the entry)."""
    from armour_amd import _lib
    from armour_amd.planner import ArmourNLP
    from armour_amd.worlds import moving_frames, random_batch
    out = {}
    for B in SHAPES:
        bp = random_batch(300, B, O)
        st = (bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"])
        frames = np.stack([moving_frames(bp["obstacles"][b], _velocity(300 + b, (O,)), T) for b in range(B)])
        nlp = ArmourNLP(T=T, limits=_lib.ArmourLimits(max_batch=B, max_obstacles=O))
        kinds = [("static", lambda: nlp.set_parameters(*st, bp["obstacles"]))]
        if moving:
            kinds.append(("moving", lambda: nlp.set_parameters_moving(*st, frames)))
        for kind, call in kinds:
            wall, dev = [], []
            for i in range(reps + 2):
                t0 = time.perf_counter()
                call()                                   # synchronous: returns after the build's one wait
                if i >= 2:
                    wall.append((time.perf_counter() - t0) * 1e3)
                    dev.append(nlp.build_ms)
            out[f"{kind}/B={B}"] = dict(wall_ms=_median(wall), wall_ms_all=wall, device_ms=_median(dev))
        nlp.close()
    return out


def worker_eval(B=128, calls=40):
    import torch

    from armour_amd import _lib
    from armour_amd.planner import ArmourNLP
    from armour_amd.worlds import moving_frames, random_batch, random_k
    dev = torch.device("cuda:0")
    bp = random_batch(300, B, O)
    st = (bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"])
    frames = np.stack([moving_frames(bp["obstacles"][b], _velocity(300 + b, (O,)), T) for b in range(B)])
    out = {}
    for kind in ("static", "moving", "static", "moving"):
        nlp = ArmourNLP(T=T, limits=_lib.ArmourLimits(max_batch=B, max_obstacles=O))
        nlp.set_parameters(*st, bp["obstacles"]) if kind == "static" else nlp.set_parameters_moving(*st, frames)
        ks = torch.from_numpy(random_k(5, B)).to(dev)
        d_g = torch.empty((B, nlp.m), device=dev, dtype=torch.float64)
        d_j = torch.empty((B, nlp.m, nlp.n), device=dev, dtype=torch.float64)
        s = torch.cuda.Stream(device=dev)
        for _ in range(5):
            nlp.eval_g_jac_device(ks.data_ptr(), d_g.data_ptr(), d_j.data_ptr(), s.cuda_stream)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(calls):
            nlp.eval_g_jac_device(ks.data_ptr(), d_g.data_ptr(), d_j.data_ptr(), s.cuda_stream)
        e1.record(s)
        torch.cuda.synchronize()
        out.setdefault(kind, []).append(e0.elapsed_time(e1) * 1e3 / calls)
        nlp.close()
    return {f"{k}/B={B}": dict(us_per_eval=min(v), us_per_eval_all=v) for k, v in out.items()}


def worker_audit(P=4096, launches=10):
    from armour_amd.path_audit import audit, audit_items, audit_moving
    from armour_amd.planner import kinova_robot
    from armour_amd.scenes import as_batch, reference_worlds
    robot = kinova_robot()
    obs = as_batch(reference_worlds())["obstacles"]
    W = obs.shape[0]
    rng = np.random.default_rng(9)
    cont = np.array(robot.continuous[:7]).astype(bool)
    lb, ub = np.where(cont, -np.pi, np.array(robot.state_limits_lb[:7])), np.where(cont, np.pi, np.array(robot.state_limits_ub[:7]))
    q0 = lb + (ub - lb) * rng.random((P, 7))
    qd0, qdd0, k = rng.uniform(-0.6, 0.6, (P, 7)), rng.uniform(-1.5, 1.5, (P, 7)), rng.uniform(-1, 1, (P, 7))
    world = rng.integers(0, W, P).astype(np.int32)
    t_world = rng.uniform(0.0, 2.0, P)
    vel = _velocity(10, obs.shape[:2])
    kr = np.full(7, np.pi / 48)
    out = {}
    for step in (0.01, 0.002):
        items = int(audit_items(robot, q0, qd0, qdd0, k, kr, 1.0, 0.0, 0.5, step=step).sum())
        for mode, clearance in (("verdict", False), ("clearance", True)):
            row = dict(items=items)
            for kind, call in (("static", lambda: audit(robot, obs, world, q0, qd0, qdd0, k, kr, 1.0, 0.0, 0.5, step=step, clearance=clearance)),
                               ("moving_zero_velocity", lambda: audit_moving(robot, obs, np.zeros_like(vel), world, t_world, q0, qd0, qdd0, k, kr, 1.0, 0.0, 0.5,
                                                                            step=step, clearance=clearance)),
                               ("moving", lambda: audit_moving(robot, obs, vel, world, t_world, q0, qd0, qdd0, k, kr, 1.0, 0.0, 0.5, step=step,
                                                               clearance=clearance))):
                ms = [call().ms for _ in range(launches + 2)][2:]
                row[kind] = dict(kernel_ms=_median(ms), items_per_s=items / (_median(ms) * 1e-3), verdicts=np.bincount(call().verdict, minlength=3).tolist())
            row["moving_zero_velocity_over_static"] = row["moving_zero_velocity"]["items_per_s"] / row["static"]["items_per_s"]
            out[f"step_{step}/{mode}"] = row
    return out


ROADMAPS = (("radius_0.3", 0.3), ("radius_1.5", 1.5))


def worker_roadmap(moving, N=20000, k_max=16, edge_step=0.05, launches=10):
    """Per roadmap and W: kernel ms and checks/s of the static check (and, where the library has the entry, of the moving check at v = 0 and at 0.2 .. 1.0 m/s)."""
    from armour_amd.planner import kinova_robot
    from armour_amd.roadmap import Roadmap, device_roadmap
    from armour_amd.scenes import as_batch, reference_worlds
    robot = kinova_robot()
    n = robot.num_factors
    cont = np.array(robot.continuous[:n]).astype(bool)
    lb, ub = np.array(robot.state_limits_lb[:n]), np.array(robot.state_limits_ub[:n])
    obs = np.ascontiguousarray(as_batch(reference_worlds())["obstacles"])
    vel = _velocity(10, obs.shape[:2])
    out = {}
    for key, radius in ROADMAPS:
        nodes, edges = device_roadmap(robot, N, radius, k_max, 0, lb, ub, cont)
        rm = Roadmap(robot, nodes, edges, continuous=cont.astype(np.uint8), edge_step=edge_step)
        row = dict(N=rm.N, E=rm.E, edge_samples=rm.edge_samples, O=int(obs.shape[1]))
        for W in (obs.shape[0], 1):
            kinds = [("static", lambda: rm.check(obs[:W]))]
            if moving:
                kinds += [("moving_zero_velocity", lambda: rm.check_moving(obs[:W], np.zeros_like(vel[:W]), 0.0, 1.0)),
                          ("moving", lambda: rm.check_moving(obs[:W], vel[:W], 0.0, 1.0))]
            items = (rm.N + rm.edge_samples) * W
            cell = dict(items=items)
            for kind, call in kinds:
                runs = [call() for _ in range(launches + 2)][2:]
                ms = _median([r["ms"] for r in runs])
                cell[kind] = dict(kernel_ms=ms, checks_per_s=items / (ms * 1e-3), free_nodes=int(runs[-1]["node_free"].sum()), free_edges=int(runs[-1]["edge_free"].sum()))
            if moving:
                cell["moving_zero_velocity_over_static"] = cell["moving_zero_velocity"]["checks_per_s"] / cell["static"]["checks_per_s"]
                cell["moving_over_static"] = cell["moving"]["checks_per_s"] / cell["static"]["checks_per_s"]
            row[f"W={W}"] = cell
        rm.close()
        out[key] = row
    return out


def main_roadmap(a):
    runs = {"parent": [], "new": []}
    for _ in range(a.rounds):
        if a.parent_lib:
            runs["parent"].append(_child("roadmap_static", os.path.abspath(a.parent_lib)))
        runs["new"].append(_child("roadmap"))
    doc = dict(what="tools/moving_bench.py --roadmap on one MI355X in one visit (see the tool's docstring): kernel ms are medians of 10 launches per process, "
                    "the lists hold one entry per round; window [0, 1], velocities of 0.2 .. 1.0 m/s.", rounds=a.rounds)
    for key, _ in ROADMAPS:
        last = runs["new"][-1][key]
        row = {k: last[k] for k in ("N", "E", "edge_samples", "O")}
        for W in [k for k in last if k.startswith("W=")]:
            new = [r[key][W]["static"]["kernel_ms"] for r in runs["new"]]
            cell = dict(items=last[W]["items"], static_new_kernel_ms=new, static_new_median=_median(new))
            if runs["parent"]:
                par = [r[key][W]["static"]["kernel_ms"] for r in runs["parent"]]
                cell.update(static_parent_kernel_ms=par, static_parent_median=_median(par), parent_spread=max(par) - min(par),
                            new_over_parent=_median(new) / _median(par), within_parent_spread=bool(_median(new) <= _median(par) + (max(par) - min(par))))
            for kind in ("static", "moving_zero_velocity", "moving"):
                cell[kind] = dict(kernel_ms=_median([r[key][W][kind]["kernel_ms"] for r in runs["new"]]),
                                  checks_per_s=_median([r[key][W][kind]["checks_per_s"] for r in runs["new"]]),
                                  free_nodes=last[W][kind]["free_nodes"], free_edges=last[W][kind]["free_edges"])
            cell["moving_zero_velocity_over_static"] = _median([r[key][W]["moving_zero_velocity_over_static"] for r in runs["new"]])
            cell["moving_over_static"] = _median([r[key][W]["moving_over_static"] for r in runs["new"]])
            row[W] = cell
        doc[key] = row
    out = a.out or os.path.join(ROOT, "profiles", "moving_roadmap_bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


def _child(what, lib=None):
    env = dict(os.environ)
    if lib:
        env["ARMOUR_HIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", what], capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"worker {what} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--roadmap", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        from armour_amd import _lib
        if not _lib.load().armour_device_available():
            raise SystemExit("moving_bench: no HIP device visible (nothing here can be measured without one)")
        res = {"build_static": lambda: worker_build(False), "build": lambda: worker_build(True), "eval": worker_eval, "audit": worker_audit,
               "roadmap_static": lambda: worker_roadmap(False), "roadmap": lambda: worker_roadmap(True)}[a.worker]()
        print(json.dumps(res))
        return
    if a.roadmap:
        return main_roadmap(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "moving_bench.json")
    runs = {"parent": [], "new": []}
    for _ in range(a.rounds):
        if a.parent_lib:
            runs["parent"].append(_child("build_static", os.path.abspath(a.parent_lib)))
        runs["new"].append(_child("build"))
    build = {}
    for B in SHAPES:
        new = [r[f"static/B={B}"]["wall_ms"] for r in runs["new"]]
        mov = [r[f"moving/B={B}"]["wall_ms"] for r in runs["new"]]
        row = dict(static_new_wall_ms=new, static_new_median=_median(new), moving_wall_ms=mov, moving_median=_median(mov),
                   static_new_device_ms=_median([r[f"static/B={B}"]["device_ms"] for r in runs["new"]]),
                   moving_device_ms=_median([r[f"moving/B={B}"]["device_ms"] for r in runs["new"]]),
                   moving_excess_ms=_median(mov) - _median(new),
                   obstacle_bytes_static=B * O * 96, obstacle_bytes_moving=B * T * O * 96, d_column_bytes=B * 7 * T * O * 24 * 8 if B >= 8 else 0)
        if runs["parent"]:
            par = [r[f"static/B={B}"]["wall_ms"] for r in runs["parent"]]
            row.update(static_parent_wall_ms=par, static_parent_median=_median(par), parent_spread=max(par) - min(par),
                       static_parent_device_ms=_median([r[f"static/B={B}"]["device_ms"] for r in runs["parent"]]),
                       new_over_parent=_median(new) / _median(par), within_parent_spread=bool(_median(new) <= _median(par) + (max(par) - min(par))))
        build[f"B={B}"] = row
    doc = dict(what="tools/moving_bench.py on one MI355X in one visit (see the tool's docstring for what each row is): T = 100, O = 20; d_column_bytes = the d "
                    "entries of the 24 live planes of a box world that a moving table of >= 8 problems stores and a static one does not.",
               rounds=a.rounds, build=build, evaluation=_child("eval"), audit=_child("audit"),
               audit_yardstick="profiles/refactor_audit_ab.json world_audit rows (executed pieces of run_trials, not the random pieces used here)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["build"], indent=1))
    print(json.dumps(doc["evaluation"], indent=1))
    print(json.dumps({k: {kk: (vv["items_per_s"] if isinstance(vv, dict) else vv) for kk, vv in v.items()} for k, v in doc["audit"].items()}, indent=1))


if __name__ == "__main__":
    main()
