#!/usr/bin/env python3
"""armour_track on the MI355X: device ms per call and rollout-steps/s for whole rollouts of the reference's controller study
(T = 2.5 s, dt = 1e-3, robust controller, Kinova, true plants 1.01 x nominal) at B = 1, 16, 128, 700 (the reference study's 7 x 100)
and 4096; the per-step cost of the robust, the passive and the Althoff mode behind armour_track's automatic steps per launch (tracking.hip
kStepMs*); writes profiles/track_bench.json.

    python tools/track_bench.py [--out profiles/track_bench.json] [--batches 1,16,128,700,4096] [--T 2.5]
    python tools/track_bench.py --tau-study      # host restatement only (no GPU): maxima at dt = 1e-3 against dt = 5e-4
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _inputs(rb, B, rng):
    n = rb.num_factors
    q0 = rng.uniform(-np.pi / 2, np.pi / 2, (B, n))
    qd0 = rng.uniform(-np.pi / 2, np.pi / 2, (B, n))
    return q0, qd0


def per_step(rb, controller, B=64, steps=60, S=20):
    """device ms per RK4 step of one lane (every lane in parallel): a run of `steps` steps with S steps per launch, minus nothing --
    the launches are back to back on one stream, so the event time is the kernels' own."""
    from armour_amd.tracking import simulate_tracking
    n = rb.num_factors
    rng = np.random.default_rng(1)
    q0, qd0 = _inputs(rb, B, rng)
    kw = dict(t1=steps * 1e-3, dt=1e-3, controller=controller, steps_per_launch=S)
    simulate_tracking(rb, q0, qd0 * 0, np.zeros((B, n)), -q0, np.ones(n), 2.5, **kw)   # warm-up (code object load)
    res = simulate_tracking(rb, q0, qd0 * 0, np.zeros((B, n)), -q0, np.ones(n), 2.5, **kw)
    return res.device_ms / (steps + 1)


def bench(args):
    from armour_amd import _lib
    from armour_amd.planner import kinova_robot
    from armour_amd.tracking import simulate_tracking
    L = _lib.load()
    rb = kinova_robot()
    n = rb.num_factors
    out = dict(what="armour_track, Kinova, robust controller, T = %g s, dt = 1e-3, true plant 1.01 x nominal; device ms = events around the launches" % args.T,
               per_step_ms={c: per_step(rb, c) for c in ("robust", "none", "althoff")},
               auto_steps_per_launch={c: L.armour_track_auto_steps(v) for c, v in (("robust", 0), ("nominal", 1), ("none", 2), ("althoff", 4))}, rows=[])
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}), flush=True)
    for B in [int(x) for x in args.batches.split(",")]:
        rng = np.random.default_rng(B)
        q0, qd0 = _inputs(rb, B, rng)
        t = time.perf_counter()
        res = simulate_tracking(rb, q0, qd0, np.zeros((B, n)), -q0, np.ones(n), args.T, mass_scale=np.full((B, n), 0.01),
                                inertia_scale=np.full((B, n), 0.01))
        wall = time.perf_counter() - t
        steps = int(res.steps.sum())
        row = dict(B=B, device_ms=res.device_ms, wall_s=wall, rollout_steps=steps, rollout_steps_per_s=steps / (res.device_ms * 1e-3),
                   status_counts={int(s): int((res.status == s).sum()) for s in np.unique(res.status)})
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def tau_study(args):
    """The host restatement (tests/test_tracking.py host_track) at dt and dt / 2 for a few robust rollouts of the guarantee test's
    kind: the relative change of every monitored maximum bounds what the step size adds to the continuous-time guarantee."""
    from armour_amd.planner import kinova_robot
    from armour_amd.tracking import plant_samples
    from test_tracking import _plans, _start_inside, host_track
    rb = kinova_robot()
    n = rb.num_factors
    rng = np.random.default_rng(12)
    B, kr = args.tau_rollouts, np.full(n, np.pi / 48)
    q0, qd0, qdd0, k = _plans(rng, B)
    sm, sI = plant_samples(rb, B, rb.mass_uncertainty, rng)
    z0 = _start_inside(rb, rng, q0, qd0, qdd0, k, kr, 1.0, sm, sI)
    worst = 0.0
    for b in range(B):
        a, c = [host_track(rb, q0[b], qd0[b], qdd0[b], k[b], kr, 1.0, t1=args.tau_t1, dt=dt, z0=z0[b], sm=sm[b], sI=sI[b]) for dt in (1e-3, 5e-4)]
        rel = {m: abs(a[m] - c[m]) / c[m] for m in ("max_V", "max_pos_error", "max_vel_error")}
        worst = max(worst, max(rel.values()))
        print(json.dumps(dict(rollout=b, V_over_Vmax=a["max_V"] / rb.V_m, **rel)), flush=True)
    print(json.dumps(dict(worst_relative_change=worst)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_bench.json"))
    ap.add_argument("--batches", default="1,16,128,700,4096")
    ap.add_argument("--T", type=float, default=2.5)
    ap.add_argument("--tau-study", action="store_true")
    ap.add_argument("--tau-rollouts", type=int, default=4)
    ap.add_argument("--tau-t1", type=float, default=1.0)
    a = ap.parse_args()
    tau_study(a) if a.tau_study else bench(a)
