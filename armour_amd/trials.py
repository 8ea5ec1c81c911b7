"""Whole planning trials: the reference's experiment loop (kinova_src/scripts/kinova_run_100_worlds.m driving KSI/simulator_armtd.m:159-349)
for W worlds in lockstep, composed of the library's entries.

    res = run_trials(scenes.reference_worlds())          # [(name, problem)] records: start q0, goal, obstacles, lookahead
    res["summary"]                                        # goals reached / collisions / stuck, planning time per iteration
    res["worlds"][w]["outcome"], ["iterations"], ["records"]
    states = moving_states(res)                           # (q0, qd0, qdd0, q_des, obstacles) of every iteration after the first

Per iteration, for the worlds still live, in ONE batch on one ArmourNLP handle: waypoint from the high-level planner (the global goal when
it yields none, KSI/uarmtd_planner.m:241-245), armour_set_problems + armour_solve, then per world
  * feasible: the new plan is executed on [0, t_plan]; the next (q0, qd0, qdd0) is the plan at t_plan (armour_desired_trajectory), so the
    hand-over is C2; the failure count returns to 0;
  * infeasible: the previous plan is executed on [t_plan, duration] -- its braking half -- and the arm is then at rest at that plan's end;
    with no previous plan, or already at rest, the arm stays; the failure count goes up and the trial ends `stuck` when it EXCEEDS
    stop_threshold (simulator_armtd.m:189-200);
  * the executed pieces of all live worlds are audited in one armour_path_audit call (verdict 1 ends the trial `collision`; verdict 2,
    undecided, is counted and ends nothing);
  * goal check as KSI/kinova_world_static.m:417-425: |angdiff(q, goal)|_2 <= goal_radius at the piece's end or at one of `goal_nodes`
    evenly spaced nodes on it, in closed form on the host;
  * the iteration cap ends the trial `iteration_limit`.
With velocities (obstacles in linear motion) every world has a clock: the tables are built from worlds.moving_frames at the world's clock, the
executed piece goes to armour_path_audit_moving with the world time of its plan time 0, and the clock advances by the executed window.
A world that ends leaves the next batch.  With per_step_build=True (ARMOUR_OPT_P1_BUILD held to the per-step kernel) a world's record does
not depend on which other worlds share its batch -- the header's own contract.
"""
import time

import numpy as np

from . import _lib, scenes
from .path_audit import FREE, HIT, UNDECIDED, audit, audit_moving, audit_self
from .planner import ArmourNLP, default_params, desired_trajectory, kinova_robot

OUTCOMES = ("goal", "collision", "stuck", "iteration_limit")
SELF_OUTCOME = "self_collision"   # only with run_trials(self_check="stop")
STRUCK_OUTCOME = "struck_at_rest"  # only with run_trials(velocities=...): a moving obstacle ran into an arm that stood still


def bezier_q(q0, qd0, qdd0, k, k_range, duration, t):
    """q of the plan at times t [K] -> [K, n]: the closed form of armour_desired_trajectory (bezier.h q_des) in numpy."""
    q0, qd0, qdd0, k = (np.asarray(a, dtype=np.float64) for a in (q0, qd0, qdd0, k))
    D = float(duration)
    a, b, ka = qd0 * D, qdd0 * D * D, np.asarray(k_range, dtype=np.float64) * k
    s = (np.asarray(t, dtype=np.float64) / D)[:, None]
    u = s - 1
    B0, B1, B2, B3, B4, B5 = -u ** 5, 5 * s * u ** 4, -10 * s ** 2 * u ** 3, 10 * s ** 3 * u ** 2, -5 * s ** 4 * u, s ** 5
    b0, b1, b2, b3 = q0, q0 + a / 5, q0 + (2 * a) / 5 + b / 20, q0 + ka
    return B0 * b0 + B1 * b1 + B2 * b2 + (B3 + B4 + B5) * b3


def goal_reached(q_nodes, goal, goal_radius):
    """kinova_world_static.goal_check, 'configuration': any node with |angdiff(q, goal)|_2 <= goal_radius (every joint wrapped)."""
    dz = np.abs(scenes.angdiff(np.atleast_2d(q_nodes), np.asarray(goal, dtype=np.float64)))
    return bool(np.any(np.sqrt((dz * dz).sum(-1)) <= goal_radius))


class StraightLineHLP:
    """robot_arm_straight_line_HLP: the point `lookahead` along the (wrapped) straight line to the goal; None at the goal itself."""

    def __init__(self, goal):
        self.goal = np.asarray(goal, dtype=np.float64)

    def get_waypoint(self, q_cur, lookahead):
        d = self.goal - q_cur
        d[scenes.CONTINUOUS] = scenes.angdiff(q_cur[scenes.CONTINUOUS], self.goal[scenes.CONTINUOUS])
        if not np.any(d):
            return None
        return scenes.straight_line_waypoint(q_cur, self.goal, lookahead)


class DevicePlanner:
    """The planning backend of run_trials: one ArmourNLP handle; plan() is armour_set_problems + armour_solve for one batch."""

    def __init__(self, robot=None, T=128, max_batch=128, max_obstacles=16, per_step_build=False, device=0, solve_options=None, rescue_candidates=0):
        self.robot = robot if robot is not None else kinova_robot()
        self.T = int(T)
        self.params = default_params(T)
        n = self.robot.num_factors
        self.k_range = np.array(self.params.k_range[:n])
        self.duration, self.t_plan = self.params.duration, self.params.t_plan
        self.nlp = ArmourNLP(robot=self.robot, params=self.params, device=device,
                             limits=_lib.ArmourLimits(max_batch=int(max_batch), max_obstacles=int(max_obstacles)))
        if per_step_build:
            self.nlp.set_option(_lib.OPT_P1_BUILD, 1)
        self.solve_options = dict(solve_options or {})
        # > 0: an infeasible solve is followed by a sweep of this many candidates and one more solve from the safe ones (ArmourNLP.solve_rescued)
        self.rescue_candidates = int(rescue_candidates)

    def plan(self, q0, qd0, qdd0, q_des, obstacles):
        """[B, n] x 4 and [B, O, 12] -> (results [B] of dict(k_opt, feasible, iterations, time_ms, ...), build_ms, solve_ms) -- the two times
        are the batch's: device time of the reach-set build and wall time of the solve."""
        self.nlp.set_parameters(q0, qd0, qdd0, q_des, obstacles)
        return self._solve()

    def plan_moving(self, q0, qd0, qdd0, q_des, frames):
        """plan() against moving obstacles: frames [B, T, O, 12] as worlds.moving_frames builds them (ArmourNLP.set_parameters_moving)."""
        self.nlp.set_parameters_moving(q0, qd0, qdd0, q_des, frames)
        return self._solve()

    def _solve(self):
        build_ms = self.nlp.build_ms
        t0 = time.perf_counter()
        if self.rescue_candidates > 0:
            res, rescued = self.nlp.solve_rescued(S=self.rescue_candidates, **self.solve_options)
            res = [dict(r, rescued=int(c)) for r, c in zip(res, rescued)]
        else:
            res = self.nlp.solve(**self.solve_options)
        return res, build_ms, (time.perf_counter() - t0) * 1e3

    def close(self):
        self.nlp.close()


def _world_record(world):
    name, p = world
    q0 = np.asarray(p["q0"], dtype=np.float64)
    return dict(name=name, start=q0.copy(), goal=np.asarray(p["goal"], dtype=np.float64), obstacles=np.asarray(p["obstacles"], dtype=np.float64).reshape(-1, 12),
                lookahead=float(p.get("lookahead", 1.0)))


def run_trials(worlds, robot=None, *, hlp="straight", goal_radius=np.pi / 30, stop_threshold=4, max_iterations=300, audit_step=0.01, tube=None,
               tracked=False, track_samples=1, track_dt=1e-3, track_seed=0, goal_nodes=10, T=128, per_step_build=False, solve_options=None,
               backend=None, audit_on_host=False, clearance=True, device=0, rescue_candidates=0, self_check=None, self_pairs=None, self_shrink=None,
               velocities=None):
    """Run every world of `worlds` ([(name, problem)] as scenes.reference_worlds() gives them; a problem holds q0 = the start at rest, goal,
    obstacles [O, 12] and lookahead) to its end.  hlp: "straight" or a factory (world index, world record) -> object with
    get_waypoint(q_cur, lookahead) (e.g. a RoadmapHLP; None = no waypoint: the goal is used); a factory that also has
    get_waypoints(indices, qs, lookaheads) -> list is asked once per iteration for all live worlds instead.  batches[] records hlp_ms, the
    wall time of an iteration's waypoint queries.  tube: None or "ultimate_bound" (every joint's
    radius = the controller's ultimate position bound, tracking.ultimate_bound) or an [n] array: the radius the audit takes about each
    executed piece.  tracked: also execute every piece with armour_track on `track_samples` sampled plants per world (slow; opt-in).
    backend: an object with plan(), robot, k_range, duration, t_plan (default: DevicePlanner).  rescue_candidates > 0 (default 0: today's path):
    the default backend answers an infeasible solve with a candidate sweep and a second solve from the safe candidates (ArmourNLP.solve_rescued);
    every record carries `rescued` (0 not needed, 1 a candidate became the plan, 2 the solve from it did, -1 no safe candidate) and the summary
    counts `rescued_iterations`.  self_check: None (default: no extra call, records unchanged), "record" (one armour_path_audit_self call per
    iteration for the executed pieces, with the world audit's tube and step and the table self_pairs / self_shrink; every record carries
    `self_verdict`, `self_t_hit` and `self_clearance`, the summary counts `self_hit_pieces` and `self_undecided_pieces`) or "stop" (as "record",
    and verdict 1 ends the world with the outcome `self_collision`, after a world collision and before the goal check).
    velocities: None (default: static worlds, today's path) or a list of [O_w, 3], every obstacle's constant velocity; `obstacles` are then the
    poses at world time 0.  Every world has a clock t_world that starts at 0.  A factory that has set_world_times(t_world [W]) is given all
    worlds' clocks before the waypoint query (roadmap.moving_field_hlps).  The backend is asked plan_moving(q0, qd0, qdd0, q_des, frames
    [B, T, O, 12]) with frames[b] = worlds.moving_frames(obstacles_w, velocity_w, backend.T, duration, t_world_w), and the state keeps with a
    plan the world time of its plan time 0.  The executed pieces go to audit_moving: a `plan` or `stay` piece with t_world = the clock, a
    `brake` piece with the stored world time of its plan (its window [t_plan, duration] belongs to the plan made one iteration earlier, whose
    frames covered that span).  The clock then advances by the executed window: t_plan, duration - t_plan for a `brake`.  Every record carries
    `t_world`, the clock at which the iteration planned.  A proved hit on a `stay` piece -- a moving obstacle ran into an arm that stood still,
    which no planner can prevent -- ends the world `struck_at_rest` (counted in the summary only with velocities); on a `plan` or `brake` piece
    it stays `collision`.
    Returns dict(worlds, summary, ...)."""
    if self_check not in (None, "record", "stop"):
        raise ValueError(f"unknown self_check {self_check!r}")
    ws = [_world_record(w) for w in worlds]
    W = len(ws)
    own_backend = backend is None
    if own_backend:
        backend = DevicePlanner(robot=robot, T=T, max_batch=max(W, 1), max_obstacles=max([w["obstacles"].shape[0] for w in ws] + [1]),
                                per_step_build=per_step_build, device=device, solve_options=solve_options, rescue_candidates=rescue_candidates)
    robot = backend.robot
    n = robot.num_factors
    k_range, D, t_plan = np.asarray(backend.k_range, dtype=np.float64), float(backend.duration), float(backend.t_plan)
    O = max([w["obstacles"].shape[0] for w in ws] + [1])
    obstacles = np.stack([scenes.pad_obstacles(w["obstacles"], O) for w in ws]) if W else np.zeros((0, O, 12))
    moving = velocities is not None
    if moving:
        from .worlds import moving_frames
        vel = [np.asarray(v, dtype=np.float64).reshape(-1, 3) for v in velocities]
        if len(vel) != W or any(v.shape[0] != w["obstacles"].shape[0] for v, w in zip(vel, ws)):
            raise ValueError("run_trials: velocities holds one [O_w, 3] per world")
        velocity = np.stack([np.concatenate([v, np.zeros((O - v.shape[0], 3))]) for v in vel]) if W else np.zeros((0, O, 3))
        t_world = np.zeros(W)
    if isinstance(tube, str):
        if tube != "ultimate_bound":
            raise ValueError(f"unknown tube {tube!r}")
        from .tracking import ultimate_bound
        tube_e = np.full(n, ultimate_bound(robot)[1])
    else:
        tube_e = None if tube is None else np.broadcast_to(np.asarray(tube, dtype=np.float64), (n,)).copy()
    hlps = [StraightLineHLP(w["goal"]) if hlp == "straight" else hlp(i, w) for i, w in enumerate(ws)]
    batch_hlp = getattr(hlp, "get_waypoints", None)      # a factory that answers all live worlds in one call (roadmap.field_hlps(batched=True))
    z = np.zeros(n)
    st = [dict(q=w["start"].copy(), qd=z.copy(), qdd=z.copy(), plan=None, at_rest=True, fails=0, outcome=None, records=[], undecided=0) for w in ws]
    if tracked:
        from .tracking import plant_samples, simulate_tracking, ultimate_bound
        rng = np.random.default_rng(track_seed)
        sm, sI = plant_samples(robot, W * track_samples, robot.mass_uncertainty, rng)
        sm, sI = sm.reshape(W, track_samples, n), sI.reshape(W, track_samples, n)
        for s in st:
            s["z"] = None
    batches = []
    for it in range(1, max_iterations + 1):
        live = [i for i in range(W) if st[i]["outcome"] is None]
        if not live:
            break
        # 1. waypoints
        t_hlp = time.perf_counter()
        if moving and hasattr(hlp, "set_world_times"):
            hlp.set_world_times(t_world.copy())
        if batch_hlp is not None:      # one call for all live worlds
            wps = batch_hlp(list(live), [st[i]["q"].copy() for i in live], [ws[i]["lookahead"] for i in live])
        else:
            wps = [hlps[i].get_waypoint(st[i]["q"].copy(), ws[i]["lookahead"]) for i in live]
        q_des = [ws[i]["goal"].copy() if wp is None else np.asarray(wp, dtype=np.float64) for i, wp in zip(live, wps)]
        hlp_ms = (time.perf_counter() - t_hlp) * 1e3
        q0, qd0, qdd0, q_des = (np.stack(a) for a in ([st[i]["q"] for i in live], [st[i]["qd"] for i in live], [st[i]["qdd"] for i in live], q_des))
        # 2. one batch
        if moving:
            frames = np.stack([moving_frames(obstacles[i], velocity[i], backend.T, D, t_world[i]) for i in live])
            res, build_ms, solve_ms = backend.plan_moving(q0, qd0, qdd0, q_des, frames)
        else:
            res, build_ms, solve_ms = backend.plan(q0, qd0, qdd0, q_des, obstacles[live])
        batches.append(dict(iteration=it, live=len(live), hlp_ms=hlp_ms, build_ms=build_ms, solve_ms=solve_ms))
        # 3 / 4. what every world executes: (plan q0, qd0, qdd0, k, ta, tb) and its next state
        pieces, piece_t0 = [], []   # piece_t0 (moving worlds): the world time of every piece's plan time 0
        for b, i in enumerate(live):
            s, r = st[i], res[b]
            rec = dict(iteration=it, q0=q0[b].copy(), qd0=qd0[b].copy(), qdd0=qdd0[b].copy(), q_des=q_des[b].copy(), k_opt=np.array(r["k_opt"], dtype=np.float64),
                       feasible=bool(r["feasible"]), sqp_iterations=int(r.get("iterations", 0)), build_ms=build_ms, solve_ms=float(r.get("time_ms", solve_ms)),
                       rescued=int(r.get("rescued", 0)))
            if rec["feasible"]:
                plan = (q0[b].copy(), qd0[b].copy(), qdd0[b].copy(), rec["k_opt"].copy())
                piece, kind = plan + (0.0, t_plan), "plan"
                s["q"], s["qd"], s["qdd"] = desired_trajectory(*plan, t_plan, k_range=k_range, duration=D)
                s["plan"], s["at_rest"], s["fails"] = plan, False, 0
                if moving:
                    s["plan_t_world"] = float(t_world[i])
            else:
                s["fails"] += 1
                if s["plan"] is not None and not s["at_rest"]:
                    piece, kind = s["plan"] + (t_plan, D), "brake"
                    s["q"] = desired_trajectory(*s["plan"], D, k_range=k_range, duration=D)[0]
                    s["qd"], s["qdd"], s["at_rest"] = z.copy(), z.copy(), True
                else:
                    piece, kind = (s["q"].copy(), z.copy(), z.copy(), z.copy(), 0.0, t_plan), "stay"
            rec.update(executed=kind, piece=piece, fails=s["fails"])
            if moving:
                rec["t_world"] = float(t_world[i])
                piece_t0.append(s["plan_t_world"] if kind == "brake" else float(t_world[i]))
                t_world[i] += (D - t_plan) if kind == "brake" else t_plan
            pieces.append(piece)
            s["records"].append(rec)
        # 5. one audit call for all live worlds
        cols = [np.stack([p[c] for p in pieces]) for c in range(4)]
        ta, tb = np.array([p[4] for p in pieces]), np.array([p[5] for p in pieces])
        if moving:
            au = audit_moving(robot, obstacles[live], velocity[live], np.arange(len(live), dtype=np.int32), np.array(piece_t0), *cols, k_range, D, ta, tb,
                              tube=tube_e, step=audit_step, clearance=clearance, host=audit_on_host)
        else:
            au = audit(robot, obstacles[live], np.arange(len(live), dtype=np.int32), *cols, k_range, D, ta, tb, tube=tube_e, step=audit_step,
                       clearance=clearance, host=audit_on_host)
        batches[-1]["audit_ms"] = au.ms
        if self_check is not None:
            sa = audit_self(robot, *cols, k_range, D, ta, tb, tube=tube_e, step=audit_step, pairs=self_pairs, shrink=self_shrink, clearance=clearance,
                            host=audit_on_host)
            batches[-1]["self_audit_ms"] = sa.ms
        if tracked:
            z0 = None if st[live[0]]["z"] is None else np.concatenate([st[i]["z"] for i in live])
            # the windows differ with the kind of piece: one armour_track call per window present
            tr_rows = {}
            for kind_t0, kind_t1 in sorted(set(zip(ta.tolist(), tb.tolist()))):
                sel = np.flatnonzero((ta == kind_t0) & (tb == kind_t1))
                ix = np.repeat(sel, track_samples)
                zz = None if z0 is None else z0.reshape(len(live), track_samples, 2 * n)[sel].reshape(-1, 2 * n)
                out = simulate_tracking(robot, *(c[ix] for c in cols), k_range, D, t0=kind_t0, t1=kind_t1, dt=track_dt, z0=zz,
                                        mass_scale=sm[np.array(live)[sel]].reshape(-1, n), inertia_scale=sI[np.array(live)[sel]].reshape(-1, n))
                for j, b in enumerate(sel):
                    rows = slice(j * track_samples, (j + 1) * track_samples)
                    tr_rows[int(b)] = dict(max_pos_error=float(out.max_pos_error[rows].max()), max_vel_error=float(out.max_vel_error[rows].max()),
                                           limit_flags=int(np.bitwise_or.reduce(out.limit_flags[rows])), status=int(out.status[rows].max()),
                                           z=np.concatenate([out.q[rows], out.qd[rows]], axis=1))
        # 6 / 7. verdicts, goal check, caps
        for b, i in enumerate(live):
            s, rec, p = st[i], st[i]["records"][-1], pieces[b]
            rec.update(audit_verdict=int(au.verdict[b]), t_hit=float(au.t_hit[b]), clearance=None if au.clearance is None else float(au.clearance[b]))
            if tracked:
                s["z"] = tr_rows[b].pop("z")
                rec["tracking"] = tr_rows[b]
            s["undecided"] += int(au.verdict[b] == UNDECIDED)
            if self_check is not None:
                rec.update(self_verdict=int(sa.verdict[b]), self_t_hit=float(sa.t_hit[b]), self_clearance=None if sa.clearance is None else float(sa.clearance[b]))
            nodes = bezier_q(p[0], p[1], p[2], p[3], k_range, D, np.linspace(p[4], p[5], goal_nodes + 1))
            rec["goal_reached"] = goal_reached(nodes, ws[i]["goal"], goal_radius)
            if au.verdict[b] == HIT:
                s["outcome"] = STRUCK_OUTCOME if moving and rec["executed"] == "stay" else "collision"
            elif self_check == "stop" and sa.verdict[b] == HIT:
                s["outcome"] = SELF_OUTCOME
            elif rec["goal_reached"]:
                s["outcome"] = "goal"
            elif s["fails"] > stop_threshold:
                s["outcome"] = "stuck"
            elif it == max_iterations:
                s["outcome"] = "iteration_limit"
    if own_backend:
        backend.close()
    out_worlds = [dict(name=w["name"], outcome=s["outcome"], iterations=len(s["records"]), undecided=s["undecided"], records=s["records"],
                       goal=w["goal"], obstacles=w["obstacles"]) for w, s in zip(ws, st)]
    plan_ms = np.array([b["build_ms"] + b["solve_ms"] for b in batches]) if batches else np.zeros(0)
    pieces_n = sum(len(s["records"]) for s in st)
    summary = dict(worlds=W, **{o: sum(1 for s in st if s["outcome"] == o) for o in OUTCOMES},
                   iterations=int(sum(b["live"] for b in batches)), batches=len(batches), pieces=pieces_n,
                   undecided_pieces=int(sum(s["undecided"] for s in st)),
                   rescued_iterations=int(sum(1 for s in st for r in s["records"] if r["rescued"] > 0)),
                   batch_planning_ms_mean=float(plan_ms.mean()) if plan_ms.size else 0.0, batch_planning_ms_max=float(plan_ms.max()) if plan_ms.size else 0.0,
                   planning_ms_per_world_iteration=float(plan_ms.sum() / max(1, sum(b["live"] for b in batches))),
                   audit_ms_total=float(sum(b.get("audit_ms", 0.0) for b in batches)))
    if self_check is not None:
        sv = [r["self_verdict"] for s in st for r in s["records"]]
        summary.update(self_hit_pieces=sum(1 for v in sv if v == HIT), self_undecided_pieces=sum(1 for v in sv if v == UNDECIDED))
        if self_check == "stop":
            summary[SELF_OUTCOME] = sum(1 for s in st if s["outcome"] == SELF_OUTCOME)
    if moving:
        summary[STRUCK_OUTCOME] = sum(1 for s in st if s["outcome"] == STRUCK_OUTCOME)
    if tracked:
        ub, qe, qde = ultimate_bound(robot)
        trk = [r["tracking"] for s in st for r in s["records"]]
        summary["tracking"] = dict(ultimate_bound_position=qe, ultimate_bound_velocity=qde, max_pos_error=max(t["max_pos_error"] for t in trk),
                                   max_vel_error=max(t["max_vel_error"] for t in trk), limit_flags=int(np.bitwise_or.reduce([t["limit_flags"] for t in trk])),
                                   worst_status=max(t["status"] for t in trk))
    return dict(worlds=out_worlds, summary=summary, batches=batches, k_range=k_range, duration=D, t_plan=t_plan)


def moving_states(result):
    """(q0, qd0, qdd0, q_des, obstacles) of every planning iteration after a world's first -- the states a re-planning arm really plans from
    (a list; obstacles are the world's own, unpadded), with a sixth element dict(world, name, iteration, feasible)."""
    out = []
    for w, wr in enumerate(result["worlds"]):
        for rec in wr["records"][1:]:
            out.append((rec["q0"], rec["qd0"], rec["qdd0"], rec["q_des"], wr["obstacles"], dict(world=w, name=wr["name"], iteration=rec["iteration"],
                                                                                              feasible=rec["feasible"])))
    return out
