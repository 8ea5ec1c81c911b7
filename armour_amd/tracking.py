"""Closed-loop tracking on the device: the planner's Bezier plan executed by an arm with uncertain masses and inertias under the
tracking controller (armour_track, include/armour_hip.h).

    res = simulate_tracking(robot, q0, qd0, qdd0, k, k_range, duration, ...)   # B rollouts, numpy in / numpy out
    s_m, s_I = plant_samples(robot, B, uncertainty, rng)                       # true plants within +-uncertainty
    runs = simulate_plans(nlp, nlp.solve(), samples=8, rng=rng)                # every feasible plan of an ArmourNLP
    summary = compare_robust_controller(levels, samples, seed)                 # kinova_compare_robust_controller.m, ARMOUR's half
    study = compare_robust_controller(..., controllers=("robust", "althoff"))  # both halves and the summary script's per-joint medians

The reference integrates one rollout at a time with ode15s and the controller MEX in the right-hand side
(KSI/uarmtd_agent.m:280-293, :360-405); here every rollout is a device lane running fixed-step RK4, all arithmetic in libarmour_hip.so.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import ArmourTrackOptions, ArmourTrackResult, _dp, check
from .planner import kinova_robot

CONTROLLERS = {"robust": _lib.TRACK_CTL_ROBUST, "nominal": _lib.TRACK_CTL_NOMINAL, "none": _lib.TRACK_CTL_NONE, "althoff": _lib.TRACK_CTL_ALTHOFF}


def ultimate_bound(robot, V_max=None, Kr=None):
    """(ub, qe, qde) of KSI/uarmtd_robust_CBF_LLC.m:36-40: ub = sqrt(2 V_max / M_min), qe = ub / min(Kr), qde = 2 ub."""
    V_max = robot.V_m if V_max is None else V_max
    kr = robot.K if Kr is None else float(np.min(Kr))
    ub = float(np.sqrt(2 * V_max / robot.M_min))
    return ub, ub / kr, 2 * ub


def default_options(robot):
    opt = ArmourTrackOptions()
    _lib.load().armour_track_options_default(C.byref(robot), C.byref(opt))
    return opt


@dataclass
class TrackResult:
    """Per rollout ([B] / [B, n]): status (0 reached t1, 1 nominal torque outside the interval torque, 2 non-finite state), steps,
    limit_flags (bit 0 torque, 1 position, 2 speed), t_end, the last node's q / qd, the running maxima, first_violation_t (NaN: none);
    trace [B, nodes, 3, n] (q, qd, u per recorded node) or None; device_ms of the call."""
    status: np.ndarray
    steps: np.ndarray
    limit_flags: np.ndarray
    t_end: np.ndarray
    q: np.ndarray
    qd: np.ndarray
    max_pos_error: np.ndarray
    max_vel_error: np.ndarray
    max_V: np.ndarray
    max_robust_input: np.ndarray
    max_torque_ratio: np.ndarray
    first_violation_t: np.ndarray
    trace: np.ndarray
    device_ms: float


def simulate_tracking(robot, q0, qd0, qdd0, k, k_range, duration, t0=0.0, t1=None, dt=1e-3, controller="robust", z0=None,
                      mass_scale=None, inertia_scale=None, Kr=None, alpha=None, V_max=None, r_norm_threshold=None, model_uncertainty=None,
                      record_every=0, steps_per_launch=0, althoff_Kp=None):
    """B rollouts of armour_track.  q0 / qd0 / qdd0 / k: [B, n] (or [n]); k_range: [n]; z0: [B, 2n] actual (q, qd) at t0 or None (on the
    reference); mass_scale / inertia_scale: [B, n] or None.  Controller constants default to armour_track_options_default (the robot's;
    althoff_Kp: the (phi, kappa) pair of controller "althoff", default the reference's 28.1037 twice)."""
    L = _lib.load()
    robot = robot if robot is not None else kinova_robot()
    n = robot.num_factors
    q0, qd0, qdd0, k = [np.ascontiguousarray(np.atleast_2d(np.asarray(a, dtype=np.float64))) for a in (q0, qd0, qdd0, k)]
    B = q0.shape[0]
    for a in (q0, qd0, qdd0, k):
        if a.shape != (B, n):
            raise ValueError(f"expected shape ({B},{n}), got {a.shape}")
    k_range = np.ascontiguousarray(np.broadcast_to(np.asarray(k_range, dtype=np.float64), (n,)))
    z0 = None if z0 is None else np.ascontiguousarray(np.asarray(z0, dtype=np.float64).reshape(B, 2 * n))
    sm = None if mass_scale is None else np.ascontiguousarray(np.broadcast_to(np.asarray(mass_scale, dtype=np.float64), (B, n)))
    sI = None if inertia_scale is None else np.ascontiguousarray(np.broadcast_to(np.asarray(inertia_scale, dtype=np.float64), (B, n)))
    opt = default_options(robot)
    opt.controller = CONTROLLERS[controller] if isinstance(controller, str) else int(controller)
    opt.record_every, opt.steps_per_launch = int(record_every), int(steps_per_launch)
    if Kr is not None:
        kr = np.broadcast_to(np.asarray(Kr, dtype=np.float64), (n,))
        for i in range(n):
            opt.Kr[i] = kr[i]
    for name, val in (("alpha", alpha), ("V_max", V_max), ("r_norm_threshold", r_norm_threshold), ("model_uncertainty", model_uncertainty)):
        if val is not None:
            setattr(opt, name, float(val))
    if althoff_Kp is not None:
        opt.althoff_Kp[0], opt.althoff_Kp[1] = [float(x) for x in np.broadcast_to(np.asarray(althoff_Kp, dtype=np.float64), (2,))]
    opt.dt, opt.t0, opt.duration = float(dt), float(t0), float(duration)
    opt.t1 = float(duration if t1 is None else t1)
    N = int(np.ceil((opt.t1 - opt.t0) / opt.dt - 1e-9)) if opt.dt > 0 and opt.t1 > opt.t0 else 0
    trace = np.zeros((B, N // record_every + 1, 3, n)) if record_every > 0 and N > 0 else None
    res = (ArmourTrackResult * B)()
    ms = C.c_double(0.0)
    check(L.armour_track(C.byref(robot), C.byref(opt), B, _dp(q0), _dp(qd0), _dp(qdd0), _dp(k), _dp(k_range), _dp(z0), _dp(sm), _dp(sI),
                         res, _dp(trace), C.byref(ms)))
    f = lambda name: np.array([getattr(r, name) for r in res])
    return TrackResult(status=f("status"), steps=f("steps"), limit_flags=f("limit_flags"), t_end=f("t_end"),
                       q=np.array([r.q[:n] for r in res]), qd=np.array([r.qd[:n] for r in res]),
                       max_pos_error=f("max_pos_error"), max_vel_error=f("max_vel_error"), max_V=f("max_V"),
                       max_robust_input=f("max_robust_input"), max_torque_ratio=f("max_torque_ratio"),
                       first_violation_t=f("first_violation_t"), trace=trace, device_ms=ms.value)


def plant_samples(robot, B, uncertainty, rng):
    """Per-body mass and inertia scales of B true plants, uniform in [-uncertainty, +uncertainty] and drawn independently: ([B, n], [B, n])."""
    n = robot.num_factors
    return rng.uniform(-uncertainty, uncertainty, (B, n)), rng.uniform(-uncertainty, uncertainty, (B, n))


def simulate_plans(nlp, solve_results, samples, rng, uncertainty=None, **kw):
    """Execute every feasible plan of an ArmourNLP (the problems of its last set_parameters, the k_opt of `solve_results`) over
    [0, duration] on `samples` true plants each within +-uncertainty (default: the robot's mass_uncertainty), with the robot's
    controller constants.  Returns dict(problems [P] indices of the simulated problems, skipped [..] the infeasible ones,
    result: TrackResult over P * samples rollouts, problem-major)."""
    prob = getattr(nlp, "problem", None)
    if prob is None:
        raise ValueError("simulate_plans needs an ArmourNLP after set_parameters")
    robot, params = nlp.robot, nlp.params
    n = robot.num_factors
    eps = robot.mass_uncertainty if uncertainty is None else uncertainty
    feasible = [b for b, r in enumerate(solve_results) if r["feasible"]]
    skipped = [b for b, r in enumerate(solve_results) if not r["feasible"]]
    if not feasible:
        return dict(problems=[], skipped=skipped, result=None)
    idx = np.repeat(np.array(feasible), samples)
    k = np.stack([solve_results[b]["k_opt"] for b in idx])
    sm, sI = plant_samples(robot, len(idx), eps, rng)
    res = simulate_tracking(robot, prob["q0"][idx], prob["qd0"][idx], prob["qdd0"][idx], k, np.array(params.k_range[:n]), params.duration,
                            mass_scale=sm, inertia_scale=sI, **kw)
    return dict(problems=feasible, skipped=skipped, result=res)


def node_robust_inputs(robot, controller, res, q0, qd0, qdd0, k, k_range, duration, t0=0.0, t1=None, dt=1e-3, record_every=1, Kr=None, alpha=None,
                       V_max=None, r_norm_threshold=None, model_uncertainty=None, althoff_Kp=None):
    """The robust input v at every recorded node of the rollouts in `res` (a TrackResult with a trace): kinova_compare_robust_controller.m's
    get_control_inputs loop over (tout, zout), as ONE batched armour_robust_controller / armour_althoff_controller call on the traced
    (q, qd) and the reference at each node's time.  The arguments are those of the simulate_tracking call that made `res`.  Returns
    [B, nodes, n]; nodes a rollout did not reach (NaN in the trace) are NaN."""
    from .controller import kinova_controller, kinova_controller_althoff
    L = _lib.load()
    n = robot.num_factors
    opt = default_options(robot)
    B, nodes = res.trace.shape[:2]
    q0, qd0, qdd0, k = [np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (B, n))) for a in (q0, qd0, qdd0, k)]
    k_range = np.ascontiguousarray(np.broadcast_to(np.asarray(k_range, dtype=np.float64), (n,)))
    t1 = duration if t1 is None else t1
    N = int(np.ceil((t1 - t0) / dt - 1e-9))
    h = (t1 - t0) / N
    times = [t1 if s == N else t0 + s * h for s in range(0, N + 1, record_every)]   # armour_track's node rule
    assert len(times) == nodes
    ref = np.zeros((3, B, nodes, n))
    out3 = [np.zeros(n) for _ in range(3)]
    for b in range(B):
        for j, t in enumerate(times):
            check(L.armour_desired_trajectory(n, _dp(q0[b]), _dp(qd0[b]), _dp(qdd0[b]), _dp(k_range), float(duration), _dp(k[b]), float(t), *[_dp(o) for o in out3]))
            ref[:, b, j] = out3
    reached = np.isfinite(res.trace[:, :, 0, :]).all(axis=2) & np.isfinite(res.trace[:, :, 1, :]).all(axis=2)
    idx = np.nonzero(reached)
    v = np.full((B, nodes, n), np.nan)
    if idx[0].size == 0:
        return v
    states = [res.trace[:, :, 0][idx], res.trace[:, :, 1][idx], ref[0][idx], ref[1][idx], ref[2][idx]]
    kr = np.array(opt.Kr[:n]) if Kr is None else np.broadcast_to(np.asarray(Kr, dtype=np.float64), (n,))
    eps = opt.model_uncertainty if model_uncertainty is None else model_uncertainty
    code = CONTROLLERS[controller] if isinstance(controller, str) else int(controller)
    if code == _lib.TRACK_CTL_ROBUST:
        pick = lambda val, default: default if val is None else val
        v[idx] = kinova_controller(kr, pick(alpha, opt.alpha), pick(V_max, opt.V_max), pick(r_norm_threshold, opt.r_norm_threshold), *states,
                                   eps=eps, robot=robot)[2]
    elif code == _lib.TRACK_CTL_ALTHOFF:
        kp = np.array(opt.althoff_Kp[:]) if althoff_Kp is None else althoff_Kp
        v[idx] = kinova_controller_althoff(kr, kp, np.zeros(2), 0.0, *states, eps=eps, robot=robot)[2]
    else:
        v[idx] = 0.0   # the nominal controller and the passive plant have no robust input
    return v


def compare_robust_controller(levels=(0.0, 0.05, 0.1, 0.15, 0.2, 0.25, 0.3), samples=100, seed=0, T=2.5, dt=1e-3, robot=None,
                              controllers=("robust",), study_record_every=10, **kw):
    """The workload of kinova_src/scripts/kinova_compare_robust_controller.m: per uncertainty level, `samples` random starts q0, qd0 in
    U[-pi/2, pi/2]; the reference starts 0.025 pi / 0.05 pi away in position / velocity along random unit directions and comes to rest at
    q = 0 at T; the true plant has 1.01 x the nominal masses and inertias (load_robot_params' true_mass_range); the controller's
    model_uncertainty is the level.

    controllers = ("robust",), the default: the ARMOUR controller alone.  Returns dict(levels, median_max_v [levels] -- the median over
    samples of the rollout's max |v| --, max_v [levels, samples], status [levels, samples], result: [TrackResult per level]).

    Any other tuple of CONTROLLERS names, e.g. ("robust", "althoff") -- the script's two: every controller runs on the same z0, reference
    and plants (the random draws are those of the default call with the same seed).  Each rollout records a trace every
    study_record_every steps (10 at dt = 1e-3: the script's 251 output times), v is recomputed at every recorded node (node_robust_inputs:
    the script's get_control_inputs loop) and the result is dict(levels, controllers, per_joint_max_v [levels, C, samples, n] -- max over
    recorded nodes of |v_i| --, per_joint_median_max_v [levels, C, n] -- its median over samples, the quantity
    kinova_compare_robust_controller_summary.m:19-20 plots --, max_v / status [levels, C, samples] and median_max_v [levels, C] from the
    rollouts' own monitors (every node), result: [[TrackResult per controller] per level], plans: [dict(q0, qd0, qdd0, k, k_range, z0) per
    level], wall_s [levels])."""
    import time
    robot = robot if robot is not None else kinova_robot()
    n = robot.num_factors
    rng = np.random.default_rng(seed)
    controllers = tuple(controllers)
    study = controllers != ("robust",)
    out = dict(levels=np.asarray(levels, dtype=np.float64), median_max_v=[], max_v=[], status=[], result=[])
    if study:
        out.update(controllers=controllers, per_joint_max_v=[], per_joint_median_max_v=[], plans=[], wall_s=[])

    def unit(shape):
        d = rng.uniform(-1, 1, shape)
        return d / np.linalg.norm(d, axis=1, keepdims=True)

    for level in levels:
        q0 = rng.uniform(-np.pi / 2, np.pi / 2, (samples, n))
        qd0 = rng.uniform(-np.pi / 2, np.pi / 2, (samples, n))
        traj_q0 = q0 + 0.025 * np.pi * unit((samples, n))
        traj_qd0 = qd0 + 0.05 * np.pi * unit((samples, n))
        k_range = np.ones(n)
        if study:
            t_start = time.perf_counter()
            plan = dict(q0=traj_q0, qd0=traj_qd0, qdd0=np.zeros((samples, n)), k=-traj_q0 / k_range, k_range=k_range, z0=np.concatenate([q0, qd0], axis=1))
            node_kw = {name: kw[name] for name in ("Kr", "alpha", "V_max", "r_norm_threshold", "althoff_Kp") if name in kw}
            runs, per_joint = [], []
            for c in controllers:
                res = simulate_tracking(robot, plan["q0"], plan["qd0"], plan["qdd0"], plan["k"], k_range, T, dt=dt, z0=plan["z0"],
                                        mass_scale=np.full((samples, n), 0.01), inertia_scale=np.full((samples, n), 0.01),
                                        model_uncertainty=level, **{**kw, "controller": c, "record_every": study_record_every})
                v = node_robust_inputs(robot, c, res, plan["q0"], plan["qd0"], plan["qdd0"], plan["k"], k_range, T, dt=dt,
                                       record_every=study_record_every, model_uncertainty=level, **node_kw)
                with np.errstate(invalid="ignore"):
                    per_joint.append(np.fmax.reduce(np.abs(v), axis=1))   # (fmax: nodes after a stop are NaN and count for nothing)
                runs.append(res)
            per_joint = np.array(per_joint)
            out["per_joint_max_v"].append(per_joint)
            out["per_joint_median_max_v"].append(np.median(per_joint, axis=1))
            out["max_v"].append(np.array([r.max_robust_input for r in runs]))
            out["median_max_v"].append(np.array([np.median(r.max_robust_input) for r in runs]))
            out["status"].append(np.array([r.status for r in runs]))
            out["result"].append(runs)
            out["plans"].append(plan)
            out["wall_s"].append(time.perf_counter() - t_start)
            continue
        res = simulate_tracking(robot, traj_q0, traj_qd0, np.zeros((samples, n)), -traj_q0 / k_range, k_range, T, dt=dt,
                                z0=np.concatenate([q0, qd0], axis=1), mass_scale=np.full((samples, n), 0.01),
                                inertia_scale=np.full((samples, n), 0.01), model_uncertainty=level, **kw)
        out["max_v"].append(res.max_robust_input)
        out["median_max_v"].append(float(np.median(res.max_robust_input)))
        out["status"].append(res.status)
        out["result"].append(res)
    out["max_v"], out["status"], out["median_max_v"] = np.array(out["max_v"]), np.array(out["status"]), np.array(out["median_max_v"])
    if study:
        for name in ("per_joint_max_v", "per_joint_median_max_v", "wall_s"):
            out[name] = np.array(out[name])
    return out
