"""Batched collision-aware inverse kinematics for workspace goals on the MI355X (include/armour_hip.h, armour_ik).

Every planner of the library takes its goal as a configuration; the reference's end-effector planner (arm_end_effector_RRT_star_HLP) takes
points of the workspace and turns each into a configuration with the agent's position-only inverse kinematics.  Here N targets are solved
from S start points each in one launch, every converged solution is judged by the node rule against its target's world, and the free one
nearest to a reference configuration is picked:

    p = end_effector(robot, Q)                                    # [K,n] -> [K,3]   (jacobian=True: also [K,3,n])
    res = solve_ik(robot, targets, q_ref, obstacles, world)       # [N,3], [N,n], [W,O,12], [N] -> status / best [N], q [N,n]
    goals, status = goal_configurations(worlds, robot, ee_goals)  # one target per world, q_ref = the world's start
    worlds2 = with_workspace_goals(worlds, robot, ee_goals)       # the world records with `goal` replaced: run_trials and every HLP take them

The rule (end-effector point, Jacobian, damped least-squares step, free test, pick), the statuses and the limits are stated in
include/armour_hip.h; DESIGN.md 4.12e.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import _dp, check
from .scenes import pad_obstacles, straight_line_waypoint
from .tree_planner import _motion, call_seed, sampling_box

NONE_CONVERGED, FOUND, ALL_BLOCKED = _lib.IK_NONE_CONVERGED, _lib.IK_FOUND, _lib.IK_ALL_BLOCKED
CONVERGED_BIT, FREE_BIT = 1, 2


class IKSolutions(_lib.Result):
    """What solve_ik returns: status [N] (NONE_CONVERGED / FOUND / ALL_BLOCKED), best [N] (the picked seed, -1 without one), q [N,n] (the
    picked configuration; NaN rows where status != FOUND), ms (device time of the launch; 0 on the host), margin [N] (host only, else None:
    the smallest |clearance| over the target's converged items), and with details=True the per-item arrays q_all [N,S,n], err [N,S],
    iterations [N,S], flags [N,S] (bit 0 converged, bit 1 free)."""


def _tool(tool):
    return np.zeros(3) if tool is None else np.ascontiguousarray(tool, dtype=np.float64).reshape(3)


def end_effector(robot, Q, tool=None, jacobian=False):
    """Q [K,n] (or [n]) -> the end-effector points [K,3] (or [3]): the origin of the last link frame plus R tool.  jacobian=True: also the
    position Jacobian [K,3,n] (columns of joints that are not actuated are zero).  Host arithmetic, the rule's own functions."""
    L = _lib.load()
    n = robot.num_factors
    q = np.ascontiguousarray(Q, dtype=np.float64)
    one = q.ndim == 1
    q = np.ascontiguousarray(q.reshape(-1, n))
    K = q.shape[0]
    p = np.zeros((K, 3))
    jac = np.zeros((K, 3, n)) if jacobian else None
    check(L.armour_ik_end_effector_host(C.byref(robot), K, _dp(q), _dp(_tool(tool)), _dp(p), _dp(jac)))
    if one:
        p, jac = p[0], None if jac is None else jac[0]
    return (p, jac) if jacobian else p


def solve_ik(robot, targets, q_ref, obstacles=None, world=None, seeds=0, S=32, tool=None, lb=None, ub=None, continuous=None, lam=0.05, e_max=0.1, tol=1e-9,
             max_iterations=200, host=False, details=False, velocity=None, t_from=None, t_to=None):
    """targets [N,3], q_ref [N,n] (or [n] for all), obstacles [W,O,12] (or [O,12]: W = 1; None: no obstacles), world [N] (the world of every
    target, -1: none; default: target i in world i when W == N, else world 0), seeds [N] (uint64, or one for all) -> IKSolutions.  S start
    points per target: q_ref, then S - 1 points of the box lb / ub (default: tree_planner.sampling_box).  host=True: the same rule in the
    library's host loop (no device), which also reports `margin`.
    velocity [W,O,3] with t_from / t_to ([W] or scalars): the obstacles move in a line from their poses `obstacles` of world time 0, and the
    free test of a target is armour_ik_moving's, free at every time of the window of the target's world; all three None (the default): the
    static entry."""
    L = _lib.load()
    n = robot.num_factors
    tg = np.ascontiguousarray(np.asarray(targets, dtype=np.float64).reshape(-1, 3))
    N = tg.shape[0]
    ref = np.ascontiguousarray(np.broadcast_to(np.asarray(q_ref, dtype=np.float64), (N, n)))
    obs, W, O = _lib.as_worlds(np.zeros((0, 0, 12)) if obstacles is None else obstacles)
    motion = _motion("solve_ik", W, O, velocity, t_from, t_to)
    if world is None:
        world = np.full(N, -1) if W == 0 else (np.arange(N) if W == N else np.zeros(N))
    wd = np.ascontiguousarray(np.broadcast_to(np.asarray(world, dtype=np.int32), (N,)))
    sd = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (N,)))
    cont = None if continuous is None else np.ascontiguousarray(continuous, dtype=np.uint8).reshape(n)
    dlb, dub = sampling_box(robot, cont)
    lb = np.ascontiguousarray(dlb if lb is None else lb, dtype=np.float64).reshape(n)
    ub = np.ascontiguousarray(dub if ub is None else ub, dtype=np.float64).reshape(n)
    S = int(S)
    i32, u8 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    status, best = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    q_best = np.full((N, n), np.nan)
    rows = max(S, 0) if details else 0
    q_all, err = np.zeros((N, rows, n)), np.zeros((N, rows))
    iterations, flags = np.zeros((N, rows), dtype=np.int32), np.zeros((N, rows), dtype=np.int32)
    margin = np.zeros(N) if host else None
    ms = C.c_double()
    if motion is None:
        fn, mv = L.armour_ik_host if host else L.armour_ik, ()
    else:
        fn, mv = L.armour_ik_moving_host if host else L.armour_ik_moving, motion[0]
    check(fn(C.byref(robot), None if cont is None else cont.ctypes.data_as(u8), _dp(lb), _dp(ub), _dp(_tool(tool)), N, S, W, O, _dp(obs) if obs.size else None,
             *mv, wd.ctypes.data_as(i32), _dp(tg), _dp(ref), sd.ctypes.data_as(C.POINTER(C.c_uint64)), float(lam), float(e_max), float(tol), int(max_iterations),
             status.ctypes.data_as(i32), best.ctypes.data_as(i32), _dp(q_best), _dp(q_all) if details else None, _dp(err) if details else None,
             iterations.ctypes.data_as(i32) if details else None, flags.ctypes.data_as(i32) if details else None, _dp(margin) if host else C.byref(ms)))
    out = IKSolutions(status=status, best=best, q=q_best, margin=margin, ms=0.0 if host else ms.value)
    if details:
        out.q_all, out.err, out.iterations, out.flags = q_all, err, iterations, flags
    return out


def _world_arrays(worlds):
    probs = [p for _, p in worlds]
    obs = [np.asarray(p["obstacles"], dtype=np.float64).reshape(-1, 12) for p in probs]
    O = max([o.shape[0] for o in obs] + [1])
    obstacles = np.stack([pad_obstacles(o, O) for o in obs]) if obs else np.zeros((0, O, 12))
    starts = np.stack([np.asarray(p["q0"], dtype=np.float64) for p in probs]) if probs else np.zeros((0, 0))
    return obstacles, starts


def goal_configurations(worlds, robot, ee_goals, seed=0, **ik_options):
    """`worlds` as trials.run_trials takes them ([(name, problem)]), ee_goals [W,3]: one target per world, in that world's obstacles (padded to
    the worlds' largest count), q_ref = the world's start q0, target i's seed = tree_planner.call_seed(seed, i, 0) -> (configurations [W,n]
    with NaN rows where no free solution was found, status [W]).  ik_options go to solve_ik."""
    n = robot.num_factors
    if not worlds:
        return np.zeros((0, n)), np.zeros(0, dtype=np.int32)
    obstacles, starts = _world_arrays(worlds)
    W = len(worlds)
    res = solve_ik(robot, np.asarray(ee_goals, dtype=np.float64).reshape(W, 3), starts, obstacles, np.arange(W),
                   np.array([call_seed(seed, i, 0) for i in range(W)], dtype=np.uint64), **ik_options)
    return res.q, res.status


def with_workspace_goals(worlds, robot, ee_goals, on_fail="keep", **ik_options):
    """Copies of the world records with `goal` replaced by goal_configurations' answer (and, where a record carries the first straight-line
    waypoint q_des, that waypoint towards the new goal), so that run_trials and every high-level planner take them unchanged.  A target
    without a free solution: on_fail='keep' leaves the record's own goal in place (the reference's fall-back to the goal configuration),
    'raise' raises RuntimeError."""
    if on_fail not in ("keep", "raise"):
        raise ValueError(f"on_fail = {on_fail!r} ('keep' or 'raise')")
    goals, status = goal_configurations(worlds, robot, ee_goals, **ik_options)
    out = []
    for (name, p), g, st in zip(worlds, goals, status):
        p = dict(p)
        if st == FOUND:
            p["goal"] = g.copy()
            if "q_des" in p and "lookahead" in p:
                p["q_des"] = straight_line_waypoint(p["q0"], g, p["lookahead"])
        elif on_fail == "raise":
            raise RuntimeError(f"world {name}: no free configuration reaches its workspace goal (status {int(st)})")
        out.append((name, p))
    return out
