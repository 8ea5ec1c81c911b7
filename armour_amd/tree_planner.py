"""Batched tree planner: bidirectional RRT-Connect for W worlds in one launch on the MI355X (include/armour_hip.h, armour_tree_plan).

The reference's experiment scripts plan with a single-query tree planner in 'new' mode (RRT_HLP / RRT_connect_HLP / robot_arm_RRT_HLP, a fresh
tree from where the arm is, every planning iteration).  Here a query needs no graph built beforehand, and all live worlds of a trial are
planned by one call:

    res = plan_trees(robot, obstacles, starts, goals, seeds)     # [W,O,12], [W,n], [W,n], [W] -> status [W], iterations [W], paths [W]
    res.paths[w]                                                 # [P,n] from start to goal (None unless res.status[w] == FOUND)
    hlp = TreeHLP(robot, world_obstacles, goal, seed); q_des = hlp.get_waypoint(q_cur, lookahead)
    out = run_trials(worlds, hlp=tree_hlps(worlds, robot))       # the trees as the trials' high-level planner, one call per iteration

Raw tree paths follow every kink of a random tree.  shortcut_paths (armour_path_shortcut) proves W polylines free and returns shorter ones made
of free segments, in one launch; TreeHLP / tree_hlps use it with shortcut=p (every found path is shortened with p passes) and mode='seed'
(the reference's HLP_grow_tree_mode = 'seed': the last path, from where the arm is now, is offered first and a tree grows only when it fails).

Obstacles in linear motion: plan_trees and shortcut_paths take velocity, t_from and t_to and then judge every node and sub-segment by the
roadmap's window rule (armour_tree_plan_moving, armour_path_shortcut_moving: free at every time of the world's window); TreeHLP takes a
velocity and a horizon and keeps a world clock (set_world_time), and moving_tree_hlps is tree_hlps for run_trials(velocities=...):

    res = plan_trees(robot, obstacles, starts, goals, seeds, velocity=vel, t_from=t, t_to=t + horizon)     # vel [W,O,3]
    out = run_trials(worlds, hlp=moving_tree_hlps(worlds, robot, velocities, mode="seed", shortcut=2), velocities=velocities)

The rules (hash, steer, free prefix, join; validate, prune, refine), their soundness claims and the limits are stated in
include/armour_hip.h; DESIGN.md 4.12c, 4.12d, 4.16b.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import _dp, check
from .roadmap import waypoint_along
from .scenes import pad_obstacles, straight_line_waypoint

SHORTCUT_OK, SHORTCUT_INVALID = _lib.SHORTCUT_OK, _lib.SHORTCUT_INVALID
NOT_FOUND, FOUND, START_BLOCKED, GOAL_BLOCKED, TREE_FULL = (_lib.TREE_NOT_FOUND, _lib.TREE_FOUND, _lib.TREE_START_BLOCKED, _lib.TREE_GOAL_BLOCKED,
                                                            _lib.TREE_FULL)


class TreePlans(_lib.Result):
    """What plan_trees returns: status / iterations [W], paths (a list; [P,n] where status == FOUND, else None), ms (device time of the
    launch; 0 on the host), margin [W] (host only, else None: the smallest |clearance| that decided the run), and with trees=True count
    [W,2], nodes [W,2,max_nodes,n], parent [W,2,max_nodes] (rows past count are zero)."""


def sampling_box(robot, continuous=None):
    """The default sampling box: the robot's position limits, [-pi, pi] on continuous joints."""
    n = robot.num_factors
    cont = np.array([robot.continuous[j] for j in range(n)], dtype=bool) if continuous is None else np.asarray(continuous, dtype=bool).reshape(n)
    lb = np.where(cont, -np.pi, np.array(robot.state_limits_lb[:n]))
    ub = np.where(cont, np.pi, np.array(robot.state_limits_ub[:n]))
    return lb, ub


def _motion(who, W, O, velocity, t_from, t_to):
    """The three arguments a moving entry takes after `obstacles`, as ctypes pointers (with the arrays that back them), or None when all three
    are None.  velocity [W,O,3]; t_from / t_to [W], scalars broadcast.  A partial set is a ValueError."""
    given = [x is not None for x in (velocity, t_from, t_to)]
    if not any(given):
        return None
    if not all(given):
        raise ValueError(f"{who}: velocity, t_from and t_to go together (all three or none)")
    vel = np.ascontiguousarray(velocity, dtype=np.float64)
    if vel.size != W * O * 3:
        raise ValueError(f"{who}: velocity holds {vel.size} numbers, [W, O, 3] = [{W}, {O}, 3] is expected")
    ta, tb = (np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.float64), (W,))) for t in (t_from, t_to))
    return (_dp(vel) if vel.size else None, _dp(ta), _dp(tb)), (vel, ta, tb)


def plan_trees(robot, obstacles, starts, goals, seeds, lb=None, ub=None, continuous=None, step=0.5, edge_step=0.05, max_iterations=2000, max_nodes=2048,
               trees=False, host=False, velocity=None, t_from=None, t_to=None):
    """obstacles [W,O,12] (or [O,12]: W = 1), starts / goals [W,n], seeds [W] (uint64) -> TreePlans.  lb / ub [n]: the sampling box (default:
    sampling_box).  host=True: the same rule in the library's host loop (no device), which also reports `margin`.
    velocity [W,O,3] with t_from / t_to ([W] or scalars): the obstacles move in a line from their poses `obstacles` of world time 0, and
    every check is armour_tree_plan_moving's window rule on [t_from[w], t_to[w]]; all three None (the default): the static entry."""
    L = _lib.load()
    n = robot.num_factors
    obs, W, O = _lib.as_worlds(obstacles)
    motion = _motion("plan_trees", W, O, velocity, t_from, t_to)
    s = np.ascontiguousarray(starts, dtype=np.float64).reshape(W, n)
    g = np.ascontiguousarray(goals, dtype=np.float64).reshape(W, n)
    sd = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (W,)))
    cont = None if continuous is None else np.ascontiguousarray(continuous, dtype=np.uint8).reshape(n)
    dlb, dub = sampling_box(robot, cont)
    lb = np.ascontiguousarray(dlb if lb is None else lb, dtype=np.float64).reshape(n)
    ub = np.ascontiguousarray(dub if ub is None else ub, dtype=np.float64).reshape(n)
    cap, max_points = int(max_nodes), 2 * max(int(max_nodes), 0)      # a path has at most one point per node: capacity never bites from here
    i32, u8 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    status, iterations, points = (np.zeros(W, dtype=np.int32) for _ in range(3))
    path = np.zeros((W, max_points, n))
    rows = max(cap, 0) if trees else 0
    count = np.zeros((W, 2), dtype=np.int32)
    nodes, parent = np.zeros((W, 2, rows, n)), np.zeros((W, 2, rows), dtype=np.int32)
    margin = np.zeros(W) if host else None
    ms = C.c_double()
    if motion is None:
        fn, mv = L.armour_tree_plan_host if host else L.armour_tree_plan, ()
    else:
        fn, mv = L.armour_tree_plan_moving_host if host else L.armour_tree_plan_moving, motion[0]
    check(fn(C.byref(robot), None if cont is None else cont.ctypes.data_as(u8), _dp(lb), _dp(ub), W, O, _dp(obs) if obs.size else None, *mv, _dp(s), _dp(g),
             sd.ctypes.data_as(C.POINTER(C.c_uint64)), float(step), float(edge_step), int(max_iterations), cap, max_points, status.ctypes.data_as(i32),
             iterations.ctypes.data_as(i32), points.ctypes.data_as(i32), _dp(path), count.ctypes.data_as(i32), _dp(nodes) if trees else None,
             parent.ctypes.data_as(i32) if trees else None, _dp(margin) if host else C.byref(ms)))
    paths = [path[w, :points[w]].copy() if status[w] == FOUND else None for w in range(W)]
    out = TreePlans(status=status, iterations=iterations, paths=paths, count=count, nodes=None, parent=None, margin=margin, ms=0.0 if host else ms.value)
    if trees:
        out.nodes, out.parent = nodes, parent
    return out


class ShortPaths(_lib.Result):
    """What shortcut_paths returns: status [W] (SHORTCUT_OK / SHORTCUT_INVALID), paths (a list; [P,n] where OK, else None), first_bad [W]
    (the first edge that is not free; -1 where OK), passes_done [W], length_in / length_out [W], ms (device time of the launch; 0 on the
    host) and margin [W] (host only, else None: the smallest |clearance| over the checks made)."""


def shortcut_paths(robot, obstacles, paths, edge_step=0.05, passes=2, continuous=None, host=False, velocity=None, t_from=None, t_to=None):
    """obstacles [W,O,12] (or [O,12]: W = 1), paths: W arrays [P_w,n] (P_w >= 2; the lengths may differ, they are padded) -> ShortPaths.
    Every edge of a path is proved free (else INVALID), then the path is pruned, and refined and pruned again passes - 1 times.
    host=True: the same rule in the library's host loop (no device), which also reports `margin`.
    velocity [W,O,3] with t_from / t_to ([W] or scalars): "free" is armour_path_shortcut_moving's, free at every time of the world's window;
    all three None (the default): the static entry."""
    L = _lib.load()
    n = robot.num_factors
    obs, W, O = _lib.as_worlds(obstacles)
    motion = _motion("shortcut_paths", W, O, velocity, t_from, t_to)
    ps = [np.asarray(p, dtype=np.float64).reshape(-1, n) for p in paths]
    if len(ps) != W:
        raise ValueError(f"{len(ps)} paths for {W} worlds")
    counts = np.array([p.shape[0] for p in ps], dtype=np.int32)
    max_in = max(int(counts.max()) if W else 2, 2)
    max_points = min(max(2 * max_in - 1, 2), _lib.SHORTCUT_MAX_POINTS)     # room for one refine of a path that prune could not shorten
    padded = np.zeros((W, max_in, n))
    for w, p in enumerate(ps):
        padded[w, :p.shape[0]] = p
    cont = None if continuous is None else np.ascontiguousarray(continuous, dtype=np.uint8).reshape(n)
    i32, u8 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    status, points, first_bad, passes_done = (np.zeros(W, dtype=np.int32) for _ in range(4))
    out = np.zeros((W, max_points, n))
    length_in, length_out = np.zeros(W), np.zeros(W)
    margin = np.zeros(W) if host else None
    ms = C.c_double()
    if motion is None:
        fn, mv = L.armour_path_shortcut_host if host else L.armour_path_shortcut, ()
    else:
        fn, mv = L.armour_path_shortcut_moving_host if host else L.armour_path_shortcut_moving, motion[0]
    check(fn(C.byref(robot), None if cont is None else cont.ctypes.data_as(u8), W, O, _dp(obs) if obs.size else None, *mv, max_in, _dp(padded),
             counts.ctypes.data_as(i32), float(edge_step), int(passes), max_points, status.ctypes.data_as(i32), points.ctypes.data_as(i32),
             first_bad.ctypes.data_as(i32), passes_done.ctypes.data_as(i32), _dp(out), _dp(length_in), _dp(length_out), _dp(margin) if host else C.byref(ms)))
    short = [out[w, :points[w]].copy() if status[w] == SHORTCUT_OK else None for w in range(W)]
    return ShortPaths(status=status, paths=short, first_bad=first_bad, passes_done=passes_done, length_in=length_in, length_out=length_out, margin=margin,
                      ms=0.0 if host else ms.value)


def call_seed(seed, world, call):
    """The seed of world `world`'s call number `call` (from 0) in a trial: (seed + (world << 32) + call) mod 2^64."""
    return (int(seed) + (int(world) << 32) + int(call)) % (1 << 64)


class TreeHLP:
    """High-level planner over the batched trees: get_waypoint(q_cur, lookahead) is the point `lookahead` along this call's path
    (roadmap.waypoint_along); with no path it falls back to scenes.straight_line_waypoint.  The c-th call uses the seed
    call_seed(seed, world, c) when it grows trees.
      mode='new' (the default; the reference's HLP_grow_tree_mode = 'new'): a fresh pair of trees from q_cur at every call, one one-world
        plan_trees call.
      mode='seed': the path of the last call is kept, and the next call first offers [q_cur] + path[1:] to shortcut_paths with
        max(shortcut, 1) passes; when that is OK it is the path and no tree is grown (`reused` counts these), otherwise -- or with no
        last path -- trees grow as in 'new'.
      shortcut=p > 0: every path the trees find goes through shortcut_paths(passes=p) before the waypoint is taken.
      velocity [O,3] (default None: a static world, today's calls): the obstacles move in a line from their poses `world_obstacles` of world
        time 0.  Every launch of a call -- the re-validation of a kept path, the trees, the shortening of a new path -- then judges by the
        window rule on [t, t + horizon], t the world time of the last set_world_time (0 before the first) and horizon the plan's duration
        unless given.  With mode='seed' a kept path that the new window blocks is SHORTCUT_INVALID, and trees grow."""

    def __init__(self, robot, world_obstacles, goal, seed=0, world=0, host=False, shortcut=0, mode="new", velocity=None, horizon=None, **plan_options):
        if mode not in ("new", "seed") or int(shortcut) < 0:
            raise ValueError(f"mode = {mode!r} ('new' or 'seed'), shortcut = {shortcut} (>= 0)")
        if velocity is None and horizon is not None:
            raise ValueError("horizon belongs to a moving world: give a velocity")
        self.robot, self.goal, self.seed, self.world, self.host = robot, np.asarray(goal, dtype=np.float64), int(seed), int(world), bool(host)
        self.shortcut, self.mode = int(shortcut), mode
        self.obstacles = np.asarray(world_obstacles, dtype=np.float64).reshape(-1, 12)
        self.velocity, self.horizon, self.t_world = None, None, 0.0
        if velocity is not None:
            self.velocity = np.asarray(velocity, dtype=np.float64).reshape(-1, 3)
            if self.velocity.shape[0] != self.obstacles.shape[0]:
                raise ValueError("TreeHLP: one velocity per obstacle")
            if horizon is None:
                from .planner import default_params
                horizon = default_params(1).duration
            self.horizon = float(horizon)
            if not self.horizon >= 0.0:
                raise ValueError(f"horizon = {horizon} (>= 0)")
        self.options = plan_options
        n = robot.num_factors
        cont = plan_options.get("continuous")
        self.continuous = np.array([robot.continuous[j] for j in range(n)], dtype=bool) if cont is None else np.asarray(cont, dtype=bool)
        self.calls, self.path, self.status, self.margin_min = 0, None, None, np.inf      # margin_min: over the calls so far (host only)
        self.reused = 0

    def _noted(self, res, k):
        if res.margin is not None:
            self.margin_min = min(self.margin_min, float(res.margin[k]))

    def set_world_time(self, t):
        """The world time at which the next call plans (a moving world): its window is [t, t + horizon]."""
        if self.velocity is None:
            raise ValueError("set_world_time belongs to a moving world: give a velocity")
        self.t_world = float(t)

    def get_waypoint(self, q_cur, lookahead):
        return _waypoints([self], [q_cur], [lookahead])[0][0]


def _waypoints(hl, qs, lookaheads):
    """One call of each of the HLPs `hl` (one robot, one obstacle count, the same options, all static or all moving) from qs, in at most
    three launches: the shortening of the kept paths ('seed'), the trees for the rest, the shortening of the new paths -> (waypoints, the
    launches' ms).  Moving worlds: every launch gets the window [t_world, t_world + horizon] of each of its worlds."""
    h0 = hl[0]
    robot, host, opts = h0.robot, h0.host, h0.options
    if any((h.velocity is None) != (h0.velocity is None) for h in hl):
        raise ValueError("static and moving worlds cannot share a launch")

    def motion(ks):      # the moving entries' three arguments for the worlds ks of this call
        if h0.velocity is None:
            return {}
        t = np.array([hl[k].t_world for k in ks])
        return dict(velocity=np.stack([hl[k].velocity for k in ks]), t_from=t, t_to=t + np.array([hl[k].horizon for k in ks]))

    short = dict(edge_step=opts.get("edge_step", 0.05), continuous=opts.get("continuous"), host=host)
    qs = [np.asarray(q, dtype=np.float64) for q in qs]
    paths, ms = [None] * len(hl), 0.0
    kept = [k for k, h in enumerate(hl) if h.mode == "seed" and h.path is not None]
    if kept:
        res = shortcut_paths(robot, np.stack([hl[k].obstacles for k in kept]), [np.vstack([qs[k][None], hl[k].path[1:]]) for k in kept],
                             passes=max(h0.shortcut, 1), **short, **motion(kept))
        ms += res.ms
        for i, k in enumerate(kept):
            hl[k]._noted(res, i)
            if res.status[i] == SHORTCUT_OK:
                paths[k], hl[k].status = res.paths[i], FOUND
                hl[k].reused += 1
    grow = [k for k in range(len(hl)) if paths[k] is None]
    if grow:
        res = plan_trees(robot, np.stack([hl[k].obstacles for k in grow]), np.stack([qs[k] for k in grow]), np.stack([hl[k].goal for k in grow]),
                         [call_seed(hl[k].seed, hl[k].world, hl[k].calls) for k in grow], host=host, **opts, **motion(grow))
        ms += res.ms
        for i, k in enumerate(grow):
            hl[k]._noted(res, i)
            paths[k], hl[k].status = res.paths[i], int(res.status[i])
        found = [k for k in grow if paths[k] is not None]
        if h0.shortcut > 0 and found:
            res = shortcut_paths(robot, np.stack([hl[k].obstacles for k in found]), [paths[k] for k in found], passes=h0.shortcut, **short, **motion(found))
            ms += res.ms
            for i, k in enumerate(found):
                hl[k]._noted(res, i)
                if res.status[i] != SHORTCUT_OK:
                    raise RuntimeError(f"world {hl[k].world}: edge {int(res.first_bad[i])} of a path the tree planner just proved is not free")
                paths[k] = res.paths[i]
    out = []
    for h, q, la, path in zip(hl, qs, lookaheads, paths):
        h.calls += 1
        h.path = path
        out.append(straight_line_waypoint(q, h.goal, la) if path is None else waypoint_along(path, q, la, h.continuous))
    return out, ms


def hlp_factory(worlds, build, waypoints, batched):
    """What tree_hlps and ws_planner.workspace_hlps return: the factory make(i, world) -> build(i, world i's obstacles padded to the worlds'
    largest count, its goal), with make.hlps (the objects made so far) and, when batched, make.get_waypoints(indices, qs, lookaheads) =
    waypoints(the objects of `indices`, made on demand, qs, lookaheads)[0]; make.last_ms is that call's second result."""
    probs = [p for _, p in worlds]
    obs = [np.asarray(p["obstacles"], dtype=np.float64).reshape(-1, 12) for p in probs]
    O = max([o.shape[0] for o in obs] + [1])
    obstacles = np.stack([pad_obstacles(o, O) for o in obs]) if obs else np.zeros((0, O, 12))
    goals = [np.asarray(p["goal"], dtype=np.float64) for p in probs]
    made = {}

    def make(i, world):
        made[i] = build(i, obstacles[i], goals[i])
        return made[i]

    def get_waypoints(indices, qs, lookaheads):
        hl = [made[int(i)] if int(i) in made else make(int(i), None) for i in indices]
        out, make.last_ms = waypoints(hl, qs, lookaheads)
        return out

    make.hlps = made
    if batched:
        make.get_waypoints = get_waypoints
    return make


def tree_hlps(worlds, robot, seed=0, host=False, batched=True, shortcut=0, mode="new", **plan_options):
    """`worlds` as trials.run_trials takes them ([(name, problem)]) -> the factory (i, world) -> TreeHLP that run_trials(hlp=...) accepts
    (world i's obstacles padded to the worlds' largest count, its goal, the trial's seed).  With batched (the default) the factory also
    carries get_waypoints(indices, qs, lookaheads), which serves ALL live worlds of an iteration with at most three launches -- one
    armour_path_shortcut call for the worlds that hold a path (mode='seed'), ONE armour_tree_plan call for the rest, one
    armour_path_shortcut call for the new paths (shortcut > 0) -- make.last_ms is their sum; the seeds are the per-world objects'
    (call_seed), so the waypoints are the same either way.  shortcut / mode: TreeHLP's.  plan_options go to plan_trees (step, edge_step,
    max_iterations, max_nodes, lb, ub, continuous)."""
    return hlp_factory(worlds, lambda i, obstacles, goal: TreeHLP(robot, obstacles, goal, seed=seed, world=i, host=host, shortcut=shortcut, mode=mode, **plan_options),
                       _waypoints, batched)


def moving_tree_hlps(worlds, robot, velocities, horizon=None, seed=0, host=False, shortcut=0, mode="new", **plan_options):
    """tree_hlps(batched=True) for worlds whose obstacles move: `velocities` is a list of [O_w, 3], one per world (padded with zeros as the
    obstacles are padded with pad_obstacles).  The factory carries set_world_times(t_world [W]), which run_trials(velocities=...) calls
    before every waypoint query and which sets the clock of every object made so far (and of those made later), and
    get_waypoints(indices, qs, lookaheads) as tree_hlps': at most three launches for all live worlds, each world judged by the window rule on
    [t_world[w], t_world[w] + horizon]; make.last_ms is their sum.  horizon=None: the plan's duration (planner.default_params), the span the
    half-space tables of the same iteration cover.  With mode='seed' a kept path is re-validated in the new window at every call and
    dropped for fresh trees once the window blocks it.  The trees only propose waypoints: safety rests on the solver's tables and the moving
    audit.  Zero velocities give tree_hlps' waypoints.  Worlds that have finished keep their last clock."""
    obs = [np.asarray(p["obstacles"], dtype=np.float64).reshape(-1, 12) for _, p in worlds]
    vel = [np.asarray(v, dtype=np.float64).reshape(-1, 3) for v in velocities]
    if len(vel) != len(obs) or any(v.shape[0] != o.shape[0] for v, o in zip(vel, obs)):
        raise ValueError("moving_tree_hlps: one velocity per obstacle of every world")
    O = max([o.shape[0] for o in obs] + [1])
    vel_p = [np.concatenate([v, np.zeros((O - v.shape[0], 3))]) for v in vel]
    if horizon is None:
        from .planner import default_params
        horizon = default_params(1).duration
    state = dict(t_world=np.zeros(len(obs)))

    def build(i, obstacles, goal):
        h = TreeHLP(robot, obstacles, goal, seed=seed, world=i, host=host, shortcut=shortcut, mode=mode, velocity=vel_p[i], horizon=horizon, **plan_options)
        h.set_world_time(state["t_world"][i])
        return h

    make = hlp_factory(worlds, build, _waypoints, True)

    def set_world_times(t_world):
        state["t_world"] = np.array(np.broadcast_to(np.asarray(t_world, dtype=np.float64), (len(obs),)))
        for i, h in make.hlps.items():
            h.set_world_time(state["t_world"][i])

    make.set_world_times = set_world_times
    make.last_ms = 0.0
    return make
