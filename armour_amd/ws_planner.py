"""Batched workspace RRT* and the end-effector high-level planner on the MI355X (include/armour_hip.h, armour_ws_tree_plan).

The reference's experiment scripts plan their waypoints with arm_end_effector_RRT_star_HLP: an RRT* for the end-effector POINT in the 3-D
workspace, the point `lookahead_distance` along its best path, and inverse kinematics from 0.5 (q_cur + goal) to turn that point into a
configuration (the goal configuration when that fails).  Here the trees of all live worlds of a trial grow in one launch and their waypoints
are solved by one armour_ik call:

    res = plan_workspace_trees(obstacles, starts, goals, seeds, lb, ub)    # [W,O,12], [W,3], [W,3], [W] -> status [W], paths [W], path_cost [W]
    res.paths[w]                                                           # [P,3] from start to the best node (None when the start is blocked)
    z_des = waypoint_along_points(res.paths[w], z, 0.1)                    # the point 0.1 m past z's projection on the path
    hlp = WorkspaceTreeHLP(robot, world_obstacles, goal); q_des = hlp.get_waypoint(q_cur, 0.1)
    out = run_trials(worlds, hlp=workspace_hlps(worlds, robot))            # the end-effector planner as the trials' high-level planner
    trees = WorkspaceTrees(obstacles, goals, seeds, lb, ub)                # resident trees: the reference's grow_tree_mode = 'keep'
    res = trees.grow(worlds, starts, 100)                                  # 100 more iterations for the listed worlds -> WorkspacePlans
    out = run_trials(worlds, hlp=workspace_hlps(worlds, robot, mode='keep', max_iterations=100, max_nodes=4096))

Obstacles in linear motion: plan_workspace_trees and ik.solve_ik take velocity, t_from and t_to and then judge every box, and every inverse-
kinematics solution, by the window rule (armour_ws_tree_plan_moving, armour_ik_moving: free at every time of the world's window);
WorkspaceTreeHLP takes a velocity and a horizon and keeps a world clock (set_world_time), and moving_workspace_hlps is workspace_hlps for
run_trials(velocities=...).  The resident trees stay static:

    res = plan_workspace_trees(obstacles, starts, goals, seeds, lb, ub, velocity=vel, t_from=t, t_to=t + horizon)     # vel [W,O,3]
    out = run_trials(worlds, hlp=moving_workspace_hlps(worlds, robot, velocities, mode="seed"), velocities=velocities)

The rule (point and edge tests, samples, parent choice, rewiring, cost re-derivation, best node), its two deliberate departures from the
reference, the soundness arguments and the limits are stated in include/armour_hip.h; DESIGN.md 4.12f, and 4.12g for the resident trees.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import _dp, check
from . import ik
from .scenes import pad_obstacles
from .tree_planner import _motion, call_seed, hlp_factory

PARTIAL, REACHED, START_BLOCKED = _lib.WS_PARTIAL, _lib.WS_REACHED, _lib.WS_START_BLOCKED

# Arm-sized defaults.  The reference's step 0.5 m and rewire distance 1 m are sized for ground vehicles in rooms of tens of metres; an arm's
# workspace is a ball of about 1 m.  The same proportions to the workspace -- a step of a tenth of the reach, a rewire radius of twice the
# step, as 1 m is twice 0.5 m -- give 0.1 m and 0.2 m; goal_tol is one edge_step.  DESIGN.md 4.12f.
STEP, EDGE_STEP, REWIRE_RADIUS, GOAL_RATE, GOAL_TOL = 0.1, 0.01, 0.2, 0.1, 0.01
MAX_ITERATIONS, MAX_NODES = 1000, 1024


class WorkspacePlans(_lib.Result):
    """What plan_workspace_trees returns: status [W] (PARTIAL / REACHED / START_BLOCKED), iterations / rewires / chain_kept / count [W],
    path_cost / goal_dist [W], paths (a list; [P,3] from the start to the best node, None where the start is blocked), ms (device time of
    the launch; 0 on the host), margin [W] (host only, else None: the smallest |clearance| that decided the run), and with trees=True nodes
    [W,max_nodes,3], parent [W,max_nodes], node_cost [W,max_nodes] (rows past count are zero)."""


def workspace_box(robot, tool=None):
    """A default sampling box from the chain's reach: the cube about the base whose half-side is the sum of the links' translation lengths
    (plus |tool|), i.e. a box no end-effector point can leave -> (lb [3], ub [3])."""
    J = robot.num_joints
    trans = np.array(robot.trans[:3 * J], dtype=np.float64).reshape(J, 3)
    reach = float(np.sqrt((trans * trans).sum(1)).sum()) + (0.0 if tool is None else float(np.linalg.norm(np.asarray(tool, dtype=np.float64))))
    return np.full(3, -reach), np.full(3, reach)


def plan_workspace_trees(obstacles, starts, goals, seeds, lb, ub, step=STEP, edge_step=EDGE_STEP, rewire_radius=REWIRE_RADIUS, goal_rate=GOAL_RATE, buffer=0.0,
                         goal_tol=GOAL_TOL, max_iterations=MAX_ITERATIONS, max_nodes=MAX_NODES, init=None, host=False, trees=False, max_points=None, velocity=None,
                         t_from=None, t_to=None):
    """obstacles [W,O,12] (or [O,12]: W = 1), starts / goals [W,3] (points of the workspace), seeds [W] (uint64), lb / ub [3] (the sampling box)
    -> WorkspacePlans.  edge_step and goal_rate default to the reference's (arm_end_effector_RRT_star_HLP.m:5, RRT_star_HLP.m:24); step,
    rewire_radius and goal_tol are arm-sized (see STEP above).  rewire_radius = 0 is plain RRT.  init: None, or W entries, each None or a
    chain [C,3] offered before the loop (the reference's 'seed' mode).  max_points: the path rows to reserve (default: max_nodes, which a
    path cannot exceed).  host=True: the same rule in the library's host loop (no device), which also reports `margin`.
    velocity [W,O,3] with t_from / t_to ([W] or scalars): the obstacles move in a line from their poses `obstacles` of world time 0, and
    every box test is armour_ws_tree_plan_moving's window rule on [t_from[w], t_to[w]]; all three None (the default): the static entry."""
    L = _lib.load()
    obs, W, O = _lib.as_worlds(obstacles)
    motion = _motion("plan_workspace_trees", W, O, velocity, t_from, t_to)
    s = np.ascontiguousarray(np.asarray(starts, dtype=np.float64).reshape(W, 3))
    g = np.ascontiguousarray(np.asarray(goals, dtype=np.float64).reshape(W, 3))
    sd = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (W,)))
    lb = np.ascontiguousarray(lb, dtype=np.float64).reshape(3)
    ub = np.ascontiguousarray(ub, dtype=np.float64).reshape(3)
    cap = int(max_nodes)
    max_points = max(cap, 0) if max_points is None else int(max_points)
    i32 = C.POINTER(C.c_int32)
    chain, chain_count, max_init = None, None, 0
    if init is not None:
        chains = [np.zeros((0, 3)) if c is None else np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in init]
        if len(chains) != W:
            raise ValueError(f"{len(chains)} chains for {W} worlds")
        chain_count = np.array([c.shape[0] for c in chains], dtype=np.int32)
        max_init = max(int(chain_count.max()) if W else 1, 1)
        chain = np.zeros((W, max_init, 3))
        for w, c in enumerate(chains):
            chain[w, :c.shape[0]] = c
    status, iterations, points, rewires, chain_kept, count = (np.zeros(W, dtype=np.int32) for _ in range(6))
    path_cost, goal_dist = np.zeros(W), np.zeros(W)
    path = np.zeros((W, max(max_points, 0), 3))
    rows = max(cap, 0) if trees else 0
    nodes, parent, node_cost = np.zeros((W, rows, 3)), np.zeros((W, rows), dtype=np.int32), np.zeros((W, rows))
    margin = np.zeros(W) if host else None
    ms = C.c_double()
    if motion is None:
        fn, mv = L.armour_ws_tree_plan_host if host else L.armour_ws_tree_plan, ()
    else:
        fn, mv = L.armour_ws_tree_plan_moving_host if host else L.armour_ws_tree_plan_moving, motion[0]
    check(fn(_dp(lb), _dp(ub), W, O, _dp(obs) if obs.size else None, *mv, _dp(s), _dp(g), sd.ctypes.data_as(C.POINTER(C.c_uint64)), max_init, _dp(chain),
             None if chain_count is None else chain_count.ctypes.data_as(i32), float(step), float(edge_step), float(rewire_radius), float(goal_rate), float(buffer),
             float(goal_tol), int(max_iterations), cap, max_points, status.ctypes.data_as(i32), iterations.ctypes.data_as(i32), points.ctypes.data_as(i32),
             rewires.ctypes.data_as(i32), chain_kept.ctypes.data_as(i32), _dp(path_cost), _dp(goal_dist), _dp(path), count.ctypes.data_as(i32),
             _dp(nodes) if trees else None, parent.ctypes.data_as(i32) if trees else None, _dp(node_cost) if trees else None,
             _dp(margin) if host else C.byref(ms)))
    paths = [path[w, :points[w]].copy() if status[w] != START_BLOCKED else None for w in range(W)]
    out = WorkspacePlans(status=status, iterations=iterations, rewires=rewires, chain_kept=chain_kept, count=count, path_cost=path_cost, goal_dist=goal_dist,
                         paths=paths, nodes=None, parent=None, node_cost=None, margin=margin, ms=0.0 if host else ms.value)
    if trees:
        out.nodes, out.parent, out.node_cost = nodes, parent, node_cost
    return out


class WorkspaceTrees:
    """Resident workspace trees (include/armour_hip.h, armour_ws_trees_*): the trees of W worlds with fixed obstacles [W,O,12], goals [W,3],
    seeds [W] and parameters, kept between calls and grown in instalments -- the reference's grow_tree_mode = 'keep'.  After grows of
    n_1, ..., n_k iterations a world's tree, its cumulative iterations / rewires and the last grow's status and path are bit for bit those
    of plan_workspace_trees from the point that planted it with max_iterations = sum n.  host=True: the library's host loop (no device).
      grow(worlds, starts, iterations, margin=False) -> WorkspacePlans, one entry per listed world, in that order
      read(worlds) -> Result(nodes [L,max_nodes,3], parent [L,max_nodes], node_cost [L,max_nodes], count [L]) (rows past count are zero)
      close() frees the handle (also on garbage collection)."""
    handles_created = 0                   # over the process: a batched 'keep' planner makes ONE for all its worlds

    def __init__(self, obstacles, goals, seeds, lb, ub, step=STEP, edge_step=EDGE_STEP, rewire_radius=REWIRE_RADIUS, goal_rate=GOAL_RATE, buffer=0.0,
                 goal_tol=GOAL_TOL, max_nodes=MAX_NODES, host=False):
        self._h = None
        L = _lib.load()
        obs, W, O = _lib.as_worlds(obstacles)
        g = np.ascontiguousarray(np.asarray(goals, dtype=np.float64).reshape(W, 3))
        sd = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (W,)))
        lb = np.ascontiguousarray(lb, dtype=np.float64).reshape(3)
        ub = np.ascontiguousarray(ub, dtype=np.float64).reshape(3)
        self.W, self.O, self.max_nodes, self.host = W, O, int(max_nodes), bool(host)
        h = C.c_void_p()
        fn = L.armour_ws_trees_create_host if host else L.armour_ws_trees_create
        check(fn(_dp(lb), _dp(ub), W, O, _dp(obs) if obs.size else None, _dp(g), sd.ctypes.data_as(C.POINTER(C.c_uint64)), float(step), float(edge_step),
                 float(rewire_radius), float(goal_rate), float(buffer), float(goal_tol), self.max_nodes, C.byref(h)))
        self._h = h
        WorkspaceTrees.handles_created += 1

    def _worlds(self, worlds):
        return np.ascontiguousarray(np.asarray(worlds, dtype=np.int32).reshape(-1))

    def grow(self, worlds, starts, iterations, margin=False, max_points=None):
        """worlds [L] (indices, none twice), starts [L,3] (read only for the worlds whose tree is empty; None when none is), `iterations`
        more iterations for each -> WorkspacePlans (iterations / rewires cumulative; chain_kept zeros; margin [L] of THIS call when asked
        for, host handles only)."""
        wl = self._worlds(worlds)
        n = len(wl)
        s = None if starts is None else np.ascontiguousarray(np.asarray(starts, dtype=np.float64).reshape(n, 3))
        max_points = self.max_nodes if max_points is None else int(max_points)
        i32 = C.POINTER(C.c_int32)
        status, iterations_done, points, rewires, count = (np.zeros(n, dtype=np.int32) for _ in range(5))
        path_cost, goal_dist = np.zeros(n), np.zeros(n)
        path = np.zeros((n, max(max_points, 0), 3))
        mg = np.zeros(n) if margin else None
        ms = C.c_double()
        check(_lib.load().armour_ws_trees_grow(self._h, n, wl.ctypes.data_as(i32), _dp(s), int(iterations), max_points, status.ctypes.data_as(i32),
                                              iterations_done.ctypes.data_as(i32), points.ctypes.data_as(i32), rewires.ctypes.data_as(i32), _dp(path_cost),
                                              _dp(goal_dist), _dp(path), count.ctypes.data_as(i32), C.byref(ms), _dp(mg)))
        paths = [path[k, :points[k]].copy() if status[k] != START_BLOCKED else None for k in range(n)]
        return WorkspacePlans(status=status, iterations=iterations_done, rewires=rewires, chain_kept=np.zeros(n, dtype=np.int32), count=count, path_cost=path_cost,
                              goal_dist=goal_dist, paths=paths, nodes=None, parent=None, node_cost=None, margin=mg, ms=ms.value)

    def read(self, worlds):
        wl = self._worlds(worlds)
        n = len(wl)
        i32 = C.POINTER(C.c_int32)
        nodes, parent, node_cost = np.zeros((n, self.max_nodes, 3)), np.zeros((n, self.max_nodes), dtype=np.int32), np.zeros((n, self.max_nodes))
        count = np.zeros(n, dtype=np.int32)
        check(_lib.load().armour_ws_trees_read(self._h, n, wl.ctypes.data_as(i32), _dp(nodes), parent.ctypes.data_as(i32), _dp(node_cost), count.ctypes.data_as(i32)))
        return _lib.Result(nodes=nodes, parent=parent, node_cost=node_cost, count=count)

    def close(self):
        if self._h is not None:
            _lib.load().armour_ws_trees_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _project(path, z):
    """(segment, t, distance along the path) of the point of the polyline nearest to z; the first segment on a tie."""
    best, along = None, 0.0
    for k in range(len(path) - 1):
        a, d = path[k], path[k + 1] - path[k]
        dd = float(d @ d)
        t = 0.0 if dd == 0.0 else min(max(float((z - a) @ d) / dd, 0.0), 1.0)
        e = z - (a + t * d)
        dist2, seg = float(e @ e), float(np.sqrt(dd))
        if best is None or dist2 < best[0]:
            best = (dist2, k, t, along + t * seg)
        along += seg
    return best[1:]


def waypoint_along_points(path, z, lookahead):
    """The point `lookahead` metres past the projection of z on the polyline path [P,3] (RRT_HLP.m:341-359: the agent's distance along the
    best path, plus the lookahead, clipped to the path's length, interpolated on the path); the last point when the path ends sooner.
    Host only."""
    path = np.asarray(path, dtype=np.float64).reshape(-1, 3)
    z = np.asarray(z, dtype=np.float64).reshape(3)
    if path.shape[0] == 1:
        return path[0].copy()
    _, _, d = _project(path, z)
    target, along = d + float(lookahead), 0.0
    for k in range(path.shape[0] - 1):
        seg = float(np.linalg.norm(path[k + 1] - path[k]))
        if seg > 0.0 and target <= along + seg:
            return path[k] + ((target - along) / seg) * (path[k + 1] - path[k])
        along += seg
    return path[-1].copy()


class WorkspaceTreeHLP:
    """The reference's arm_end_effector_RRT_star_HLP for one world: get_waypoint(q_cur, lookahead) grows a workspace tree from the end
    effector of q_cur towards the end effector of the goal configuration, takes the point `lookahead` METRES along its path and returns
    the configuration that inverse kinematics finds for it (q_ref = 0.5 (q_cur + goal) with ik_reference='mid', q_cur with 'current'),
    judged free in this world; the goal configuration when no free solution is found (the reference's fall-back) or the start is blocked.
    The c-th call uses the seed call_seed(seed, world, c) for the tree and for the inverse kinematics.
      mode='new' (the default; the reference's grow_tree_mode = 'new'): a fresh tree at every call.
      mode='seed': [the current point] + the rest of the last path, from the vertex after the one nearest to the current point, is offered
        as the initial chain.
      mode='keep' (the reference's grow_tree_mode = 'keep', the mode of its hard scenarios): the tree planted at the first call stays in a
        WorkspaceTrees handle and every call grows it by max_iterations more iterations (the tree's seed is call_seed(seed, world, 0), fixed;
        max_nodes bounds the tree over ALL calls); the waypoint is taken on the tree's current best path from the projection of the current
        point, as ever.  A call whose start is blocked while the tree is empty falls back to the goal and the next call plants from the
        new point.  The object does not own its tree: `trees` is the WorkspaceTrees that holds it (or a callable that returns it, called
        at the first waypoint) and `slot` this world's index there -- made from this world's padded obstacles, goal POINT and
        call_seed(seed, world, 0), as workspace_hlps does for all its worlds at once; whoever made the handle closes it.  mode='keep'
        without `trees` is a ValueError.
    velocity [O,3] (default None: a static world, today's calls): the obstacles move in a line from their poses `world_obstacles` of world
      time 0.  Both launches of a call -- the tree (with its 'seed' chain) and the inverse kinematics -- then judge by the window rule on
      [t, t + horizon], t the world time of the last set_world_time (0 before the first) and horizon the plan's duration unless given.  With
      mode='seed' the chain ends at its first edge that the new window blocks.  A waypoint without a solution free over the window falls
      back to the goal configuration.  mode='keep' with a velocity is a ValueError: the resident trees stay static.
    plan_options go to plan_workspace_trees (step, edge_step, rewire_radius, goal_rate, buffer, goal_tol, max_iterations, max_nodes; lb /
    ub default to workspace_box); ik_options go to ik.solve_ik (S, lam, e_max, tol, max_iterations, tool)."""

    def __init__(self, robot, world_obstacles, goal, seed=0, world=0, host=False, mode="new", ik_reference="mid", ik_options=None, trees=None, slot=0,
                 velocity=None, horizon=None, **plan_options):
        if mode not in ("new", "seed", "keep") or ik_reference not in ("mid", "current"):
            raise ValueError(f"mode = {mode!r} ('new', 'seed' or 'keep'), ik_reference = {ik_reference!r} ('mid' or 'current')")
        if velocity is None and horizon is not None:
            raise ValueError("horizon belongs to a moving world: give a velocity")
        if mode == "keep" and velocity is not None:
            raise ValueError("mode = 'keep' is for static worlds: a kept tree's edges were proved against windows that have passed")
        if (mode == "keep") != (trees is not None):
            raise ValueError("mode = 'keep' takes the WorkspaceTrees that holds this world's tree (trees=, slot=), and no other mode does")
        self.robot, self.goal, self.seed, self.world, self.host = robot, np.asarray(goal, dtype=np.float64), int(seed), int(world), bool(host)
        self.mode, self.ik_reference = mode, ik_reference
        self.obstacles = np.asarray(world_obstacles, dtype=np.float64).reshape(-1, 12)
        self.velocity, self.horizon, self.t_world = None, None, 0.0
        if velocity is not None:
            self.velocity = np.asarray(velocity, dtype=np.float64).reshape(-1, 3)
            if self.velocity.shape[0] != self.obstacles.shape[0]:
                raise ValueError("WorkspaceTreeHLP: one velocity per obstacle")
            if horizon is None:
                from .planner import default_params
                horizon = default_params(1).duration
            self.horizon = float(horizon)
            if not self.horizon >= 0.0:
                raise ValueError(f"horizon = {horizon} (>= 0)")
        self.ik_options = dict(ik_options or {})
        self.options = dict(plan_options)
        lb, ub = workspace_box(robot, self.ik_options.get("tool"))
        self.options.setdefault("lb", lb)
        self.options.setdefault("ub", ub)
        self.goal_point = ik.end_effector(robot, self.goal, self.ik_options.get("tool"))
        self.calls, self.path, self.status, self.ik_status, self.waypoint, self.margin_min = 0, None, None, None, None, np.inf
        self.fallbacks = 0                 # calls that returned the goal configuration
        self.trees, self.slot, self.count = trees, int(slot), 0      # 'keep': the handle (a callable: made at the first call), this world's index in it, the tree's nodes

    def _handle(self):
        """'keep': the handle that holds this world's tree"""
        if callable(self.trees):
            self.trees = self.trees()
        return self.trees

    def set_world_time(self, t):
        """The world time at which the next call plans (a moving world): its window is [t, t + horizon]."""
        if self.velocity is None:
            raise ValueError("set_world_time belongs to a moving world: give a velocity")
        self.t_world = float(t)

    def get_waypoint(self, q_cur, lookahead):
        return _waypoints([self], [q_cur], [lookahead])[0][0]


def keep_trees(obstacles, goal_points, seeds, host, options):
    """The WorkspaceTrees of a 'keep' planner from its plan options (max_iterations is a grow's, not the handle's)"""
    o = {k: v for k, v in options.items() if k != "max_iterations"}
    return WorkspaceTrees(obstacles, np.stack(goal_points), np.array(seeds, dtype=np.uint64), host=host, **o)


def _grow_kept(hl, z):
    """One instalment for each of the 'keep' HLPs `hl` from the points z: ONE armour_ws_trees_grow call per handle (the batched factory's
    worlds share one) -> a WorkspacePlans in hl's order"""
    iterations = hl[0].options.get("max_iterations", MAX_ITERATIONS)
    groups = {}
    for k, h in enumerate(hl):
        groups.setdefault(id(h._handle()), []).append(k)
    parts, ms = {}, 0.0
    for ks in groups.values():
        trees = hl[ks[0]].trees
        res = trees.grow([hl[k].slot for k in ks], z[ks], iterations, margin=trees.host)
        ms += res.ms
        for j, k in enumerate(ks):
            parts[k] = (res, j)
            hl[k].count = int(res.count[j])
    pick = lambda name: np.array([getattr(parts[k][0], name)[parts[k][1]] for k in range(len(hl))])
    return WorkspacePlans(status=pick("status"), iterations=pick("iterations"), rewires=pick("rewires"), chain_kept=pick("chain_kept"), count=pick("count"),
                          path_cost=pick("path_cost"), goal_dist=pick("goal_dist"), paths=[parts[k][0].paths[parts[k][1]] for k in range(len(hl))], nodes=None,
                          parent=None, node_cost=None, margin=pick("margin") if hl[0].host else None, ms=ms)


def _chain(h, z):
    if h.mode != "seed" or h.path is None:
        return None
    k = int(np.argmin(((h.path - z) ** 2).sum(1)))
    return np.vstack([z[None], h.path[k + 1:]])


def _waypoints(hl, qs, lookaheads):
    """One call of each of the HLPs `hl` (one robot, one obstacle count, the same options) from qs: ONE armour_ws_tree_plan call (mode 'keep': one
    armour_ws_trees_grow call on the shared handle) and ONE armour_ik call -> (waypoint configurations, the launches' ms).  Moving worlds (all
    or none of hl): both launches get the window [t_world, t_world + horizon] of each world."""
    h0 = hl[0]
    robot, host = h0.robot, h0.host
    if any((h.velocity is None) != (h0.velocity is None) for h in hl):
        raise ValueError("static and moving worlds cannot share a launch")
    motion = {}
    if h0.velocity is not None:
        t = np.array([h.t_world for h in hl])
        motion = dict(velocity=np.stack([h.velocity for h in hl]), t_from=t, t_to=t + np.array([h.horizon for h in hl]))
    qs = np.stack([np.asarray(q, dtype=np.float64) for q in qs])
    obstacles = np.stack([h.obstacles for h in hl])
    z = ik.end_effector(robot, qs, h0.ik_options.get("tool")).reshape(-1, 3)
    seeds = np.array([call_seed(h.seed, h.world, h.calls) for h in hl], dtype=np.uint64)
    if h0.mode == "keep":
        res = _grow_kept(hl, z)
    else:
        chains = [_chain(h, z[k]) for k, h in enumerate(hl)]
        res = plan_workspace_trees(obstacles, z, np.stack([h.goal_point for h in hl]), seeds, init=chains if any(c is not None for c in chains) else None,
                                   host=host, **h0.options, **motion)
    points = np.stack([z[k] if p is None else waypoint_along_points(p, z[k], la) for k, (p, la) in enumerate(zip(res.paths, lookaheads))])
    goals = np.stack([h.goal for h in hl])
    sol = ik.solve_ik(robot, points, 0.5 * (qs + goals) if h0.ik_reference == "mid" else qs, obstacles, np.arange(len(hl)), seeds, host=host, **h0.ik_options, **motion)
    out = []
    for k, h in enumerate(hl):
        found = res.paths[k] is not None and sol.status[k] == ik.FOUND
        h.calls += 1
        h.path, h.status, h.ik_status, h.waypoint = res.paths[k], int(res.status[k]), int(sol.status[k]), points[k]
        h.fallbacks += 0 if found else 1
        if res.margin is not None:
            h.margin_min = min(h.margin_min, float(res.margin[k]))
        out.append(sol.q[k].copy() if found else h.goal.copy())
    return out, res.ms + sol.ms


def workspace_hlps(worlds, robot, seed=0, lookahead=0.1, mode="new", ik_reference="mid", host=False, batched=True, ik_options=None, **options):
    """`worlds` as trials.run_trials takes them ([(name, problem)]) -> the factory (i, world) -> WorkspaceTreeHLP that run_trials(hlp=...)
    accepts (world i's obstacles padded to the worlds' largest count, its goal configuration, the trial's seed).  With batched (the default)
    the factory carries get_waypoints(indices, qs, lookaheads), which serves ALL live worlds of an iteration with ONE armour_ws_tree_plan call and ONE armour_ik
    call (make.last_ms is their device time): the end-effector points of qs (ik.end_effector), the trees, the workspace waypoints, then
    solve_ik(targets = the waypoints, q_ref = 0.5 (q_cur + goal) | q_cur, world = the target's world); a target that is not IK_FOUND yields
    the goal configuration.  The seeds are the per-world objects' (tree_planner.call_seed), so the waypoints are the same either way.
    lookahead is in METRES of end-effector travel (default: the reference scripts' 0.1): the trials' own `lookahead` values are distances in
    joint space and are ignored, per world and batched alike.  mode / ik_reference / ik_options / options: WorkspaceTreeHLP's."""
    lookahead = float(lookahead)

    class _Metres(WorkspaceTreeHLP):
        def get_waypoint(self, q_cur, _joint_space_lookahead):
            return _waypoints([self], [q_cur], [lookahead])[0][0]

    # mode='keep': the factory owns the trees.  Batched: ONE WorkspaceTrees for all the worlds (world i is its tree i), made at the first call
    # and grown on the live worlds alone; per world: a one-world handle each, made at that world's first call.  make.close() frees them.
    shared = {}

    def handle(key, indices):
        if key not in shared:
            lb, ub = workspace_box(robot, (ik_options or {}).get("tool"))
            o = dict(options)
            o.setdefault("lb", lb)
            o.setdefault("ub", ub)
            probs = [p for _, p in worlds]
            O = max([np.asarray(p["obstacles"]).reshape(-1, 12).shape[0] for p in probs] + [1])
            obstacles = np.stack([pad_obstacles(np.asarray(probs[i]["obstacles"], dtype=np.float64).reshape(-1, 12), O) for i in indices])
            points = [ik.end_effector(robot, np.asarray(probs[i]["goal"], dtype=np.float64), (ik_options or {}).get("tool")) for i in indices]
            shared[key] = keep_trees(obstacles, points, [call_seed(seed, i, 0) for i in indices], host, o)
        return shared[key]

    def keep(i):
        if mode != "keep":
            return {}
        return dict(trees=lambda: handle("trees", range(len(worlds))), slot=i) if batched else dict(trees=lambda: handle(i, [i]), slot=0)

    make = hlp_factory(worlds, lambda i, obstacles, goal: _Metres(robot, obstacles, goal, seed=seed, world=i, host=host, mode=mode, ik_reference=ik_reference,
                                                                  ik_options=ik_options, **keep(i), **options),
                       lambda hl, qs, _joint_space_lookaheads: _waypoints(hl, qs, [lookahead] * len(hl)), batched)
    make.shared = shared                  # 'keep': {'trees': the one handle} (batched) or {world: its handle}, once called

    def close():
        for t in shared.values():
            t.close()
        shared.clear()

    make.close = close
    return make


def moving_workspace_hlps(worlds, robot, velocities, horizon=None, seed=0, lookahead=0.1, mode="new", ik_reference="mid", host=False, ik_options=None, **options):
    """workspace_hlps(batched=True) for worlds whose obstacles move: `velocities` is a list of [O_w, 3], one per world (padded with zeros as the
    obstacles are padded with pad_obstacles).  The factory carries set_world_times(t_world [W]), which run_trials(velocities=...) calls
    before every waypoint query and which sets the clock of every object made so far (and of those made later), and
    get_waypoints(indices, qs, lookaheads) as workspace_hlps': ONE armour_ws_tree_plan_moving call and ONE armour_ik_moving call for all live
    worlds, each world judged by the window rule on [t_world[w], t_world[w] + horizon]; make.last_ms is their sum.  horizon=None: the plan's
    duration (planner.default_params).  mode: 'new' or 'seed' ('keep' is a ValueError: the resident trees stay static).  The planner only
    proposes waypoints: safety rests on the solver's tables and the moving audit.  Zero velocities give workspace_hlps' waypoints.  Worlds
    that have finished keep their last clock."""
    obs = [np.asarray(p["obstacles"], dtype=np.float64).reshape(-1, 12) for _, p in worlds]
    vel = [np.asarray(v, dtype=np.float64).reshape(-1, 3) for v in velocities]
    if len(vel) != len(obs) or any(v.shape[0] != o.shape[0] for v, o in zip(vel, obs)):
        raise ValueError("moving_workspace_hlps: one velocity per obstacle of every world")
    if mode == "keep":
        raise ValueError("mode = 'keep' is for static worlds: a kept tree's edges were proved against windows that have passed")
    O = max([o.shape[0] for o in obs] + [1])
    vel_p = [np.concatenate([v, np.zeros((O - v.shape[0], 3))]) for v in vel]
    if horizon is None:
        from .planner import default_params
        horizon = default_params(1).duration
    lookahead = float(lookahead)
    state = dict(t_world=np.zeros(len(obs)))

    def build(i, obstacles, goal):
        h = WorkspaceTreeHLP(robot, obstacles, goal, seed=seed, world=i, host=host, mode=mode, ik_reference=ik_reference, ik_options=ik_options,
                             velocity=vel_p[i], horizon=horizon, **options)
        h.set_world_time(state["t_world"][i])
        return h

    make = hlp_factory(worlds, build, lambda hl, qs, _joint_space_lookaheads: _waypoints(hl, qs, [lookahead] * len(hl)), True)

    def set_world_times(t_world):
        state["t_world"] = np.array(np.broadcast_to(np.asarray(t_world, dtype=np.float64), (len(obs),)))
        for i, h in make.hlps.items():
            h.set_world_time(state["t_world"][i])

    make.set_world_times = set_world_times
    make.last_ms = 0.0
    return make
