"""Batched tree planner: bidirectional RRT-Connect for W worlds in one launch on the MI355X (include/armour_hip.h, armour_tree_plan).

The reference's experiment scripts plan with a single-query tree planner in 'new' mode (RRT_HLP / RRT_connect_HLP / robot_arm_RRT_HLP, a fresh
tree from where the arm is, every planning iteration).  Here a query needs no graph built beforehand, and all live worlds of a trial are
planned by one call:

    res = plan_trees(robot, obstacles, starts, goals, seeds)     # [W,O,12], [W,n], [W,n], [W] -> status [W], iterations [W], paths [W]
    res.paths[w]                                                 # [P,n] from start to goal (None unless res.status[w] == FOUND)
    hlp = TreeHLP(robot, world_obstacles, goal, seed); q_des = hlp.get_waypoint(q_cur, lookahead)
    out = run_trials(worlds, hlp=tree_hlps(worlds, robot))       # the trees as the trials' high-level planner, one call per iteration

The rule (hash, steer, free prefix, join), its soundness claim and the limits are stated in include/armour_hip.h; DESIGN.md 4.12c.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import _dp, check
from .roadmap import waypoint_along
from .scenes import pad_obstacles, straight_line_waypoint

NOT_FOUND, FOUND, START_BLOCKED, GOAL_BLOCKED, TREE_FULL = (_lib.TREE_NOT_FOUND, _lib.TREE_FOUND, _lib.TREE_START_BLOCKED, _lib.TREE_GOAL_BLOCKED,
                                                            _lib.TREE_FULL)


class TreePlans:
    """What plan_trees returns: status / iterations [W], paths (a list; [P,n] where status == FOUND, else None), ms (device time of the
    launch; 0 on the host), margin [W] (host only, else None: the smallest |clearance| that decided the run), and with trees=True count
    [W,2], nodes [W,2,max_nodes,n], parent [W,2,max_nodes] (rows past count are zero)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def sampling_box(robot, continuous=None):
    """The default sampling box: the robot's position limits, [-pi, pi] on continuous joints."""
    n = robot.num_factors
    cont = np.array([robot.continuous[j] for j in range(n)], dtype=bool) if continuous is None else np.asarray(continuous, dtype=bool).reshape(n)
    lb = np.where(cont, -np.pi, np.array(robot.state_limits_lb[:n]))
    ub = np.where(cont, np.pi, np.array(robot.state_limits_ub[:n]))
    return lb, ub


def plan_trees(robot, obstacles, starts, goals, seeds, lb=None, ub=None, continuous=None, step=0.5, edge_step=0.05, max_iterations=2000, max_nodes=2048,
               trees=False, host=False):
    """obstacles [W,O,12] (or [O,12]: W = 1), starts / goals [W,n], seeds [W] (uint64) -> TreePlans.  lb / ub [n]: the sampling box (default:
    sampling_box).  host=True: the same rule in the library's host loop (no device), which also reports `margin`."""
    L = _lib.load()
    n = robot.num_factors
    obs = np.asarray(obstacles, dtype=np.float64)
    obs = np.ascontiguousarray(obs.reshape((1,) + obs.shape) if obs.ndim == 2 else obs)
    W, O = obs.shape[0], obs.shape[1]
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
    fn = L.armour_tree_plan_host if host else L.armour_tree_plan
    check(fn(C.byref(robot), None if cont is None else cont.ctypes.data_as(u8), _dp(lb), _dp(ub), W, O, _dp(obs) if obs.size else None, _dp(s), _dp(g),
             sd.ctypes.data_as(C.POINTER(C.c_uint64)), float(step), float(edge_step), int(max_iterations), cap, max_points, status.ctypes.data_as(i32),
             iterations.ctypes.data_as(i32), points.ctypes.data_as(i32), _dp(path), count.ctypes.data_as(i32), _dp(nodes) if trees else None,
             parent.ctypes.data_as(i32) if trees else None, _dp(margin) if host else C.byref(ms)))
    paths = [path[w, :points[w]].copy() if status[w] == FOUND else None for w in range(W)]
    out = TreePlans(status=status, iterations=iterations, paths=paths, count=count, nodes=None, parent=None, margin=margin, ms=0.0 if host else ms.value)
    if trees:
        out.nodes, out.parent = nodes, parent
    return out


def call_seed(seed, world, call):
    """The seed of world `world`'s call number `call` (from 0) in a trial: (seed + (world << 32) + call) mod 2^64."""
    return (int(seed) + (int(world) << 32) + int(call)) % (1 << 64)


class TreeHLP:
    """High-level planner that grows a fresh pair of trees from q_cur at every call (the reference's HLP_grow_tree_mode = 'new'):
    get_waypoint(q_cur, lookahead) is one one-world plan_trees call, then the point `lookahead` along the path (roadmap.waypoint_along);
    with no path it falls back to scenes.straight_line_waypoint.  The c-th call uses the seed call_seed(seed, world, c)."""

    def __init__(self, robot, world_obstacles, goal, seed=0, world=0, host=False, **plan_options):
        self.robot, self.goal, self.seed, self.world, self.host = robot, np.asarray(goal, dtype=np.float64), int(seed), int(world), bool(host)
        self.obstacles = np.asarray(world_obstacles, dtype=np.float64).reshape(-1, 12)
        self.options = plan_options
        n = robot.num_factors
        cont = plan_options.get("continuous")
        self.continuous = np.array([robot.continuous[j] for j in range(n)], dtype=bool) if cont is None else np.asarray(cont, dtype=bool)
        self.calls, self.path, self.status, self.margin_min = 0, None, None, np.inf      # margin_min: over the calls so far (host only)

    def _took(self, res, k):
        self.calls += 1
        self.path, self.status = res.paths[k], int(res.status[k])
        if res.margin is not None:
            self.margin_min = min(self.margin_min, float(res.margin[k]))

    def get_waypoint(self, q_cur, lookahead):
        res = plan_trees(self.robot, self.obstacles, [q_cur], [self.goal], [call_seed(self.seed, self.world, self.calls)], host=self.host, **self.options)
        self._took(res, 0)
        if self.path is None:
            return straight_line_waypoint(q_cur, self.goal, lookahead)
        return waypoint_along(self.path, q_cur, lookahead, self.continuous)


def tree_hlps(worlds, robot, seed=0, host=False, batched=True, **plan_options):
    """`worlds` as trials.run_trials takes them ([(name, problem)]) -> the factory (i, world) -> TreeHLP that run_trials(hlp=...) accepts
    (world i's obstacles padded to the worlds' largest count, its goal, the trial's seed).  With batched (the default) the factory also
    carries get_waypoints(indices, qs, lookaheads), which plans ALL live worlds of an iteration with ONE armour_tree_plan call; the seeds are
    the per-world objects' (call_seed), so the waypoints are the same either way.  plan_options go to plan_trees (step, edge_step,
    max_iterations, max_nodes, lb, ub, continuous)."""
    probs = [p for _, p in worlds]
    obs = [np.asarray(p["obstacles"], dtype=np.float64).reshape(-1, 12) for p in probs]
    O = max([o.shape[0] for o in obs] + [1])
    obstacles = np.stack([pad_obstacles(o, O) for o in obs]) if obs else np.zeros((0, O, 12))
    goals = [np.asarray(p["goal"], dtype=np.float64) for p in probs]
    made = {}

    def make(i, world):
        made[i] = TreeHLP(robot, obstacles[i], goals[i], seed=seed, world=i, host=host, **plan_options)
        return made[i]

    def get_waypoints(indices, qs, lookaheads):
        idx = [int(i) for i in indices]
        hl = [made[i] if i in made else make(i, None) for i in idx]
        res = plan_trees(robot, obstacles[idx], np.stack(qs), np.stack([goals[i] for i in idx]), [call_seed(seed, i, h.calls) for i, h in zip(idx, hl)],
                         host=host, **plan_options)
        make.last_ms = res.ms
        out = []
        for k, (h, q, la) in enumerate(zip(hl, qs, lookaheads)):
            h._took(res, k)
            out.append(straight_line_waypoint(q, h.goal, la) if h.path is None else waypoint_along(h.path, q, la, h.continuous))
        return out

    make.hlps = made
    if batched:
        make.get_waypoints = get_waypoints
    return make
