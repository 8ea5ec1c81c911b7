"""Roadmap high-level planner: a joint-space roadmap checked against worlds' obstacles on the MI355X (include/armour_hip.h,
armour_roadmap_*), and waypoints through its free graph.

The reference ships this as a prebuilt CUDA binary without source (kinova_samplebased_HLP_realtime/collision_checker: a roadmap of joint
configurations + an adjacency list in, node feasibility / link_c / the collision-free adjacency out, then a graph search in MATLAB).  Here:

    rm = Roadmap(robot, *uniform_roadmap(20000, 0.3, 16, seed=0, lb=lb, ub=ub, continuous=cont), continuous=cont)
    v = rm.check(obstacles)                 # [W,O,12] -> node_free [W,N], edge_free [W,E] (+ node_clearance), one launch
    path = rm.plan(w, q_start, q_goal)      # host A* over world w's free graph, [P,n] (None: no path)
    hlp = RoadmapHLP(rm, goal); q_des = hlp.get_waypoint(q_cur, lookahead)
    f = rm.field(goals)                     # [W,n] -> every world's cost-to-go cost [W,N] and successors next [W,N], one launch
    path, length = rm.descend(w, q_start)   # host, no search: nearest nodes + the successor pointers
    res = run_trials(worlds, hlp=field_hlps(rm, worlds))    # the roadmap as the trials' high-level planner
    index, dist, count = rm.knn(queries, k=8)               # [Q,n] -> each query's k nearest nodes in the order (distance, index), one call
    rm = Roadmap(robot, *device_roadmap(robot, 200000, 0.3, 16, 0, lb, ub, cont), continuous=cont)    # the edges by that search
    paths = rm.descend_many(worlds, starts)                 # descend() for Q queries with one device call
    v = rm.check_moving(obstacles, velocity, t_from, t_to)  # check() against obstacles in linear motion over a time window per world
    res = run_trials(worlds, hlp=moving_field_hlps(rm, worlds, velocities), velocities=velocities)   # whole trials in moving worlds

The node and edge rules (exact node test, conservative edge test with enlarged boxes) are stated in include/armour_hip.h and DESIGN.md.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import _dp, check
from .scenes import angdiff, pad_obstacles, straight_line_waypoint

NEXT_GOAL = -2          # ARMOUR_ROADMAP_NEXT_GOAL: the successor of a node that is joined to the goal itself


def wrapped_diff(a, b, continuous):
    """b - a, wrapped to [-pi, pi) on continuous joints (the library's formula: d - 2 pi floor((d + pi) / (2 pi)))."""
    d = np.asarray(b, dtype=np.float64) - np.asarray(a, dtype=np.float64)
    w = d - 2 * np.pi * np.floor((d + np.pi) / (2 * np.pi))
    return np.where(np.asarray(continuous, dtype=bool), w, d)


def uniform_roadmap(N, radius, k_max, seed, lb, ub, continuous):
    """N seeded uniform samples within [lb, ub] ([-pi, pi] on continuous joints) and the edges to neighbours within `radius` by wrapped
    joint distance: every node proposes its k_max nearest such neighbours and the edge set is the union of the proposals (so a node can
    end up with more than k_max edges).  Returns (nodes [N,n], edges [E,2] int32 with i < j, sorted).  The analogue of the reference's
    joint_positions_uniform_hardware_dense_rand.csv / adj_matrix_..._range0p3.txt."""
    cont = np.asarray(continuous, dtype=bool)
    lo = np.where(cont, -np.pi, np.asarray(lb, dtype=np.float64))
    hi = np.where(cont, np.pi, np.asarray(ub, dtype=np.float64))
    rng = np.random.default_rng(seed)
    nodes = lo + (hi - lo) * rng.random((int(N), cont.size))
    pairs = []
    chunk = max(1, 4_000_000 // max(1, int(N)))
    for i0 in range(0, int(N), chunk):
        blk = nodes[i0:i0 + chunk]
        d = wrapped_diff(blk[:, None, :], nodes[None, :, :], cont)
        dist = np.sqrt((d * d).sum(-1))
        dist[np.arange(blk.shape[0]), i0 + np.arange(blk.shape[0])] = np.inf
        k = min(int(k_max), int(N) - 1)
        if k <= 0:
            break
        near = np.argpartition(dist, k - 1, axis=1)[:, :k] if k < int(N) else np.argsort(dist, axis=1)
        rows = np.repeat(np.arange(i0, i0 + blk.shape[0]), near.shape[1])
        cols = near.ravel()
        keep = dist[rows - i0, cols] <= radius
        pairs.append(np.stack([rows[keep], cols[keep]], axis=1))
    if not pairs:
        return nodes, np.zeros((0, 2), dtype=np.int32)
    e = np.sort(np.concatenate(pairs), axis=1)
    e = np.unique(e, axis=0)
    return nodes, np.ascontiguousarray(e, dtype=np.int32)


class Roadmap:
    """A roadmap on one device: nodes [N,n], edges [E,2], the edge rule's step (radians per sub-segment)."""

    def __init__(self, robot, nodes, edges, continuous=None, edge_step=0.05, device=0, host=False):
        """host=True: a handle that holds nothing on a device (armour_roadmap_create_host); it serves knn(host=True), check_moving(host=True)
        and plan() after that check, and nothing else."""
        self.L = _lib.load()
        self.robot = robot
        self.n = robot.num_factors
        self.nodes = np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1, self.n)
        self.edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
        self.continuous = np.array([robot.continuous[j] for j in range(self.n)], dtype=np.uint8) if continuous is None \
            else np.ascontiguousarray(continuous, dtype=np.uint8).reshape(self.n)
        self.edge_step = float(edge_step)
        h = C.c_void_p()
        args = (C.byref(robot), self.nodes.shape[0], _dp(self.nodes), self.edges.shape[0], self.edges.ctypes.data_as(C.POINTER(C.c_int32)),
                self.continuous.ctypes.data_as(C.POINTER(C.c_uint8)), self.edge_step)
        check(self.L.armour_roadmap_create_host(*args, C.byref(h)) if host else self.L.armour_roadmap_create(*args, device, C.byref(h)))
        self.h = h
        N, E, M = C.c_int32(), C.c_int32(), C.c_int64()
        check(self.L.armour_roadmap_get_sizes(self.h, C.byref(N), C.byref(E), C.byref(M)))
        self.N, self.E, self.edge_samples = N.value, E.value, M.value
        self.W = None           # the worlds of the last successful check (None: none yet)

    def close(self):
        if getattr(self, "h", None):
            self.L.armour_roadmap_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, obstacles, clearance=False):
        """obstacles [W,O,12] (or [O,12]: W = 1) -> dict node_free [W,N] bool, edge_free [W,E] bool, ms (device time of the launch),
        and node_clearance [W,N] when `clearance`."""
        obs, W, O = _lib.as_worlds(obstacles)
        nf = np.zeros((W, self.N), dtype=np.uint8)
        ef = np.zeros((W, self.E), dtype=np.uint8)
        cl = np.zeros((W, self.N)) if clearance else None
        ms = C.c_double()
        u8 = C.POINTER(C.c_uint8)
        check(self.L.armour_roadmap_check(self.h, W, O, _dp(obs) if obs.size else None, nf.ctypes.data_as(u8), ef.ctypes.data_as(u8),
                                          _dp(cl) if clearance else None, C.byref(ms)))
        self.W = W              # (a check that fails after its arguments passed leaves the library without worlds: field() is ESTATE)
        out = dict(node_free=nf.astype(bool), edge_free=ef.astype(bool), ms=ms.value)
        if clearance:
            out["node_clearance"] = cl
        return out

    def check_moving(self, obstacles, velocity, t_from, t_to, clearance=False, host=False):
        """check() over a time window per world against obstacles in linear motion (armour_roadmap_check_moving): obstacles [W,O,12] (or
        [O,12]) are the poses at world time 0, velocity [W,O,3] (or [O,3]) the constant velocities, t_from / t_to [W] (or scalars, for every
        world) the windows in world time.  Returns the dict check() returns (ms = 0 on the host).  Until the next check, plan / descend /
        connect_many / descend_many join points to the roadmap by the window rule.  host=True: the library's host loop, on a Roadmap(host=True)."""
        obs, W, O = _lib.as_worlds(obstacles)
        vel = np.ascontiguousarray(np.asarray(velocity, dtype=np.float64).reshape(W, O, 3))
        t0 = np.ascontiguousarray(np.broadcast_to(np.asarray(t_from, dtype=np.float64), (W,)))
        t1 = np.ascontiguousarray(np.broadcast_to(np.asarray(t_to, dtype=np.float64), (W,)))
        nf = np.zeros((W, self.N), dtype=np.uint8)
        ef = np.zeros((W, self.E), dtype=np.uint8)
        cl = np.zeros((W, self.N)) if clearance else None
        ms = C.c_double(0.0)
        u8 = C.POINTER(C.c_uint8)
        args = (self.h, W, O, _dp(obs) if obs.size else None, _dp(vel) if vel.size else None, _dp(t0), _dp(t1), nf.ctypes.data_as(u8), ef.ctypes.data_as(u8),
                _dp(cl) if clearance else None)
        check(self.L.armour_roadmap_check_moving_host(*args) if host else self.L.armour_roadmap_check_moving(*args, C.byref(ms)))
        self.W = W
        out = dict(node_free=nf.astype(bool), edge_free=ef.astype(bool), ms=ms.value)
        if clearance:
            out["node_clearance"] = cl
        return out

    def check_self(self, pairs=None, shrink=None, clearance=False):
        """The roadmap's self-collision masks (world-independent; once per roadmap): dict node_free [N] bool, edge_free [E] bool, ms, and
        node_clearance [N] when `clearance`.  pairs / shrink [J,J] as armour_amd.self_check.check takes them.  The handle keeps the masks."""
        from .self_check import table_args
        pairs, shrink, pp, sp = table_args(self.robot, pairs, shrink)
        nf = np.zeros(self.N, dtype=np.uint8)
        ef = np.zeros(self.E, dtype=np.uint8)
        cl = np.zeros(self.N) if clearance else None
        ms = C.c_double()
        u8 = C.POINTER(C.c_uint8)
        check(self.L.armour_roadmap_check_self(self.h, pp, sp, nf.ctypes.data_as(u8), ef.ctypes.data_as(u8), _dp(cl) if clearance else None, C.byref(ms)))
        out = dict(node_free=nf.astype(bool), edge_free=ef.astype(bool), ms=ms.value)
        if clearance:
            out["node_clearance"] = cl
        return out

    def use_self(self, on=True):
        """on: plan() takes a node or edge as free only if it is free in the world's mask and the self mask, and checks the edges that join
        start and goal with the self edge rule too (an error before check_self).  Default off: plan() is unchanged."""
        check(self.L.armour_roadmap_use_self(self.h, 1 if on else 0))
        return self

    def plan(self, w, start, goal, connect_k=8, max_points=None):
        """Path [P,n] from start to goal through world w's free graph of the last check (start and goal included), None if none."""
        s = np.ascontiguousarray(start, dtype=np.float64).reshape(self.n)
        g = np.ascontiguousarray(goal, dtype=np.float64).reshape(self.n)
        cap = self.N + 2 if max_points is None else int(max_points)
        path = np.zeros((cap, self.n))
        pts = C.c_int32()
        check(self.L.armour_roadmap_plan(self.h, int(w), _dp(s), _dp(g), int(connect_k), cap, _dp(path), C.byref(pts)))
        return path[:pts.value].copy() if pts.value else None

    def field(self, goals, connect_k=8):
        """goals [W,n], one per world of the last check ([n] when that check had one world) -> dict cost [W,N] (shortest free-graph distance
        to the goal, inf where there is none), next [W,N] (successor node, NEXT_GOAL at a node joined to the goal, -1 unreachable),
        reached [W], sweeps [W], ms (device time of the launch).  The library takes W from the last check, so any other number of goals is
        a ValueError here.  The handle keeps the field for descend() until the next check / check_self / use_self."""
        g = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, self.n)
        W = g.shape[0]
        if self.W is None:      # no check to take W from: the library says so (ESTATE) before it reads or writes anything
            check(self.L.armour_roadmap_field(self.h, None, int(connect_k), None, None, None, None, None))
            raise RuntimeError("armour_roadmap_field accepted a roadmap without a check")
        if W != self.W:
            raise ValueError(f"Roadmap.field: {W} goals for the {self.W} worlds of the last check")
        cost = np.zeros((W, self.N))
        nxt = np.zeros((W, self.N), dtype=np.int32)
        reached, sweeps = np.zeros(W, dtype=np.int32), np.zeros(W, dtype=np.int32)
        ms = C.c_double()
        i32 = C.POINTER(C.c_int32)
        check(self.L.armour_roadmap_field(self.h, _dp(g) if g.size else None, int(connect_k), _dp(cost), nxt.ctypes.data_as(i32),
                                          reached.ctypes.data_as(i32), sweeps.ctypes.data_as(i32), C.byref(ms)))
        self.field_goals = g.copy()
        return dict(cost=cost, next=nxt, reached=reached, sweeps=sweeps, ms=ms.value)

    def descend(self, w, start, connect_k=8, max_points=None):
        """(path [P,n] from start to world w's goal of the last field(), its length) by the field's successors; (None, inf) if none."""
        s = np.ascontiguousarray(start, dtype=np.float64).reshape(self.n)
        cap = self.N + 2 if max_points is None else int(max_points)
        path = np.zeros((cap, self.n))
        pts, length = C.c_int32(), C.c_double()
        check(self.L.armour_roadmap_descend(self.h, int(w), _dp(s), int(connect_k), cap, _dp(path), C.byref(pts), C.byref(length)))
        return (path[:pts.value].copy() if pts.value else None), length.value


    def knn(self, queries, k, radius=np.inf, worlds=None, exclude=None, host=False):
        """queries [Q,n] -> (index [Q,k] int32, dist [Q,k], count [Q]): each query's first k candidates in the order (wrapped distance, node
        index); the slots past count[i] hold -1 / inf.  Candidates: nodes within `radius`, other than node exclude[i] (exclude [Q], -1: none),
        and free in world worlds[i] of the last check ([Q]; -1 or worlds=None: every node; with use_self on, free in the self mask too).
        host=True: the same rule in the library's host loop.  The rule is stated in include/armour_hip.h."""
        q = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, self.n)
        Q, k = q.shape[0], int(k)
        i32 = C.POINTER(C.c_int32)
        opt = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.int32), (Q,)))
        w, ex = opt(worlds), opt(exclude)
        slots = max(k, 0)
        index, dist, count = np.full((Q, slots), -1, dtype=np.int32), np.full((Q, slots), np.inf), np.zeros(Q, dtype=np.int32)
        ms = C.c_double()
        fn = self.L.armour_roadmap_knn_host if host else self.L.armour_roadmap_knn
        check(fn(self.h, Q, _dp(q), None if w is None else w.ctypes.data_as(i32), None if ex is None else ex.ctypes.data_as(i32), k, float(radius),
                 index.ctypes.data_as(i32), _dp(dist), count.ctypes.data_as(i32), C.byref(ms)))
        self.knn_ms = ms.value
        return index, dist, count

    def connect_many(self, worlds, starts, targets=None, connect_k=8):
        """starts [Q,n] in the worlds `worlds` [Q] of the last check -> dict node [Q,connect_k] (each start's nearest free nodes, -1 padded),
        dist [Q,connect_k], edge_ok [Q,connect_k] bool (the edge start -> node is free by the edge rule), count [Q], ms, and with targets
        [Q,n] direct [Q] bool (the edge start -> target is free): what plan / field / descend compute to join a point, for Q points in one
        device call."""
        q = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, self.n)
        Q, k = q.shape[0], int(connect_k)
        w = np.ascontiguousarray(np.broadcast_to(np.asarray(worlds, dtype=np.int32), (Q,)))
        tg = None if targets is None else np.ascontiguousarray(targets, dtype=np.float64).reshape(Q, self.n)
        slots = max(k, 0)
        node, dist = np.full((Q, slots), -1, dtype=np.int32), np.full((Q, slots), np.inf)
        ok, count, direct = np.zeros((Q, slots), dtype=np.uint8), np.zeros(Q, dtype=np.int32), np.zeros(Q, dtype=np.uint8)
        ms = C.c_double()
        i32, u8 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        check(self.L.armour_roadmap_connect_batch(self.h, Q, w.ctypes.data_as(i32), _dp(q), _dp(tg), k, node.ctypes.data_as(i32), _dp(dist), ok.ctypes.data_as(u8),
                                                  count.ctypes.data_as(i32), direct.ctypes.data_as(u8), C.byref(ms)))
        out = dict(node=node, dist=dist, edge_ok=ok.astype(bool), count=count, ms=ms.value)
        if tg is not None:
            out["direct"] = direct.astype(bool)
        return out

    def descend_many(self, worlds, starts, connect_k=8, seq_capacity=None):
        """descend() for Q queries with one device call: worlds [Q], starts [Q,n] -> [(path [P,n] | None, length)] as descend returns them."""
        q = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, self.n)
        Q = q.shape[0]
        w = np.ascontiguousarray(np.broadcast_to(np.asarray(worlds, dtype=np.int32), (Q,)))
        cap = Q * 64 if seq_capacity is None else int(seq_capacity)
        i32 = C.POINTER(C.c_int32)
        while True:
            off, seq = np.zeros(Q + 1, dtype=np.int32), np.zeros(max(cap, 1), dtype=np.int32)
            status, length = np.zeros(Q, dtype=np.uint8), np.full(Q, np.inf)
            rc = self.L.armour_roadmap_descend_batch(self.h, Q, w.ctypes.data_as(i32), _dp(q), int(connect_k), cap, off.ctypes.data_as(i32), seq.ctypes.data_as(i32),
                                                     status.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(length))
            if rc == _lib.ECAPACITY and seq_capacity is None and off[Q] > cap:
                cap = int(off[Q])          # seq_off is complete on ECAPACITY: once more with the room it names
                continue
            check(rc)
            break
        out = []
        for i in range(Q):
            if status[i] == 0:
                out.append((None, float(length[i])))
            else:
                goal = self.field_goals[w[i]]
                out.append((np.vstack([q[i], self.nodes[seq[off[i]:off[i + 1]]], goal]), float(length[i])))
        return out


def device_roadmap(robot, N, radius, k_max, seed, lb, ub, continuous, device=0):
    """uniform_roadmap with the neighbour search on the device: the same seeded nodes, and the edges from ONE self-query of an edge-less
    handle (every node's k_max nearest other nodes within `radius`), their union sorted and deduplicated with i < j.  Returns (nodes, edges)
    as uniform_roadmap does, so Roadmap(robot, *device_roadmap(...)) reads like today's call."""
    cont = np.asarray(continuous, dtype=bool)
    lo = np.where(cont, -np.pi, np.asarray(lb, dtype=np.float64))
    hi = np.where(cont, np.pi, np.asarray(ub, dtype=np.float64))
    nodes = lo + (hi - lo) * np.random.default_rng(seed).random((int(N), cont.size))
    k = min(int(k_max), _lib.ROADMAP_KNN_MAX)
    if k < int(k_max) and int(N) - 1 > k:
        raise ValueError(f"device_roadmap: k_max = {k_max} above the search's {_lib.ROADMAP_KNN_MAX}")
    if int(N) < 2 or k <= 0:
        return nodes, np.zeros((0, 2), dtype=np.int32)
    bare = Roadmap(robot, nodes, np.zeros((0, 2), dtype=np.int32), continuous=cont.astype(np.uint8), device=device)
    try:
        index, _, _ = bare.knn(nodes, k, radius=radius, exclude=np.arange(int(N), dtype=np.int32))
    finally:
        bare.close()
    rows = np.repeat(np.arange(int(N), dtype=np.int32), k)
    cols = index.ravel()
    keep = cols >= 0
    e = np.sort(np.stack([rows[keep], cols[keep]], axis=1), axis=1)
    if not e.shape[0]:
        return nodes, np.zeros((0, 2), dtype=np.int32)
    e = np.unique(e, axis=0)
    return nodes, np.ascontiguousarray(e, dtype=np.int32)


def waypoint_along(path, q_cur, lookahead, continuous):
    """The point at arc length `lookahead` from q_cur along the polyline q_cur -> path[1] -> ... (segments wrapped on continuous joints),
    continued along the last segment past the goal (no clipping, as robot_arm_straight_line_HLP.get_waypoint)."""
    pts = [np.asarray(q_cur, dtype=np.float64)] + [np.asarray(p, dtype=np.float64) for p in path[1:]]
    cont = np.asarray(continuous, dtype=bool)
    rest = float(lookahead)
    p = pts[0]
    for i in range(1, len(pts)):
        d = pts[i] - p                                   # the straight-line rule's arithmetic (scenes.angdiff on continuous joints)
        d[cont] = angdiff(p[cont], pts[i][cont])
        L = np.linalg.norm(d)
        if L == 0.0:
            continue
        if rest <= L or i == len(pts) - 1:
            return p + rest * d / L
        rest -= L
        p = p + d
    return p.copy()


class RoadmapHLP:
    """High-level planner over a checked Roadmap: get_waypoint(q_cur, lookahead) plans q_cur -> goal in world `world` of the last check
    and returns the point `lookahead` along the path.  A direct free edge gives the straight-line rule's point; with no path it falls
    back to scenes.straight_line_waypoint, as the reference's HLPs do."""

    def __init__(self, roadmap, goal, world=0, connect_k=8):
        self.roadmap, self.goal, self.world, self.connect_k = roadmap, np.asarray(goal, dtype=np.float64), int(world), int(connect_k)
        self.path = None

    def get_waypoint(self, q_cur, lookahead):
        self.path = self.roadmap.plan(self.world, q_cur, self.goal, connect_k=self.connect_k)
        if self.path is None:
            return straight_line_waypoint(q_cur, self.goal, lookahead)
        return waypoint_along(self.path, q_cur, lookahead, self.roadmap.continuous.astype(bool))


class RoadmapFieldHLP:
    """RoadmapHLP without the search: get_waypoint(q_cur, lookahead) follows world `world`'s cost-to-go field of the roadmap's last
    field() (Roadmap.descend) and returns the point `lookahead` along that path; with no path it falls back to
    scenes.straight_line_waypoint towards the field's goal."""

    def __init__(self, roadmap, world, connect_k=8):
        self.roadmap, self.world, self.connect_k = roadmap, int(world), int(connect_k)
        self.goal = np.array(roadmap.field_goals[self.world])
        self.path = None

    def get_waypoint(self, q_cur, lookahead):
        self.path, _ = self.roadmap.descend(self.world, q_cur, connect_k=self.connect_k)
        if self.path is None:
            return straight_line_waypoint(q_cur, self.goal, lookahead)
        return waypoint_along(self.path, q_cur, lookahead, self.roadmap.continuous.astype(bool))


def field_hlps(roadmap, worlds, connect_k=8, batched=False):
    """`worlds` as trials.run_trials takes them ([(name, problem)]): checks the roadmap against all of them in one launch (obstacles padded
    to one count), computes every world's field towards its goal in one call, and returns the factory (i, world) -> RoadmapFieldHLP that
    run_trials(hlp=...) accepts.  The roadmap serves these worlds until its next check.  batched=True: the factory also carries
    get_waypoints(indices, qs, lookaheads) -> the waypoints of those worlds from ONE descend_many, which run_trials calls once per iteration
    in place of a get_waypoint per world (the same waypoints)."""
    probs = [p for _, p in worlds]
    obs = [np.asarray(p["obstacles"], dtype=np.float64).reshape(-1, 12) for p in probs]
    O = max([o.shape[0] for o in obs] + [1])
    roadmap.check(np.stack([pad_obstacles(o, O) for o in obs]))
    roadmap.field(np.stack([np.asarray(p["goal"], dtype=np.float64) for p in probs]), connect_k=connect_k)

    def make(i, world):
        return RoadmapFieldHLP(roadmap, i, connect_k=connect_k)

    def get_waypoints(indices, qs, lookaheads):
        cont = roadmap.continuous.astype(bool)
        paths = roadmap.descend_many(indices, qs, connect_k=connect_k)
        return [straight_line_waypoint(q, roadmap.field_goals[i], la) if path is None else waypoint_along(path, q, la, cont)
                for i, q, la, (path, _) in zip(indices, qs, lookaheads, paths)]

    if batched:
        make.get_waypoints = get_waypoints
    return make


def moving_field_hlps(roadmap, worlds, velocities, horizon=None, connect_k=8):
    """field_hlps(batched=True) for worlds whose obstacles move: `velocities` is a list of [O_w, 3], one per world (padded with zeros as the
    obstacles are padded with pad_obstacles).  The factory carries set_world_times(t_world [W]), which run_trials(velocities=...) calls
    before every waypoint query, and get_waypoints(indices, qs, lookaheads), which does per call ONE check_moving of all W worlds on the
    windows [t_world[w], t_world[w] + horizon], ONE field and ONE descend_many, with field_hlps' fall-back to the straight-line waypoint.
    horizon=None: the plan's duration (planner.default_params), the span the half-space tables of the same iteration cover.  Worlds that have
    finished keep their last clock, so a world's index is its index in the trial.  The factory's last_check is the dict the last check_moving
    returned (None before the first call)."""
    probs = [p for _, p in worlds]
    obs = [np.asarray(p["obstacles"], dtype=np.float64).reshape(-1, 12) for p in probs]
    vel = [np.asarray(v, dtype=np.float64).reshape(-1, 3) for v in velocities]
    if len(vel) != len(obs) or any(v.shape[0] != o.shape[0] for v, o in zip(vel, obs)):
        raise ValueError("moving_field_hlps: one velocity per obstacle of every world")
    O = max([o.shape[0] for o in obs] + [1])
    obs_p = np.stack([pad_obstacles(o, O) for o in obs])
    vel_p = np.stack([np.concatenate([v, np.zeros((O - v.shape[0], 3))]) for v in vel])
    goals = np.stack([np.asarray(p["goal"], dtype=np.float64) for p in probs])
    if horizon is None:
        from .planner import default_params
        horizon = default_params(1).duration
    state = dict(t_world=np.zeros(len(probs)))

    class _One:
        """One world's view of the factory, for a caller that asks world by world: each question is a get_waypoints of its own."""

        def __init__(self, i):
            self.i = int(i)

        def get_waypoint(self, q_cur, lookahead):
            return get_waypoints([self.i], [np.asarray(q_cur, dtype=np.float64)], [lookahead])[0]

    def make(i, world):
        return _One(i)

    def set_world_times(t_world):
        state["t_world"] = np.array(np.broadcast_to(np.asarray(t_world, dtype=np.float64), (len(probs),)))

    def get_waypoints(indices, qs, lookaheads):
        cont = roadmap.continuous.astype(bool)
        make.last_check = roadmap.check_moving(obs_p, vel_p, state["t_world"], state["t_world"] + float(horizon))
        roadmap.field(goals, connect_k=connect_k)
        paths = roadmap.descend_many(indices, qs, connect_k=connect_k)
        return [straight_line_waypoint(q, goals[i], la) if path is None else waypoint_along(path, q, la, cont)
                for i, q, la, (path, _) in zip(indices, qs, lookaheads, paths)]

    make.last_check = None
    make.set_world_times = set_world_times
    make.get_waypoints = get_waypoints
    return make
