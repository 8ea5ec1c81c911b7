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
    s = rm.check_slices(obstacles, velocity, t0, dt, K)     # the window rule on K consecutive slices of every world's clock, one launch
    a = rm.arrival(step_len, ...)                           # earliest arrival over (node, slice) states of those tables, waiting allowed
    plans = rm.plan_slices(starts, goals, obstacles, velocity, t0, dt, K, speed)   # knn + check_slices + arrival -> timed polylines
    res = run_trials(worlds, hlp=spacetime_hlps(rm, worlds, velocities, speed), velocities=velocities)

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


    def check_slices(self, obstacles, velocity, t0, dt, K, extra_world=None, extra_a=None, extra_b=None, host=False, tables=True):
        """The window rule of check_moving on K <= 64 consecutive slices [t0[w] + k dt, t0[w] + (k + 1) dt] of every world's clock in one
        launch (armour_roadmap_check_slices): obstacles [W,O,12] / velocity [W,O,3] as check_moving takes them, t0 [W] (or a scalar).  Extra
        edges: extra_world [Q], extra_a / extra_b [Q,n], judged by the edge rule in their world (a == b: the node rule).  Returns dict
        node_slices [W,N] uint64, edge_slices [W,E] uint64 (bit k: free in slice k; None with tables=False, which leaves them on the device
        for arrival()), extra_slices [Q] uint64, slice_times [W,K+1], ms.  The last check's state (plan, field, descend) is untouched.
        host=True: the library's host loop, on a Roadmap(host=True)."""
        obs, W, O = _lib.as_worlds(obstacles)
        vel = np.ascontiguousarray(np.asarray(velocity, dtype=np.float64).reshape(W, O, 3))
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(t0, dtype=np.float64), (W,)))
        K = int(K)
        if extra_world is None:
            Q, xw, xa, xb = 0, None, None, None
        else:
            xa = np.ascontiguousarray(extra_a, dtype=np.float64).reshape(-1, self.n)
            xb = np.ascontiguousarray(extra_b, dtype=np.float64).reshape(-1, self.n)
            Q = xa.shape[0]
            xw = np.ascontiguousarray(np.broadcast_to(np.asarray(extra_world, dtype=np.int32), (Q,)))
            if xb.shape[0] != Q:
                raise ValueError("Roadmap.check_slices: extra_a and extra_b differ in length")
        keep = tables or host
        ns = np.zeros((W, self.N), dtype=np.uint64) if keep else None
        es = np.zeros((W, self.E), dtype=np.uint64) if keep else None
        xs = np.zeros(Q, dtype=np.uint64)
        times = np.zeros((W, max(K, 0) + 1))
        ms = C.c_double(0.0)
        u64, i32 = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
        p64 = lambda a: None if a is None else a.ctypes.data_as(u64)
        args = (self.h, W, O, _dp(obs) if obs.size else None, _dp(vel) if vel.size else None, _dp(t), float(dt), K, Q,
                None if xw is None else xw.ctypes.data_as(i32), _dp(xa), _dp(xb), p64(ns), p64(es), p64(xs), _dp(times))
        check(self.L.armour_roadmap_check_slices_host(*args) if host else self.L.armour_roadmap_check_slices(*args, C.byref(ms)))
        self.slices_W, self.slices_K = W, K
        return dict(node_slices=ns, edge_slices=es, extra_slices=xs, slice_times=times, ms=ms.value)

    def arrival(self, step_len, start_mask, goal_mask, x_world=None, x_u=None, x_v=None, x_len=None, x_mask=None, host=False, reach=True):
        """Earliest arrival over (node, slice) states of the last check_slices (armour_roadmap_arrival), all its worlds in one launch: node N
        is the start with mask start_mask[w] | 1, node N + 1 the goal with mask goal_mask[w]; the extra edges (x_world sorted, x_u / x_v in
        [0, N + 2), x_len in radians, x_mask) join them to the roadmap; an edge of length len takes max(1, ceil(len / step_len)) slices and
        every slice of a traversal must be free; waiting at a node is allowed while it stays free.  Returns dict reach [W,N+2] uint64 (None
        with reach=False), goal_slice [W] (-1: not reached within the slices), path_len [W], path_node / path_slice [W,64] (-1 padded: the
        visits from the start on, a node with the slice at which it is reached, the start with the slice at which it is left), sweeps [W],
        ms.  host=True: the library's host loop after check_slices(host=True)."""
        W = getattr(self, "slices_W", None)
        if W is None:           # no sliced check to take W from: the library says so (ESTATE)
            check(self.L.armour_roadmap_arrival_host(self.h, float(step_len), 0, *([None] * 13)) if host else
                  self.L.armour_roadmap_arrival(self.h, float(step_len), 0, *([None] * 14)))
            raise RuntimeError("armour_roadmap_arrival accepted a roadmap without a sliced check")
        sm = np.ascontiguousarray(np.broadcast_to(np.asarray(start_mask, dtype=np.uint64), (W,)))
        gm = np.ascontiguousarray(np.broadcast_to(np.asarray(goal_mask, dtype=np.uint64), (W,)))
        i32, u64 = C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
        if x_world is None:
            X, xw, xu, xv, xl, xm = 0, None, None, None, None, None
        else:
            xw, xu, xv = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (x_world, x_u, x_v))
            xl = np.ascontiguousarray(x_len, dtype=np.float64).reshape(-1)
            xm = np.ascontiguousarray(x_mask, dtype=np.uint64).reshape(-1)
            X = xw.size
            if not (xu.size == xv.size == xl.size == xm.size == X):
                raise ValueError("Roadmap.arrival: the extra edges' arrays differ in length")
        ip = lambda a: None if a is None else a.ctypes.data_as(i32)
        up = lambda a: None if a is None else a.ctypes.data_as(u64)
        rows = np.zeros((W, self.N + 2), dtype=np.uint64) if reach else None
        goal_slice, path_len, sweeps = (np.zeros(W, dtype=np.int32) for _ in range(3))
        path_node, path_slice = np.full((W, 64), -1, dtype=np.int32), np.full((W, 64), -1, dtype=np.int32)
        ms = C.c_double(0.0)
        args = (self.h, float(step_len), X, ip(xw), ip(xu), ip(xv), _dp(xl), up(xm), up(sm), up(gm), up(rows), ip(goal_slice), ip(path_len), ip(path_node),
                ip(path_slice), ip(sweeps))
        check(self.L.armour_roadmap_arrival_host(*args) if host else self.L.armour_roadmap_arrival(*args, C.byref(ms)))
        return dict(reach=rows, goal_slice=goal_slice, path_len=path_len, path_node=path_node, path_slice=path_slice, sweeps=sweeps, ms=ms.value)

    def plan_slices(self, starts, goals, obstacles, velocity, t0, dt, K, speed, connect_k=8, host=False):
        """Timed paths through moving worlds, one per world: starts / goals [W,n], the worlds as check_slices takes them, `speed` the arm's
        nominal joint-space speed in rad/s (an edge of length len takes max(1, ceil(len / (speed dt))) slices).  Four steps: ONE knn of all
        starts and goals with no mask; ONE check_slices whose extra edges are start -> node and goal -> node for the connect_k nearest,
        start -> goal, and the degenerate edges start -> start and goal -> goal for the two masks; ONE arrival; then per world the timed
        polyline.  Returns a list of W dicts: path [P,n] (start, nodes..., goal; None when the goal is not reached within the K slices),
        node [P] (N: the start, N + 1: the goal), slice [P], time [P] (slice_times at those slices: when each point is reached, for the
        start when it is left), goal_slice; and keeps the raw results in self.last_slices / self.last_arrival."""
        s = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, self.n)
        g = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, self.n)
        W, N, k = s.shape[0], self.N, min(int(connect_k), self.N)
        if g.shape[0] != W:
            raise ValueError("Roadmap.plan_slices: one goal per start")
        if k > 0:
            index, dist, count = self.knn(np.concatenate([s, g]), k, host=host)
        else:
            index, dist, count = np.zeros((2 * W, 0), dtype=np.int32), np.zeros((2 * W, 0)), np.zeros(2 * W, dtype=np.int32)
        per = 2 * k + 3                                  # a world's extra edges: k from the start, k from the goal, start -> goal, the two masks
        cont = self.continuous.astype(bool)
        xw = np.repeat(np.arange(W, dtype=np.int32), per)
        xa, xb = np.zeros((W * per, self.n)), np.zeros((W * per, self.n))
        xu, xv, xl = np.zeros(W * per, dtype=np.int32), np.zeros(W * per, dtype=np.int32), np.zeros(W * per)
        used = np.zeros(W * per, dtype=bool)
        for w in range(W):
            base = w * per
            for side, (q, end) in enumerate(((s[w], N), (g[w], N + 1))):
                for c in range(int(count[side * W + w])):
                    i = base + side * k + c
                    v = int(index[side * W + w, c])
                    xa[i], xb[i], xu[i], xv[i], xl[i], used[i] = q, self.nodes[v], end, v, dist[side * W + w, c], True
                for c in range(int(count[side * W + w]), k):     # (fewer than k nodes: a slot that joins nothing, judged and dropped)
                    xa[base + side * k + c] = xb[base + side * k + c] = q
            i = base + 2 * k
            xa[i], xb[i], xu[i], xv[i], used[i] = s[w], g[w], N, N + 1, True
            d = wrapped_diff(s[w], g[w], cont)
            xl[i] = np.sqrt((d * d).sum())
            xa[i + 1] = xb[i + 1] = s[w]
            xa[i + 2] = xb[i + 2] = g[w]
        sl = self.check_slices(obstacles, velocity, t0, dt, K, extra_world=xw, extra_a=xa, extra_b=xb, host=host, tables=False)
        xm = sl["extra_slices"]
        masks = xm.reshape(W, per)
        ar = self.arrival(float(speed) * float(dt), masks[:, 2 * k + 1], masks[:, 2 * k + 2], x_world=xw[used], x_u=xu[used], x_v=xv[used], x_len=xl[used],
                          x_mask=xm[used], host=host, reach=False)
        self.last_slices, self.last_arrival = sl, ar
        out = []
        for w in range(W):
            P = int(ar["path_len"][w])
            if P == 0:
                out.append(dict(path=None, node=None, slice=None, time=None, goal_slice=int(ar["goal_slice"][w])))
                continue
            node, sli = ar["path_node"][w, :P].copy(), ar["path_slice"][w, :P].copy()
            pts = np.stack([s[w] if v == N else g[w] if v == N + 1 else self.nodes[v] for v in node])
            out.append(dict(path=pts, node=node, slice=sli, time=sl["slice_times"][w, sli], goal_slice=int(ar["goal_slice"][w])))
        return out

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


def spacetime_hlps(roadmap, worlds, velocities, speed, dt=0.25, K=32, connect_k=8):
    """moving_field_hlps with a search over (node, time slice) states in place of one window per world: `worlds` and `velocities` as
    moving_field_hlps takes them, `speed` the arm's nominal joint-space speed in rad/s.  The factory carries set_world_times(t_world [W]),
    which run_trials(velocities=...) calls before every waypoint query, and get_waypoints(indices, qs, lookaheads), which does per call ONE
    Roadmap.plan_slices of all W worlds from the worlds' current configurations at the worlds' clocks (K slices of dt seconds ahead).
    Waypoint rule: the polyline is the current configuration followed by the path's nodes up to the first node at which the path waits at
    least one planning period (planner.default_params t_plan), or up to the goal; when that wait is at the start itself the waypoint is the
    current configuration (stand still: "wait until the box has passed"), otherwise waypoint_along(polyline, q, lookahead); with no path
    within the K slices it falls back to the straight-line waypoint, as field_hlps does.  The search only proposes waypoints: safety rests on
    the solver's tables and the moving audit.  `speed`, dt = 0.25 and K = 32 are starting values that nobody has tuned.  Worlds that have
    finished keep their last clock and configuration.  The factory's last_check is the dict the last check_slices returned, last_plans the
    list plan_slices returned (None before the first call)."""
    probs = [p for _, p in worlds]
    obs = [np.asarray(p["obstacles"], dtype=np.float64).reshape(-1, 12) for p in probs]
    vel = [np.asarray(v, dtype=np.float64).reshape(-1, 3) for v in velocities]
    if len(vel) != len(obs) or any(v.shape[0] != o.shape[0] for v, o in zip(vel, obs)):
        raise ValueError("spacetime_hlps: one velocity per obstacle of every world")
    O = max([o.shape[0] for o in obs] + [1])
    obs_p = np.stack([pad_obstacles(o, O) for o in obs])
    vel_p = np.stack([np.concatenate([v, np.zeros((O - v.shape[0], 3))]) for v in vel])
    goals = np.stack([np.asarray(p["goal"], dtype=np.float64) for p in probs])
    from .planner import default_params
    period = float(default_params(1).t_plan)
    step_len = float(speed) * float(dt)
    state = dict(t_world=np.zeros(len(probs)), q=np.stack([np.asarray(p["q0"], dtype=np.float64) for p in probs]))

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

    def hop_slices(a, b):
        d = wrapped_diff(a, b, cont)
        return max(1, int(np.ceil(np.sqrt((d * d).sum()) / step_len)))

    def get_waypoints(indices, qs, lookaheads):
        for i, q in zip(indices, qs):
            state["q"][i] = np.asarray(q, dtype=np.float64)
        plans = roadmap.plan_slices(state["q"], goals, obs_p, vel_p, state["t_world"], dt, K, speed, connect_k=connect_k)
        make.last_check, make.last_plans = roadmap.last_slices, plans
        out = []
        for i, q, la in zip(indices, qs, lookaheads):
            plan = plans[i]
            if plan["path"] is None:
                out.append(straight_line_waypoint(q, goals[i], la))
                continue
            path, sli = plan["path"], plan["slice"]
            if sli[0] * float(dt) >= period:             # the path leaves the start a planning period from now, or later
                out.append(np.array(q, dtype=np.float64))
                continue
            last = 1
            while last < path.shape[0] - 1:              # the wait at path[last]: from its arrival to the departure of the next hop
                leave = sli[last + 1] - hop_slices(path[last], path[last + 1])
                if (leave - sli[last]) * float(dt) >= period:
                    break
                last += 1
            out.append(waypoint_along(path[:last + 1], q, la, cont))
        return out

    cont = roadmap.continuous.astype(bool)
    make.last_check = make.last_plans = None
    make.set_world_times = set_world_times
    make.get_waypoints = get_waypoints
    return make
