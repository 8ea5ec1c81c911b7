"""Moving obstacles in the workspace RRT*, the inverse kinematics and the end-effector HLP, CPU half (include/armour_hip.h
armour_ws_tree_plan_moving(_host), armour_ik_moving(_host); armour_amd/ws_planner.py plan_workspace_trees and armour_amd/ik.py solve_ik with
velocity, t_from, t_to, WorkspaceTreeHLP with a velocity, moving_workspace_hlps).

The rule is the window rule and nothing else changes, so the restatements are test_ws_tree.py's plan_ws_np with boxes_clearance replaced by
its window form (per obstacle the centres shifted by -v mid and the half-sizes grown by |v| half) and test_ik.py's solve_np with
config_clearance replaced by test_moving_audit.py's config_clearance_moving at the window's mid and half.  The host twins have to
reproduce them bit for bit wherever their `margin` is above 1e-9, which the seeds below were chosen for (asserted, not skipped).  Then: zero
velocity is the static entry, soundness by sampling over the window, hand-made scenes in which only the window decides, the refusals, and
the HLP with its clock.  The device is compared to the host twins in test_ws_moving_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import test_ik
import test_ws_tree
from test_ik import Q_A, Q_TOL, blocking_box, chain_np, solve_np
from test_moving_audit import config_clearance_moving, random_motion, velocity_norm
from test_path_audit import CL_TOL
from test_roadmap import _limits, _robot, config_clearance, geometry, pair_clearance, robot_dict
from test_tree_plan import _same_bits
from test_trials import START as Q_START, _world
from test_trials_moving import DUR, T_PLAN, ScriptedMovingPlanner
from test_ws_tree import GOAL, LB, MARGIN, OPTS, START, UB, _box, assert_equals_restatement, assert_same_plans, boxes_clearance, plan_ws_np, wall_with_window

WINDOWS = ((0.0, 0.5), (1.25, 1.25), (-0.1, 0.2))      # one per world; the second is an instant
EXTRA = 4                                               # small moving boxes beside the wall
WORLD_SEED = 2                                          # of the worlds' boxes and velocities: with the tree seeds 1, 2, 3 every margin of the twins is
                                                        # above 1e-9 (asserted above MARGIN), trees and inverse kinematics, and worlds plan differently frozen
CHAIN = np.array([[0.2, -0.2, 0.3], [0.4, 0.0, 0.5], [0.6, 0.3, 0.5], [0.8, 0.3, 0.7]])      # test_ws_tree's: the third edge crosses the wall
IK_S = 8


# ----------------------------------------------------------------------------------------------------------- helpers
def window_boxes_clearance(V, t_from, t_to):
    """boxes_clearance's signature with the window rule of one world inside: per obstacle o the boxes' centres x - v_o mid and half-sizes
    h + |v_o| half, each product and sum rounded on its own"""
    mid, half = 0.5 * (t_from + t_to), 0.5 * (t_to - t_from)
    V = np.asarray(V, dtype=np.float64).reshape(-1, 3)
    nv = velocity_norm(V)

    def clearance(x, h, Z):
        Z = np.asarray(Z, dtype=np.float64).reshape(-1, 12)
        x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
        out = np.full(len(x), np.inf)
        U = np.broadcast_to(np.eye(3), (len(x), 3, 3))
        for o in range(Z.shape[0]):
            out = np.minimum(out, pair_clearance(x - V[o][None] * mid, U, h + nv[o] * half, Z[o:o + 1])[:, 0])
        return out
    return clearance


def plan_moving_np(monkeypatch, Z, V, window, *args, **kw):
    with monkeypatch.context() as m:
        m.setattr(test_ws_tree, "boxes_clearance", window_boxes_clearance(V, *window))
        return plan_ws_np(Z, *args, **kw)


def solve_moving_np(monkeypatch, g, targets, q_ref, obs, vel, windows, world, seeds, S, lb, ub):
    """solve_np target by target, each with the window rule of its own world in place of config_clearance -> a list of solve_np's dicts"""
    out = []
    for t in range(len(targets)):
        w = world[t]
        mid, half = (0.5 * (windows[w][0] + windows[w][1]), 0.5 * (windows[w][1] - windows[w][0])) if w >= 0 else (0.0, 0.0)
        V = vel[w] if w >= 0 else np.zeros((0, 3))
        with monkeypatch.context() as m:
            m.setattr(test_ik, "config_clearance", lambda g_, Q, Z, r=None, V=V, mid=mid, half=half: config_clearance_moving(g_, Q, Z, V, mid, r, half))
            out.append(solve_np(g, targets[t:t + 1], q_ref[t:t + 1], obs, [w], seeds[t:t + 1], S, lb, ub))
    return out


def moving_worlds(seed=WORLD_SEED, W=len(WINDOWS), extra=EXTRA, lo=0.05, hi=0.3, wall=None):
    """(obstacles [W,5+extra,12], velocity [W,5+extra,3]): wall_with_window() (or the boxes `wall`), its boxes drifting at a tenth of the
    speed, then `extra` small boxes inside the sampling box in linear motion at lo..hi m/s"""
    rng = np.random.default_rng(seed)
    wall = wall_with_window() if wall is None else wall
    obs = np.zeros((W, len(wall) + extra, 12))
    for w in range(W):
        small = [_box(rng.uniform([0.15, -0.6, 0.0], [1.0, 0.6, 1.0]), rng.uniform(0.02, 0.06, 3)) for _ in range(extra)]
        obs[w] = np.vstack([wall] + ([np.stack(small)] if extra else []))
    vel = random_motion(rng, obs, lo, hi)
    vel[:, :len(wall)] *= 0.1
    return obs, vel


def _t(windows):
    t0, t1 = np.array(windows, dtype=np.float64).reshape(-1, 2).T
    return dict(t_from=np.ascontiguousarray(t0), t_to=np.ascontiguousarray(t1))


def _plan(obs, vel, windows, seeds, host=True, starts=None, goals=None, **kw):
    from armour_amd.ws_planner import plan_workspace_trees
    obs = np.asarray(obs)
    obs = obs[None] if obs.ndim == 2 else obs
    W = obs.shape[0]
    o = dict(OPTS, lb=LB, ub=UB, trees=True)
    o.update(kw)
    return plan_workspace_trees(obs, np.stack([START] * W) if starts is None else starts, np.stack([GOAL] * W) if goals is None else goals, seeds, host=host,
                                velocity=vel, **_t(windows), **o)


def kinova():
    robot = _robot("kinova")
    lb, ub, _ = _limits(robot)
    return dict(robot=robot, g=geometry(robot_dict(robot)), lb=lb, ub=ub)


def ik_problem(s, W=len(WINDOWS), per=3, seed=5):
    """per targets in each of W worlds and one in world -1: the end effectors of random configurations, q_ref random -> (targets, q_ref, world, seeds)"""
    rng = np.random.default_rng(seed)
    N = W * per + 1
    lo, hi = np.maximum(s["lb"], -np.pi), np.minimum(s["ub"], np.pi)
    targets = chain_np(s["g"], rng.uniform(lo, hi, (N, 7)) * 0.6, np.zeros(3))[0]
    q_ref = rng.uniform(lo, hi, (N, 7)) * 0.5
    world = np.concatenate([np.repeat(np.arange(W), per), [-1]])
    return targets, q_ref, world, np.arange(N, dtype=np.uint64) + 7


def _solve(s, targets, q_ref, obs, vel, windows, world, seeds, host=True, S=IK_S, **kw):
    from armour_amd.ik import solve_ik
    return solve_ik(s["robot"], targets, q_ref, obs, world, seeds, S=S, host=host, details=True, velocity=vel, **_t(windows), **kw)


def moved(Z, V, time):
    Zt = np.array(Z, dtype=np.float64).reshape(-1, 12).copy()
    Zt[:, 0:3] += np.asarray(V).reshape(-1, 3) * time
    return Zt


def assert_path_sound_over_the_window(path, Z, V, window, buffer, tag):
    """every edge of `path`: 20 points x 11 times of the window, the point's buffered box against the obstacles themselves moved to that time"""
    rng = np.random.default_rng(3)
    for k, (a, b) in enumerate(zip(path[:-1], path[1:])):
        t = np.concatenate([[0.0, 1.0], rng.random(18)])
        pts = a + t[:, None] * (b - a)
        for time in np.linspace(window[0], window[1], 11):
            assert boxes_clearance(pts, np.full(pts.shape, buffer), moved(Z, V, time)).min() > -CL_TOL, (tag, k, time)


@pytest.fixture(scope="module")
def case():
    """The moving worlds and the host twins' results in them, computed once: the trees (seeds 1, 2, 3), a run with a seeded chain, and the
    inverse kinematics of ten targets."""
    s = kinova()
    obs, vel = moving_worlds()
    plans = _plan(obs, vel, WINDOWS, [1, 2, 3])
    chained = _plan(obs, vel, WINDOWS, [1, 2, 3], init=[CHAIN] * 3, max_iterations=60)
    targets, q_ref, world, seeds = ik_problem(s)
    sol = _solve(s, targets, q_ref, obs, vel, WINDOWS, world, seeds)
    return dict(s, obs=obs, vel=vel, plans=plans, chained=chained, targets=targets, q_ref=q_ref, world=world, seeds=seeds, sol=sol)


# ----------------------------------------------------------------------------------------------------------- the rule
def test_the_tree_twin_equals_the_numpy_restatement(case, monkeypatch):
    c = case
    print("tree margins", c["plans"].margin, c["chained"].margin)
    assert (c["plans"].margin > MARGIN).all() and (c["chained"].margin > MARGIN).all(), (c["plans"].margin, c["chained"].margin)
    for w, window in enumerate(WINDOWS):
        ref = plan_moving_np(monkeypatch, c["obs"][w], c["vel"][w], window, START, GOAL, w + 1, **OPTS)
        print(f"world {w}: status {ref['status']}, count {ref['count']}, rewires {ref['rewires']}, margin {ref['margin']:.2e}")
        assert_equals_restatement(c["plans"], w, ref)
        assert abs(c["plans"].margin[w] - ref["margin"]) <= 1e-12
        ref = plan_moving_np(monkeypatch, c["obs"][w], c["vel"][w], window, START, GOAL, w + 1, init=CHAIN, **dict(OPTS, max_iterations=60))
        assert_equals_restatement(c["chained"], w, ref)
    assert (c["plans"].rewires > 0).all() and (c["plans"].count > 50).all()                # the trees had to grow, and rewired
    # the same worlds judged frozen at time 0 plan differently somewhere: the motion shows in the result
    frozen = test_ws_tree._plan(c["obs"], [1, 2, 3])
    assert any(frozen.count[w] != c["plans"].count[w] or not _same_bits(frozen.nodes[w], c["plans"].nodes[w]) for w in range(len(WINDOWS)))


def test_the_ik_twin_equals_the_numpy_restatement(case, monkeypatch):
    c = case
    sol = c["sol"]
    print("ik margins", sol.margin, "status", sol.status)
    assert (sol.margin > MARGIN).all(), sol.margin
    refs = solve_moving_np(monkeypatch, c["g"], c["targets"], c["q_ref"], c["obs"], c["vel"], WINDOWS, c["world"], c["seeds"], IK_S, c["lb"], c["ub"])
    for t, ref in enumerate(refs):
        assert sol.status[t] == ref["status"][0] and sol.best[t] == ref["best"][0], t
        assert np.array_equal(sol.iterations[t], ref["iterations"][0]) and np.array_equal(sol.flags[t], ref["flags"][0]), t
        assert np.abs(sol.q_all[t] - ref["q_all"][0]).max() <= Q_TOL and np.abs(sol.err[t] - ref["err"][0]).max() <= Q_TOL
        cl = np.abs(ref["clearance"][0])
        if np.isfinite(sol.margin[t]):
            assert abs(np.nanmin(cl) - sol.margin[t]) <= 1e-11, t
    assert (sol.status == 1).any() and ((sol.flags & 3) == 1).any()                       # some solution is free, some converged one is blocked
    # frozen at time 0 some item is judged differently
    from armour_amd.ik import solve_ik
    frozen = solve_ik(c["robot"], c["targets"], c["q_ref"], c["obs"], c["world"], c["seeds"], S=IK_S, host=True, details=True)
    assert np.array_equal(frozen.iterations, sol.iterations) and not np.array_equal(frozen.flags, sol.flags)


def test_zero_velocity_is_the_static_entry_for_any_window(case):
    from armour_amd.ik import solve_ik
    c = case
    W = len(WINDOWS)
    zero = np.zeros(c["obs"].shape[:2] + (3,))
    static = test_ws_tree._plan(c["obs"], [1, 2, 3], init=[CHAIN] * 3)
    static_ik = solve_ik(c["robot"], c["targets"], c["q_ref"], c["obs"], c["world"], c["seeds"], S=IK_S, host=True, details=True)
    for windows in (((0.0, 0.0),) * W, ((-3.0, 4.0), (0.25, 0.25), (7.0, 11.5))):
        moving = _plan(c["obs"], zero, windows, [1, 2, 3], init=[CHAIN] * 3)
        for w in range(W):
            assert_same_plans(moving, w, static, w)
            assert moving.margin[w] == static.margin[w]
        assert _same_bits(moving.nodes, static.nodes) and np.array_equal(moving.parent, static.parent) and _same_bits(moving.node_cost, static.node_cost)
        sol = _solve(c, c["targets"], c["q_ref"], c["obs"], zero, windows, c["world"], c["seeds"])
        for k in ("status", "best", "q", "q_all", "err", "iterations", "flags", "margin"):
            assert np.array_equal(getattr(sol, k), getattr(static_ik, k), equal_nan=True), k


def test_paths_and_configurations_are_sound_over_their_windows_by_sampling(case):
    c = case
    edges = 0
    for res in (c["plans"], c["chained"]):
        for w, window in enumerate(WINDOWS):
            assert res.paths[w] is not None and _same_bits(res.paths[w][0], START)
            assert_path_sound_over_the_window(res.paths[w], c["obs"][w], c["vel"][w], window, OPTS["buffer"], w)
            edges += len(res.paths[w]) - 1
    buffered = _plan(c["obs"], c["vel"], WINDOWS, [1, 2, 3], buffer=0.03, max_iterations=150)
    for w, window in enumerate(WINDOWS):
        assert_path_sound_over_the_window(buffered.paths[w], c["obs"][w], c["vel"][w], window, 0.03, ("buffer", w))
    found = np.flatnonzero((c["sol"].status == 1) & (c["world"] >= 0))
    assert edges >= 10 and len(found) >= 2, (edges, found)
    for t in found:
        w = c["world"][t]
        for time in np.linspace(WINDOWS[w][0], WINDOWS[w][1], 11):
            assert config_clearance(c["g"], c["sol"].q[t][None], moved(c["obs"][w], c["vel"][w], time))[0] > -CL_TOL, (t, time)


# ----------------------------------------------------------------------------------------------------------- hand-made scenes
def test_a_box_arriving_at_the_start_point_and_on_a_chain():
    """A box 1 m from the start point comes at 0.5 m/s: its centre arrives at t = 2.  On [0, 1] the start is free; on [0, 3] the grown box
    covers it.  And a box that arrives on the third edge of a chain: kept whole early, cut late."""
    box = _box(START + np.array([0.0, 0.0, 1.0]), (0.05, 0.05, 0.05))[None]
    vel = np.array([[0.0, 0.0, -0.5]])
    early = _plan(box, vel[None], [(0.0, 1.0)], [1], max_iterations=40)
    late = _plan(box, vel[None], [(0.0, 3.0)], [1], max_iterations=40)
    assert early.status[0] != 2 and early.count[0] > 1 and early.margin[0] > MARGIN
    assert late.status[0] == 2 and late.count[0] == 0 and late.paths[0] is None and late.margin[0] > MARGIN
    chain = np.array([[0.2, -0.2, 0.3], [0.4, 0.0, 0.5], [0.6, 0.0, 0.5], [0.8, 0.2, 0.7]])
    on_edge = 0.5 * (chain[1] + chain[2])
    box = _box(on_edge + np.array([0.0, 1.0, 0.0]), (0.03, 0.03, 0.03))[None]
    vel = np.array([[0.0, -0.5, 0.0]])
    res = _plan(np.stack([box] * 2), np.stack([vel] * 2), [(0.0, 1.0), (1.95, 2.05)], [1, 1], init=[chain] * 2, max_iterations=0)
    assert (res.margin > MARGIN).all() and list(res.chain_kept) == [4, 2] and list(res.count) == [5, 3]
    frozen = test_ws_tree._plan(box, [1], init=[chain], max_iterations=0)
    assert frozen.chain_kept[0] == 4


def test_a_box_arriving_on_the_static_pick_of_the_inverse_kinematics():
    from armour_amd.ik import solve_ik
    s = kinova()
    p_a = chain_np(s["g"], Q_A[None], np.zeros(3))[0][0]
    box = blocking_box(s["g"], p_a)
    box[0:3] += np.array([0.0, 0.0, 2.0])                                                  # 2 m above the target, coming down at 1 m/s
    vel = np.array([[[0.0, 0.0, -1.0]]])
    static = solve_ik(s["robot"], [p_a], Q_A, box[None, None], [0], [3], S=IK_S, host=True, details=True)
    assert static.status[0] == 1 and static.best[0] == 0
    early = _solve(s, [p_a], Q_A, box[None, None], vel, [(0.0, 0.5)], [0], [3])
    assert early.status[0] == 1 and early.best[0] == 0 and _same_bits(early.q, static.q) and early.margin[0] > MARGIN
    late = _solve(s, [p_a], Q_A, box[None, None], vel, [(1.9, 2.1)], [0], [3])
    assert late.margin[0] > MARGIN and (late.status[0] == 2 or late.best[0] != 0)
    assert late.flags[0, 0] == 1                                                           # the static pick converged and is blocked
    # world -1 has no obstacles and reads no window (the reversed one would be refused, a window of world 0 is ignored)
    none = _solve(s, [p_a], Q_A, box[None, None], vel, [(1.9, 2.1)], [-1], [3])
    assert none.status[0] == 1 and none.best[0] == 0 and none.margin[0] == np.inf and _same_bits(none.q, static.q)


# ----------------------------------------------------------------------------------------------------------- the C ABI
def _raw_plan(host, W, O, obs, vel, t0, t1):
    """armour_ws_tree_plan_moving(_host) itself with the pointers as given (None = NULL) -> rc"""
    from armour_amd import _lib
    L = _lib.load()
    rows = max(W, 1)
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    lb, ub, starts, goals = (np.ascontiguousarray(x, dtype=np.float64) for x in (LB, UB, np.stack([START] * rows), np.stack([GOAL] * rows)))
    seeds = np.arange(1, rows + 1, dtype=np.uint64)
    ints = [np.zeros(rows, dtype=np.int32) for _ in range(5)]
    reals = [np.zeros(rows) for _ in range(2)]
    path = np.zeros((rows, 512, 3))
    fn = L.armour_ws_tree_plan_moving_host if host else L.armour_ws_tree_plan_moving
    return fn(_lib._dp(lb), _lib._dp(ub), W, O, _lib._dp(obs), _lib._dp(vel), _lib._dp(t0), _lib._dp(t1), _lib._dp(starts), _lib._dp(goals),
              seeds.ctypes.data_as(C.POINTER(C.c_uint64)), 0, None, None, *(float(OPTS[k]) for k in ("step", "edge_step", "rewire_radius", "goal_rate", "buffer", "goal_tol")),
              20, 64, 512, *(x.ctypes.data_as(i32) for x in ints), *(x.ctypes.data_as(f64) for x in reals), path.ctypes.data_as(f64), None, None, None, None, None)


def _raw_ik(s, host, W, O, obs, vel, t0, t1, N=1, world=0):
    """armour_ik_moving(_host) itself on one target in world `world` -> rc"""
    from armour_amd import _lib
    L = _lib.load()
    rows = max(N, 1)
    i32 = C.POINTER(C.c_int32)
    lb, ub, tool, targets, q_ref = (np.ascontiguousarray(x, dtype=np.float64) for x in (s["lb"], s["ub"], np.zeros(3), np.tile([0.4, 0.1, 0.6], (rows, 1)), np.tile(Q_A, (rows, 1))))
    wd = np.full(rows, world, dtype=np.int32)
    seeds = np.arange(1, rows + 1, dtype=np.uint64)
    status, best, q_best = np.zeros(rows, dtype=np.int32), np.zeros(rows, dtype=np.int32), np.zeros((rows, 7))
    fn = L.armour_ik_moving_host if host else L.armour_ik_moving
    return fn(C.byref(s["robot"]), None, _lib._dp(lb), _lib._dp(ub), _lib._dp(tool), N, 4, W, O, _lib._dp(obs), _lib._dp(vel), _lib._dp(t0), _lib._dp(t1),
              wd.ctypes.data_as(i32), _lib._dp(targets), _lib._dp(q_ref), seeds.ctypes.data_as(C.POINTER(C.c_uint64)), 0.05, 0.1, 1e-9, 20, status.ctypes.data_as(i32),
              best.ctypes.data_as(i32), _lib._dp(q_best), None, None, None, None, None)


@pytest.mark.parametrize("host", [False, True])
def test_bad_arguments_are_refused_before_a_device_is_touched(host):
    """Every refusal the moving entries add to their static forms', and a few of those: ARMOUR_EINVAL each, from both entries.  The device
    entries too answer EINVAL, not EDEVICE, on a machine without a device: the checks come first."""
    from armour_amd import _lib
    s = kinova()
    box = np.ascontiguousarray(wall_with_window()[None, :1])
    vel, t0, t1 = np.zeros((1, 1, 3)), np.zeros(1), np.ones(1)
    bad_box, bad_vel = box.copy(), vel.copy()
    bad_box[0, 0, 4] = np.inf
    bad_vel[0, 0, 1] = np.nan
    cases = dict(negative_W=(-1, 1, box, vel, t0, t1), negative_O=(1, -1, box, vel, t0, t1), too_many_obstacles=(1, 257, box, vel, t0, t1),
                 null_obstacles=(1, 1, None, vel, t0, t1), obstacle_not_finite=(1, 1, bad_box, vel, t0, t1),
                 null_velocity=(1, 1, box, None, t0, t1), velocity_not_finite=(1, 1, box, bad_vel, t0, t1),
                 velocity_infinite=(1, 1, box, np.full((1, 1, 3), np.inf), t0, t1),
                 null_t_from=(1, 1, box, vel, None, t1), null_t_to=(1, 1, box, vel, t0, None),
                 t_from_not_finite=(1, 1, box, vel, np.array([np.nan]), t1), t_to_not_finite=(1, 1, box, vel, t0, np.array([np.inf])),
                 window_reversed=(1, 1, box, vel, np.array([1.0]), np.array([0.5])))
    for tag, args in cases.items():
        assert _raw_plan(host, *args) == _lib.EINVAL, ("trees", tag)
        assert _raw_ik(s, host, *args) == _lib.EINVAL, ("ik", tag)
    # the second world's window alone is reversed (the target's own world is the first)
    two = (2, 1, np.concatenate([box, box]), np.zeros((2, 1, 3)), np.array([0.0, 2.0]), np.array([1.0, 1.5]))
    assert _raw_plan(host, *two) == _lib.EINVAL and _raw_ik(s, host, *two) == _lib.EINVAL
    assert _raw_ik(s, host, 1, 1, box, vel, t0, t1, world=1) == _lib.EINVAL and _raw_ik(s, host, 1, 1, box, vel, t0, t1, world=-2) == _lib.EINVAL
    # no world, no target: successes that do nothing, with or without a device
    assert _raw_plan(host, 0, 1, box, vel, t0, t1) == _lib.OK and _raw_ik(s, host, 1, 1, box, vel, t0, t1, N=0) == _lib.OK
    assert _raw_ik(s, host, 0, 1, None, None, None, None, N=0) == _lib.OK


def test_the_bindings_argument_rules():
    from armour_amd.ik import solve_ik
    from armour_amd.ws_planner import WorkspaceTreeHLP, plan_workspace_trees
    s = kinova()
    Z = wall_with_window()
    vel = np.zeros((1, len(Z), 3))
    for kw in (dict(velocity=vel), dict(t_from=0.0), dict(t_to=1.0), dict(velocity=vel, t_from=0.0), dict(t_from=0.0, t_to=1.0), dict(velocity=vel, t_to=1.0)):
        with pytest.raises(ValueError):
            plan_workspace_trees(Z, [START], [GOAL], [1], LB, UB, host=True, **OPTS, **kw)
        with pytest.raises(ValueError):
            solve_ik(s["robot"], [[0.4, 0.1, 0.6]], Q_A, Z, [0], [1], S=2, host=True, **kw)
    with pytest.raises(ValueError):                                                      # two windows for one world: the broadcast refuses
        plan_workspace_trees(Z, [START], [GOAL], [1], LB, UB, host=True, velocity=vel, t_from=[0.0, 1.0], t_to=[1.0, 2.0], **OPTS)
    with pytest.raises(ValueError):                                                      # a velocity of another shape
        solve_ik(s["robot"], [[0.4, 0.1, 0.6]], Q_A, Z, [0], [1], S=2, host=True, velocity=np.zeros((1, 2, 3)), t_from=0.0, t_to=1.0)
    # scalars broadcast to every world
    a = plan_workspace_trees(np.stack([Z] * 2), [START] * 2, [GOAL] * 2, [1, 2], LB, UB, host=True, trees=True, velocity=np.zeros((2, len(Z), 3)), t_from=0.5, t_to=1.5,
                             **dict(OPTS, max_iterations=60))
    b = test_ws_tree._plan(np.stack([Z] * 2), [1, 2], max_iterations=60)
    assert_same_plans(a, 0, b, 0), assert_same_plans(a, 1, b, 1)
    _, p = _world(0, Q_START, Q_A)
    with pytest.raises(ValueError, match="windows that have passed"):
        WorkspaceTreeHLP(s["robot"], p["obstacles"], Q_A, mode="keep", trees=object(), velocity=np.zeros((1, 3)))
    with pytest.raises(ValueError):
        WorkspaceTreeHLP(s["robot"], p["obstacles"], Q_A, horizon=1.0)
    with pytest.raises(ValueError):
        WorkspaceTreeHLP(s["robot"], p["obstacles"], Q_A, velocity=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        WorkspaceTreeHLP(s["robot"], p["obstacles"], Q_A).set_world_time(1.0)


def test_a_batch_of_three_worlds_equals_its_worlds_one_by_one(case):
    c = case
    for w, window in enumerate(WINDOWS):
        one = _plan(c["obs"][w:w + 1], c["vel"][w:w + 1], [window], [w + 1])
        assert_same_plans(c["plans"], w, one, 0)
        assert one.margin[0] == c["plans"].margin[w]
    sol = c["sol"]
    for t in range(len(c["targets"])):
        w = c["world"][t]
        sl = slice(w, w + 1) if w >= 0 else slice(0, 1)
        one = _solve(c, c["targets"][t:t + 1], c["q_ref"][t:t + 1], c["obs"][sl], c["vel"][sl], [WINDOWS[max(w, 0)]], [0 if w >= 0 else -1], c["seeds"][t:t + 1])
        for k in ("status", "best", "q", "q_all", "err", "iterations", "flags", "margin"):
            assert np.array_equal(getattr(sol, k)[t:t + 1], getattr(one, k), equal_nan=True), (t, k)


# ----------------------------------------------------------------------------------------------------------- the HLP
def arriving_wall_world():
    """A reference-like world for the Kinova: the goal turns joint 0 by 2 rad, and a wall that at t = 0 stands 1 m further out moves in at
    0.5 m/s to stand across the end effector's straight way at t = 2."""
    s = kinova()
    start = np.array([0.0, 0.6, 0.0, 1.2, 0.0, 0.6, 0.0])
    goal = start.copy()
    goal[0] = 1.0
    za, zb = chain_np(s["g"], np.stack([start, goal]), np.zeros(3))[0]
    m = 0.5 * (za + zb)
    u = np.array([m[0], m[1], 0.0]) / np.hypot(m[0], m[1])
    wall = _box(m + 1.0 * u, (0.03, 0.03, 0.25))
    return dict(s, start=start, goal=goal, wall=wall[None], vel=(-0.5 * u)[None], za=za, zb=zb)


HLP_OPTS = dict(max_iterations=150, max_nodes=256, ik_options=dict(S=8))


def test_seed_mode_keeps_its_chain_while_the_window_is_free_and_loses_it_when_the_wall_arrives():
    from armour_amd.ws_planner import WorkspaceTreeHLP
    a = arriving_wall_world()
    h = WorkspaceTreeHLP(a["robot"], a["wall"], a["goal"], seed=5, host=True, mode="seed", velocity=a["vel"], horizon=0.2, **HLP_OPTS)
    straight = np.stack([a["za"], a["zb"]])
    kept = np.stack([a["za"], a["za"], a["zb"]])                                         # the tree of a chain kept whole: the start, then the chain [z, zb]
    h.path = straight                                                                    # the straight way, offered as the chain of the next call
    h.set_world_time(0.4)
    h.get_waypoint(a["start"], 0.1)                                                      # window [0.4, 0.6]: the wall is away, the chain is kept whole
    assert h.calls == 1 and h.status == 1 and _same_bits(h.path, kept) and h.margin_min > MARGIN
    h.path = straight
    h.set_world_time(1.9)
    h.get_waypoint(a["start"], 0.1)                                                      # window [1.9, 2.1]: the wall stands on the way
    assert h.calls == 2 and h.margin_min > MARGIN and not (len(h.path) == 3 and _same_bits(h.path, kept))
    if h.status == 1:
        assert len(h.path) > 3
        assert_path_sound_over_the_window(h.path, a["wall"], a["vel"], (1.9, 2.1), 0.0, "late")
    # the static HLP, which sees the wall where it stands at t = 0, never notices
    frozen = WorkspaceTreeHLP(a["robot"], a["wall"], a["goal"], seed=5, host=True, mode="seed", **HLP_OPTS)
    for _ in range(2):
        frozen.path = straight
        frozen.get_waypoint(a["start"], 0.1)
        assert frozen.status == 1 and _same_bits(frozen.path, kept)


def _trial_worlds(a):
    walled = _world(0, Q_START, a["goal"], lookahead=0.3)
    walled[1]["obstacles"] = np.vstack([walled[1]["obstacles"], a["wall"]])              # (the scripted backend knows a world by its first box)
    return [walled, _world(1, Q_START, a["goal"], lookahead=0.5)]


VEL = [np.array([[0.0, 0.0, 0.0], [0.0, 0.05, 0.02]]), np.array([[0.0, 0.0, 0.0]])]     # the marker boxes stand still, the wall drifts


def test_the_factory_batched_equals_per_world_objects_and_zero_velocities_give_workspace_hlps_waypoints():
    from armour_amd.planner import default_params
    from armour_amd.scenes import pad_obstacles
    from armour_amd.ws_planner import WorkspaceTreeHLP, moving_workspace_hlps, workspace_hlps
    a = arriving_wall_world()
    worlds = _trial_worlds(a)
    make = moving_workspace_hlps(worlds, a["robot"], VEL, horizon=0.8, seed=11, lookahead=0.15, host=True, mode="seed", **HLP_OPTS)
    assert make.last_ms == 0.0 and make.hlps == {}
    own = [WorkspaceTreeHLP(a["robot"], pad_obstacles(p["obstacles"], 2), p["goal"], seed=11, world=i, host=True, mode="seed",
                            velocity=np.concatenate([VEL[i], np.zeros((2 - len(VEL[i]), 3))]), horizon=0.8, **HLP_OPTS) for i, (_, p) in enumerate(worlds)]
    qs = [Q_START.copy(), Q_START.copy()]
    clock = np.zeros(2)
    for call in range(3):
        make.set_world_times(clock)
        got = make.get_waypoints([0, 1], qs, [0.3, 0.5])
        for i in range(2):
            own[i].set_world_time(clock[i])
            assert _same_bits(got[i], own[i].get_waypoint(qs[i], 0.15)), (call, i)
            assert (make.hlps[i].t_world, make.hlps[i].horizon) == (clock[i], 0.8)
        qs = [np.array(x) for x in got]
        clock = clock + np.array([0.4, 0.6])
    assert make.hlps[0].margin_min > MARGIN and make.last_ms == 0.0
    # zero velocities: workspace_hlps' waypoints, whatever the clocks
    still = moving_workspace_hlps(worlds, a["robot"], [np.zeros((2, 3)), np.zeros((1, 3))], seed=11, lookahead=0.15, host=True, mode="seed", **HLP_OPTS)
    plain = workspace_hlps(worlds, a["robot"], seed=11, lookahead=0.15, host=True, mode="seed", **HLP_OPTS)
    qs = [Q_START.copy(), Q_START.copy()]
    for call in range(3):
        still.set_world_times(np.array([0.7, 1.9]) * call)
        x, y = still.get_waypoints([0, 1], qs, [0.3, 0.5]), plain.get_waypoints([0, 1], qs, [0.3, 0.5])
        assert all(_same_bits(p, q) for p, q in zip(x, y)), call
        qs = [np.array(p) for p in x]
    assert still.hlps[0].horizon == default_params(1).duration                          # horizon=None: the plan's duration
    with pytest.raises(ValueError):
        moving_workspace_hlps(worlds, a["robot"], VEL[:1])
    with pytest.raises(ValueError):
        moving_workspace_hlps(worlds, a["robot"], [np.zeros((1, 3)), np.zeros((1, 3))])
    with pytest.raises(ValueError, match="windows that have passed"):
        moving_workspace_hlps(worlds, a["robot"], VEL, mode="keep")


def test_in_a_trial_the_windows_follow_the_worlds_clocks(monkeypatch):
    from armour_amd import ik, ws_planner
    from armour_amd.trials import run_trials
    from armour_amd.ws_planner import moving_workspace_hlps
    a = arriving_wall_world()
    worlds = _trial_worlds(a)
    k = np.zeros(7)
    k[3] = 0.5
    scripts = {0: [(True, k), (False, None), (True, k)], 1: [(True, k), (True, k), (True, k)]}
    seen, seen_ik = [], []
    real, real_ik = ws_planner.plan_workspace_trees, ik.solve_ik
    monkeypatch.setattr(ws_planner, "plan_workspace_trees", lambda *x, **kw: seen.append((kw["t_from"].copy(), kw["t_to"].copy())) or real(*x, **kw))
    monkeypatch.setattr(ik, "solve_ik", lambda *x, **kw: seen_ik.append((kw["t_from"].copy(), kw["t_to"].copy())) or real_ik(*x, **kw))
    make = moving_workspace_hlps(worlds, a["robot"], VEL, horizon=0.8, seed=11, host=True, **HLP_OPTS)
    res = run_trials(worlds, backend=ScriptedMovingPlanner(scripts), audit_on_host=True, velocities=VEL, hlp=make, max_iterations=3, stop_threshold=5)
    recs = [w["records"] for w in res["worlds"]]
    assert [r["executed"] for r in recs[0]] == ["plan", "brake", "plan"] and [r["executed"] for r in recs[1]] == ["plan"] * 3
    assert len(seen) == 3 and len(seen_ik) == 3
    for it, ((t0, t1), (i0, i1)) in enumerate(zip(seen, seen_ik)):
        clocks = np.array([recs[0][it]["t_world"], recs[1][it]["t_world"]])
        assert np.array_equal(t0, clocks) and np.array_equal(t1, clocks + 0.8) and np.array_equal(i0, t0) and np.array_equal(i1, t1), it
    assert [r["t_world"] for r in recs[0]] == [0.0, T_PLAN, T_PLAN + (DUR - T_PLAN)] and [r["t_world"] for r in recs[1]] == [0.0, T_PLAN, T_PLAN + T_PLAN]
