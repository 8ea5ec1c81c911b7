"""Moving obstacles in the tree planner, the path shortener and TreeHLP, CPU half (include/armour_hip.h armour_tree_plan_moving(_host),
armour_path_shortcut_moving(_host); armour_amd/tree_planner.py plan_trees / shortcut_paths with velocity, t_from, t_to, TreeHLP with a
velocity, moving_tree_hlps).

The rule is the roadmap's window rule and nothing else changes, so the restatements are test_tree_plan.py's plan_np and
test_path_shortcut.py's shortcut_np with their clearance function replaced by test_moving_audit.py's config_clearance_moving at the
window's mid and half.  As there, the host twins have to reproduce the restatement bit for bit wherever their `margin` is above 1e-9.
Then: zero velocity is the static entry, soundness by sampling over the window, a hand-made scene in which only the window decides, the
refusals, and the HLP with its clock.  The device is compared to the host twins in test_tree_moving_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import test_path_shortcut
import test_tree_plan
from test_moving_audit import config_clearance_moving, random_motion
from test_path_audit import CL_TOL
from test_path_shortcut import shortcut_np
from test_roadmap import _limits, _robot, _wall_world, config_clearance, edge_samples, geometry, robot_dict  # noqa: F401  (edge_samples: plan_np's)
from test_roadmap_moving import arriving_box_scene
from test_tree_plan import EDGE_STEP, MARGIN, STEP, _fetch_world, _same_bits, assert_same_plans, box_at_link, plan_np, wdiff
from test_trials import START, _world
from test_trials_moving import DUR, T_PLAN, ScriptedMovingPlanner

OPTS = dict(step=STEP, edge_step=EDGE_STEP, max_iterations=400, max_nodes=512)
WINDOWS = ((0.0, 0.5), (1.25, 1.25), (-0.1, 0.2))      # one per world; the second is an instant
EXTRA = 4                                               # moving boxes beside the wall
SEEDS = {"kinova": 3, "fetch": 1}                       # of the worlds' boxes: all six worlds are FOUND by grown trees, every margin is
                                                        # above 1e-5 (asserted above MARGIN), and five of six plan differently frozen at t = 0


# ----------------------------------------------------------------------------------------------------------- helpers
def window_clearance(V, t_from, t_to):
    """config_clearance's signature with the window rule of one world inside: what plan_np and shortcut_np are handed in place of it"""
    mid, half = 0.5 * (t_from + t_to), 0.5 * (t_to - t_from)
    return lambda g, Q, Z, r=None: config_clearance_moving(g, Q, Z, V, mid, r, half)


def plan_moving_np(monkeypatch, g, Z, V, window, *args, **kw):
    with monkeypatch.context() as m:
        m.setattr(test_tree_plan, "config_clearance", window_clearance(V, *window))
        return plan_np(g, Z, *args, **kw)


def shortcut_moving_np(monkeypatch, g, Z, V, window, path, passes, **kw):
    with monkeypatch.context() as m:
        m.setattr(test_path_shortcut, "config_clearance", window_clearance(V, *window))
        return shortcut_np(g, Z, path, passes, **kw)


def scene(name):
    if name == "fetch":
        return _fetch_world()
    robot = _robot("kinova")
    g = geometry(robot_dict(robot))
    lb, ub, _ = _limits(robot)
    start, goal, wall, _ = _wall_world(g)
    return dict(robot=robot, g=g, lb=lb, ub=ub, start=start, goal=goal, wall=wall[None])


def moving_worlds(s, seed, W=len(WINDOWS), extra=EXTRA, lo=0.05, hi=0.3):
    """(obstacles [W,1+extra,12], velocity [W,1+extra,3]): the scene's wall, drifting slowly, then `extra` small boxes within the arm's reach
    in linear motion at lo..hi m/s"""
    from armour_amd.scenes import boxes_to_obstacles
    rng = np.random.default_rng(seed)
    obs = np.zeros((W, 1 + extra, 12))
    for w in range(W):
        boxes = np.concatenate([rng.uniform([-0.8, -0.8, 0.1], [0.8, 0.8, 1.1], (extra, 3)), rng.uniform(0.02, 0.06, (extra, 3))], axis=1)
        obs[w] = np.vstack([s["wall"], boxes_to_obstacles(boxes)])
    vel = random_motion(rng, obs, lo, hi)
    vel[:, 0] *= 0.1
    return obs, vel


def _plan(s, obs, vel, windows, seeds, host=True, **kw):
    from armour_amd.tree_planner import plan_trees
    W = obs.shape[0]
    t0, t1 = np.array(windows, dtype=np.float64).reshape(-1, 2).T
    return plan_trees(s["robot"], obs, [s["start"]] * W, [s["goal"]] * W, seeds, host=host, trees=True, velocity=vel, t_from=t0, t_to=t1, **dict(OPTS, **kw))


def _short(s, obs, vel, windows, paths, passes=2, host=True, edge_step=EDGE_STEP):
    from armour_amd.tree_planner import shortcut_paths
    t0, t1 = np.array(windows, dtype=np.float64).reshape(-1, 2).T
    return shortcut_paths(s["robot"], obs, paths, edge_step=edge_step, passes=passes, host=host, velocity=vel, t_from=t0, t_to=t1)


def assert_sound_over_the_window(g, path, Z, V, window, tag):
    """every segment of `path`: 20 configurations x 11 times of the window against the obstacles themselves moved to that time"""
    rng = np.random.default_rng(3)
    for k, (a, b) in enumerate(zip(path[:-1], path[1:])):
        t = np.concatenate([[0.0, 1.0], rng.random(18)])
        Q = a + t[:, None] * wdiff(g, a, b)
        for time in np.linspace(window[0], window[1], 11):
            Zt = np.array(Z, dtype=np.float64).reshape(-1, 12).copy()
            Zt[:, 0:3] += V * time
            assert config_clearance(g, Q, Zt).min() > -CL_TOL, (tag, k, time)


@pytest.fixture(scope="module", params=["kinova", "fetch"])
def case(request):
    """A scene, its moving worlds, and the host twins' results in them, computed once: plans (seeds 1, 2, 3) and their shortened paths."""
    s = scene(request.param)
    obs, vel = moving_worlds(s, SEEDS[request.param])
    plans = _plan(s, obs, vel, WINDOWS, [1, 2, 3])
    found = [w for w in range(len(WINDOWS)) if plans.paths[w] is not None]
    short = _short(s, obs[found], vel[found], [WINDOWS[w] for w in found], [plans.paths[w] for w in found]) if found else None
    return dict(s, name=request.param, obs=obs, vel=vel, plans=plans, found=found, short=short)


# ----------------------------------------------------------------------------------------------------------- the rule
def test_host_twins_equal_the_numpy_restatement(case, monkeypatch):
    c, g = case, case["g"]
    grown = 0
    assert (c["plans"].margin > MARGIN).all(), c["plans"].margin
    for w, window in enumerate(WINDOWS):
        ref = plan_moving_np(monkeypatch, g, c["obs"][w], c["vel"][w], window, c["start"], c["goal"], w + 1, c["lb"], c["ub"])
        print(f"{c['name']} world {w}: status {ref['status']}, iterations {ref['iterations']}, margin {ref['margin']:.2e}")
        test_tree_plan.assert_equals_restatement(c["plans"], w, ref)
        assert abs(c["plans"].margin[w] - ref["margin"]) <= 1e-12
        grown += ref["status"] == 1 and len(ref["path"]) > 2
    assert grown >= 2, grown                                                             # the trees had to grow
    assert len(c["found"]) >= 2 and (c["short"].margin > MARGIN).all(), c["short"].margin
    shorter = 0
    for i, w in enumerate(c["found"]):
        ref = shortcut_moving_np(monkeypatch, g, c["obs"][w], c["vel"][w], WINDOWS[w], c["plans"].paths[w], 2)
        test_path_shortcut.assert_equals_restatement(c["short"], i, ref)
        shorter += ref["status"] == 0 and len(ref["path"]) < len(c["plans"].paths[w])
    assert shorter >= 1
    # the same worlds judged frozen at time 0 plan differently somewhere: the motion shows in the result
    from armour_amd.tree_planner import plan_trees
    W = len(WINDOWS)
    frozen = plan_trees(c["robot"], c["obs"], [c["start"]] * W, [c["goal"]] * W, [1, 2, 3], host=True, trees=True, **OPTS)
    assert any(list(frozen.count[w]) != list(c["plans"].count[w]) or frozen.iterations[w] != c["plans"].iterations[w] for w in range(W))


@pytest.mark.parametrize("name", ["kinova", "fetch"])
def test_zero_velocity_is_the_static_entry_for_any_window(name):
    from armour_amd.tree_planner import plan_trees, shortcut_paths
    s = scene(name)
    obs, _ = moving_worlds(s, SEEDS[name])
    W = obs.shape[0]
    zero = np.zeros(obs.shape[:2] + (3,))
    static = plan_trees(s["robot"], obs, [s["start"]] * W, [s["goal"]] * W, [1, 2, 3], host=True, trees=True, **OPTS)
    found = [w for w in range(W) if static.paths[w] is not None]
    assert len(found) >= 2
    paths = [static.paths[w] for w in found]
    static_short = shortcut_paths(s["robot"], obs[found], paths, edge_step=EDGE_STEP, passes=2, host=True)
    for windows in (((0.0, 0.0),) * W, ((-3.0, 4.0), (0.25, 0.25), (7.0, 11.5))):
        moving = _plan(s, obs, zero, windows, [1, 2, 3])
        for w in range(W):
            assert_same_plans(moving, w, static, w)
            assert moving.margin[w] == static.margin[w]
        short = _short(s, obs[found], zero[found], [windows[w] for w in found], paths)
        for key in ("status", "first_bad", "passes_done", "length_in", "length_out", "margin"):
            assert np.array_equal(getattr(short, key), getattr(static_short, key)), key
        assert all(_same_bits(a, b) for a, b in zip(short.paths, static_short.paths))


def test_paths_are_sound_over_their_windows_by_sampling(case):
    c = case
    checked = 0
    for i, w in enumerate(c["found"]):
        for path in (c["plans"].paths[w], c["short"].paths[i]):
            assert _same_bits(path[0], c["start"]) and _same_bits(path[-1], c["goal"])
            assert_sound_over_the_window(c["g"], path, c["obs"][w], c["vel"][w], WINDOWS[w], (c["name"], w))
            checked += len(path) - 1
    print(f"{c['name']}: {checked} segments sampled")
    assert checked >= 10, checked


# ----------------------------------------------------------------------------------------------------------- a hand-made scene
ARRIVING = dict(step=STEP, edge_step=0.1, max_iterations=400, max_nodes=512)


def arriving():
    robot = _robot("kinova")
    g = geometry(robot_dict(robot))
    lb, ub, _ = _limits(robot)
    nodes, _, _, box, vel = arriving_box_scene(robot)
    return dict(robot=robot, g=g, lb=lb, ub=ub, start=nodes[0], goal=nodes[1], box=box, vel=vel)


def arriving_wall():
    """The wall world with its wall 1 m further out from the base at t = 0, moving in at 0.5 m/s: it stands where the wall world has it at
    t = 2.  Start and goal stay free throughout; the direct edge is free while the wall is away."""
    s = scene("kinova")
    wall = s["wall"].copy()
    u = np.array([wall[0, 0], wall[0, 1], 0.0]) / np.hypot(wall[0, 0], wall[0, 1])
    wall[0, 0:3] += 1.0 * u
    return dict(s, box=wall, vel=(-0.5 * u)[None])


def test_the_window_decides_in_the_arriving_box_scene():
    """The box's centre arrives on the edge start -> goal at t = 2: the direct edge is the path on [0, 1] and is not taken on [0, 3] (there
    the grown box covers the start itself).  With the arriving wall the ends stay free, and the late window's path is a grown one."""
    a = arriving()
    two = np.stack([a["start"], a["goal"]])
    early = _plan(a, a["box"][None], a["vel"][None], [(0.0, 1.0)], [1], edge_step=0.1)
    assert early.status[0] == 1 and early.iterations[0] == 0 and _same_bits(early.paths[0], two) and not early.count.any()
    late = _plan(a, a["box"][None], a["vel"][None], [(0.0, 3.0)], [1], edge_step=0.1)
    assert late.margin[0] > MARGIN
    assert late.paths[0] is None or len(late.paths[0]) > 2                               # never the direct edge
    if late.paths[0] is not None:
        assert_sound_over_the_window(a["g"], late.paths[0], a["box"], a["vel"], (0.0, 3.0), "late")
    ok = _short(a, a["box"][None], a["vel"][None], [(0.0, 1.0)], [two], edge_step=0.1)
    assert ok.status[0] == 0 and ok.first_bad[0] == -1 and _same_bits(ok.paths[0], two)
    bad = _short(a, a["box"][None], a["vel"][None], [(0.0, 3.0)], [two], edge_step=0.1)
    assert bad.status[0] == 1 and bad.first_bad[0] == 0 and bad.paths[0] is None and bad.margin[0] > MARGIN
    # both windows in one call, and the instant of arrival itself
    both = _short(a, np.stack([a["box"]] * 3), np.stack([a["vel"]] * 3), [(0.0, 1.0), (0.0, 3.0), (2.0, 2.0)], [two] * 3, edge_step=0.1)
    assert list(both.status) == [0, 1, 1] and list(both.first_bad) == [-1, 0, 0]
    w = arriving_wall()
    windows = [(0.0, 1.0), (1.2, 2.2)]
    res = _plan(w, np.stack([w["box"]] * 2), np.stack([w["vel"]] * 2), windows, [1, 1])
    assert (res.margin > MARGIN).all() and list(res.status) == [1, 1] and res.iterations[0] == 0 and res.iterations[1] > 0
    assert len(res.paths[0]) == 2 and len(res.paths[1]) > 2
    for k in range(2):
        assert_sound_over_the_window(w["g"], res.paths[k], w["box"], w["vel"], windows[k], ("wall", k))


# ----------------------------------------------------------------------------------------------------------- the C ABI
def _raw_plan(s, host, W, O, obs, vel, t0, t1):
    """armour_tree_plan_moving(_host) itself with the pointers as given (None = NULL) -> (rc, status, points, path)"""
    from armour_amd import _lib
    L = _lib.load()
    n, rows = s["robot"].num_factors, max(W, 1)
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    lb, ub, starts, goals = (np.ascontiguousarray(x, dtype=np.float64) for x in (s["lb"], s["ub"], np.stack([s["start"]] * rows), np.stack([s["goal"]] * rows)))
    seeds = np.arange(1, rows + 1, dtype=np.uint64)
    status, iterations, points = (np.zeros(rows, dtype=np.int32) for _ in range(3))
    path = np.zeros((rows, 1024, n))
    fn = L.armour_tree_plan_moving_host if host else L.armour_tree_plan_moving
    rc = fn(C.byref(s["robot"]), None, _lib._dp(lb), _lib._dp(ub), W, O, _lib._dp(obs), _lib._dp(vel), _lib._dp(t0), _lib._dp(t1), _lib._dp(starts), _lib._dp(goals),
            seeds.ctypes.data_as(C.POINTER(C.c_uint64)), STEP, EDGE_STEP, 400, 512, 1024, status.ctypes.data_as(i32), iterations.ctypes.data_as(i32),
            points.ctypes.data_as(i32), path.ctypes.data_as(f64), None, None, None, None)
    return rc, status, points, path


def _raw_short(s, host, W, O, obs, vel, t0, t1):
    """armour_path_shortcut_moving(_host) itself on the two-point path start -> goal per world -> (rc, status, first_bad)"""
    from armour_amd import _lib
    L = _lib.load()
    n, rows = s["robot"].num_factors, max(W, 1)
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    paths = np.ascontiguousarray(np.stack([np.stack([s["start"], s["goal"]])] * rows))
    counts = np.full(rows, 2, dtype=np.int32)
    status, points, first_bad, passes_done = (np.full(rows, -5, dtype=np.int32) for _ in range(4))
    out, li, lo = np.zeros((rows, 8, n)), np.zeros(rows), np.zeros(rows)
    fn = L.armour_path_shortcut_moving_host if host else L.armour_path_shortcut_moving
    rc = fn(C.byref(s["robot"]), None, W, O, _lib._dp(obs), _lib._dp(vel), _lib._dp(t0), _lib._dp(t1), 2, paths.ctypes.data_as(f64), counts.ctypes.data_as(i32),
            EDGE_STEP, 2, 8, status.ctypes.data_as(i32), points.ctypes.data_as(i32), first_bad.ctypes.data_as(i32), passes_done.ctypes.data_as(i32),
            out.ctypes.data_as(f64), li.ctypes.data_as(f64), lo.ctypes.data_as(f64), None)
    return rc, status, first_bad


def refusals(s, host):
    """every refusal the moving entries add to their static forms', and a few of those: ARMOUR_EINVAL each, from both entries"""
    from armour_amd import _lib
    box = np.ascontiguousarray(s["wall"][None])
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
        assert _raw_plan(s, host, *args)[0] == _lib.EINVAL, ("plan", tag)
        assert _raw_short(s, host, *args)[0] == _lib.EINVAL, ("shortcut", tag)
    # the second world's window alone is reversed
    two = (2, 1, np.concatenate([box, box]), np.zeros((2, 1, 3)), np.array([0.0, 2.0]), np.array([1.0, 1.5]))
    assert _raw_plan(s, host, *two)[0] == _lib.EINVAL and _raw_short(s, host, *two)[0] == _lib.EINVAL
    # no world: a success that does nothing, with or without a device
    assert _raw_plan(s, host, 0, 1, box, vel, t0, t1)[0] == _lib.OK and _raw_short(s, host, 0, 1, box, vel, t0, t1)[0] == _lib.OK


@pytest.mark.parametrize("host", [False, True])
def test_bad_arguments_are_refused_before_a_device_is_touched(host):
    """The device entries too answer EINVAL, not EDEVICE, on a machine without a device: the checks come first."""
    refusals(scene("kinova"), host)


def test_no_obstacles_and_the_bindings_argument_rules():
    from armour_amd import _lib
    from armour_amd.tree_planner import plan_trees, shortcut_paths
    s = scene("kinova")
    t0, t1 = np.zeros(1), np.ones(1)
    rc, status, points, path = _raw_plan(s, True, 1, 0, None, None, t0, t1)                # O = 0 with null obstacles and velocity: the empty world
    assert rc == _lib.OK and status[0] == 1 and points[0] == 2 and _same_bits(path[0, :2], np.stack([s["start"], s["goal"]]))
    rc, status, first_bad = _raw_short(s, True, 1, 0, None, None, t0, t1)
    assert rc == _lib.OK and status[0] == 0 and first_bad[0] == -1
    two = [np.stack([s["start"], s["goal"]])]
    vel = np.zeros((1, 1, 3))
    for kw in (dict(velocity=vel), dict(t_from=0.0), dict(t_to=1.0), dict(velocity=vel, t_from=0.0), dict(t_from=0.0, t_to=1.0), dict(velocity=vel, t_to=1.0)):
        with pytest.raises(ValueError):
            plan_trees(s["robot"], s["wall"], [s["start"]], [s["goal"]], [1], host=True, **OPTS, **kw)
        with pytest.raises(ValueError):
            shortcut_paths(s["robot"], s["wall"], two, host=True, **kw)
    with pytest.raises(ValueError):                                                      # two windows for one world: the broadcast refuses
        plan_trees(s["robot"], s["wall"], [s["start"]], [s["goal"]], [1], host=True, velocity=vel, t_from=[0.0, 1.0], t_to=[1.0, 2.0], **OPTS)
    with pytest.raises(ValueError):                                                      # a velocity of another shape
        shortcut_paths(s["robot"], s["wall"], two, host=True, velocity=np.zeros((1, 2, 3)), t_from=0.0, t_to=1.0)
    # scalars broadcast to every world
    a = plan_trees(s["robot"], np.stack([s["wall"]] * 2), [s["start"]] * 2, [s["goal"]] * 2, [1, 2], host=True, trees=True, velocity=np.zeros((2, 1, 3)), t_from=0.5,
                   t_to=1.5, **OPTS)
    b = plan_trees(s["robot"], np.stack([s["wall"]] * 2), [s["start"]] * 2, [s["goal"]] * 2, [1, 2], host=True, trees=True, **OPTS)
    assert_same_plans(a, 0, b, 0), assert_same_plans(a, 1, b, 1)


def test_a_batch_of_three_worlds_equals_its_worlds_one_by_one(case):
    c = case
    for w, window in enumerate(WINDOWS):
        one = _plan(c, c["obs"][w:w + 1], c["vel"][w:w + 1], [window], [w + 1])
        assert_same_plans(c["plans"], w, one, 0)
        assert one.margin[0] == c["plans"].margin[w]
    for i, w in enumerate(c["found"]):
        one = _short(c, c["obs"][w:w + 1], c["vel"][w:w + 1], [WINDOWS[w]], [c["plans"].paths[w]])
        for key in ("status", "first_bad", "passes_done", "length_in", "length_out", "margin"):
            assert getattr(one, key)[0] == getattr(c["short"], key)[i], key
        assert _same_bits(one.paths[0], c["short"].paths[i])


# ----------------------------------------------------------------------------------------------------------- the HLP
def test_seed_mode_keeps_a_path_while_its_window_is_free_and_grows_trees_when_the_wall_arrives(monkeypatch):
    from armour_amd import tree_planner
    from armour_amd.tree_planner import TreeHLP
    a = arriving_wall()
    grown, validated = [], []
    real_plan, real_short = tree_planner.plan_trees, tree_planner.shortcut_paths
    monkeypatch.setattr(tree_planner, "plan_trees", lambda *x, **kw: grown.append((float(kw["t_from"][0]), float(kw["t_to"][0]))) or real_plan(*x, **kw))

    def short(*x, **kw):
        res = real_short(*x, **kw)
        validated.append((float(kw["t_from"][0]), float(kw["t_to"][0]), int(res.status[0])))
        return res
    monkeypatch.setattr(tree_planner, "shortcut_paths", short)
    h = TreeHLP(a["robot"], a["box"], a["goal"], seed=5, host=True, mode="seed", velocity=a["vel"], horizon=0.2, **OPTS)
    two = np.stack([a["start"], a["goal"]])
    h.get_waypoint(a["start"], 0.2)                                                      # window [0, 0.2]: the direct edge, by a (trivial) tree call
    assert (h.calls, h.reused, h.status) == (1, 0, 1) and _same_bits(h.path, two) and grown == [(0.0, 0.2)] and validated == []
    h.set_world_time(0.4)
    h.get_waypoint(a["start"], 0.2)                                                      # window [0.4, 0.6]: still free, the path is kept
    assert (h.calls, h.reused) == (2, 1) and _same_bits(h.path, two) and len(grown) == 1 and validated == [(0.4, 0.4 + 0.2, 0)]
    h.set_world_time(1.4)
    h.get_waypoint(a["start"], 0.2)                                                      # window [1.4, 1.6]: the wall has come over the edge
    assert (h.calls, h.reused) == (3, 1) and validated[-1] == (1.4, 1.4 + 0.2, 1) and grown[-1] == (1.4, 1.4 + 0.2) and len(grown) == 2
    assert h.status == 1 and len(h.path) > 2 and h.margin_min > MARGIN                   # INVALID, and the trees grew a way round
    assert_sound_over_the_window(a["g"], h.path, a["box"], a["vel"], (1.4, 1.6), "grown")
    # the static HLP, which sees the wall where it stands at t = 0, never notices
    monkeypatch.undo()
    frozen = TreeHLP(a["robot"], a["box"], a["goal"], seed=5, host=True, mode="seed", **OPTS)
    for _ in range(3):
        frozen.get_waypoint(a["start"], 0.2)
    assert frozen.reused == 2 and _same_bits(frozen.path, two)
    with pytest.raises(ValueError):
        frozen.set_world_time(1.0)
    with pytest.raises(ValueError):
        TreeHLP(a["robot"], a["box"], a["goal"], horizon=1.0)
    with pytest.raises(ValueError):
        TreeHLP(a["robot"], a["box"], a["goal"], velocity=np.zeros((2, 3)))


def _trial_worlds(s):
    walled = _world(0, START, s["goal"], lookahead=0.3)
    walled[1]["obstacles"] = np.vstack([walled[1]["obstacles"], s["wall"]])             # (the scripted backend knows a world by its first box)
    return [walled, _world(1, START, s["goal"], lookahead=0.5)]


def test_the_factory_batched_equals_per_world_objects_and_zero_velocities_give_tree_hlps_waypoints():
    from armour_amd.tree_planner import TreeHLP, moving_tree_hlps, tree_hlps
    from armour_amd.scenes import pad_obstacles
    s = scene("kinova")
    assert _same_bits(START, s["start"])
    worlds = _trial_worlds(s)
    vel = [np.array([[0.0, 0.0, 0.0], [0.0, 0.05, 0.02]]), np.array([[0.0, 0.0, 0.0]])]     # the marker boxes stand still, the wall drifts
    make = moving_tree_hlps(worlds, s["robot"], vel, horizon=0.8, seed=11, host=True, shortcut=2, mode="seed", **OPTS)
    assert make.last_ms == 0.0 and make.hlps == {}
    own = [TreeHLP(s["robot"], pad_obstacles(p["obstacles"], 2), p["goal"], seed=11, world=i, host=True, shortcut=2, mode="seed",
                   velocity=np.concatenate([vel[i], np.zeros((2 - len(vel[i]), 3))]), horizon=0.8, **OPTS) for i, (_, p) in enumerate(worlds)]
    qs = [START.copy(), START.copy()]
    clock = np.zeros(2)
    for call in range(3):
        make.set_world_times(clock)
        got = make.get_waypoints([0, 1], qs, [0.3, 0.5])
        for i in range(2):
            own[i].set_world_time(clock[i])
            assert _same_bits(got[i], own[i].get_waypoint(qs[i], [0.3, 0.5][i])), (call, i)
            assert (make.hlps[i].t_world, make.hlps[i].horizon) == (clock[i], 0.8)
        qs = [np.array(x) for x in got]
        clock = clock + np.array([0.4, 0.6])
    assert [(make.hlps[i].calls, make.hlps[i].reused) for i in range(2)] == [(own[i].calls, own[i].reused) for i in range(2)]
    assert make.hlps[0].margin_min > MARGIN and make.last_ms == 0.0
    # zero velocities: tree_hlps' waypoints, whatever the clocks
    still = moving_tree_hlps(worlds, s["robot"], [np.zeros((2, 3)), np.zeros((1, 3))], seed=11, host=True, shortcut=2, mode="seed", **OPTS)
    plain = tree_hlps(worlds, s["robot"], seed=11, host=True, shortcut=2, mode="seed", **OPTS)
    from armour_amd.planner import default_params
    qs = [START.copy(), START.copy()]
    for call in range(3):
        still.set_world_times(np.array([0.7, 1.9]) * call)
        a, b = still.get_waypoints([0, 1], qs, [0.3, 0.5]), plain.get_waypoints([0, 1], qs, [0.3, 0.5])
        assert all(_same_bits(x, y) for x, y in zip(a, b)), call
        qs = [np.array(x) for x in a]
    assert still.hlps[0].horizon == default_params(1).duration                          # horizon=None: the plan's duration
    with pytest.raises(ValueError):
        moving_tree_hlps(worlds, s["robot"], vel[:1])
    with pytest.raises(ValueError):
        moving_tree_hlps(worlds, s["robot"], [np.zeros((1, 3)), np.zeros((1, 3))])


def test_in_a_trial_the_windows_follow_the_worlds_clocks(monkeypatch):
    from armour_amd import tree_planner
    from armour_amd.tree_planner import moving_tree_hlps
    from armour_amd.trials import run_trials
    s = scene("kinova")
    worlds = _trial_worlds(s)
    vel = [np.array([[0.0, 0.0, 0.0], [0.0, 0.05, 0.02]]), np.array([[0.0, 0.0, 0.0]])]
    k = np.zeros(7)
    k[3] = 0.5
    scripts = {0: [(True, k), (False, None), (True, k)], 1: [(True, k), (True, k), (True, k)]}
    seen = []
    real = tree_planner.plan_trees
    monkeypatch.setattr(tree_planner, "plan_trees", lambda *x, **kw: seen.append((kw["t_from"].copy(), kw["t_to"].copy())) or real(*x, **kw))
    make = moving_tree_hlps(worlds, s["robot"], vel, horizon=0.8, seed=11, host=True, **OPTS)      # mode='new': one tree call per iteration, both worlds
    res = run_trials(worlds, backend=ScriptedMovingPlanner(scripts), audit_on_host=True, velocities=vel, hlp=make, max_iterations=3, stop_threshold=5)
    recs = [w["records"] for w in res["worlds"]]
    assert [r["executed"] for r in recs[0]] == ["plan", "brake", "plan"] and [r["executed"] for r in recs[1]] == ["plan"] * 3
    assert len(seen) == 3
    for it, (t0, t1) in enumerate(seen):
        clocks = np.array([recs[0][it]["t_world"], recs[1][it]["t_world"]])
        assert np.array_equal(t0, clocks) and np.array_equal(t1, clocks + 0.8), it
    assert [r["t_world"] for r in recs[0]] == [0.0, T_PLAN, T_PLAN + (DUR - T_PLAN)] and [r["t_world"] for r in recs[1]] == [0.0, T_PLAN, T_PLAN + T_PLAN]
