"""Batched tree planner, CPU half (include/armour_hip.h armour_tree_plan / armour_tree_plan_host, armour_amd/tree_planner.py).

The rule -- counter hash, nearest node in the total order, steer, free prefix, join -- is restated below in numpy from the header's text, on
top of the node / edge restatement of test_roadmap.py, and the library's host twin has to reproduce it bit for bit: node coordinates involve
no trigonometry, so the two can only part where a clearance is within rounding (of sin / cos) of zero, and every comparison first asserts
that the host twin's `margin` is above 1e-9.  Then: soundness of the found paths on dense samples, the five statuses, the argument rules,
path capacity, batching, and whole trials with a scripted backend.  The device is compared to the host twin in test_tree_plan_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from test_roadmap import _limits, _robot, _wall_world, config_clearance, edge_samples, geometry, link_boxes, robot_dict, wrap
from test_trials import START, ScriptedPlanner, _world

STEP, EDGE_STEP = 0.5, 0.05
M64 = (1 << 64) - 1
MARGIN = 1e-9


# ----------------------------------------------------------------------------------------------------------- numpy restatement
def u(seed, i, j):
    z = (seed + 0x9E3779B97F4A7C15 * (((i << 8) | j) + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return float(z >> 11) * 2.0 ** -53


def wdiff(g, a, b):
    return np.where(g["cont"], wrap(b - a), b - a)


def wrapped_sq(g, a, b):
    acc = 0.0
    for d in wdiff(g, a, b):
        acc = acc + d * d
    return acc


def nearest(g, tree, q):
    return min((wrapped_sq(g, x, q), v) for v, x in enumerate(tree))[::-1]


def plan_np(g, Z, start, goal, seed, lb, ub, step=STEP, es=EDGE_STEP, max_iter=400, cap=512):
    """-> dict(status, iterations, count, nodes, parent, path, margin), the header's run of one world."""
    margin = [np.inf]

    def node_ok(q):
        cl = config_clearance(g, q[None], Z)[0]
        margin[0] = min(margin[0], abs(cl))
        return cl > 0

    def prefix(a, b):
        q, r = edge_samples(g, a, b, es)
        cl = config_clearance(g, q, Z, r)
        S = len(cl)
        hit = np.flatnonzero(~(cl > 0))
        m = int(hit[0]) if hit.size else S
        margin[0] = min(margin[0], np.abs(cl[:min(m, S - 1) + 1]).min())
        return m, S

    out = dict(status=0, iterations=0, count=[0, 0], nodes=[[], []], parent=[[], []], path=None)
    done = lambda **kw: dict(out, margin=margin[0], **kw)
    for q, st in ((start, 2), (goal, 3)):
        if not node_ok(q):
            return done(status=st)
    m, S = prefix(start, goal)
    if m == S:
        return done(status=1, path=np.stack([start, goal]))
    nodes, par = [[start.copy()], [goal.copy()]], [[-1], [-1]]
    trees = lambda: dict(count=[len(nodes[0]), len(nodes[1])], nodes=nodes, parent=par)
    n = len(start)
    for i in range(max_iter):
        a, b = i & 1, 1 - (i & 1)
        if len(nodes[a]) >= cap or len(nodes[b]) >= cap:
            return done(status=4, iterations=i, **trees())
        qr = np.array([lb[j] + u(seed, i, j) * (ub[j] - lb[j]) for j in range(n)])
        v, acc = nearest(g, nodes[a], qr)
        if acc == 0.0:
            continue
        dist = np.sqrt(acc)
        near = nodes[a][v]
        D = wdiff(g, near, qr)
        qn = near + D if dist <= step else near + (step / dist) * D
        m, S = prefix(near, qn)
        if m == 0:
            continue
        if m < S:
            qn = near + (float(m) / float(S)) * wdiff(g, near, qn)
        nodes[a].append(qn)
        par[a].append(v)
        vb, _ = nearest(g, nodes[b], qn)
        other = nodes[b][vb]
        m, S = prefix(other, qn)
        if m == S:
            join = (len(nodes[a]) - 1, vb) if a == 0 else (vb, len(nodes[a]) - 1)
            chain = [[], []]
            for k in range(2):
                x = join[k]
                while x != -1:
                    chain[k].append(nodes[k][x])
                    x = par[k][x]
            return done(status=1, iterations=i + 1, path=np.stack(chain[0][::-1] + chain[1]), **trees())
        if m >= 1:
            nodes[b].append(other + (float(m) / float(S)) * wdiff(g, other, qn))
            par[b].append(vb)
    return done(status=0, iterations=max_iter, **trees())


# ----------------------------------------------------------------------------------------------------------- helpers
def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_equals_restatement(res, w, ref):
    """world w of a plan_trees(trees=True) result against plan_np's dict"""
    assert ref["margin"] > MARGIN, ref["margin"]
    assert res.status[w] == ref["status"] and res.iterations[w] == ref["iterations"], (res.status[w], res.iterations[w], ref["status"], ref["iterations"])
    assert list(res.count[w]) == list(ref["count"])
    for k in range(2):
        c = ref["count"][k]
        assert _same_bits(res.nodes[w, k, :c], np.reshape(ref["nodes"][k], (c, res.nodes.shape[-1])))       # (c = 0: a run that grew no tree)
        assert list(res.parent[w, k, :c]) == list(ref["parent"][k])
    assert (res.paths[w] is None) == (ref["path"] is None)
    if ref["path"] is not None:
        assert _same_bits(res.paths[w], ref["path"])


def assert_same_plans(a, wa, b, wb):
    """world wa of result a and world wb of result b (both with trees=True), bit for bit"""
    assert a.status[wa] == b.status[wb] and a.iterations[wa] == b.iterations[wb], (a.status[wa], a.iterations[wa], b.status[wb], b.iterations[wb])
    assert list(a.count[wa]) == list(b.count[wb]), (a.count[wa], b.count[wb])
    for k in range(2):
        c = a.count[wa, k]
        assert _same_bits(a.nodes[wa, k, :c], b.nodes[wb, k, :c]) and np.array_equal(a.parent[wa, k, :c], b.parent[wb, k, :c]), k
    assert (a.paths[wa] is None) == (b.paths[wb] is None)
    assert a.paths[wa] is None or _same_bits(a.paths[wa], b.paths[wb])


@pytest.fixture(scope="module")
def kinova():
    robot = _robot("kinova")
    g = geometry(robot_dict(robot))
    lb, ub, _ = _limits(robot)
    start, goal, wall, _ = _wall_world(g)
    return dict(robot=robot, g=g, lb=lb, ub=ub, start=start, goal=goal, wall=wall[None])


def _plan(s, seeds, obstacles=None, starts=None, goals=None, host=True, **kw):
    from armour_amd.tree_planner import plan_trees
    W = len(seeds)
    opts = dict(step=STEP, edge_step=EDGE_STEP, max_iterations=400, max_nodes=512, trees=True)
    opts.update(kw)
    return plan_trees(s["robot"], np.stack([s["wall"]] * W) if obstacles is None else obstacles, [s["start"]] * W if starts is None else starts,
                      [s["goal"]] * W if goals is None else goals, seeds, host=host, **opts)


def box_at_link(g, q, link=5):
    """a box about the centre of `link` at configuration q: q collides with it"""
    c = link_boxes(g, np.asarray(q)[None])[2][0, link]
    return np.array([c[0], c[1], c[2], 0.06, 0, 0, 0, 0.06, 0, 0, 0, 0.12])


# ----------------------------------------------------------------------------------------------------------- the rule
def test_the_hash_is_the_splitmix_finaliser_and_stays_inside_the_unit_interval():
    assert u(0, 0, 0) == float(0xE220A8397B1DCDAF >> 11) * 2.0 ** -53          # splitmix64's first output from state 0
    us = np.array([u(s, i, j) for s in (0, 7, M64) for i in (0, 1, 99999) for j in range(8)])
    assert us.min() >= 0.0 and us.max() < 1.0 and len(set(us)) == us.size


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_twin_equals_the_numpy_restatement_on_the_wall_world(kinova, seed):
    s = kinova
    res = _plan(s, [seed])
    assert res.margin[0] > MARGIN, res.margin
    ref = plan_np(s["g"], s["wall"], s["start"], s["goal"], seed, s["lb"], s["ub"])
    assert_equals_restatement(res, 0, ref)
    assert ref["status"] == 1 and ref["iterations"] >= 1 and len(ref["path"]) > 2          # the trees had to grow
    assert abs(res.margin[0] - ref["margin"]) <= 1e-12


def _fetch_world(name="fetch"):
    """name "fetch8" (the 8-factor ABI's preset): the same arm behind a torso yaw joint, so every joint and link index moves up by one"""
    robot = _robot(name)
    g = geometry(robot_dict(robot))
    lb, ub, _ = _limits(robot)
    up = robot.num_factors - 7
    start = np.zeros(robot.num_factors)
    start[1 + up], start[3 + up] = 0.4, 0.8
    goal = start.copy()
    goal[up] = 1.2
    c = link_boxes(g, (0.5 * (start + goal))[None])[2][0, 5 + up]
    wall = np.array([[c[0], c[1], c[2], 0.05, 0, 0, 0, 0.05, 0, 0, 0, 0.10]])
    return dict(robot=robot, g=g, lb=lb, ub=ub, start=start, goal=goal, wall=wall)


def test_host_twin_equals_the_numpy_restatement_on_fetch():
    s = _fetch_world()
    res = _plan(s, [1])
    assert res.margin[0] > MARGIN, res.margin
    ref = plan_np(s["g"], s["wall"], s["start"], s["goal"], 1, s["lb"], s["ub"])
    assert_equals_restatement(res, 0, ref)
    assert ref["status"] == 1 and len(ref["path"]) > 2


@pytest.mark.parametrize("name", ["kinova", "fetch"])
def test_found_paths_are_sound_on_dense_samples(kinova, name):
    s = kinova if name == "kinova" else _fetch_world()
    g = s["g"]
    res = _plan(s, [1, 2, 3])
    rng = np.random.default_rng(5)
    for w in range(3):
        path = res.paths[w]
        assert res.status[w] == 1 and _same_bits(path[0], s["start"]) and _same_bits(path[-1], s["goal"])
        for a, b in zip(path[:-1], path[1:]):
            t = np.sort(rng.random(200))
            Q = a + t[:, None] * wdiff(g, a, b)
            assert config_clearance(g, Q, s["wall"]).min() > 0, (name, w)


def test_statuses(kinova):
    from armour_amd.scenes import FAR_BOX
    s = kinova
    g, start, goal = s["g"], s["start"], s["goal"]
    at_start, at_goal = box_at_link(g, start)[None], box_at_link(g, goal)[None]
    assert config_clearance(g, start[None], at_start)[0] < -MARGIN and config_clearance(g, goal[None], at_goal)[0] < -MARGIN
    assert config_clearance(g, start[None], at_goal)[0] > MARGIN
    res = _plan(s, [1, 1, 1], obstacles=np.stack([at_start, at_goal, FAR_BOX[None]]))
    assert list(res.status) == [2, 3, 1] and list(res.iterations) == [0, 0, 0] and not res.count.any()
    assert res.paths[0] is None and res.paths[1] is None
    assert _same_bits(res.paths[2], np.stack([start, goal]))                     # the empty world: the direct edge, no trees
    none = _plan(s, [1], max_iterations=0)
    assert none.status[0] == 0 and none.iterations[0] == 0 and list(none.count[0]) == [1, 1] and none.paths[0] is None
    assert _same_bits(none.nodes[0, :, 0], np.stack([start, goal])) and list(none.parent[0, :, 0]) == [-1, -1]
    full = _plan(s, [1], max_nodes=2)
    assert full.status[0] == 4 and 1 <= full.iterations[0] <= 2 and full.count[0].max() == 2 and full.paths[0] is None
    ref = plan_np(g, s["wall"], start, goal, 1, s["lb"], s["ub"], cap=2)
    assert (ref["status"], ref["iterations"], ref["count"]) == (4, full.iterations[0], list(full.count[0]))


# ----------------------------------------------------------------------------------------------------------- the C ABI
def _raw(s, host, W=1, O=1, max_points=1024, **kw):
    """armour_tree_plan(_host) itself on W copies of the wall world (seeds 1 .. W), every argument replaceable -> (rc, points [W], path [W,max_points,n])"""
    from armour_amd import _lib
    L = _lib.load()
    n, rows = s["robot"].num_factors, max(W, 1)
    a = dict(lb=s["lb"], ub=s["ub"], obstacles=np.stack([s["wall"]] * rows), starts=np.stack([s["start"]] * rows), goals=np.stack([s["goal"]] * rows),
             step=STEP, edge_step=EDGE_STEP, max_iterations=400, max_nodes=512)
    a.update(kw)
    seeds = np.arange(1, rows + 1, dtype=np.uint64)
    status, iterations, points = (np.zeros(rows, dtype=np.int32) for _ in range(3))
    path = np.zeros((rows, max(max_points, 1), n))
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    lb, ub, obstacles, starts, goals = (np.ascontiguousarray(a[k], dtype=np.float64) for k in ("lb", "ub", "obstacles", "starts", "goals"))
    fn = L.armour_tree_plan_host if host else L.armour_tree_plan
    rc = fn(C.byref(s["robot"]), None, lb.ctypes.data_as(f64), ub.ctypes.data_as(f64), W, O, obstacles.ctypes.data_as(f64), starts.ctypes.data_as(f64),
            goals.ctypes.data_as(f64), seeds.ctypes.data_as(C.POINTER(C.c_uint64)), float(a["step"]), float(a["edge_step"]), int(a["max_iterations"]),
            int(a["max_nodes"]), int(max_points), status.ctypes.data_as(i32), iterations.ctypes.data_as(i32), points.ctypes.data_as(i32), path.ctypes.data_as(f64),
            None, None, None, None)
    return rc, points, path


def _with(x, j, v):
    x = np.array(x, dtype=np.float64)
    x.flat[j] = v
    return x


@pytest.mark.parametrize("host", [False, True])
def test_bad_arguments_are_refused_before_a_device_is_touched(kinova, host):
    """The device entry too answers EINVAL, not EDEVICE, on a machine without a device: the checks come first."""
    from armour_amd import _lib
    s = kinova
    bad = [dict(O=_lib_max_obstacles() + 1, obstacles=np.zeros((1, _lib_max_obstacles() + 1, 12))), dict(W=-1), dict(max_nodes=1), dict(max_nodes=_lib.TREE_MAX_NODES + 1),
           dict(max_iterations=-1), dict(max_iterations=_lib.TREE_MAX_ITERATIONS + 1), dict(step=0.0), dict(step=-0.5), dict(step=np.nan), dict(step=np.inf),
           dict(edge_step=0.0), dict(edge_step=-0.05), dict(edge_step=np.nan), dict(lb=_with(s["lb"], 1, s["ub"][1] + 0.1)), dict(lb=_with(s["lb"], 2, -np.inf)),
           dict(ub=_with(s["ub"], 3, np.inf)), dict(ub=_with(s["ub"], 0, np.nan)), dict(starts=_with(s["start"][None], 4, np.nan)),
           dict(goals=_with(s["goal"][None], 6, np.inf)), dict(obstacles=_with(s["wall"][None], 0, np.nan)), dict(max_points=-1)]
    for kw in bad:
        rc, _, _ = _raw(s, host, **kw)
        assert rc == _lib.EINVAL, kw
    rc, _, _ = _raw(s, host, W=0)                      # no world: a success that does nothing, with or without a device
    assert rc == _lib.OK
    rc, _, _ = _raw(s, host, edge_step=1e-9)           # an edge could have more sub-segments than a prefix walks
    assert rc == _lib.ECAPACITY


def _lib_max_obstacles():
    return 256          # ARMOUR_ROADMAP_MAX_OBSTACLES


def test_a_path_longer_than_max_points_is_ecapacity_with_the_points_complete(kinova):
    from armour_amd import _lib
    s = kinova
    rc, points, path = _raw(s, True, W=3)
    assert rc == _lib.OK and (points > 2).all()
    rc2, points2, path2 = _raw(s, True, W=3, max_points=int(points.max()) - 1)
    assert rc2 == _lib.ECAPACITY and np.array_equal(points, points2)
    for w in range(3):
        if points[w] == points.max():
            assert not path2[w].any()                                                   # unwritten
        else:
            assert _same_bits(path2[w, :points[w]], path[w, :points[w]])
    rc3, points3, path3 = _raw(s, True, W=3, max_points=int(points.max()))
    assert rc3 == _lib.OK and all(_same_bits(path3[w, :points[w]], path[w, :points[w]]) for w in range(3))


def test_a_batch_equals_its_worlds_one_by_one_and_a_seed_repeats(kinova):
    from armour_amd.scenes import FAR_BOX
    s = kinova
    obs = np.stack([s["wall"]] * 3 + [FAR_BOX[None]])
    seeds = [1, 2, 3, 1]
    batch = _plan(s, seeds, obstacles=obs)
    assert (batch.margin > MARGIN).all()
    for w in range(4):
        one = _plan(s, [seeds[w]], obstacles=obs[w:w + 1])
        assert_same_plans(batch, w, one, 0)
        assert one.margin[0] == batch.margin[w]
    again = _plan(s, seeds, obstacles=obs)
    for w in range(4):
        assert_same_plans(batch, w, again, w)
    assert list(batch.iterations[:3]) != [batch.iterations[0]] * 3                      # the seeds matter


# ----------------------------------------------------------------------------------------------------------- trials
def test_trials_take_their_waypoints_from_the_trees(kinova):
    from armour_amd.roadmap import waypoint_along
    from armour_amd.scenes import CONTINUOUS, straight_line_waypoint
    from armour_amd.tree_planner import call_seed, plan_trees, tree_hlps
    from armour_amd.trials import run_trials
    s = kinova
    assert _same_bits(START, s["start"])
    walled = _world(0, START, s["goal"], lookahead=0.3)
    walled[1]["obstacles"] = np.vstack([walled[1]["obstacles"], s["wall"]])             # (the scripted backend knows a world by its first box)
    worlds = [walled, _world(1, START, s["goal"], lookahead=0.5)]
    k = np.zeros(7)
    k[3] = 0.5
    scripts = {0: [(True, k), (True, k), (False, None)], 1: [(True, k)]}
    opts = dict(step=STEP, edge_step=EDGE_STEP, max_iterations=400, max_nodes=512)
    res = {}
    for batched in (True, False):
        make = tree_hlps(worlds, s["robot"], seed=11, host=True, batched=batched, **opts)
        assert hasattr(make, "get_waypoints") == batched
        res[batched] = run_trials(worlds, backend=ScriptedPlanner(scripts), audit_on_host=True, hlp=make, max_iterations=3, stop_threshold=5)
    grown = 0
    for i, (wa, wb) in enumerate(zip(res[True]["worlds"], res[False]["worlds"])):
        assert len(wa["records"]) == len(wb["records"]) == 3
        for c, (ra, rb) in enumerate(zip(wa["records"], wb["records"])):
            assert _same_bits(ra["q_des"], rb["q_des"]) and _same_bits(ra["q0"], rb["q0"]), (i, c)      # batched equals per-world
            own = plan_trees(s["robot"], worlds[i][1]["obstacles"], [ra["q0"]], [s["goal"]], [call_seed(11, i, c)], host=True, **opts)
            assert own.margin[0] > MARGIN
            la = worlds[i][1]["lookahead"]
            want = straight_line_waypoint(ra["q0"], s["goal"], la) if own.paths[0] is None else waypoint_along(own.paths[0], ra["q0"], la, CONTINUOUS)
            assert _same_bits(ra["q_des"], want), (i, c)
            grown += own.paths[0] is not None and len(own.paths[0]) > 2
    assert grown >= 2                                                                    # the walled world's waypoints came from grown trees
    assert call_seed(M64, 1, 5) == ((1 << 32) + 4) and call_seed(0, 3, 2) == (3 << 32) + 2
