"""Resident workspace trees, CPU half (include/armour_hip.h armour_ws_trees_*, armour_amd/ws_planner.py WorkspaceTrees and the 'keep' mode
of the end-effector planner), on the host handle.

The property that defines the entries: after grows of n_1, ..., n_k iterations a world's stored tree, its cumulative iterations and rewires
and the last grow's status, path, path_cost and goal_dist are BIT FOR BIT those of armour_ws_tree_plan_host from the point that planted it
with max_iterations = sum n.  The reference of every comparison is therefore the plan entry's host twin, which test_ws_tree.py holds to a
numpy restatement of the rule.  Then the schedules a handle of several worlds allows, a full tree, a blocked start, an empty instalment,
the refusals (on both kinds of handle: no device is needed to be refused), and the 'keep' planner under run_trials.  The device handle is
compared to the host handle in test_ws_trees_gpu.py.  Nothing here grows more than 512 nodes or 250 iterations."""
import ctypes as C

import numpy as np
import pytest

from test_roadmap import _robot
from test_tree_plan import _same_bits, _with
from test_trials import ScriptedPlanner
from test_ws_tree import GOAL, LB, MARGIN, OPEN, OPTS, START, UB, _marked, _plan, wall_with_window

HANDLE = {k: v for k, v in OPTS.items() if k != "max_iterations"}
INSIDE = np.array([0.5, 0.35, 0.5])                   # inside the wall


def _trees(Z, seeds, host=True, goals=None, **kw):
    from armour_amd.ws_planner import WorkspaceTrees
    Z = np.asarray(Z)
    Z = Z[None] if Z.ndim == 2 else Z
    return WorkspaceTrees(Z, np.stack([GOAL] * Z.shape[0]) if goals is None else goals, seeds, LB, UB, host=host, **dict(HANDLE, **kw))


def assert_equals_plan(res, k, tree, j, ref, w=0):
    """slot k of a grow's result and slot j of a read against world w of a plan_workspace_trees(trees=True) result, bit for bit"""
    for name in ("status", "iterations", "count", "rewires"):
        assert getattr(res, name)[k] == getattr(ref, name)[w], (name, getattr(res, name)[k], getattr(ref, name)[w])
    c = int(ref.count[w])
    assert tree.count[j] == c
    assert _same_bits(tree.nodes[j], ref.nodes[w]) and np.array_equal(tree.parent[j], ref.parent[w]) and _same_bits(tree.node_cost[j], ref.node_cost[w])
    assert _same_bits(res.path_cost[k], ref.path_cost[w]) and _same_bits(res.goal_dist[k], ref.goal_dist[w])
    assert (res.paths[k] is None) == (ref.paths[w] is None)
    assert res.paths[k] is None or _same_bits(res.paths[k], ref.paths[w])


@pytest.fixture(scope="module")
def wall_plans():
    """armour_ws_tree_plan_host on the wall world at 250 iterations, seeds 1, 2, 3: computed once, shared, never written"""
    Z = wall_with_window()
    plans = {seed: _plan(Z, [seed]) for seed in (1, 2, 3)}
    assert all(p.margin[0] > MARGIN for p in plans.values())
    return Z, plans


@pytest.mark.parametrize("split", [(0, 250), (1, 249), (125, 125), (249, 1), (10,) * 25], ids=lambda s: "%dx%d" % (len(s), s[-1]) if len(s) > 2 else "%d+%d" % s)
def test_instalments_equal_one_plan(wall_plans, split):
    Z, plans = wall_plans
    for seed in (1, 2, 3):
        t = _trees(Z, [seed])
        for n in split:
            res = t.grow([0], START[None], n, margin=True)
            assert res.margin[0] > MARGIN
        assert_equals_plan(res, 0, t.read([0]), 0, plans[seed])
        assert res.chain_kept[0] == 0 and res.ms == 0.0
        t.close()


def test_a_resumed_instalment_rewires(wall_plans):
    """a: the single plans at a and at 250 differ in rewires, so the rewiring -- and with it the cost re-derivation -- of the iterations
    a .. 249 runs inside the resumed instalment."""
    Z, plans = wall_plans
    a = 125
    first = _plan(Z, [1], max_iterations=a)
    assert 0 < first.rewires[0] < plans[1].rewires[0]
    t = _trees(Z, [1])
    r1 = t.grow([0], START[None], a)
    assert_equals_plan(r1, 0, t.read([0]), 0, first)
    r2 = t.grow([0], None, 250 - a)                   # planted: no start is read
    assert r2.rewires[0] > r1.rewires[0]
    tree = t.read([0])
    assert_equals_plan(r2, 0, tree, 0, plans[1])
    c = tree.count[0]
    assert (tree.parent[0, :r1.count[0]] >= r1.count[0]).any()      # a node of the first instalment hangs from a node of the second
    for k in range(1, c):                             # the costs are the recursive definition's, bit for bit, after the resumed re-derivation
        D = tree.nodes[0, k] - tree.nodes[0, tree.parent[0, k]]
        assert tree.node_cost[0, k] == tree.node_cost[0, tree.parent[0, k]] + np.sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2])


def test_a_full_tree_takes_no_more_iterations(wall_plans):
    Z, _ = wall_plans
    ref = _plan(Z, [1], max_nodes=64)
    assert ref.count[0] == 64 and ref.iterations[0] < 250
    t = _trees(Z, [1], max_nodes=64)
    r1 = t.grow([0], START[None], 250)
    before = t.read([0])
    assert_equals_plan(r1, 0, before, 0, ref)
    r2 = t.grow([0], START[None], 100)
    after = t.read([0])
    assert_equals_plan(r2, 0, after, 0, ref)
    assert r2.iterations[0] == ref.iterations[0] < 250 + 100
    assert all(_same_bits(getattr(before, k), getattr(after, k)) for k in ("nodes", "node_cost")) and np.array_equal(before.parent, after.parent)
    # a tree that fills up INSIDE a resumed instalment stops at the same iteration
    t2 = _trees(Z, [1], max_nodes=64)
    t2.grow([0], START[None], 30)
    r = t2.grow([0], None, 220)
    assert_equals_plan(r, 0, t2.read([0]), 0, ref)


def test_schedules_of_four_worlds_in_one_handle():
    Z = wall_with_window()
    free = np.vstack([OPEN] * Z.shape[0])
    obs, seeds = np.stack([Z, Z, free, free]), [1, 2, 3, 4]
    t = _trees(obs, seeds)
    starts = np.stack([START] * 4)
    last = {}
    r = t.grow([0, 1, 2, 3], starts, 50)
    last.update({w: (r, w) for w in range(4)})
    one_before = t.read([1])
    r = t.grow([2, 0], starts[:2], 100)               # a permuted subset: slot 0 is world 2
    last.update({2: (r, 0), 0: (r, 1)})
    r = t.grow([3], None, 200)
    last[3] = (r, 0)
    sums = {0: 150, 1: 50, 2: 150, 3: 250}
    trees = t.read([3, 2, 1, 0])                      # read in another order than stored
    for w in range(4):
        ref = _plan(obs[w], [seeds[w]], max_iterations=sums[w])
        assert ref.margin[0] > MARGIN
        assert_equals_plan(last[w][0], last[w][1], trees, 3 - w, ref)
    one_after = t.read([1])
    assert one_before.count[0] == one_after.count[0] > 1
    assert _same_bits(one_before.nodes, one_after.nodes) and _same_bits(one_before.node_cost, one_after.node_cost) and np.array_equal(one_before.parent, one_after.parent)


def test_a_blocked_start_leaves_the_tree_empty_and_a_later_call_plants_it(wall_plans):
    Z, _ = wall_plans
    t = _trees(np.stack([Z, Z]), [1, 1])
    r = t.grow([0, 1], np.stack([INSIDE, START]), 40)
    assert list(r.status) == [2, 0] or list(r.status) == [2, 1]
    assert r.count[0] == 0 and r.iterations[0] == 0 and r.rewires[0] == 0 and r.paths[0] is None and r.path_cost[0] == 0.0
    D = GOAL - INSIDE
    assert r.goal_dist[0] == np.sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2])
    assert t.read([0]).count[0] == 0
    other = np.array([0.15, -0.2, 0.3])
    r = t.grow([0, 1], np.stack([other, INSIDE]), 60)  # world 0 is planted from the new point; world 1 is planted already and ignores its start
    tree = t.read([0, 1])
    ref = _plan(Z, [1], starts=other[None], max_iterations=60)
    assert ref.margin[0] > MARGIN
    assert_equals_plan(r, 0, tree, 0, ref)
    assert_equals_plan(r, 1, tree, 1, _plan(Z, [1], max_iterations=100))


def test_no_iterations_plant_the_root_or_return_the_current_path(wall_plans):
    Z, plans = wall_plans
    t = _trees(Z, [2])
    r0 = t.grow([0], START[None], 0)
    assert_equals_plan(r0, 0, t.read([0]), 0, _plan(Z, [2], max_iterations=0))
    assert r0.count[0] == 1 and _same_bits(r0.paths[0], START[None])
    r1 = t.grow([0], None, 250)
    r2 = t.grow([0], None, 0)
    for k in ("status", "iterations", "count", "rewires", "path_cost", "goal_dist"):
        assert _same_bits(getattr(r1, k), getattr(r2, k)), k
    assert _same_bits(r1.paths[0], r2.paths[0])
    assert_equals_plan(r2, 0, t.read([0]), 0, plans[2])


def test_the_path_never_costs_more_once_the_goal_is_a_node(wall_plans):
    """goal_tol = 0: only a node AT the goal counts, so path_cost is the smallest cost of such a node, and costs can only fall."""
    Z, _ = wall_plans
    fell = 0
    for seed in (1, 5, 6):
        t = _trees(Z, [seed], goal_tol=0.0)
        runs = [t.grow([0], START[None], 25) for _ in range(10)]
        for a, b in zip(runs, runs[1:]):
            assert b.count[0] >= a.count[0] and b.iterations[0] == a.iterations[0] + 25
            if a.status[0] == 1:
                assert b.status[0] == 1 and b.goal_dist[0] == 0.0 and b.path_cost[0] <= a.path_cost[0]
                fell += b.path_cost[0] < a.path_cost[0]
        assert runs[-1].status[0] == 1
    assert fell >= 2


# ----------------------------------------------------------------------------------------------------------- the C ABI
def _create(host, W=1, O=None, **kw):
    """armour_ws_trees_create(_host) itself on W copies of the wall world (seeds 1 .. W), every argument replaceable -> (rc, handle)"""
    from armour_amd import _lib
    L = _lib.load()
    rows = max(W, 1)
    Z = wall_with_window()
    a = dict(HANDLE, lb=LB, ub=UB, obstacles=np.stack([Z] * rows), goals=np.stack([GOAL] * rows))
    a.update(kw)
    O = Z.shape[0] if O is None else O
    seeds = np.arange(1, rows + 1, dtype=np.uint64)
    f64 = C.POINTER(C.c_double)
    lb, ub, obstacles, goals = (np.ascontiguousarray(a[k], dtype=np.float64) for k in ("lb", "ub", "obstacles", "goals"))
    h = C.c_void_p()
    fn = L.armour_ws_trees_create_host if host else L.armour_ws_trees_create
    rc = fn(lb.ctypes.data_as(f64), ub.ctypes.data_as(f64), W, O, obstacles.ctypes.data_as(f64), goals.ctypes.data_as(f64), seeds.ctypes.data_as(C.POINTER(C.c_uint64)),
            *(float(a[k]) for k in ("step", "edge_step", "rewire_radius", "goal_rate", "buffer", "goal_tol")), int(a["max_nodes"]), C.byref(h))
    return rc, h


def _grow(h, worlds, starts, iterations, max_points=512, margin=False, with_starts=True):
    """armour_ws_trees_grow itself -> (rc, points [L], path [L,max_points,3])"""
    from armour_amd import _lib
    L = _lib.load()
    n = len(worlds)
    rows = max(n, 1)
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    wl = np.ascontiguousarray(worlds, dtype=np.int32)
    s = np.ascontiguousarray(starts, dtype=np.float64)
    ints = [np.zeros(rows, dtype=np.int32) for _ in range(5)]
    reals = [np.zeros(rows) for _ in range(2)]
    path = np.zeros((rows, max(max_points, 1), 3))
    mg, ms = np.zeros(rows), C.c_double()
    rc = L.armour_ws_trees_grow(h, n, wl.ctypes.data_as(i32), s.ctypes.data_as(f64) if with_starts else None, int(iterations), int(max_points),
                                *(x.ctypes.data_as(i32) for x in ints[:4]), *(x.ctypes.data_as(f64) for x in reals), path.ctypes.data_as(f64),
                                ints[4].ctypes.data_as(i32), C.byref(ms), mg.ctypes.data_as(f64) if margin else None)
    return rc, ints[2], path


@pytest.mark.parametrize("host", [False, True])
def test_create_refuses_what_the_plan_entry_refuses(host):
    """The same cases as the plan entry's test, from the one copy of the rule -- on the device entry too, without a device."""
    from armour_amd import _lib
    from test_ws_tree import _raw
    Z = wall_with_window()
    bad = [dict(O=257, obstacles=np.zeros((1, 257, 12))), dict(W=-1), dict(max_nodes=0), dict(max_nodes=_lib.WS_MAX_NODES + 1)]
    for k in ("step", "edge_step"):
        bad += [{k: 0.0}, {k: -0.1}, {k: np.nan}, {k: np.inf}]
    for k in ("rewire_radius", "buffer", "goal_tol"):
        bad += [{k: -1e-3}, {k: np.nan}, {k: np.inf}]
    bad += [dict(goal_rate=-0.1), dict(goal_rate=1.1), dict(goal_rate=np.nan)]
    bad += [dict(lb=_with(LB, 1, UB[1] + 0.1)), dict(lb=_with(LB, 2, -np.inf)), dict(ub=_with(UB, 0, np.nan)), dict(goals=_with(GOAL[None], 2, np.inf)),
            dict(obstacles=_with(Z[None], 7, np.nan))]
    bad += [dict(step=0.1, rewire_radius=0.0, edge_step=0.1 / (_lib.WS_MAX_SEGMENTS + 1)), dict(rewire_radius=1.0, edge_step=1.0 / (_lib.WS_MAX_SEGMENTS + 1))]
    for kw in bad:
        rc, h = _create(host, **kw)
        assert rc == _lib.EINVAL and not h.value, kw
        assert _raw(host, **kw)[0] == _lib.EINVAL, kw                                   # the plan entry agrees
    for kw in (dict(), dict(W=0), dict(step=0.1, rewire_radius=0.05, edge_step=0.1 / _lib.WS_MAX_SEGMENTS)):      # accepted (the last: at the cap)
        rc, h = _create(host, **kw)
        assert rc == _lib.OK and h.value, kw
        _lib.load().armour_ws_trees_destroy(h)


@pytest.mark.parametrize("host", [False, True])
def test_grow_and_read_refuse_bad_arguments_before_a_device_is_touched(host):
    """A device handle too answers EINVAL, not EDEVICE, on a machine without a device: create touches none and the checks come first."""
    from armour_amd import _lib
    L = _lib.load()
    rc, h = _create(host, W=3)
    assert rc == _lib.OK
    s3 = np.stack([START] * 3)
    bad = [dict(worlds=[3]), dict(worlds=[-1]), dict(worlds=[0, 1, 0]), dict(worlds=[2, 2]), dict(iterations=-1), dict(iterations=_lib.TREE_MAX_ITERATIONS + 1),
           dict(max_points=-1), dict(starts=_with(s3, 4, np.nan)), dict(starts=_with(s3, 0, np.inf)), dict(with_starts=False)]
    if not host:
        bad.append(dict(margin=True))
    for kw in bad:
        a = dict(worlds=[0, 1, 2], starts=s3, iterations=10)
        a.update(kw)
        rc, _, _ = _grow(h, a.pop("worlds"), a.pop("starts"), a.pop("iterations"), **a)
        assert rc == _lib.EINVAL, kw
    i32 = C.POINTER(C.c_int32)
    for worlds in ([3], [-1], [0, 5]):
        wl = np.array(worlds, dtype=np.int32)
        assert L.armour_ws_trees_read(h, len(wl), wl.ctypes.data_as(i32), None, None, None, None) == _lib.EINVAL
    assert L.armour_ws_trees_read(None, 0, None, None, None, None, None) == _lib.EINVAL
    assert _grow(None, [0], s3[:1], 1)[0] == _lib.EINVAL
    assert _grow(h, [], s3[:0], 10)[0] == _lib.OK                                      # L = 0: a success that does nothing, with or without a device
    count = np.full(3, -1, dtype=np.int32)
    wl = np.array([0, 1, 2], dtype=np.int32)
    assert L.armour_ws_trees_read(h, 3, wl.ctypes.data_as(i32), None, None, None, count.ctypes.data_as(i32)) == _lib.OK and not count.any()   # nothing was grown
    if host:
        assert _grow(h, [0], s3[:1], 5, margin=True)[0] == _lib.OK
        assert _grow(h, [0], _with(s3[:1], 1, np.nan), 5)[0] == _lib.OK                # a planted tree: its start is not read
        assert _grow(h, [0], s3[:1], 5, with_starts=False)[0] == _lib.OK
        assert _grow(h, [1, 0], _with(s3[:2], 1, np.nan), 5)[0] == _lib.EINVAL         # world 1 is still empty
    L.armour_ws_trees_destroy(h)
    # a cumulative count that would pass INT32_MAX: 2^31 iterations cannot be run in a test, so the test hook sets what a world has done
    rc, h = _create(host, W=2)
    assert rc == _lib.OK
    assert L.armour_debug_ws_trees_set_iterations(h, 1, 2**31 - 1 - 10) == _lib.OK
    assert L.armour_debug_ws_trees_set_iterations(h, 2, 0) == _lib.EINVAL and L.armour_debug_ws_trees_set_iterations(h, 0, -1) == _lib.EINVAL
    assert _grow(h, [0, 1], s3[:2], 11)[0] == _lib.EINVAL
    assert _grow(h, [1], s3[:1], _lib.TREE_MAX_ITERATIONS)[0] == _lib.EINVAL
    if host:
        assert _grow(h, [1], s3[:1], 10, max_points=16)[0] == _lib.OK                  # exactly INT32_MAX: accepted
        assert _grow(h, [1], s3[:1], 1)[0] == _lib.EINVAL and _grow(h, [1], s3[:1], 0)[0] == _lib.OK
        assert _grow(h, [0], s3[:1], 250)[0] == _lib.OK                                # every world has a count of its own
    L.armour_ws_trees_destroy(h)


def test_a_path_longer_than_max_points_is_ecapacity_with_the_points_complete():
    from armour_amd import _lib
    rc, h = _create(True, W=3)
    assert rc == _lib.OK
    s3 = np.stack([START] * 3)
    rc, points, path = _grow(h, [0, 1, 2], s3, 250)
    assert rc == _lib.OK and (points > 2).all() and len(set(points)) > 1
    rc2, points2, path2 = _grow(h, [0, 1, 2], s3, 0, max_points=int(points.max()) - 1)
    assert rc2 == _lib.ECAPACITY and np.array_equal(points, points2)
    for w in range(3):
        if points[w] == points.max():
            assert not path2[w].any()                                                   # unwritten
        else:
            assert _same_bits(path2[w, :points[w]], path[w, :points[w]])
    rc3, points3, path3 = _grow(h, [2, 0], s3[:2], 0, max_points=int(points.max()))       # by slot: slot 0 is world 2
    assert rc3 == _lib.OK and _same_bits(path3[0, :points[2]], path[2, :points[2]]) and _same_bits(path3[1, :points[0]], path[0, :points[0]])
    _lib.load().armour_ws_trees_destroy(h)


# ----------------------------------------------------------------------------------------------------------- the HLP layer
def test_trials_keep_their_trees():
    from armour_amd import ik
    from armour_amd.trials import run_trials
    from armour_amd.scenes import reference_worlds
    from armour_amd.ws_planner import WorkspaceTrees, waypoint_along_points, workspace_hlps
    robot = _robot("kinova")
    worlds = _marked(reference_worlds()[:3])
    k = np.zeros(7)
    k[1] = 0.4
    scripts = {w: [(True, k), (True, k), (False, None)] for w in range(3)}
    opts = dict(max_iterations=80, max_nodes=512)
    res, makes, handles = {}, {}, {}
    for batched in (True, False):
        made = WorkspaceTrees.handles_created
        makes[batched] = workspace_hlps(worlds, robot, seed=11, lookahead=0.15, mode="keep", host=True, batched=batched, ik_options=dict(S=8), **opts)
        counts = []
        if batched:                                   # note every world's node count after each call of the batch
            inner = makes[True].get_waypoints

            def noting(indices, qs, lookaheads, inner=inner):
                out = inner(indices, qs, lookaheads)
                counts.append({int(i): makes[True].hlps[int(i)].count for i in indices})
                return out
            makes[True].get_waypoints = noting
        res[batched] = run_trials(worlds, backend=ScriptedPlanner(scripts), audit_on_host=True, hlp=makes[batched], max_iterations=3, stop_threshold=5)
        handles[batched] = WorkspaceTrees.handles_created - made
        if batched:
            assert len(counts) == 3 and all(b[w] >= a[w] > 0 for a, b in zip(counts, counts[1:]) for w in b if w in a)
            assert any(b[w] > a[w] for a, b in zip(counts, counts[1:]) for w in b if w in a)
    assert handles == {True: 1, False: 3}             # ONE handle for all worlds of the batched factory
    assert makes[True].shared["trees"].W == 3
    for i, (wa, wb) in enumerate(zip(res[True]["worlds"], res[False]["worlds"])):
        assert len(wa["records"]) == len(wb["records"]) == 3
        for c, (ra, rb) in enumerate(zip(wa["records"], wb["records"])):
            assert _same_bits(ra["q_des"], rb["q_des"]) and _same_bits(ra["q0"], rb["q0"]), (i, c)      # batched equals per-world
    # every call's waypoint is waypoint_along_points of THAT call's path, and the tree after c calls is the plan of (c + 1) * 80 iterations
    # from the first call's point: replayed on a handle of one's own
    fresh = workspace_hlps(worlds, robot, seed=11, lookahead=0.15, mode="keep", host=True, ik_options=dict(S=8), **opts)
    new = workspace_hlps(worlds, robot, seed=11, lookahead=0.15, mode="new", host=True, ik_options=dict(S=8), **opts)
    for c in range(3):
        qs = [res[True]["worlds"][i]["records"][c]["q0"] for i in range(3)]
        got = fresh.get_waypoints([0, 1, 2], qs, [1.0] * 3)
        for i in range(3):
            h = fresh.hlps[i]
            assert h.margin_min > MARGIN
            assert _same_bits(got[i], res[True]["worlds"][i]["records"][c]["q_des"])
            z = ik.end_effector(robot, qs[i])
            assert _same_bits(h.waypoint, waypoint_along_points(h.path, z, 0.15))
            assert h.calls == c + 1 and h.count >= len(h.path)
        if c == 0:                                    # the same seed, the same start, the same iterations: the same tree as mode='new', so the same waypoint
            first = new.get_waypoints([0, 1, 2], qs, [1.0] * 3)
            for i in range(3):
                assert _same_bits(new.hlps[i].path, fresh.hlps[i].path) and _same_bits(new.hlps[i].waypoint, fresh.hlps[i].waypoint)
                assert _same_bits(first[i], got[i])
    assert _same_bits(fresh.shared["trees"].read([0]).nodes[0, 0], ik.end_effector(robot, res[True]["worlds"][0]["records"][0]["q0"]).reshape(3))
    assert sorted(makes[False].shared) == [0, 1, 2] and all(t.W == 1 for t in makes[False].shared.values())
    for m in (makes[True], makes[False], fresh):
        m.close()
        assert not m.shared


def test_a_keep_planner_whose_start_is_blocked_falls_back_and_plants_later():
    from armour_amd import ik
    from armour_amd.scenes import reference_worlds
    from armour_amd.tree_planner import call_seed
    from armour_amd.ws_planner import START_BLOCKED, WorkspaceTreeHLP, WorkspaceTrees, workspace_box
    robot = _robot("kinova")
    name, p = reference_worlds()[0]
    q0, goal = np.asarray(p["q0"], dtype=np.float64), np.asarray(p["goal"], dtype=np.float64)
    z = ik.end_effector(robot, q0).reshape(3)
    cage = np.array([[z[0], z[1], z[2], 0.02, 0, 0, 0, 0.02, 0, 0, 0, 0.02]])      # a box about the end effector of q0
    lb, ub = workspace_box(robot)
    trees = WorkspaceTrees(cage[None], ik.end_effector(robot, goal).reshape(1, 3), [call_seed(3, 0, 0)], lb, ub, max_nodes=128, host=True)
    with pytest.raises(ValueError):                   # the object does not make its own tree
        WorkspaceTreeHLP(robot, cage, goal, seed=3, host=True, mode="keep", max_iterations=40, max_nodes=128)
    with pytest.raises(ValueError):
        WorkspaceTreeHLP(robot, cage, goal, seed=3, host=True, mode="new", trees=trees)
    hlp = WorkspaceTreeHLP(robot, cage, goal, seed=3, host=True, mode="keep", trees=trees, slot=0, max_iterations=40, max_nodes=128,
                           ik_options=dict(S=4, max_iterations=50))
    q = hlp.get_waypoint(q0, 0.1)
    assert hlp.status == START_BLOCKED and hlp.count == 0 and hlp.fallbacks == 1 and _same_bits(q, goal)
    q1 = q0 + 0.3 * (goal - q0)
    assert np.abs(ik.end_effector(robot, q1).reshape(3) - z).max() > 0.03
    hlp.get_waypoint(q1, 0.1)
    assert hlp.status != START_BLOCKED and hlp.count > 1 and _same_bits(hlp.path[0], ik.end_effector(robot, q1).reshape(3))
    assert hlp.trees.grow([0], None, 0).iterations[0] == 40                            # the blocked call consumed no iteration
    trees.close()
