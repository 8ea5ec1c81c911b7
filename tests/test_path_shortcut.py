"""Path shortening, CPU half (include/armour_hip.h armour_path_shortcut / armour_path_shortcut_host, armour_amd/tree_planner.py).

The rule -- validate, prune with descending candidates, refine -- is restated below in numpy from the header's text, on top of the edge
restatement of test_roadmap.py and the wrapped difference of test_tree_plan.py, and the library's host twin has to reproduce it bit for
bit: points are copied or are midpoints (no trigonometry), so the two can only part where a clearance is within rounding (of sin / cos) of
zero, and every comparison first asserts that the host twin's `margin` is above 1e-9.  Then: what every output must satisfy (a subsequence
after one pass, the ends kept, not longer, free on dense samples, a fixed point of one more pass), a case where refine earns its place,
invalid paths, the argument rules and capacities, batching, and the tree HLP's `shortcut` and `mode='seed'` options.  The device is
compared to the host twin in test_path_shortcut_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from test_roadmap import _limits, _robot, _wall_world, config_clearance, edge_samples, geometry, robot_dict
from test_tree_plan import EDGE_STEP, MARGIN, STEP, _fetch_world, _same_bits, _with, wdiff, wrapped_sq
from test_trials import START, ScriptedPlanner, _world

OPTS = dict(step=STEP, edge_step=EDGE_STEP, max_iterations=400, max_nodes=512)
SENTINEL = -7.25


# ----------------------------------------------------------------------------------------------------------- numpy restatement
def length_np(g, path):
    acc = 0.0
    for a, b in zip(path[:-1], path[1:]):
        acc = acc + np.sqrt(wrapped_sq(g, a, b))
    return acc


def shortcut_np(g, Z, path, passes, es=EDGE_STEP, max_points=None):
    """-> dict(status, first_bad, passes_done, path, margin, length_in, length_out), the header's run of one world."""
    margin = [np.inf]
    path = [np.array(p, dtype=np.float64) for p in path]
    max_points = max(2 * len(path) - 1, 2) if max_points is None else max_points

    def free(a, b):
        q, r = edge_samples(g, a, b, es)
        cl = config_clearance(g, q, Z, r)
        S = len(cl)
        hit = np.flatnonzero(~(cl > 0))
        m = int(hit[0]) if hit.size else S
        margin[0] = min(margin[0], np.abs(cl[:min(m, S - 1) + 1]).min())
        return m == S

    def prune(pts):
        out, i, last = [pts[0]], 0, len(pts) - 1
        while i < last:
            j = last
            while j > i + 1 and not free(pts[i], pts[j]):
                j -= 1
            out.append(pts[j])
            i = j
        return out

    def refine(pts):
        out = []
        for a, b in zip(pts[:-1], pts[1:]):
            out.append(a)
            if a.tobytes() != b.tobytes():
                mid = a + 0.5 * wdiff(g, a, b)
                if free(a, mid) and free(mid, b):
                    out.append(mid)
        return out + [pts[-1]]

    res = dict(status=0, first_bad=-1, passes_done=0, path=None, length_in=length_np(g, path), length_out=0.0)
    for s in range(len(path) - 1):
        if not free(path[s], path[s + 1]):
            return dict(res, status=1, first_bad=s, margin=margin[0])
    pts = prune(path)
    done = 1
    for _ in range(1, passes):
        if 2 * len(pts) - 1 > max_points:
            break
        pts = prune(refine(pts))
        done += 1
    return dict(res, passes_done=done, path=np.stack(pts), length_out=length_np(g, pts), margin=margin[0])


# ----------------------------------------------------------------------------------------------------------- helpers
@pytest.fixture(scope="module")
def kinova():
    """The wall world and the host tree planner's raw paths for seeds 1, 2 and 3 in it, computed once."""
    from armour_amd.tree_planner import plan_trees
    robot = _robot("kinova")
    g = geometry(robot_dict(robot))
    lb, ub, _ = _limits(robot)
    start, goal, wall, _ = _wall_world(g)
    res = plan_trees(robot, np.stack([wall[None]] * 3), [start] * 3, [goal] * 3, [1, 2, 3], host=True, **OPTS)
    assert [len(p) for p in res.paths] == [12, 15, 11]
    return dict(robot=robot, g=g, lb=lb, ub=ub, start=start, goal=goal, wall=wall[None], raw=res.paths)


def _short(s, paths, passes, obstacles=None, host=True):
    from armour_amd.tree_planner import shortcut_paths
    return shortcut_paths(s["robot"], np.stack([s["wall"]] * len(paths)) if obstacles is None else obstacles, paths, edge_step=EDGE_STEP, passes=passes, host=host)


def assert_equals_restatement(res, w, ref):
    assert ref["margin"] > MARGIN and res.margin[w] > MARGIN, (ref["margin"], res.margin[w])
    assert (res.status[w], res.first_bad[w], res.passes_done[w]) == (ref["status"], ref["first_bad"], ref["passes_done"])
    assert (res.paths[w] is None) == (ref["path"] is None)
    if ref["path"] is not None:
        assert _same_bits(res.paths[w], ref["path"]), (len(res.paths[w]), len(ref["path"]))
    assert res.length_in[w] == ref["length_in"] and res.length_out[w] == ref["length_out"]
    assert abs(res.margin[w] - ref["margin"]) <= 1e-12


def plate_world(g, start, d, factor=1.7):
    """A world in which no point of a long path can be dropped: a plate just below the box of link 0, and a path that turns joint 0 alone
    by d per point.  Link 0 turns about the vertical, so its clearance to the plate is the gap whatever the angle; with an edge_step so
    large that every edge is one sub-segment, the edge's enlargement of link 0 is rho_00 |D_0| / 2, and the gap of `factor` times one
    step's enlargement lets edges of up to `factor` steps through and no longer one.  -> (obstacles [1,12], path(P) -> [P,n])"""
    from test_roadmap import link_boxes
    _, Rs, X = link_boxes(g, start[None])
    bottom = X[0, 0, 2] - np.abs(Rs[0, 0][2]) @ g["h"][0]
    gap = factor * g["rho"][0][0] * d / 2
    plate = np.array([[0, 0, bottom - gap - 0.01, 0.3, 0, 0, 0, 0.3, 0, 0, 0, 0.01]])

    def path(P):
        out = np.repeat(start[None], P, 0)
        out[:, 0] = np.arange(P) * d
        return out
    return plate, path


def _is_subsequence(short, long):
    k = 0
    for p in short:
        while k < len(long) and long[k].tobytes() != p.tobytes():
            k += 1
        if k == len(long):
            return False
        k += 1
    return True


# ----------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("passes", [1, 2])
def test_host_twin_equals_the_numpy_restatement_on_the_wall_world(kinova, passes):
    s = kinova
    res = _short(s, s["raw"], passes)
    for w in range(3):
        ref = shortcut_np(s["g"], s["wall"], s["raw"][w], passes)
        assert_equals_restatement(res, w, ref)
        assert ref["status"] == 0 and ref["passes_done"] == passes and 2 < len(ref["path"]) < len(s["raw"][w])       # shorter, and the wall still bites


def test_host_twin_equals_the_numpy_restatement_on_fetch():
    from armour_amd.tree_planner import plan_trees, shortcut_paths
    s = _fetch_world()
    raw = plan_trees(s["robot"], s["wall"], [s["start"]], [s["goal"]], [1], host=True, **OPTS).paths[0]
    assert len(raw) > 2
    for passes in (1, 2):
        res = shortcut_paths(s["robot"], s["wall"], [raw], edge_step=EDGE_STEP, passes=passes, host=True)
        assert_equals_restatement(res, 0, shortcut_np(s["g"], s["wall"], raw, passes))


def test_properties_of_the_shortened_paths(kinova):
    s = kinova
    g = s["g"]
    one, two = _short(s, s["raw"], 1), _short(s, s["raw"], 2)
    assert (one.margin > MARGIN).all() and (two.margin > MARGIN).all()
    rng = np.random.default_rng(5)
    for w in range(3):
        assert _is_subsequence(one.paths[w], s["raw"][w])                                # one pass only drops points
        for res in (one, two):
            path = res.paths[w]
            assert _same_bits(path[0], s["start"]) and _same_bits(path[-1], s["goal"])
            assert res.length_in[w] == length_np(g, s["raw"][w])
            assert res.length_out[w] <= res.length_in[w] * (1 + 1e-12)
            for a, b in zip(path[:-1], path[1:]):
                t = np.sort(rng.random(200))
                assert config_clearance(g, a + t[:, None] * wdiff(g, a, b), s["wall"]).min() > 0, w
    again = _short(s, one.paths, 1)
    assert all(_same_bits(again.paths[w], one.paths[w]) for w in range(3))               # a pruned path is a fixed point of prune


def _corner_path(s):
    """start -> corner -> goal around the wall: halfway, with the shoulder swung 2 rad back -- about twice as far as the wall asks for, so
    that both legs are free, the straight edge is not, and an edge from an end to the other leg's midpoint is (found by trying corners on
    the CPU against the restatement below)"""
    corner = 0.5 * (s["start"] + s["goal"])
    corner[1] -= 2.0
    return np.stack([s["start"], corner, s["goal"]])


def test_refine_earns_its_place(kinova):
    """Prune alone cannot cut a corner whose two legs are the only edges between the given points; with the legs' midpoints it can."""
    s = kinova
    path = _corner_path(s)
    ref1, ref2 = (shortcut_np(s["g"], s["wall"], path, p) for p in (1, 2))
    assert ref1["status"] == 0 and _same_bits(ref1["path"], path)                        # a -> b is blocked: one pass keeps the corner
    assert ref2["passes_done"] == 2 and ref2["length_out"] < 0.95 * ref1["length_out"]   # the restatement first ...
    for passes, ref in ((1, ref1), (2, ref2)):
        assert_equals_restatement(_short(s, [path], passes), 0, ref)                     # ... then the library
    res = _short(s, [path], 2)
    assert res.length_out[0] < 0.95 * res.length_in[0] and not _is_subsequence(res.paths[0], path)


# ----------------------------------------------------------------------------------------------------------- the C ABI
def _raw(s, host, paths=None, W=None, O=1, max_in=None, max_points=64, passes=2, edge_step=EDGE_STEP, obstacles=None, counts=None):
    """armour_path_shortcut(_host) itself on the wall world, every argument replaceable -> (rc, status, points, first_bad, passes_done, out)"""
    from armour_amd import _lib
    L = _lib.load()
    n = s["robot"].num_factors
    paths = s["raw"] if paths is None else paths
    rows = len(paths)
    W = rows if W is None else W
    cnt = np.array([len(p) for p in paths] if counts is None else counts, dtype=np.int32)
    max_in = max(len(p) for p in paths) if max_in is None else max_in
    padded = np.zeros((rows, max(max_in, max(len(p) for p in paths)), n))
    for w, p in enumerate(paths):
        padded[w, :len(p)] = p
    obstacles = np.ascontiguousarray(np.stack([s["wall"]] * rows) if obstacles is None else obstacles, dtype=np.float64)
    status, points, first_bad, passes_done = (np.full(rows, -5, dtype=np.int32) for _ in range(4))
    out = np.full((rows, max(max_points, 1), n), SENTINEL)
    li, lo, last = np.zeros(rows), np.zeros(rows), np.zeros(rows)
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    fn = L.armour_path_shortcut_host if host else L.armour_path_shortcut
    rc = fn(C.byref(s["robot"]), None, W, O, obstacles.ctypes.data_as(f64), int(max_in), padded.ctypes.data_as(f64), cnt.ctypes.data_as(i32), float(edge_step),
            int(passes), int(max_points), status.ctypes.data_as(i32), points.ctypes.data_as(i32), first_bad.ctypes.data_as(i32), passes_done.ctypes.data_as(i32),
            out.ctypes.data_as(f64), li.ctypes.data_as(f64), lo.ctypes.data_as(f64), last.ctypes.data_as(f64))
    return rc, status, points, first_bad, passes_done, out


def test_invalid_paths_name_their_first_bad_edge_and_write_nothing(kinova):
    from armour_amd import _lib
    s = kinova
    near = s["start"].copy()
    near[1] -= 0.1                                                                       # a short free step, then the wall
    paths = [np.stack([s["start"], s["goal"]]), np.stack([s["start"], near, s["goal"]]), s["raw"][0]]
    refs = [shortcut_np(s["g"], s["wall"], p, 2) for p in paths]
    assert [(r["status"], r["first_bad"]) for r in refs] == [(1, 0), (1, 1), (0, -1)] and min(r["margin"] for r in refs) > MARGIN
    rc, status, points, first_bad, passes_done, out = _raw(s, True, paths=paths)
    assert rc == _lib.OK and list(status) == [1, 1, 0] and list(first_bad) == [0, 1, -1] and list(points[:2]) == [0, 0] and list(passes_done) == [0, 0, 2]
    assert (out[:2] == SENTINEL).all()                                                   # the invalid worlds' rows are untouched
    assert _same_bits(out[2, :points[2]], refs[2]["path"]) and (out[2, points[2]:] == SENTINEL).all()
    res = _short(s, paths, 2)
    assert res.paths[0] is None and res.paths[1] is None and list(res.length_out[:2]) == [0.0, 0.0] and res.length_in[0] == refs[0]["length_in"]


@pytest.mark.parametrize("host", [False, True])
def test_bad_arguments_are_refused_before_a_device_is_touched(kinova, host):
    """The device entry too answers EINVAL, not EDEVICE, on a machine without a device: the checks come first."""
    from armour_amd import _lib
    s = kinova
    two = [np.stack([s["start"], s["goal"]])]
    long = [np.linspace(s["start"], s["goal"], _lib.SHORTCUT_MAX_POINTS + 1)]
    bad = [dict(O=257, obstacles=np.zeros((3, 257, 12))), dict(W=-1), dict(counts=[1, 15, 11]), dict(counts=[12, 16, 11]), dict(max_in=14),
           dict(paths=long, max_in=_lib.SHORTCUT_MAX_POINTS + 1), dict(max_in=_lib.SHORTCUT_MAX_POINTS + 1), dict(max_points=1),
           dict(max_points=_lib.SHORTCUT_MAX_POINTS + 1), dict(passes=0), dict(passes=_lib.SHORTCUT_MAX_PASSES + 1), dict(edge_step=0.0), dict(edge_step=-0.05),
           dict(edge_step=np.nan), dict(edge_step=np.inf), dict(paths=[_with(two[0], 9, np.nan)]), dict(paths=[_with(two[0], 3, np.inf)]),
           dict(paths=two, obstacles=_with(s["wall"][None], 0, np.nan))]
    for kw in bad:
        assert _raw(s, host, **kw)[0] == _lib.EINVAL, kw
    assert _raw(s, host, W=0)[0] == _lib.OK                # no world: a success that does nothing, with or without a device
    assert _raw(s, host, edge_step=1e-9)[0] == _lib.ECAPACITY                             # an edge could have more sub-segments than a prefix walks


def test_capacity_and_the_refine_skip(kinova):
    from armour_amd import _lib
    s = kinova
    ref = [shortcut_np(s["g"], s["wall"], p, 1) for p in s["raw"]]
    pruned = [len(r["path"]) for r in ref]
    rc, status, points, _, passes_done, out = _raw(s, True, passes=1, max_points=max(pruned) - 1)
    assert rc == _lib.ECAPACITY and list(points) == pruned and list(status) == [0, 0, 0]   # points complete
    for w in range(3):
        if pruned[w] == max(pruned):
            assert (out[w] == SENTINEL).all()                                             # unwritten
        else:
            assert _same_bits(out[w, :pruned[w]], ref[w]["path"])
    # max_points = the longest pruned path: it fits, but 2 count - 1 does not, so its refine and the passes after it are skipped
    room = max(pruned)
    rc, status, points, _, passes_done, out = _raw(s, True, passes=3, max_points=room)
    assert rc == _lib.OK
    for w in range(3):
        want = shortcut_np(s["g"], s["wall"], s["raw"][w], 3, max_points=room)
        assert want["margin"] > MARGIN and passes_done[w] == want["passes_done"] and _same_bits(out[w, :points[w]], want["path"])
    assert 1 in list(passes_done) and all(2 * p - 1 > room for p, d in zip(pruned, passes_done) if d == 1)


def test_a_batch_equals_its_worlds_one_by_one_and_duplicates_are_handled(kinova):
    from armour_amd.scenes import FAR_BOX
    s = kinova
    dup = np.repeat(s["raw"][1], [1, 2, 1, 3] + [1] * (len(s["raw"][1]) - 4), axis=0)     # consecutive equal points inside the path
    still = np.stack([s["start"]] * 3)                                                    # a path that is one point
    paths = [s["raw"][0], dup, s["raw"][2], still]
    obs = np.stack([s["wall"]] * 3 + [FAR_BOX[None]])
    batch = _short(s, paths, 2, obstacles=obs)
    assert (batch.margin > MARGIN).all() and list(batch.status) == [0] * 4
    for w in range(4):
        one = _short(s, [paths[w]], 2, obstacles=obs[w:w + 1])
        assert _same_bits(batch.paths[w], one.paths[0]) and batch.margin[w] == one.margin[0]
        assert (batch.passes_done[w], batch.length_in[w], batch.length_out[w]) == (one.passes_done[0], one.length_in[0], one.length_out[0])
    assert _same_bits(batch.paths[1], _short(s, [s["raw"][1]], 2).paths[0])                                        # the duplicates change nothing
    assert all(a.tobytes() != b.tobytes() for a, b in zip(batch.paths[1][:-1], batch.paths[1][1:]))                 # no zero-length segment
    assert _same_bits(batch.paths[3], still[[0, 2]]) and batch.length_out[3] == 0.0                                 # ... unless the whole path is one
    assert_equals_restatement(batch, 1, shortcut_np(s["g"], s["wall"], dup, 2))
    assert_equals_restatement(batch, 3, shortcut_np(s["g"], FAR_BOX[None], still, 2))


# ----------------------------------------------------------------------------------------------------------- the HLP
def test_the_hlp_shortens_and_reuses_its_path(kinova, monkeypatch):
    from armour_amd import tree_planner
    from armour_amd.roadmap import waypoint_along
    from armour_amd.scenes import CONTINUOUS
    from armour_amd.tree_planner import TreeHLP, call_seed, plan_trees
    s = kinova
    g, la = s["g"], 0.3
    raw = plan_trees(s["robot"], s["wall"], [s["start"]], [s["goal"]], [call_seed(11, 0, 0)], host=True, **OPTS)
    assert raw.margin[0] > MARGIN and len(raw.paths[0]) > 2
    grown = []
    real = tree_planner.plan_trees
    monkeypatch.setattr(tree_planner, "plan_trees", lambda *a, **kw: grown.append(1) or real(*a, **kw))
    # the defaults are what they were: the waypoint along the raw path
    plain = TreeHLP(s["robot"], s["wall"], s["goal"], seed=11, host=True, **OPTS)
    assert _same_bits(plain.get_waypoint(s["start"], la), waypoint_along(raw.paths[0], s["start"], la, CONTINUOUS))
    assert (plain.shortcut, plain.mode, plain.reused, plain.calls, len(grown)) == (0, "new", 0, 1, 1) and _same_bits(plain.path, raw.paths[0])
    # shortcut = 2: along the restatement's shortened path
    ref = shortcut_np(g, s["wall"], raw.paths[0], 2)
    assert ref["margin"] > MARGIN and len(ref["path"]) < len(raw.paths[0])
    short = TreeHLP(s["robot"], s["wall"], s["goal"], seed=11, host=True, shortcut=2, **OPTS)
    assert _same_bits(short.get_waypoint(s["start"], la), waypoint_along(ref["path"], s["start"], la, CONTINUOUS)) and _same_bits(short.path, ref["path"])
    assert short.margin_min > MARGIN
    # mode = 'seed', a second call from a point on the first path: the path is reused, no tree grows
    seed = TreeHLP(s["robot"], s["wall"], s["goal"], seed=11, host=True, shortcut=2, mode="seed", **OPTS)
    q1 = seed.get_waypoint(s["start"], la)
    assert _same_bits(q1, waypoint_along(ref["path"], s["start"], la, CONTINUOUS)) and seed.reused == 0
    before = len(grown)
    offer = np.vstack([q1[None], ref["path"][1:]])
    ref2 = shortcut_np(g, s["wall"], offer, 2)
    assert ref2["status"] == 0 and ref2["margin"] > MARGIN
    q2 = seed.get_waypoint(q1, la)
    assert (seed.reused, seed.calls, len(grown)) == (1, 2, before) and _same_bits(seed.path, ref2["path"])
    assert _same_bits(q2, waypoint_along(ref2["path"], q1, la, CONTINUOUS))
    # ... and from a point whose edge to the path is blocked: one tree grows, with the third call's seed
    away = s["start"].copy()
    away[0] = 0.5                                                                        # the kept path leaves the other way round: the wall is between
    assert shortcut_np(g, s["wall"], np.vstack([away[None], seed.path[1:]]), 2)["first_bad"] == 0
    q3 = seed.get_waypoint(away, la)
    own = real(s["robot"], s["wall"], [away], [s["goal"]], [call_seed(11, 0, 2)], host=True, **OPTS)
    want = shortcut_np(g, s["wall"], own.paths[0], 2)["path"]
    assert (seed.reused, seed.calls, len(grown)) == (1, 3, before + 1) and _same_bits(seed.path, want) and _same_bits(q3, waypoint_along(want, away, la, CONTINUOUS))
    with pytest.raises(ValueError):
        TreeHLP(s["robot"], s["wall"], s["goal"], mode="keep")


def test_trials_batched_and_per_world_give_the_same_waypoints_under_seed_mode(kinova):
    from armour_amd.tree_planner import tree_hlps
    from armour_amd.trials import run_trials
    s = kinova
    assert _same_bits(START, s["start"])
    walled = _world(0, START, s["goal"], lookahead=0.3)
    walled[1]["obstacles"] = np.vstack([walled[1]["obstacles"], s["wall"]])             # (the scripted backend knows a world by its first box)
    worlds = [walled, _world(1, START, s["goal"], lookahead=0.5)]
    k = np.zeros(7)
    k[3] = 0.5
    scripts = {0: [(True, k), (True, k), (False, None)], 1: [(True, k)]}
    res, makes = {}, {}
    for batched in (True, False):
        makes[batched] = tree_hlps(worlds, s["robot"], seed=11, host=True, batched=batched, shortcut=2, mode="seed", **OPTS)
        res[batched] = run_trials(worlds, backend=ScriptedPlanner(scripts), audit_on_host=True, hlp=makes[batched], max_iterations=3, stop_threshold=5)
    for i, (wa, wb) in enumerate(zip(res[True]["worlds"], res[False]["worlds"])):
        assert len(wa["records"]) == len(wb["records"]) == 3
        for c, (ra, rb) in enumerate(zip(wa["records"], wb["records"])):
            assert _same_bits(ra["q_des"], rb["q_des"]) and _same_bits(ra["q0"], rb["q0"]), (i, c)
    for i in range(2):
        a, b = makes[True].hlps[i], makes[False].hlps[i]
        assert (a.calls, a.reused) == (b.calls, b.reused) == (3, 2) and _same_bits(a.path, b.path) and a.margin_min > MARGIN
    assert makes[True].last_ms == 0.0                                                    # (the host route has no launches to time)
