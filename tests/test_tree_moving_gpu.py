"""Moving obstacles in the tree planner and the path shortener on the MI355X (armour_tree_plan_moving, armour_path_shortcut_moving): the
device against the host twins bit for bit -- the host twins are tied to the numpy restatement of the window rule in test_tree_moving.py.
As in test_tree_plan_gpu.py a comparison is made only where the host twin's `margin` is above 1e-9, asserted first.  Shapes are the small
ones of test_tree_plan_gpu.py / test_path_shortcut_gpu.py (400 iterations, 512 nodes, W <= 6, the wall world), chosen to reach every path of
the moving instantiations: the obstacle split with the moving stride (O = 5 and 14 on short edges, O = 1 without a split, a shortener list
that fills under half the block), the raised dynamic LDS at O = 256, and a static launch before and after a moving one."""
import ctypes as C

import numpy as np
import pytest

from test_path_shortcut import _corner_path
from test_path_shortcut_gpu import assert_same
from test_tree_moving import OPTS, WINDOWS, _plan, _short, moving_worlds, scene
from test_tree_plan import EDGE_STEP, MARGIN, STEP, _same_bits, assert_same_plans, box_at_link
from test_trials_moving import GPU_SEED, GPU_WORLDS, seeded_velocities

SOLVE = dict(tolerance=1e-7, max_iterations=100)      # tests/test_reference_scenes.py
SIX = WINDOWS + ((0.3, 0.9), (2.0, 2.0), (-0.5, 0.0))


@pytest.fixture(scope="module")
def kinova():
    return scene("kinova")


def both_plans(s, obs, vel, windows, seeds):
    """(device, host twin) of one moving plan_trees call with trees, compared; the host run's margins are asserted first"""
    host = _plan(s, obs, vel, windows, seeds)
    assert (host.margin > MARGIN).all(), host.margin
    dev = _plan(s, obs, vel, windows, seeds, host=False)
    for w in range(obs.shape[0]):
        assert_same_plans(dev, w, host, w)
    assert dev.ms > 0.0 and dev.margin is None
    return dev, host


def both_short(s, obs, vel, windows, paths, passes=2):
    host = _short(s, obs, vel, windows, paths, passes=passes)
    assert (host.margin > MARGIN).all(), host.margin
    dev = _short(s, obs, vel, windows, paths, passes=passes, host=False)
    assert_same(dev, host, range(len(paths)))
    assert np.array_equal(dev.status, host.status) and np.array_equal(dev.first_bad, host.first_bad) and np.array_equal(dev.passes_done, host.passes_done)
    assert dev.ms > 0.0 and dev.margin is None
    return dev, host


def six_worlds(s):
    """six moving worlds with different windows and velocities; in the fifth a box sits on the start (and drifts), the sixth is empty"""
    from armour_amd.scenes import FAR_BOX
    obs, vel = moving_worlds(s, 3, W=6)
    obs[4, 1] = box_at_link(s["g"], s["start"])
    vel[4, 1] *= 0.1
    obs[5] = FAR_BOX
    return obs, vel


@pytest.fixture(scope="module")
def mixed(kinova):
    obs, vel = six_worlds(kinova)
    dev, host = both_plans(kinova, obs, vel, SIX, [1, 2, 3, 4, 5, 6])
    return dict(obs=obs, vel=vel, dev=dev, host=host)


@pytest.mark.gpu
def test_mixed_batch_of_plans_equals_the_host_twin(kinova, mixed):
    host = mixed["host"]
    print("status", list(host.status), "iterations", list(host.iterations), "count", host.count.tolist())
    assert list(host.status[4:]) == [2, 1] and host.iterations[5] == 0 and (host.status[:4] == 1).sum() >= 3 and (host.iterations[:4] > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [1, 2])
def test_mixed_batch_of_paths_equals_the_host_twin(kinova, mixed, passes):
    """the found paths of the mixed batch in their worlds and windows; the direct edge, which the wall blocks; the direct edge in the empty world"""
    s, host = kinova, mixed["host"]
    direct = np.stack([s["start"], s["goal"]])
    found = [w for w in range(4) if host.paths[w] is not None]
    worlds = found + [0, 5]
    paths = [host.paths[w] for w in found] + [direct, direct]
    dev, twin = both_short(s, mixed["obs"][worlds], mixed["vel"][worlds], [SIX[w] for w in worlds], paths, passes=passes)
    k = len(found)
    assert list(twin.status) == [0] * k + [1, 0] and list(twin.first_bad[k:]) == [0, -1] and list(twin.passes_done) == [passes] * k + [0, passes]
    assert any(len(twin.paths[i]) < len(paths[i]) for i in range(k))


@pytest.mark.gpu
def test_zero_velocity_on_the_device_is_the_static_device_entry(kinova):
    from armour_amd.tree_planner import plan_trees, shortcut_paths
    s = kinova
    obs, _ = moving_worlds(s, 3)
    zero = np.zeros(obs.shape[:2] + (3,))
    static = plan_trees(s["robot"], obs, [s["start"]] * 3, [s["goal"]] * 3, [1, 2, 3], trees=True, **OPTS)
    assert all(p is not None and len(p) > 2 for p in static.paths)
    static_short = shortcut_paths(s["robot"], obs, static.paths, edge_step=EDGE_STEP, passes=2)
    for windows in (((0.0, 0.0),) * 3, ((-3.0, 4.0), (0.25, 0.25), (7.0, 11.5))):
        moving = _plan(s, obs, zero, windows, [1, 2, 3], host=False)
        for w in range(3):
            assert_same_plans(moving, w, static, w)
        short = _short(s, obs, zero, windows, static.paths, host=False)
        assert_same(short, static_short, range(3))


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [0, 4, 13])
def test_the_obstacle_split_offsets_by_the_moving_stride(kinova, extra):
    """O = 1 + extra staged obstacles.  Every extend edge is at most step = 0.5 long, 10 sub-segments of edge_step = 0.05, so with O = 5 and
    O = 14 each sub-segment's obstacles are split over G = min(O, 256 / S) > 1 lanes whose slices begin at o0 * RM_MOV_STRIDE; with O = 1
    there is no split.  The shortener's three-point corner path is 80 work items, under half the block: its validate list is split too."""
    s = kinova
    obs, vel = moving_worlds(s, 5, extra=extra)
    assert obs.shape[1] == 1 + extra
    dev, host = both_plans(s, obs, vel, WINDOWS, [1, 2, 3])
    print("O", 1 + extra, "status", list(host.status), "iterations", list(host.iterations))
    assert (host.iterations > 0).any()
    found = [w for w in range(3) if host.paths[w] is not None]
    assert found
    both_short(s, obs[found], vel[found], [WINDOWS[w] for w in found], [host.paths[w] for w in found])
    # the corner path against the drifting wall and `extra` boxes that keep away from the arm (the far ones of pad_obstacles, moving)
    from armour_amd.scenes import pad_obstacles
    corner = _corner_path(s)
    walls = pad_obstacles(s["wall"], 1 + extra)[None]
    drift = np.zeros((1, 1 + extra, 3))
    drift[0, :, 1] = 0.02
    drift[0, 1:, 2] = 0.3
    dev, host = both_short(s, walls, drift, [(0.0, 0.5)], [corner])
    assert host.status[0] == 0


def _raw_short(s, host, obs, vel, window, path, max_in, max_points):
    """armour_path_shortcut_moving(_host) itself on one world, the path padded to max_in rows -> (rc, the output columns, out rows)"""
    from armour_amd import _lib
    L = _lib.load()
    n = s["robot"].num_factors
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    padded = np.zeros((1, max_in, n))
    padded[0, :len(path)] = path
    counts = np.array([len(path)], dtype=np.int32)
    obs, vel = np.ascontiguousarray(obs, dtype=np.float64), np.ascontiguousarray(vel, dtype=np.float64)
    t0, t1 = np.array([window[0]], dtype=np.float64), np.array([window[1]], dtype=np.float64)
    ints = [np.full(1, -5, dtype=np.int32) for _ in range(4)]
    out, li, lo, last = np.zeros((1, max_points, n)), np.zeros(1), np.zeros(1), np.zeros(1)
    fn = L.armour_path_shortcut_moving_host if host else L.armour_path_shortcut_moving
    rc = fn(C.byref(s["robot"]), None, 1, obs.shape[-2], _lib._dp(obs), _lib._dp(vel), _lib._dp(t0), _lib._dp(t1), max_in, padded.ctypes.data_as(f64),
            counts.ctypes.data_as(i32), EDGE_STEP, 2, max_points, *(x.ctypes.data_as(i32) for x in ints), out.ctypes.data_as(f64), li.ctypes.data_as(f64),
            lo.ctypes.data_as(f64), last.ctypes.data_as(f64))
    return rc, [int(x[0]) for x in ints] + [float(li[0]), float(lo[0])], out[0, :max(int(ints[1][0]), 0)].copy()


@pytest.mark.gpu
def test_the_cap_of_256_obstacles_takes_the_raised_dynamic_lds(kinova):
    """O = 256: 62 KB of staged obstacles, above the 48 KB a block has without asking -- once per entry.  Then the largest sum the shortener
    can launch: max_in = max_points = 1024 rows of path (56 KB with the Kinova's 7 joints) beside them and the kernel's static 21.6 KB,
    139 KB in all, which the MI355X (160 KB of LDS per block) grants: the entry launches and equals the twin."""
    from armour_amd import _lib
    from armour_amd.scenes import pad_obstacles
    s = kinova
    obs = pad_obstacles(s["wall"], 256)[None]
    vel = np.zeros((1, 256, 3))
    vel[0, :, 1] = 0.02
    vel[0, 1:, 2] = 0.3                                                                 # the far boxes move, away from the arm
    window = (0.0, 0.5)
    dev, host = both_plans(s, obs, vel, [window], [1])
    assert host.status[0] == 1 and host.iterations[0] > 0
    both_short(s, obs, vel, [window], [host.paths[0]])
    four = host.paths[0][:4]
    rc_h, cols_h, out_h = _raw_short(s, True, obs, vel, window, four, 1024, 1024)
    rc_d, cols_d, out_d = _raw_short(s, False, obs, vel, window, four, 1024, 1024)
    print("rc", rc_d, _lib.load().armour_last_error().decode() if rc_d else "", cols_d)
    assert rc_h == _lib.OK and cols_h[0] == 0
    assert rc_d == _lib.OK and cols_d == cols_h and _same_bits(out_d, out_h)


@pytest.mark.gpu
def test_a_world_does_not_depend_on_the_other_worlds_of_its_launch(kinova, mixed):
    s, batch = kinova, mixed["dev"]
    worlds = [0, 1, 3]
    for w in worlds:
        one = _plan(s, mixed["obs"][w:w + 1], mixed["vel"][w:w + 1], [SIX[w]], [w + 1], host=False)
        assert_same_plans(batch, w, one, 0)
    paths = [batch.paths[w] for w in worlds]
    assert all(p is not None for p in paths)
    short = _short(s, mixed["obs"][worlds], mixed["vel"][worlds], [SIX[w] for w in worlds], paths, host=False)
    for i, w in enumerate(worlds):
        one = _short(s, mixed["obs"][w:w + 1], mixed["vel"][w:w + 1], [SIX[w]], [paths[i]], host=False)
        assert_same(short, one, [i], [0])


@pytest.mark.gpu
def test_static_then_moving_then_static_in_one_process(kinova):
    from armour_amd.tree_planner import plan_trees, shortcut_paths
    s = kinova
    obs, vel = moving_worlds(s, 3)

    def static():
        plans = plan_trees(s["robot"], obs, [s["start"]] * 3, [s["goal"]] * 3, [1, 2, 3], trees=True, **OPTS)
        return plans, shortcut_paths(s["robot"], obs, plans.paths, edge_step=EDGE_STEP, passes=2)
    before = static()
    moving = _plan(s, obs, vel, WINDOWS, [1, 2, 3], host=False)
    _short(s, obs, vel, WINDOWS, moving.paths, host=False)
    after = static()
    assert any(list(moving.count[w]) != list(before[0].count[w]) for w in range(3))      # the moving call did something else
    for w in range(3):
        assert_same_plans(before[0], w, after[0], w)
    assert_same(before[1], after[1], range(3))


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_trials_in_moving_worlds_record_the_host_twins_waypoints_and_no_proved_hit():
    """Two reference worlds with the 0.05 - 0.2 m/s velocities of test_trials_moving.py: the device planner's waypoints are the host twin's,
    and -- the end-to-end claim, which rests on the solver's tables, not on the planner -- no `plan` or `brake` piece is a proved hit."""
    from armour_amd import scenes
    from armour_amd.planner import kinova_robot
    from armour_amd.tree_planner import moving_tree_hlps
    from armour_amd.trials import run_trials
    robot = kinova_robot()
    all_ws = scenes.reference_worlds()
    idx = GPU_WORLDS[:2]
    ws = [all_ws[i] for i in idx]
    vel = seeded_velocities(ws, idx, GPU_SEED)
    opts = dict(step=STEP, edge_step=EDGE_STEP, max_iterations=400, max_nodes=512, shortcut=2, mode="seed")
    makes = {host: moving_tree_hlps(ws, robot, vel, seed=5, host=host, **opts) for host in (False, True)}
    res = {host: run_trials(ws, hlp=makes[host], velocities=vel, T=64, solve_options=SOLVE, max_iterations=5) for host in (False, True)}
    assert min(h.margin_min for h in makes[True].hlps.values()) > MARGIN
    records = 0
    for wa, wb in zip(res[False]["worlds"], res[True]["worlds"]):
        assert wa["outcome"] == wb["outcome"] and len(wa["records"]) == len(wb["records"]), wa["name"]
        for ra, rb in zip(wa["records"], wb["records"]):
            assert np.array_equal(ra["q_des"], rb["q_des"]) and np.array_equal(ra["q0"], rb["q0"]), (wa["name"], ra["iteration"])
            assert ra["t_world"] == rb["t_world"]
            records += 1
    assert records >= 4
    assert [(h.calls, h.reused) for h in makes[False].hlps.values()] == [(h.calls, h.reused) for h in makes[True].hlps.values()]
    recs = [(w, r) for w in res[False]["worlds"] for r in w["records"]]
    print({k: v for k, v in res[False]["summary"].items() if "_ms" not in k}, [w["outcome"] for w in res[False]["worlds"]],
          [(h.calls, h.reused) for h in makes[False].hlps.values()], "hlp_ms", [round(b["hlp_ms"], 2) for b in res[False]["batches"]])
    bad = [(w["name"], r["iteration"], r["executed"], r["t_hit"]) for w, r in recs if r["executed"] in ("plan", "brake") and r["audit_verdict"] == 1]
    assert not bad, bad
    assert makes[False].last_ms > 0.0 and all("hlp_ms" in b for b in res[False]["batches"])
