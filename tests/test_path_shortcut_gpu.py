"""Path shortening, device half: armour_path_shortcut on the MI355X against its host twin armour_path_shortcut_host, bit for bit.

The two run the same functions; only sin / cos in the link frames can differ, which can flip a verdict only where a clearance is within
rounding of zero.  So every comparison first asserts that the host twin's `margin` is above 1e-9, and then demands equality of status,
points, first_bad, passes_done and the output path (and of the two lengths, which are sums in index order on both sides).  The host twin
is held to the numpy restatement of the rule in test_path_shortcut.py.  The shapes are the smallest at which the kernel's work lists take
each of their routes: several candidates to a chunk, more candidates than lanes, a candidate longer than a chunk, the obstacle split."""
import numpy as np
import pytest

from test_path_shortcut import _corner_path, kinova, plate_world  # noqa: F401  (the fixture: the wall world and its three raw tree paths)
from test_tree_plan import EDGE_STEP, MARGIN, STEP, _same_bits, wdiff

SOLVE = dict(tolerance=1e-7, max_iterations=100)      # tests/test_reference_scenes.py
HARD = dict(step=STEP, edge_step=EDGE_STEP, max_iterations=1500, max_nodes=2048)


def both(robot, obstacles, paths, passes=2, edge_step=EDGE_STEP):
    """(device, host twin) of one shortcut_paths call, compared; the host run's margins are asserted first"""
    from armour_amd.tree_planner import shortcut_paths
    host = shortcut_paths(robot, obstacles, paths, edge_step=edge_step, passes=passes, host=True)
    assert (host.margin > MARGIN).all(), host.margin
    dev = shortcut_paths(robot, obstacles, paths, edge_step=edge_step, passes=passes)
    assert_same(dev, host, range(len(paths)))
    assert dev.ms > 0.0 and dev.margin is None
    return dev, host


def assert_same(a, b, worlds, wb=None):
    for i, w in enumerate(worlds):
        v = w if wb is None else wb[i]
        assert (a.status[w], a.first_bad[w], a.passes_done[w]) == (b.status[v], b.first_bad[v], b.passes_done[v]), w
        assert (a.paths[w] is None) == (b.paths[v] is None), w
        assert a.paths[w] is None or _same_bits(a.paths[w], b.paths[v]), (w, len(a.paths[w]), len(b.paths[v]))
        assert a.length_in[w] == b.length_in[v] and a.length_out[w] == b.length_out[v], w


def _segments(g, path, edge_step):
    """the largest S over all pairs of the path's points"""
    return max(int(np.ceil(np.abs(wdiff(g, a, b)).max() / edge_step)) for i, a in enumerate(path) for b in path[i + 1:])


def _reference(names):
    from armour_amd import scenes
    ws = dict(scenes.reference_worlds())
    O = max(ws[k]["obstacles"].shape[0] for k in names)
    return (np.stack([scenes.pad_obstacles(ws[k]["obstacles"], O) for k in names]), np.stack([ws[k]["q0"] for k in names]),
            np.stack([ws[k]["goal"] for k in names]))


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [1, 2])
def test_mixed_batch_equals_the_host_twin(kinova, passes):
    """W = 6 in one launch: the three tree paths, a two-point path in the empty world, an invalid path, a path with repeated points."""
    from armour_amd.scenes import FAR_BOX
    s = kinova
    direct = np.stack([s["start"], s["goal"]])
    dup = np.repeat(s["raw"][1], [1, 2, 1, 3] + [1] * (len(s["raw"][1]) - 4), axis=0)
    obs = np.stack([s["wall"]] * 3 + [FAR_BOX[None], s["wall"], s["wall"]])
    dev, host = both(s["robot"], obs, list(s["raw"]) + [direct, direct, dup], passes=passes)
    assert list(host.status) == [0, 0, 0, 0, 1, 0] and list(host.first_bad) == [-1, -1, -1, -1, 0, -1] and list(host.passes_done) == [passes] * 4 + [0, passes]
    assert all(2 < len(host.paths[w]) < len(s["raw"][w]) for w in range(3)) and _same_bits(host.paths[3], direct)


@pytest.mark.gpu
def test_a_long_tree_path_equals_the_host_twin(kinova):
    """hard_7_window's tree path: tens of candidates per anchor, several of them to a chunk and several chunks to an anchor."""
    from armour_amd.tree_planner import plan_trees
    robot = kinova["robot"]
    obs, starts, goals = _reference(["hard_7_window"])
    raw = plan_trees(robot, obs, starts, goals, [7], **HARD).paths[0]
    assert raw is not None and len(raw) == 44
    for passes in (1, 2):
        dev, host = both(robot, obs, [raw], passes=passes)
        assert host.status[0] == 0 and len(host.paths[0]) < len(raw) and host.length_out[0] < host.length_in[0]


@pytest.mark.gpu
def test_more_candidates_than_lanes(kinova):
    """A straight line in the empty world cut into 300 points: the first anchor has 298 candidates, and the answer is its two ends."""
    from armour_amd.scenes import FAR_BOX
    s = kinova
    line = np.linspace(s["start"], s["goal"], 300)
    dev, host = both(s["robot"], FAR_BOX[None][None], [line], passes=2)
    assert _same_bits(dev.paths[0][[0, -1]], line[[0, -1]]) and len(dev.paths[0]) == 2 and dev.passes_done[0] == 2
    # the same line through the wall: 299 edges to validate, the bad one in the middle
    dev, host = both(s["robot"], s["wall"][None], [line], passes=2)
    assert host.status[0] == 1 and 0 < host.first_bad[0] < 298
    # a tree path with every edge cut into 30: the first anchor has 299 candidates again, and the wall refuses most of them
    raw = s["raw"][2]
    dense = np.vstack([a + t * wdiff(s["g"], a, b) for a, b in zip(raw[:-1], raw[1:]) for t in np.arange(30) / 30.0] + [raw[-1:]])
    dev, host = both(s["robot"], s["wall"][None], [dense], passes=2)
    assert len(dense) == 301 and host.status[0] == 0 and 2 < len(host.paths[0]) <= len(raw)


@pytest.mark.gpu
def test_refine_moves_more_points_than_lanes_and_a_path_at_the_cap(kinova):
    """300 points of which prune can drop none (test_path_shortcut.plate_world): refine inserts 299 midpoints, so the points move up in two
    steps of 256 and the lists that follow have 598 and 597 candidates.  Then 1024 points, the cap: the path alone is 56 KB of LDS."""
    from armour_amd.scenes import FAR_BOX
    s = kinova
    plate, path = plate_world(s["g"], s["start"], 0.005)
    for passes, points in ((1, 300), (2, 201), (3, 201)):
        dev, host = both(s["robot"], plate, [path(300)], passes=passes, edge_step=10.0)
        assert host.status[0] == 0 and len(host.paths[0]) == points and host.passes_done[0] == passes
    line = np.linspace(s["start"], s["goal"], 1024)
    dev, host = both(s["robot"], FAR_BOX[None][None], [line], passes=2)
    assert len(dev.paths[0]) == 2
    dev, host = both(s["robot"], plate, [path(500)], passes=2, edge_step=10.0)         # 999 points after refine: three steps, near the cap
    assert host.status[0] == 0 and len(host.paths[0]) == 334


@pytest.mark.gpu
def test_a_candidate_longer_than_a_chunk_and_the_obstacle_split(kinova):
    from armour_amd.scenes import FAR_BOX, pad_obstacles
    s = kinova
    fine = 0.01
    assert _segments(s["g"], s["raw"][1], fine) > 256                                   # one candidate crosses a chunk's end
    both(s["robot"], s["wall"][None], [s["raw"][1]], passes=2, edge_step=fine)
    corner = _corner_path(s)
    walls = pad_obstacles(s["wall"], 4)[None]
    assert _segments(s["g"], corner, EDGE_STEP) <= 128 and walls.shape[1] == 4           # one candidate, each sub-segment on several lanes
    dev, host = both(s["robot"], walls, [corner], passes=2)
    assert host.length_out[0] < 0.95 * host.length_in[0]
    assert_same(dev, both(s["robot"], s["wall"][None], [corner], passes=2)[0], [0])      # the far boxes change nothing


@pytest.mark.gpu
def test_a_world_does_not_depend_on_the_other_worlds_of_the_launch(kinova):
    """The first 16 reference worlds, padded to one obstacle count: their tree paths shortened in one launch and in 16 launches."""
    from armour_amd import scenes
    from armour_amd.tree_planner import plan_trees, shortcut_paths
    robot = kinova["robot"]
    names = [name for name, _ in scenes.reference_worlds()[:16]]
    obs, starts, goals = _reference(names)
    plans = plan_trees(robot, obs, starts, goals, np.arange(16, dtype=np.uint64) + 3, step=STEP, edge_step=EDGE_STEP, max_iterations=400, max_nodes=512)
    assert all(p is not None for p in plans.paths) and max(len(p) for p in plans.paths) > 2
    batch, host = both(robot, obs, plans.paths, passes=2)
    for w in range(16):
        one = shortcut_paths(robot, obs[w:w + 1], [plans.paths[w]], edge_step=EDGE_STEP, passes=2)
        assert_same(batch, one, [w], [0])
    assert (host.status == 0).all() and host.length_out.sum() < host.length_in.sum()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_trials_record_the_host_twins_waypoints_under_seed_mode(kinova):
    from armour_amd import scenes
    from armour_amd.tree_planner import tree_hlps
    from armour_amd.trials import run_trials
    robot = kinova["robot"]
    worlds = scenes.reference_worlds()[:4]
    opts = dict(step=STEP, edge_step=EDGE_STEP, max_iterations=400, max_nodes=512, shortcut=2, mode="seed")
    makes = {host: tree_hlps(worlds, robot, seed=5, host=host, **opts) for host in (False, True)}
    res = {host: run_trials(worlds, hlp=makes[host], T=64, solve_options=SOLVE, max_iterations=5) for host in (False, True)}
    assert min(h.margin_min for h in makes[True].hlps.values()) > MARGIN
    records = 0
    for wa, wb in zip(res[False]["worlds"], res[True]["worlds"]):
        assert wa["outcome"] == wb["outcome"] and len(wa["records"]) == len(wb["records"]), wa["name"]
        for ra, rb in zip(wa["records"], wb["records"]):
            assert np.array_equal(ra["q_des"], rb["q_des"]) and np.array_equal(ra["q0"], rb["q0"]), (wa["name"], ra["iteration"])
            records += 1
    assert records >= 4
    assert [h.reused for h in makes[False].hlps.values()] == [h.reused for h in makes[True].hlps.values()]
    assert sum(h.reused for h in makes[True].hlps.values()) >= 1 and all("hlp_ms" in b for r in res.values() for b in r["batches"])
