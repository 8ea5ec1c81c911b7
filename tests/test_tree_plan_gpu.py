"""Batched tree planner, device half: armour_tree_plan on the MI355X against its host twin armour_tree_plan_host, bit for bit.

The two run the same functions; only sin / cos in the link frames can differ, which can flip a verdict only where a clearance is within
rounding of zero.  So every comparison first asserts that the host twin's `margin` -- the smallest |clearance| that decided the run -- is
above 1e-9, and then demands equality of status, iterations, points and path, count, nodes[:count] and parent[:count].  The host twin is
held to the numpy restatement of the rule in test_tree_plan.py."""
import numpy as np
import pytest

from test_roadmap import _robot, _wall_world, geometry, robot_dict
from test_tree_plan import EDGE_STEP, MARGIN, STEP, assert_same_plans, box_at_link

SOLVE = dict(tolerance=1e-7, max_iterations=100)      # tests/test_reference_scenes.py
HARD = dict(step=STEP, edge_step=EDGE_STEP, max_iterations=1500, max_nodes=2048)


@pytest.fixture(scope="module")
def robot():
    return _robot("kinova")


def both(robot, obstacles, starts, goals, seeds, **opts):
    """(device, host twin) of one plan_trees call with trees; the host run's margins are asserted first"""
    from armour_amd.tree_planner import plan_trees
    host = plan_trees(robot, obstacles, starts, goals, seeds, trees=True, host=True, **opts)
    assert (host.margin > MARGIN).all(), host.margin
    return plan_trees(robot, obstacles, starts, goals, seeds, trees=True, **opts), host


def _reference(names):
    from armour_amd import scenes
    ws = dict(scenes.reference_worlds())
    O = max(ws[k]["obstacles"].shape[0] for k in names)
    return (np.stack([scenes.pad_obstacles(ws[k]["obstacles"], O) for k in names]), np.stack([ws[k]["q0"] for k in names]),
            np.stack([ws[k]["goal"] for k in names]))


@pytest.mark.gpu
def test_mixed_batch_equals_the_host_twin(robot):
    """W = 6 in one launch: the wall world with seeds 1, 2, 3, the empty world, a blocked start and a blocked goal."""
    from armour_amd.scenes import FAR_BOX
    g = geometry(robot_dict(robot))
    start, goal, wall, _ = _wall_world(g)
    obs = np.stack([wall[None]] * 3 + [FAR_BOX[None], box_at_link(g, start)[None], box_at_link(g, goal)[None]])
    dev, host = both(robot, obs, [start] * 6, [goal] * 6, [1, 2, 3, 1, 1, 1], step=STEP, edge_step=EDGE_STEP, max_iterations=400, max_nodes=512)
    assert list(host.status) == [1, 1, 1, 1, 2, 3] and (host.iterations[:3] > 0).all() and not host.iterations[3:].any()
    for w in range(6):
        assert_same_plans(dev, w, host, w)
    assert dev.ms > 0.0 and dev.margin is None


@pytest.mark.gpu
@pytest.mark.parametrize("name,status", [("hard_7_window", 1), ("hard_5_inside_box", 0)])
def test_trees_across_the_wave_and_block_boundaries_equal_the_host_twin(robot, name, status):
    """Tree sizes cross 64, 256 and 512 nodes, where the nearest reduction's wave and block boundaries sit."""
    obs, starts, goals = _reference([name])
    dev, host = both(robot, obs, starts, goals, [7], **HARD)
    assert host.status[0] == status and host.count[0].max() > (512 if status == 0 else 64) and host.count[0].sum() > 512
    assert_same_plans(dev, 0, host, 0)


@pytest.mark.gpu
def test_a_full_tree_ends_both_sides_at_the_same_iteration(robot):
    obs, starts, goals = _reference(["hard_7_window"])
    dev, host = both(robot, obs, starts, goals, [7], **dict(HARD, max_nodes=64))
    assert host.status[0] == 4 and host.count[0].max() == 64 and 0 < host.iterations[0] < 1500
    assert_same_plans(dev, 0, host, 0)


@pytest.mark.gpu
def test_a_world_does_not_depend_on_the_other_worlds_of_the_launch(robot):
    """The first 16 reference worlds, padded to one obstacle count, in one launch and in 16 launches."""
    from armour_amd import scenes
    from armour_amd.tree_planner import plan_trees
    names = [name for name, _ in scenes.reference_worlds()[:16]]
    obs, starts, goals = _reference(names)
    seeds = np.arange(16, dtype=np.uint64) + 3
    opts = dict(step=STEP, edge_step=EDGE_STEP, max_iterations=400, max_nodes=512)
    batch, host = both(robot, obs, starts, goals, seeds, **opts)
    for w in range(16):
        one = plan_trees(robot, obs[w:w + 1], starts[w:w + 1], goals[w:w + 1], seeds[w:w + 1], trees=True, **opts)
        assert_same_plans(batch, w, one, 0)
        assert_same_plans(batch, w, host, w)
    assert (host.iterations > 0).any() and (host.status == 1).all()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_trials_record_the_host_twins_waypoints(robot):
    from armour_amd import scenes
    from armour_amd.tree_planner import tree_hlps
    from armour_amd.trials import run_trials
    worlds = scenes.reference_worlds()[:4]
    opts = dict(step=STEP, edge_step=EDGE_STEP, max_iterations=400, max_nodes=512)
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
    assert all("hlp_ms" in b for r in res.values() for b in r["batches"])
