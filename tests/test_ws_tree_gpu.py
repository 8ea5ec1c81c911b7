"""Batched workspace RRT*, device half: armour_ws_tree_plan on the MI355X against its host twin armour_ws_tree_plan_host, bit for bit on
every output.  The two run the same functions and no trigonometry is involved, so nothing but a clearance within rounding of zero could
part them: every comparison first asserts that the host twin's `margin` is above 1e-9.  The host twin is held to the numpy restatement of
the rule in test_ws_tree.py.  The shapes are the smallest at which each part of the kernel can go wrong: a tree that crosses one wave, one
block and two blocks of nodes, a work list of more than one chunk, more candidates than one round, a full tree, no obstacles and more
obstacles than lanes in a wave, a chain with a blocked edge, many rewires in one iteration."""
import numpy as np
import pytest

from test_roadmap import _robot
from test_ws_tree import FAR, GOAL, LB, MARGIN, OPEN, OPTS, START, UB, _box, _plan, assert_same_plans, plan_ws_np, wall_with_window

pytestmark = pytest.mark.gpu


def both(Z, seeds, **kw):
    """(device, host twin) of one plan_workspace_trees call with the trees; the host run's margins are asserted first"""
    host = _plan(Z, seeds, host=True, **kw)
    assert (host.margin > MARGIN).all(), host.margin
    return _plan(Z, seeds, host=False, **kw), host


def assert_device_equals_twin(dev, host):
    for w in range(len(host.status)):
        assert_same_plans(dev, w, host, w)
    assert dev.ms > 0.0


def test_a_mixed_batch_of_six():
    Z = wall_with_window()
    empty = np.vstack([FAR[None]] * Z.shape[0])
    inside = np.array([0.5, 0.35, 0.5])
    dev, host = both(np.stack([Z, Z, Z, empty, Z, Z]), [1, 2, 3, 1, 1, 1], starts=np.stack([START] * 4 + [inside, START]), goals=np.stack([GOAL] * 5 + [inside]))
    assert list(host.status[3:]) == [1, 2, 0] and (host.rewires[:3] > 0).all()
    assert_device_equals_twin(dev, host)


def test_a_tree_that_crosses_64_256_and_512_nodes():
    dev, host = both(OPEN, [4], max_iterations=640, max_nodes=1024)
    assert host.count[0] > 512 and host.rewires[0] > 0
    assert_device_equals_twin(dev, host)
    for it in (70, 300):                              # the runs that END just past the boundaries of a wave and of a block
        dev, host = both(OPEN, [4], max_iterations=it, max_nodes=1024)
        assert host.count[0] > (64 if it == 70 else 256)
        assert_device_equals_twin(dev, host)


def test_a_work_list_of_many_chunks_and_more_than_256_candidates():
    Z = wall_with_window()
    dev, host = both(Z, [2], rewire_radius=0.45, max_iterations=200)     # tens of candidates of up to 45 sub-segments: more than one chunk of 256 items
    assert host.count[0] > 100
    assert_device_equals_twin(dev, host)
    dev, host = both(Z, [3], rewire_radius=2.5, max_iterations=400)      # every node is a candidate: more than one round of 256 candidates
    assert host.count[0] > 320 and host.rewires[0] > 0
    assert_device_equals_twin(dev, host)


def test_a_full_tree_and_no_iterations():
    dev, host = both(wall_with_window(), [1], max_nodes=64)
    assert host.count[0] == 64 and host.iterations[0] < OPTS["max_iterations"]
    assert_device_equals_twin(dev, host)
    dev, host = both(wall_with_window(), [1], max_nodes=1)
    assert_device_equals_twin(dev, host)
    dev, host = both(wall_with_window(), [1], max_iterations=0)
    assert_device_equals_twin(dev, host)


@pytest.mark.parametrize("O", [0, 3, 64])
def test_obstacle_counts(O):
    rng = np.random.default_rng(7)
    Z = wall_with_window()
    if O <= 3:
        Z = Z[:O]
    else:                                             # the wall, then small boxes scattered over the sampling box (none on the start)
        c = rng.uniform(LB + 0.25, UB, (O - Z.shape[0], 3))
        Z = np.vstack([Z] + [_box(ci, (0.03, 0.03, 0.03))[None] for ci in c])
    dev, host = both(Z.reshape(1, O, 12), [5], max_iterations=200)
    assert host.status[0] != 2 and host.count[0] > 60
    assert_device_equals_twin(dev, host)


def test_a_seeded_chain_with_a_blocked_edge():
    Z = wall_with_window()
    chain = np.array([[0.2, -0.2, 0.3], [0.4, 0.0, 0.5], [0.6, 0.3, 0.5], [0.8, 0.3, 0.7]])
    through = np.array([[0.4, 0.0, 0.5], [0.6, 0.0, 0.5], GOAL])
    dev, host = both(np.stack([Z] * 3), [1, 2, 3], init=[chain, through, None], max_iterations=100)
    assert list(host.chain_kept) == [2, 3, 0]
    assert_device_equals_twin(dev, host)


def test_many_rewires_in_one_iteration():
    """The restatement's count decides which seed: the run whose busiest iteration rewired the most nodes."""
    o = dict(OPTS, rewire_radius=0.3, max_iterations=160)
    refs = {seed: plan_ws_np(OPEN, START, GOAL, seed, **o) for seed in (1, 2, 3, 4)}
    seed = max(refs, key=lambda s: refs[s]["most_rewires"])
    assert refs[seed]["most_rewires"] >= 3 and refs[seed]["margin"] > MARGIN
    dev, host = both(OPEN, [seed], rewire_radius=0.3, max_iterations=160)
    assert host.rewires[0] == refs[seed]["rewires"] and host.count[0] == refs[seed]["count"]
    assert (host.parent[0, :host.count[0]] > np.arange(host.count[0])).any()
    assert_device_equals_twin(dev, host)


def test_sixteen_worlds_in_one_launch_against_sixteen_launches():
    Z = wall_with_window()
    seeds = list(range(1, 17))
    batch = _plan(np.stack([Z] * 16), seeds, host=False, max_iterations=120)
    for w in range(16):
        one = _plan(Z, [seeds[w]], host=False, max_iterations=120)
        assert_same_plans(batch, w, one, 0)
    assert len({int(c) for c in batch.count}) > 4


def test_the_hlp_on_the_device_against_the_hlp_on_the_host():
    """One trial iteration's waypoints for three reference worlds.  The trees and the workspace waypoints are bit-equal; the configurations
    come from the inverse kinematics, whose device run differs from its twin by the rounding of sin / cos: test_ik_gpu.py's tolerance."""
    from armour_amd.scenes import reference_worlds
    from armour_amd.ws_planner import workspace_hlps
    from test_ik_gpu import DEV_Q_TOL
    robot = _robot("kinova")
    worlds = reference_worlds()[:3]
    qs = [np.asarray(p["q0"], dtype=np.float64) for _, p in worlds]
    made = {}
    for host in (False, True):
        make = workspace_hlps(worlds, robot, seed=11, lookahead=0.15, host=host, ik_options=dict(S=8), max_iterations=150, max_nodes=256)
        made[host] = (make.get_waypoints([0, 1, 2], qs, [1.0] * 3), make)
    for i in range(3):
        d, h = made[False][1].hlps[i], made[True][1].hlps[i]
        assert h.margin_min > MARGIN
        assert d.status == h.status and d.path.tobytes() == h.path.tobytes() and d.waypoint.tobytes() == h.waypoint.tobytes()
        assert d.ik_status == h.ik_status
        assert np.abs(made[False][0][i] - made[True][0][i]).max() <= DEV_Q_TOL
    assert made[False][1].last_ms > 0.0
