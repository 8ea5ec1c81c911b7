"""Resident workspace trees, device half: armour_ws_trees_grow / _read on the MI355X -- the plan kernel's resumed form -- against the host
handle and against one armour_ws_tree_plan launch, bit for bit on every output and on the stored trees.  The two run the same functions and
no trigonometry is involved, so nothing but a clearance within rounding of zero could part them: every comparison first asserts that the
host twin's `margin` is above 1e-9 (the committed fixtures' smallest is 1.1e-5).  The host handle is held to the plan entry's host twin in
test_ws_trees.py.  The shapes are the smallest at which the resumed form can go wrong: node counts that cross the lane-dealing boundaries
(64, 256, 512) between launches and inside one, more than one round of candidates after a resume, a grid smaller than the handle, a full
tree, an empty instalment, a blocked start, no obstacles and more obstacles than a wave has lanes."""
import numpy as np
import pytest

from test_roadmap import _robot
from test_ws_tree import FAR, GOAL, LB, MARGIN, OPEN, START, UB, _box, _plan, wall_with_window
from test_ws_trees import INSIDE, _trees, assert_equals_plan

pytestmark = pytest.mark.gpu

FIELDS = ("status", "iterations", "count", "rewires", "chain_kept", "path_cost", "goal_dist")


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def assert_same_grow(dev, host):
    """two results of a grow, every output of every slot"""
    assert (host.margin > MARGIN).all(), host.margin
    for k in FIELDS:
        assert same(getattr(dev, k), getattr(host, k)), (k, getattr(dev, k), getattr(host, k))
    for p, q in zip(dev.paths, host.paths):
        assert (p is None) == (q is None) and (p is None or same(p, q))
    assert dev.ms > 0.0


def assert_same_trees(a, b):
    assert np.array_equal(a.count, b.count) and same(a.nodes, b.nodes) and same(a.parent, b.parent) and same(a.node_cost, b.node_cost)


def grow_both(dev, host, worlds, starts, iterations):
    d, h = dev.grow(worlds, starts, iterations), host.grow(worlds, starts, iterations, margin=True)
    assert_same_grow(d, h)
    return d, h


def test_the_device_handle_equals_the_host_handle_on_a_mixed_batch_of_six():
    Z = wall_with_window()
    empty = np.vstack([FAR[None]] * Z.shape[0])
    obs, seeds = np.stack([Z, Z, Z, empty, Z, Z]), [1, 2, 3, 1, 1, 1]
    starts, goals = np.stack([START] * 4 + [INSIDE, START]), np.stack([GOAL] * 5 + [INSIDE])
    dev, host = _trees(obs, seeds, host=False, goals=goals), _trees(obs, seeds, host=True, goals=goals)
    everyone = list(range(6))
    for _ in range(3):
        d, h = grow_both(dev, host, everyone, starts, 80)
        assert_same_trees(dev.read(everyone), host.read(everyone))
    assert list(h.status[3:]) == [1, 2, 0] and (h.rewires[:3] > 0).all() and h.count[4] == 0
    ref = _plan(obs, seeds, host=True, starts=starts, goals=goals, max_iterations=240)
    trees = dev.read(everyone)
    for w in everyone:
        assert_equals_plan(d, w, trees, w, ref, w)
    dev.close()
    host.close()


def test_eight_instalments_against_one_plan_launch_across_64_256_and_512_nodes():
    plan = _plan(OPEN, [4], host=False, max_iterations=640, max_nodes=1024)
    twin = _plan(OPEN, [4], host=True, max_iterations=640, max_nodes=1024)
    assert twin.margin[0] > MARGIN and twin.count[0] > 512
    dev = _trees(OPEN, [4], host=False, max_nodes=1024)
    counts = [0]
    for _ in range(8):
        res = dev.grow([0], START[None], 80)
        counts.append(int(res.count[0]))
    for edge in (64, 256, 512):                       # crossed INSIDE a launch (a launch starts below and ends above) ...
        assert any(a < edge < b for a, b in zip(counts, counts[1:])), (edge, counts)
    assert_equals_plan(res, 0, dev.read([0]), 0, plan)
    assert_equals_plan(res, 0, dev.read([0]), 0, twin)
    dev.close()
    # ... and BETWEEN launches: instalments that end exactly at a count of 64, 256 and 512, found on the host handle
    host = _trees(OPEN, [4], host=True, max_nodes=1024)
    ends, done = [], 0
    for edge in (64, 256, 512):
        while host.grow([0], START[None], 1).count[0] < edge:
            pass
        now = int(host.grow([0], None, 0).iterations[0])
        ends.append(now - done)
        done = now
    host.close()
    ends.append(640 - done)
    assert all(n > 0 for n in ends)
    dev = _trees(OPEN, [4], host=False, max_nodes=1024)
    seen = []
    for n in ends:
        res = dev.grow([0], START[None], n)
        seen.append(int(res.count[0]))
    assert seen[:3] == [64, 256, 512]
    assert_equals_plan(res, 0, dev.read([0]), 0, plan)
    dev.close()


def test_more_than_256_candidates_after_a_resume():
    Z = wall_with_window()
    dev, host = _trees(Z, [3], host=False, rewire_radius=2.5), _trees(Z, [3], host=True, rewire_radius=2.5)
    for _ in range(4):
        d, h = grow_both(dev, host, [0], START[None], 100)
    assert h.count[0] > 320 and h.rewires[0] > 0     # every node is a candidate: more than one round of 256
    assert_same_trees(dev.read([0]), host.read([0]))
    assert_equals_plan(d, 0, dev.read([0]), 0, _plan(Z, [3], host=False, rewire_radius=2.5, max_iterations=400))
    dev.close()
    host.close()


def test_a_grid_smaller_than_the_handle_serves_the_listed_worlds_alone():
    Z = wall_with_window()
    seeds = list(range(1, 17))
    obs = np.stack([Z] * 16)
    dev, host = _trees(obs, seeds, host=False), _trees(obs, seeds, host=True)
    everyone = list(range(16))
    starts = np.stack([START] * 16)
    grow_both(dev, host, everyone, starts, 40)
    before = dev.read(everyone)
    subset = [11, 2, 7]                               # permuted: slot 0 is world 11
    d, h = grow_both(dev, host, subset, starts[:3], 80)
    after = dev.read(everyone)
    assert_same_trees(after, host.read(everyone))
    others = [w for w in everyone if w not in subset]
    for k in ("nodes", "parent", "node_cost", "count"):
        assert same(getattr(before, k)[others], getattr(after, k)[others]), k
    assert (after.count[subset] > before.count[subset]).all()
    for k, w in enumerate(subset):
        assert_equals_plan(d, k, after, w, _plan(Z, [seeds[w]], host=True, max_iterations=120))
    dev.close()
    host.close()


def test_a_full_tree_no_iterations_and_a_blocked_start_on_the_device():
    Z = wall_with_window()
    dev, host = _trees(Z, [1], host=False, max_nodes=64), _trees(Z, [1], host=True, max_nodes=64)
    d, h = grow_both(dev, host, [0], START[None], 250)
    assert h.count[0] == 64 and h.iterations[0] < 250
    d2, h2 = grow_both(dev, host, [0], START[None], 100)          # full: nothing changes, no iteration is consumed
    assert d2.iterations[0] == d.iterations[0] and same(d2.paths[0], d.paths[0])
    assert_same_trees(dev.read([0]), host.read([0]))
    dev.close()
    host.close()
    obs = np.stack([Z, Z])
    dev, host = _trees(obs, [1, 1], host=False), _trees(obs, [1, 1], host=True)
    d, h = grow_both(dev, host, [0, 1], np.stack([INSIDE, START]), 0)     # no iterations: world 0 is blocked, world 1 gets its root
    assert list(h.status) == [2, 0] and list(h.count) == [0, 1] and list(h.iterations) == [0, 0]
    other = np.array([0.15, -0.2, 0.3])
    d, h = grow_both(dev, host, [1, 0], np.stack([INSIDE, other]), 60)    # world 0 is planted from the new point; world 1 ignores its start
    assert h.count[1] > 1 and list(h.iterations) == [60, 60]
    d0, h0 = grow_both(dev, host, [0, 1], None, 0)                        # no iterations on grown trees: the paths as they stand
    assert same(d0.paths[0], d.paths[1]) and same(d0.paths[1], d.paths[0]) and list(d0.iterations) == [60, 60]
    trees = dev.read([0, 1])
    assert_same_trees(trees, host.read([0, 1]))
    assert_equals_plan(d0, 0, trees, 0, _plan(Z, [1], host=True, starts=other[None], max_iterations=60))
    dev.close()
    host.close()


@pytest.mark.parametrize("O", [0, 3, 64])
def test_obstacle_counts(O):
    rng = np.random.default_rng(7)
    Z = wall_with_window()
    if O <= 3:
        Z = Z[:O]
    else:                                             # the wall, then small boxes scattered over the sampling box (none on the start)
        c = rng.uniform(LB + 0.25, UB, (O - Z.shape[0], 3))
        Z = np.vstack([Z] + [_box(ci, (0.03, 0.03, 0.03))[None] for ci in c])
    Z = Z.reshape(1, O, 12)
    dev, host = _trees(Z, [5], host=False), _trees(Z, [5], host=True)
    for n in (70, 130):
        d, h = grow_both(dev, host, [0], START[None], n)
    assert h.status[0] != 2 and h.count[0] > 60
    assert_same_trees(dev.read([0]), host.read([0]))
    assert_equals_plan(d, 0, dev.read([0]), 0, _plan(Z, [5], host=False, max_iterations=200))
    dev.close()
    host.close()


def test_the_keep_hlp_on_the_device_against_the_keep_hlp_on_the_host():
    """Three calls of the batched 'keep' planner for three reference worlds from the same configurations.  The trees, the paths and the
    workspace waypoints are bit-equal; the configurations come from the inverse kinematics, whose device run differs from its twin by the
    rounding of sin / cos: test_ik_gpu.py's tolerance."""
    from armour_amd.scenes import reference_worlds
    from armour_amd.ws_planner import workspace_hlps
    from test_ik_gpu import DEV_Q_TOL
    robot = _robot("kinova")
    worlds = reference_worlds()[:3]
    q0 = [np.asarray(p["q0"], dtype=np.float64) for _, p in worlds]
    goals = [np.asarray(p["goal"], dtype=np.float64) for _, p in worlds]
    make = {host: workspace_hlps(worlds, robot, seed=11, lookahead=0.15, mode="keep", host=host, ik_options=dict(S=8), max_iterations=100, max_nodes=512)
            for host in (False, True)}
    for c in range(3):
        qs = [q0[i] + 0.1 * c * (goals[i] - q0[i]) for i in range(3)]
        live = [0, 1, 2] if c < 2 else [2, 0]         # the last call: a live set smaller than the handle, permuted
        got = {host: make[host].get_waypoints(live, [qs[i] for i in live], [1.0] * len(live)) for host in (False, True)}
        for k, i in enumerate(live):
            d, h = make[False].hlps[i], make[True].hlps[i]
            assert h.margin_min > MARGIN
            assert d.status == h.status and d.count == h.count and same(d.path, h.path) and same(d.waypoint, h.waypoint)
            assert d.ik_status == h.ik_status
            assert np.abs(got[False][k] - got[True][k]).max() <= DEV_Q_TOL
        assert make[False].last_ms > 0.0
    assert_same_trees(make[False].shared["trees"].read([0, 1, 2]), make[True].shared["trees"].read([0, 1, 2]))
    assert [make[False].hlps[i].calls for i in range(3)] == [3, 2, 3]
    for m in make.values():
        m.close()
