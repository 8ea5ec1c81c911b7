"""The roadmap's window rule on the device (armour_roadmap_check_moving) against its host twin on the roadmaps of tests/test_roadmap_moving.py,
against the static check at zero velocity, and the batched joins that follow the last check's rule (connect_many, descend_many) against
plan / descend of a host handle in the same state."""
import numpy as np
import pytest

from test_path_audit import CL_TOL
from test_roadmap import _robot
from test_roadmap_moving import STEP, WINDOWS, _case, _host, refusals

pytestmark = pytest.mark.gpu

T0, T1 = np.array(WINDOWS).T


@pytest.fixture(scope="module", params=["kinova", "fetch"])
def case(request):
    """The CPU tests' roadmap and worlds of one robot on a device handle and on a host handle"""
    from armour_amd.roadmap import Roadmap
    robot, g, nodes, edges, cont, obs, vel = _case(request.param)
    dev = Roadmap(robot, nodes, edges, continuous=cont, edge_step=STEP)
    host = _host(robot, nodes, edges, cont)
    yield dict(name=request.param, robot=robot, nodes=nodes, edges=edges, cont=cont, obs=obs, vel=vel, dev=dev, host=host)
    dev.close()
    host.close()


def _same_masks(a, b):
    return np.array_equal(a["node_free"], b["node_free"]) and np.array_equal(a["edge_free"], b["edge_free"])


def test_device_check_equals_the_host_twin(case):
    dev = case["dev"].check_moving(case["obs"], case["vel"], T0, T1, clearance=True)
    fast = case["dev"].check_moving(case["obs"], case["vel"], T0, T1)
    host = case["host"].check_moving(case["obs"], case["vel"], T0, T1, clearance=True, host=True)
    assert _same_masks(dev, host) and _same_masks(fast, host)
    assert 0 < host["edge_free"].sum() < host["edge_free"].size and 0 < host["node_free"].sum() < host["node_free"].size
    assert np.abs(dev["node_clearance"] - host["node_clearance"]).max() <= CL_TOL
    assert dev["ms"] > 0


def test_zero_velocity_is_the_static_device_check_bit_for_bit(case):
    rm, obs = case["dev"], case["obs"]
    st = rm.check(obs, clearance=True)
    for t0, t1 in ((0.0, 0.0), (T0 - 2.0, T1 + 3.0)):
        mv = rm.check_moving(obs, np.zeros_like(case["vel"]), t0, t1, clearance=True)
        assert _same_masks(mv, st) and np.array_equal(mv["node_clearance"], st["node_clearance"])


def test_three_worlds_in_one_call_equal_three_calls(case):
    rm, obs, vel = case["dev"], case["obs"], case["vel"]
    ones = [rm.check_moving(obs[w], vel[w], T0[w], T1[w], clearance=True) for w in range(3)]
    all_ = rm.check_moving(obs, vel, T0, T1, clearance=True)
    for w in range(3):
        for key in ("node_free", "edge_free", "node_clearance"):
            assert np.array_equal(all_[key][w], ones[w][key][0]), (w, key)


def _queries(case, seed=3, Q=24):
    """Q starts spread over the three worlds and a goal per world: roadmap nodes moved a little, so that joins both succeed and fail"""
    rng = np.random.default_rng(seed)
    nodes = case["nodes"]
    world = (np.arange(Q) % 3).astype(np.int32)
    starts = nodes[rng.integers(0, nodes.shape[0], Q)] + rng.normal(scale=0.05, size=(Q, nodes.shape[1]))
    goals = nodes[rng.integers(0, nodes.shape[0], 3)] + rng.normal(scale=0.05, size=(3, nodes.shape[1]))
    return world, starts, goals


def test_batched_joins_follow_the_window_rule(case):
    """connect_many on the device after a moving check against plan() of a host handle after the same check: an edge start -> x is free
    exactly when plan(start, x, connect_k=0), which can only answer with the direct edge, finds a path.  descend_many against descend(),
    whose joins are the host searches' (the field needs a device, so descend runs on the device handle's host half)."""
    dev, host, obs, vel = case["dev"], case["host"], case["obs"], case["vel"]
    world, starts, goals = _queries(case)
    dev.check_moving(obs, vel, T0, T1)
    hv = host.check_moving(obs, vel, T0, T1, host=True)
    got = dev.connect_many(world, starts, targets=goals[world], connect_k=6)
    n_direct = n_ok = 0
    for i, w in enumerate(world):
        path = host.plan(int(w), starts[i], goals[w], connect_k=0)           # connect_k = 0: only the direct edge can answer
        assert bool(got["direct"][i]) == (path is not None), i
        n_direct += int(got["direct"][i])
        for c in range(got["count"][i]):
            v = int(got["node"][i, c])
            assert hv["node_free"][w, v]                                    # the candidates are the nodes free in the window
            # start -> node v: host.plan towards the node itself answers with the direct edge exactly when that edge is free
            p = host.plan(int(w), starts[i], case["nodes"][v], connect_k=0)
            assert bool(got["edge_ok"][i, c]) == (p is not None), (i, c)
            n_ok += int(got["edge_ok"][i, c])
    assert 0 < n_ok < got["count"].sum(), (n_ok, got["count"].sum())       # joins of both kinds
    print(f"{case['name']}: {n_direct} direct edges, {n_ok} of {got['count'].sum()} joins free")
    # descend_many against descend on the same (device) handle, whose host half is the dispatch the host handle uses
    dev.field(goals, connect_k=6)
    many = dev.descend_many(world, starts, connect_k=6)
    for i, w in enumerate(world):
        path, length = dev.descend(int(w), starts[i], connect_k=6)
        assert (path is None) == (many[i][0] is None) and np.float64(length).tobytes() == np.float64(many[i][1]).tobytes(), i
        assert path is None or np.array_equal(path, many[i][0]), i
        if path is not None and len(path) == 2:                             # a direct edge of the field is plan()'s on the host handle
            assert host.plan(int(w), starts[i], goals[w], connect_k=0) is not None
    # the window matters: at zero velocity (the static rule) the same queries are joined differently
    dev.check_moving(obs, np.zeros_like(vel), T0, T1)
    static = dev.connect_many(world, starts, targets=goals[world], connect_k=6)
    assert not (np.array_equal(static["edge_ok"], got["edge_ok"]) and np.array_equal(static["node"], got["node"]))


def test_static_moving_static_on_one_handle(case):
    from armour_amd import _lib
    rm, obs, vel = case["dev"], case["obs"], case["vel"]
    world, starts, goals = _queries(case, seed=4)
    s1 = rm.check(obs, clearance=True)
    c1 = rm.connect_many(world, starts, targets=goals[world], connect_k=6)
    rm.field(goals, connect_k=6)
    m = rm.check_moving(obs, vel, T0, T1, clearance=True)
    with pytest.raises(_lib.ArmourError) as ei:                              # a moving check ends the field as a static one does
        rm.descend_many(world, starts)
    assert ei.value.code == _lib.ESTATE
    cm = rm.connect_many(world, starts, targets=goals[world], connect_k=6)
    assert not _same_masks(m, s1)
    assert not (np.array_equal(cm["edge_ok"], c1["edge_ok"]) and np.array_equal(cm["node"], c1["node"]))
    s2 = rm.check(obs, clearance=True)
    c2 = rm.connect_many(world, starts, targets=goals[world], connect_k=6)
    assert _same_masks(s2, s1) and np.array_equal(s2["node_clearance"], s1["node_clearance"])
    for key in ("node", "dist", "edge_ok", "count", "direct"):
        assert np.array_equal(c2[key], c1[key]), key
    m2 = rm.check_moving(obs, vel, T0, T1, clearance=True)                   # and the other order: moving -> static -> moving
    cm2 = rm.connect_many(world, starts, targets=goals[world], connect_k=6)
    assert _same_masks(m2, m) and np.array_equal(m2["node_clearance"], m["node_clearance"])
    for key in ("node", "dist", "edge_ok", "count", "direct"):
        assert np.array_equal(cm2[key], cm[key]), key


def test_the_obstacle_cap_fits_in_lds():
    """O = ARMOUR_ROADMAP_MAX_OBSTACLES, 62 KB of LDS per block, on 8 nodes: device against host twin, and the joins' kernel at the same size"""
    from armour_amd.roadmap import Roadmap
    from armour_amd.scenes import boxes_to_obstacles
    from test_moving_audit import random_motion
    from test_roadmap_moving import make_roadmap
    robot = _robot("kinova")
    nodes, edges, cont = make_roadmap(robot, N=8)
    rng = np.random.default_rng(8)
    O = 256
    boxes = np.concatenate([rng.uniform([-1.5, -1.5, 0.0], [1.5, 1.5, 1.5], (O, 3)), rng.uniform(0.02, 0.06, (O, 3))], axis=1)
    obs = boxes_to_obstacles(boxes)[None]
    vel = random_motion(rng, obs, lo=0.05, hi=0.2)
    dev, host = Roadmap(robot, nodes, edges, continuous=cont, edge_step=STEP), _host(robot, nodes, edges, cont)
    a = dev.check_moving(obs, vel, 0.0, 0.2, clearance=True)
    b = host.check_moving(obs, vel, 0.0, 0.2, clearance=True, host=True)
    assert _same_masks(a, b) and np.abs(a["node_clearance"] - b["node_clearance"]).max() <= CL_TOL
    got = dev.connect_many(np.zeros(8, dtype=np.int32), nodes + 0.01, targets=nodes[::-1].copy(), connect_k=4)
    for i in range(8):
        assert bool(got["direct"][i]) == (host.plan(0, nodes[i] + 0.01, nodes[7 - i], connect_k=0) is not None), i
    dev.close()
    host.close()


def test_device_entry_refuses_what_the_host_entry_refuses(case):
    from armour_amd import _lib
    refusals(case["dev"], host=False)
    with pytest.raises(_lib.ArmourError) as ei:                              # the host twin takes handles of armour_roadmap_create_host only
        case["dev"].check_moving(case["obs"], case["vel"], T0, T1, host=True)
    assert ei.value.code == _lib.EINVAL
