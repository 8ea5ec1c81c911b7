"""The roadmap's window rule (include/armour_hip.h armour_roadmap_check_moving, armour_amd.roadmap.Roadmap.check_moving): the host twin.

The rule is restated in numpy from the moving audit's pair test (tests/test_moving_audit.py config_clearance_moving) and the edge rule's
sub-segments (tests/test_roadmap.py edge_samples): with mid = 0.5 (t_from + t_to) and half = 0.5 (t_to - t_from) of a world, a node is free
when its clearance at tau = mid with every half-size grown by |v| half is positive, an edge when every sub-segment's is, with r_l besides.
CPU tests: the library's host loop against the restatement, zero velocity against the static restatement, soundness by sampling edges and
times, a hand-made scene through plan(), and every refusal."""
import ctypes as C

import numpy as np
import pytest

from test_moving_audit import config_clearance_moving, random_motion
from test_path_audit import CL_TOL
from test_roadmap import _limits, _robot, config_clearance, edge_free_np, edge_samples, geometry, link_boxes, robot_dict, wrap

N_NODES, STEP, O_PAD = 48, 0.25, 14
WINDOWS = ((0.0, 0.5), (1.25, 1.25), (-0.1, 0.2))      # one per world; the second is an instant


def make_roadmap(robot, N=N_NODES, seed=5):
    """(nodes [N,n], edges [E,2], cont): seeded uniform nodes, every node's 5 nearest neighbours within 6 rad -- about 150 edges"""
    from armour_amd.roadmap import uniform_roadmap
    lb, ub, cont = _limits(robot)
    nodes, edges = uniform_roadmap(N, 6.0, 5, seed, lb, ub, cont)
    return nodes, edges, cont


def random_worlds(rng, counts=(1, 5, 14), pad=O_PAD):
    """obstacles [W,pad,12]: counts[w] axis-aligned boxes within the arm's reach, then far-away boxes; velocity [W,pad,3] of 0.2 - 1.0 m/s"""
    from armour_amd.scenes import boxes_to_obstacles, pad_obstacles
    obs = []
    for c in counts:
        boxes = np.concatenate([rng.uniform([-0.9, -0.9, 0.0], [0.9, 0.9, 1.2], (c, 3)), rng.uniform(0.05, 0.2, (c, 3))], axis=1)
        obs.append(pad_obstacles(boxes_to_obstacles(boxes), pad))
    obs = np.stack(obs)
    return obs, random_motion(rng, obs)


def window_rule_np(g, nodes, edges, Z, V, t_from, t_to, step):
    """(node clearance [N], edge clearance [E]) of one world by the window rule; free = clearance > 0"""
    mid, half = 0.5 * (t_from + t_to), 0.5 * (t_to - t_from)
    node_cl = config_clearance_moving(g, nodes, Z, V, mid, None, half)
    qs, rs, owner = [], [], []
    for e, (a, b) in enumerate(edges):
        q, r = edge_samples(g, nodes[a], nodes[b], step)
        qs.append(q), rs.append(r), owner.append(np.full(q.shape[0], e))
    cl = config_clearance_moving(g, np.concatenate(qs), Z, V, mid, np.concatenate(rs), half)
    edge_cl = np.full(len(edges), np.inf)
    np.minimum.at(edge_cl, np.concatenate(owner), cl)
    return node_cl, edge_cl


def _case(name, seed=61):
    robot = _robot(name)
    nodes, edges, cont = make_roadmap(robot)
    obs, vel = random_worlds(np.random.default_rng(seed))
    return robot, geometry(robot_dict(robot)), nodes, edges, cont, obs, vel


def _host(robot, nodes, edges, cont, step=STEP):
    from armour_amd.roadmap import Roadmap
    return Roadmap(robot, nodes, edges, continuous=cont, edge_step=step, host=True)


@pytest.mark.parametrize("name", ["kinova", "fetch"])
def test_host_check_equals_the_restatement(name):
    robot, g, nodes, edges, cont, obs, vel = _case(name)
    assert nodes.shape[0] == N_NODES and 130 <= len(edges) <= 170, len(edges)
    t0, t1 = np.array(WINDOWS).T
    rm = _host(robot, nodes, edges, cont)
    v = rm.check_moving(obs, vel, t0, t1, clearance=True, host=True)
    fast = rm.check_moving(obs, vel, t0, t1, host=True)
    assert np.array_equal(v["node_free"], fast["node_free"]) and np.array_equal(v["edge_free"], fast["edge_free"])   # early exit changes nothing
    assert np.array_equal(v["node_free"], v["node_clearance"] > 0)
    counts = np.zeros(4, dtype=int)
    for w in range(obs.shape[0]):
        node_cl, edge_cl = window_rule_np(g, nodes, edges, obs[w], vel[w], t0[w], t1[w], STEP)
        margin = min(np.abs(node_cl).min(), np.abs(edge_cl).min())
        print(f"{name} world {w}: free nodes {int((node_cl > 0).sum())}/{N_NODES}, free edges {int((edge_cl > 0).sum())}/{len(edges)}, margin {margin:.2e}")
        assert margin > 1e-9, (name, w, margin)            # no decisive quantity within rounding of zero: the masks can be compared exactly
        assert np.array_equal(v["node_free"][w], node_cl > 0), (name, w)
        assert np.array_equal(v["edge_free"][w], edge_cl > 0), (name, w)
        assert np.abs(v["node_clearance"][w] - node_cl).max() <= CL_TOL, (name, w, np.abs(v["node_clearance"][w] - node_cl).max())
        ef, nf = v["edge_free"][w], v["node_free"][w]
        assert np.all(nf[edges[ef, 0]]) and np.all(nf[edges[ef, 1]])      # a free edge has free endpoints
        counts += [int(nf.sum()), int((~nf).sum()), int(ef.sum()), int((~ef).sum())]
    assert counts.min() > 0, counts
    rm.close()


@pytest.mark.parametrize("name", ["kinova", "fetch"])
def test_zero_velocity_is_the_static_rule_for_any_window(name):
    robot, g, nodes, edges, cont, obs, _ = _case(name)
    rm = _host(robot, nodes, edges, cont)
    zero = np.zeros(obs.shape[:2] + (3,))
    a = rm.check_moving(obs, zero, 0.0, 0.0, clearance=True, host=True)
    b = rm.check_moving(obs, zero, [-3.0, 0.25, 7.0], [4.0, 0.25, 11.5], clearance=True, host=True)
    for key in ("node_free", "edge_free", "node_clearance"):
        assert np.array_equal(a[key], b[key]), (name, key)
    for w in range(obs.shape[0]):
        cl = config_clearance(g, nodes, obs[w])
        assert np.abs(a["node_clearance"][w] - cl).max() <= CL_TOL and np.abs(cl).min() > 1e-9
        assert np.array_equal(a["node_free"][w], cl > 0), (name, w)
        for e, (i, j) in enumerate(edges):
            free, ecl = edge_free_np(g, nodes[i], nodes[j], obs[w], STEP)
            assert abs(ecl) > 1e-9 and bool(a["edge_free"][w, e]) == free, (name, w, e, ecl)
    rm.close()


@pytest.mark.parametrize("name", ["kinova", "fetch"])
def test_free_edges_are_sound_by_sampling(name):
    """Every free edge: 20 configurations on it x 11 times of the world's window have positive STATIC clearance against the obstacles
    themselves moved to that time (not the shifted link box of the rule)."""
    robot, g, nodes, edges, cont, obs, vel = _case(name)
    # slower obstacles and shorter windows than above leave more edges free to sample
    vel = vel * 0.5
    t0, t1 = np.array(((0.0, 0.3), (0.8, 0.8), (-0.2, 0.2))).T
    rm = _host(robot, nodes, edges, cont)
    v = rm.check_moving(obs, vel, t0, t1, host=True)
    rng = np.random.default_rng(7)
    sampled = 0
    for w in range(obs.shape[0]):
        free = np.flatnonzero(v["edge_free"][w])
        if not free.size:
            continue
        a, b = nodes[edges[free, 0]], nodes[edges[free, 1]]
        t = np.concatenate([[0.0, 1.0], rng.random(18)])
        Q = (a[:, None, :] + t[None, :, None] * np.where(cont, wrap(b - a), b - a)[:, None, :]).reshape(-1, nodes.shape[1])
        for time in np.linspace(t0[w], t1[w], 11):
            Zt = obs[w].copy()
            Zt[:, 0:3] += vel[w] * time
            assert config_clearance(g, Q, Zt).min() > 0, (name, w, time)
        sampled += free.size
    print(f"{name}: {sampled} free edges sampled")
    assert sampled >= 30, sampled
    rm.close()


# ----------------------------------------------------------------------------------------------------------- a hand-made scene
def arriving_box_scene(robot):
    """(nodes [3,n], edges, cont, obstacle [1,12], velocity [1,3]): a box that starts 1 m outside the last link's position at the middle of the
    edge node 0 -> node 1 and moves towards it at 0.5 m/s, so that its centre arrives on the edge at t = 2.  Node 2 is a detour."""
    g = geometry(robot_dict(robot))
    n = g["n"]
    lb, ub, cont = _limits(robot)
    a = np.zeros(n)
    a[1] = 0.6
    b = a.copy()
    b[0] = 0.5
    c = a.copy()
    c[0], c[1] = 0.25, -0.6
    mid = a + 0.5 * (b - a)
    x = link_boxes(g, mid[None])[2][0, -1]                      # the last link's box centre at the middle of the edge
    u = np.array([x[0], x[1], 0.0]) / np.hypot(x[0], x[1])      # away from the base, horizontally
    box = np.zeros((1, 12))
    box[0, 0:3] = x + 1.0 * u
    box[0, 3] = box[0, 7] = box[0, 11] = 0.05
    return np.stack([a, b, c]), np.array([[0, 1], [0, 2], [2, 1]], dtype=np.int32), cont, box, (-0.5 * u)[None]


def test_a_box_that_arrives_at_t_2_blocks_the_edge_only_in_a_window_that_holds_t_2():
    robot = _robot("kinova")
    g = geometry(robot_dict(robot))
    nodes, edges, cont, box, vel = arriving_box_scene(robot)
    rm = _host(robot, nodes, edges, cont, step=0.1)
    early = rm.check_moving(box, vel, 0.0, 1.0, host=True)
    assert early["edge_free"][0, 0] and early["node_free"][0].all()
    path = rm.plan(0, nodes[0], nodes[1])
    assert path is not None and path.shape[0] == 2                      # the direct edge
    late = rm.check_moving(box, vel, 0.0, 3.0, host=True)
    assert not late["edge_free"][0, 0]
    path = rm.plan(0, nodes[0], nodes[1])
    assert path is None or path.shape[0] > 2                            # a detour, or no path: never the direct edge
    # the instant t = 2 itself, and the restatement of all three
    at2 = rm.check_moving(box, vel, 2.0, 2.0, host=True)
    assert not at2["edge_free"][0, 0]
    for res, (t0, t1) in ((early, (0.0, 1.0)), (late, (0.0, 3.0)), (at2, (2.0, 2.0))):
        node_cl, edge_cl = window_rule_np(g, nodes, edges, box, vel, t0, t1, 0.1)
        assert np.array_equal(res["node_free"][0], node_cl > 0) and np.array_equal(res["edge_free"][0], edge_cl > 0)
    rm.close()


# ----------------------------------------------------------------------------------------------------------- refusals
def _raw_call(rm, W, O, obs, vel, t0, t1, host=True):
    """the C entry with the pointers as given (None = NULL); returns the status"""
    from armour_amd._lib import _dp
    nf, ef = np.zeros(max(W, 1) * rm.N, dtype=np.uint8), np.zeros(max(W, 1) * max(rm.E, 1), dtype=np.uint8)
    u8 = C.POINTER(C.c_uint8)
    args = [rm.h, W, O, _dp(obs), _dp(vel), _dp(t0), _dp(t1), nf.ctypes.data_as(u8), ef.ctypes.data_as(u8), None]
    return rm.L.armour_roadmap_check_moving_host(*args) if host else rm.L.armour_roadmap_check_moving(*args, None)


def refusals(rm, host):
    """every refusal of the window rule's entries on `rm`: ARMOUR_EINVAL each, and the handle still holds its last check's worlds"""
    from armour_amd import _lib
    box = np.array([[[0.5, 0.0, 0.5, 0.1, 0, 0, 0, 0.1, 0, 0, 0, 0.1]]])
    vel, t0, t1 = np.zeros((1, 1, 3)), np.zeros(1), np.ones(1)
    bad_box, bad_vel = box.copy(), vel.copy()
    bad_box[0, 0, 4] = np.inf
    bad_vel[0, 0, 1] = np.nan
    many = 257                                                          # ARMOUR_ROADMAP_MAX_OBSTACLES + 1
    cases = dict(negative_W=(-1, 1, box, vel, t0, t1), negative_O=(1, -1, box, vel, t0, t1), too_many_obstacles=(1, many, box, vel, t0, t1),
                 null_obstacles=(1, 1, None, vel, t0, t1), obstacle_not_finite=(1, 1, bad_box, vel, t0, t1),
                 null_velocity=(1, 1, box, None, t0, t1), velocity_not_finite=(1, 1, box, bad_vel, t0, t1),
                 null_t_from=(1, 1, box, vel, None, t1), null_t_to=(1, 1, box, vel, t0, None),
                 t_from_not_finite=(1, 1, box, vel, np.array([np.nan]), t1), t_to_not_finite=(1, 1, box, vel, t0, np.array([np.inf])),
                 window_reversed=(1, 1, box, vel, np.array([1.0]), np.array([0.5])))
    for tag, (W, O, *arrays) in cases.items():
        assert _raw_call(rm, W, O, *arrays, host=host) == _lib.EINVAL, tag
    null = C.c_void_p()
    fn = rm.L.armour_roadmap_check_moving_host if host else rm.L.armour_roadmap_check_moving
    tail = () if host else (None,)
    assert fn(null, 1, 1, _lib._dp(box), _lib._dp(vel), _lib._dp(t0), _lib._dp(t1), None, None, None, *tail) == _lib.EINVAL


def test_host_entry_refuses_bad_arguments():
    from armour_amd import _lib
    robot = _robot("kinova")
    nodes, edges, cont, box, vel = arriving_box_scene(robot)
    rm = _host(robot, nodes, edges, cont)
    refusals(rm, host=True)
    with pytest.raises(_lib.ArmourError) as ei:                          # a refused check is not a check
        rm.plan(0, nodes[0], nodes[1])
    assert ei.value.code == _lib.ESTATE
    with pytest.raises(_lib.ArmourError) as ei:                          # the device entry on a handle without a device, after its argument checks
        rm.check_moving(box, vel, 0.0, 1.0)
    assert ei.value.code == _lib.EDEVICE
    refusals(rm, host=False)                                             # ... which come first
    with pytest.raises(ValueError):
        rm.check_moving(box, vel, [0.0, 1.0], [1.0, 2.0], host=True)     # two windows for one world: the binding's broadcast refuses
    rm.close()
