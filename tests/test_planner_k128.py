"""The planner units in the 8-factor ABI (libarmour_hip_k128.so, ARMOUR_MAX_FACTORS = 8): roadmap.hip, roadmap_slices.hip, roadmap_knn.hip,
path_audit.hip, self_check.hip, tree_plan.hip, path_shortcut.hip and ik.hip with q[ARMOUR_MAX_FACTORS] and r[ARMOUR_MAX_JOINTS] both full.

Robots: fetch8 (n = 8, J = 9, axes [3,3,2,1,2,1,2,1,0], a fixed last link: both caps at once), kinova8 (tests/test_key128.py
make_eight_factor_arm: n = J = 8, continuous and limited joints mixed, no fixed joint), and the 7-factor Kinova and Fetch loaded through the
8-factor library, whose eighth slot must stay inert.  The ABI is chosen per process, so every body below runs in a child with
ARMOUR_KEY128=1 (the pattern of tests/test_tracking_edges.py); the pytest functions start the child and read its return code and last line.

CPU half: every host entry against the numpy restatement its unit's own CPU test uses (test_roadmap, test_roadmap_moving, test_roadmap_slices,
test_roadmap_knn, test_path_audit, test_moving_audit, test_self_check, test_tree_plan, test_tree_moving, test_path_shortcut, test_ik), by that
test's criterion; and the dead slot: the host entries' results for kinova and fetch in the 8-factor library against the shipped library's,
which the parent computes and hands over in an .npz -- integers equal, floats equal on their uint64 view, no field exempted (measured: every
field is bit-identical, so none is compared to the restatement instead).
GPU half: every device entry against its host twin in the same library, by the criterion of the unit's GPU test (margin > 1e-9 first where
the unit reports one, then equality of every discrete output and of every float that test compares bitwise), one child per family.

Inverse kinematics, device against host twin, |dq| and |derr| over the converged items, measured once on one MI355X over every call of the
IK child (S = 1, 8, 200 and the moving form):
  fetch8   max |dq| = 1.5e-12 (S = 200; 2.7e-15 at S = 8, static and moving), max |derr| = 7.6e-16;
  kinova8  max |dq| = 9.2e-14 (S = 200; 2.0e-15 at S = 8, static and moving), max |derr| = 4.8e-16,
with no flag and no iteration count different anywhere (0 items left out of 868 per arm); the picked configurations differ by 2.3e-16 at
most.  (Which of the 200 seeds carry the largest |dq| was not looked into; their |derr| is at rounding like everyone's.)  The tolerance is 100 x the largest seen, as headroom for other
builds of the device's sin / cos; it has to stay <= 1e-9, else something other than rounding is at work."""
import os
import subprocess
import sys

import numpy as np
import pytest

from armour_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K128_SEEN_Q, K128_SEEN_ERR = 1.5e-12, 7.6e-16
K128_Q_TOL, K128_ERR_TOL = 100 * K128_SEEN_Q, 100 * K128_SEEN_ERR
assert K128_Q_TOL <= 1e-9 and K128_ERR_TOL <= 1e-9

NAMES8, NAMES7 = ("fetch8", "kinova8"), ("kinova", "fetch")
RM_STEP = 0.25                                            # the roadmaps' edge step (tests/test_roadmap_moving.py STEP)
RM_WINDOWS = ((0.0, 0.5), (0.4, 0.6), (-0.1, 0.2))        # one per world
SLICE_T0 = np.array([0.0, 0.4, -0.3])
TREE = dict(step=0.5, edge_step=0.05, max_iterations=400, max_nodes=512)
TREE_WINDOW = (0.0, 0.5)
TREE_SEEDS = {"fetch8": 1, "kinova8": 1, "kinova": 1, "fetch": 1}
IK_SEEDS = np.array([11, 12, 13, 14], dtype=np.uint64)
IK_TOOL = np.array([0.03, -0.02, 0.11])                   # off the last joint's axis: with no tool point the last joint of these arms moves nothing
MARGIN = 1e-9


# ----------------------------------------------------------------------------------------------------------- scenes (the same in both halves)
def _arm(name):
    from test_roadmap import _limits, _robot, geometry, robot_dict
    robot = _robot(name)
    g = geometry(robot_dict(robot))
    lb, ub, cont = _limits(robot)
    sized = [l for l in range(g["J"]) if np.any(g["h"][l] != 0.0)]
    return dict(name=name, robot=robot, g=g, lb=lb, ub=ub, cont=cont, n=g["n"], J=g["J"], sized=sized)


def _roadmap_scene(a, N, k_max):
    """N seeded nodes with every node's k_max nearest neighbours, and W = 3 worlds of 5 boxes: far boxes only; a box about a link of node 7
    (static) that, in the moving form, rises through that link at 0.5 m/s in the middle of its window; 5 random boxes in
    random linear motion at 0.06 - 0.3 m/s."""
    from armour_amd.roadmap import uniform_roadmap
    from armour_amd.scenes import FAR_BOX
    from test_moving_audit import random_motion
    from test_tree_plan import box_at_link
    g = a["g"]
    nodes, edges = uniform_roadmap(N, 6.0, k_max, 5, a["lb"], a["ub"], a["cont"])
    rng = np.random.default_rng(17)
    far = np.tile(FAR_BOX, (5, 1))
    at_link = far.copy()
    at_link[0] = box_at_link(g, nodes[7], link=a["sized"][-2])
    at_link[0, [3, 7, 11]] = 0.25, 0.25, 0.25
    rnd = np.zeros((5, 12))                                  # on a ring about the base, clear of the first link, which no joint moves away
    angle, radius = rng.uniform(-np.pi, np.pi, 5), rng.uniform(0.45, 0.8, 5)
    rnd[:, 0], rnd[:, 1], rnd[:, 2] = radius * np.cos(angle), radius * np.sin(angle), rng.uniform(0.3, 1.2, 5)
    rnd[:, 3], rnd[:, 7], rnd[:, 11] = rng.uniform(0.15, 0.3, (3, 5))
    obs = np.stack([far, at_link, rnd])
    vel = random_motion(rng, obs)
    vel[0] = 0.0
    vel[1] = 0.0
    vel[1, 0] = [0.0, 0.0, 0.5]
    vel[2] *= 0.3
    moving = obs.copy()
    moving[1, 0, 0:3] -= vel[1, 0] * 0.5
    return dict(nodes=nodes, edges=edges, obs=obs, moving=moving, vel=vel)


def _decides(mask, what, least=0.1):
    """a verdict array that is compared must hold both verdicts, each on at least 10 % of its items"""
    share = float(np.asarray(mask, dtype=bool).mean())
    print(f"    {what}: {share:.0%} free of {np.asarray(mask).size}", flush=True)
    assert least <= share <= 1.0 - least, (what, share)


def _audit_case(a, P, seed):
    """P random pieces over 2 of the reference's worlds with a non-zero tube, the obstacles' velocities and the pieces' world times"""
    from test_moving_audit import random_motion
    from test_path_audit import _worlds, random_pieces
    from test_self_check import FOLDED
    rng = np.random.default_rng(seed)
    obs = _worlds()[[3, 57]]
    vel = random_motion(rng, obs)
    arrs = random_pieces(a["robot"], rng, P, still=0.3)
    if a["name"].startswith("kinova"):                       # every third piece starts near the fold of tests/test_self_check.py
        arrs[0][::3, :7] = FOLDED + rng.normal(size=(len(arrs[0][::3]), 7)) * 0.15
    world = (np.arange(P) % 2).astype(np.int32)
    t_world = rng.uniform(-1.0, 2.0, P)
    tube = 0.01 * (0.1 + rng.random((P, a["n"])))
    return dict(obs=obs, vel=vel, arrs=arrs, world=world, t_world=t_world, tube=tube, kr=np.full(a["n"], np.pi / 48))


def _self_tables(a):
    """(pairs, shrink) tables: the defaults, and the table of its own with a shrink that tests/test_self_check.py tests with"""
    from test_self_check import _variants
    return _variants(a["robot"], np.random.default_rng(3))


def _self_configs(a, N, seed=53):
    """random configurations; on the Kinova arms every eighth one is near the fold of tests/test_self_check.py, the last link inside the first"""
    from test_self_check import FOLDED
    rng = np.random.default_rng(seed)
    Q = a["lb"] + (a["ub"] - a["lb"]) * rng.random((N, a["n"]))
    if a["name"].startswith("kinova"):
        Q[::8, :7] = FOLDED + rng.normal(size=(len(Q[::8]), 7)) * 0.1
    return Q


def _tree_scene(a):
    """start, goal and a wall through the straight segment (tests/test_roadmap.py _wall_world, tests/test_tree_plan.py _fetch_world), and
    W = 3 static worlds: the wall, the empty world, a box on the start; and W = 2 moving worlds over TREE_WINDOW: the wall drifting among four
    small boxes in linear motion, and a box that arrives on a link of the goal configuration inside the window."""
    from armour_amd.scenes import FAR_BOX
    from test_roadmap import _wall_world
    from test_tree_moving import moving_worlds
    from test_tree_plan import _fetch_world, box_at_link
    g = a["g"]
    if a["name"].startswith("fetch"):
        s = _fetch_world(a["name"])
        start, goal, wall, link = s["start"], s["goal"], s["wall"], 5 + a["n"] - 7
    else:
        start, goal, wall, _ = _wall_world(g)
        wall, link = wall[None], 5
    if a["n"] == 8:                                          # the eighth joint turns too, by another angle than the seventh
        start, goal = start.copy(), goal.copy()
        start[7], goal[7] = 0.7, -0.5
    link = a["sized"][-1]                                    # the boxes on start and goal sit on the last link that has one: it decides the margins
    static = np.stack([wall, FAR_BOX[None], box_at_link(g, start, link)[None]])
    s = dict(robot=a["robot"], g=g, lb=a["lb"], ub=a["ub"], start=start, goal=goal, wall=wall)
    obs, vel = moving_worlds(s, 3, W=2)
    arriving = box_at_link(g, goal, link)
    obs[1], vel[1] = FAR_BOX, 0.0
    vel[1, 0] = [1.0, 0.0, 0.0]
    obs[1, 0] = arriving
    obs[1, 0, 0:3] -= vel[1, 0] * 0.3
    return dict(s, static=static, obs=obs, vel=vel, link=link, seed=TREE_SEEDS[a["name"]])


def _plan(sc, host, moving=False):
    from armour_amd.tree_planner import plan_trees
    if moving:
        return plan_trees(sc["robot"], sc["obs"], [sc["start"]] * 2, [sc["goal"]] * 2, [sc["seed"]] * 2, trees=True, host=host, velocity=sc["vel"],
                          t_from=TREE_WINDOW[0], t_to=TREE_WINDOW[1], **TREE)
    return plan_trees(sc["robot"], sc["static"], [sc["start"]] * 3, [sc["goal"]] * 3, [sc["seed"]] * 3, trees=True, host=host, **TREE)


def _shorten(sc, plans, host, moving=False):
    """passes = 2 on every path `plans` found -> (the worlds with a path, the ShortPaths)"""
    from armour_amd.tree_planner import shortcut_paths
    found = [w for w, p in enumerate(plans.paths) if p is not None]
    paths = [plans.paths[w] for w in found]
    if moving:
        return found, shortcut_paths(sc["robot"], sc["obs"][found], paths, edge_step=TREE["edge_step"], passes=2, host=host, velocity=sc["vel"][found],
                                     t_from=TREE_WINDOW[0], t_to=TREE_WINDOW[1])
    return found, shortcut_paths(sc["robot"], sc["static"][found], paths, edge_step=TREE["edge_step"], passes=2, host=host)


def _ik_scene(a, sc):
    """4 targets: the end effector of the tree scene's goal in the wall's world (reachable), a point out of reach, the end effector of the
    start inside a box that holds the last links, and the same point without a world; one world of two boxes for the moving form."""
    from test_ik import blocking_box, chain_np
    g = a["g"]
    ends = chain_np(g, np.stack([sc["goal"], sc["start"]]), IK_TOOL)[0]
    obs = np.stack([sc["wall"], blocking_box(g, ends[1])[None]])
    targets = np.vstack([ends[0], [3.0, 0.0, 0.0], ends[1], ends[1]])
    q_ref = np.vstack([sc["start"], sc["start"], np.zeros(a["n"]), np.zeros(a["n"])])
    moving = np.concatenate([sc["wall"], blocking_box(g, ends[1])[None]])[None]
    moving[0, 1, 0:3] += [0.0, 0.9, 0.0]
    vel = np.array([[[0.0, 0.05, 0.0], [0.0, -1.0, 0.0]]])       # the cube arrives about the start's end effector 0.9 s in
    return dict(obs=obs, targets=targets, q_ref=q_ref, world=np.array([0, 0, 1, -1]), moving=moving, vel=vel, window=(0.7, 1.0),
                moving_world=np.array([0, 0, 0, -1]), tool=IK_TOOL)


def _ik(a, ik, S, host, moving=False):
    from armour_amd.ik import solve_ik
    if moving:
        return solve_ik(a["robot"], ik["targets"], ik["q_ref"], ik["moving"], ik["moving_world"], IK_SEEDS, S=S, host=host, details=True, tool=ik["tool"], velocity=ik["vel"],
                        t_from=ik["window"][0], t_to=ik["window"][1])
    return solve_ik(a["robot"], ik["targets"], ik["q_ref"], ik["obs"], ik["world"], IK_SEEDS, S=S, host=host, details=True, tool=ik["tool"])


def _abi():
    assert _lib.MAXF == 8 and _lib.load().armour_abi_max_factors() == 8


# ----------------------------------------------------------------------------------------------------------- CPU: host entries against numpy
def _cpu_roadmap(a):
    from armour_amd.roadmap import Roadmap
    from test_path_audit import CL_TOL
    from test_roadmap import config_clearance, edge_free_np
    from test_roadmap_knn import knn_np, same
    from test_roadmap_moving import window_rule_np
    from test_roadmap_slices import arrival_np, bit, check_path, ones, search_case, some_extras, world_graph
    g = a["g"]
    sc = _roadmap_scene(a, 48, 5)
    nodes, edges, obs = sc["nodes"], sc["edges"], sc["obs"]
    rm = Roadmap(a["robot"], nodes, edges, continuous=a["cont"], edge_step=RM_STEP, host=True)
    assert (rm.N, rm.E) == (48, len(edges)) and len(edges) > 100
    # the node and edge check, static: zero velocity is the static rule for any window
    v = rm.check_moving(obs, np.zeros_like(sc["vel"]), 0.0, 0.0, clearance=True, host=True)
    for w in range(3):
        cl = config_clearance(g, nodes, obs[w])
        assert np.abs(cl).min() > MARGIN and np.abs(v["node_clearance"][w] - cl).max() <= CL_TOL
        assert np.array_equal(v["node_free"][w], cl > 0), (a["name"], w)
        for e, (i, j) in enumerate(edges):
            free, ecl = edge_free_np(g, nodes[i], nodes[j], obs[w], RM_STEP)
            assert abs(ecl) > MARGIN and bool(v["edge_free"][w, e]) == free, (a["name"], w, e, ecl)
    _decides(v["node_free"], "static nodes"), _decides(v["edge_free"], "static edges")
    # the window rule
    t0, t1 = np.array(RM_WINDOWS).T
    m = rm.check_moving(sc["moving"], sc["vel"], t0, t1, clearance=True, host=True)
    fast = rm.check_moving(sc["moving"], sc["vel"], t0, t1, host=True)
    assert np.array_equal(m["node_free"], fast["node_free"]) and np.array_equal(m["edge_free"], fast["edge_free"])
    for w in range(3):
        node_cl, edge_cl = window_rule_np(g, nodes, edges, sc["moving"][w], sc["vel"][w], t0[w], t1[w], RM_STEP)
        assert min(np.abs(node_cl).min(), np.abs(edge_cl).min()) > MARGIN, (a["name"], w)
        assert np.array_equal(m["node_free"][w], node_cl > 0) and np.array_equal(m["edge_free"][w], edge_cl > 0), (a["name"], w)
        assert np.abs(m["node_clearance"][w] - node_cl).max() <= CL_TOL
    _decides(m["node_free"], "moving nodes"), _decides(m["edge_free"], "moving edges")
    assert not (np.array_equal(m["node_free"][1], v["node_free"][1]) and np.array_equal(m["edge_free"][1], v["edge_free"][1]))   # the sweeping box is not the box at rest
    # time slices: bit k is the window check on slice k; then the search against the breadth-first search of the definition
    xw, xa, xb = some_extras(nodes, 3)
    for K, dt in ((1, 0.3), (64, 0.03)):
        s = rm.check_slices(sc["moving"], sc["vel"], SLICE_T0, dt, K, extra_world=xw, extra_a=xa, extra_b=xb, host=True)
        t = s["slice_times"]
        assert np.array_equal(t, SLICE_T0[:, None] + np.arange(K + 1)[None, :] * dt)
        for k in range(K):
            wv = rm.check_moving(sc["moving"], sc["vel"], t[:, k], t[:, k + 1], host=True)
            assert np.array_equal(bit(s["node_slices"], k), wv["node_free"]) and np.array_equal(bit(s["edge_slices"], k), wv["edge_free"]), (a["name"], K, k)
            for i in range(xw.size):
                assert bool(bit(s["extra_slices"][i:i + 1], k)[0]) == (rm.plan(int(xw[i]), xa[i], xb[i], connect_k=0) is not None), (a["name"], K, k, i)
        for fam in ("node_slices", "edge_slices"):
            assert (s[fam] != 0).any() and (s[fam] != np.uint64(ones(K))).any(), (a["name"], K, fam)
    assert ((s["edge_slices"] != 0) & (s["edge_slices"] != np.uint64(ones(64)))).any()   # an edge whose 64 slices differ
    K, step_len, reached = 64, 0.25, 0
    s, ar, extras, sm, gm = search_case(rm, sc["moving"], sc["vel"] * 0.5, SLICE_T0, 0.03, K, step_len, host=True)
    for w in range(3):
        mask, es = world_graph(rm, w, K, step_len, s["node_slices"], s["edge_slices"], sm, gm, extras)
        reach = arrival_np(rm.N, K, mask, es)
        assert [int(r) for r in ar["reach"][w]] == reach, (a["name"], w)
        want = (reach[rm.N + 1] & -reach[rm.N + 1]).bit_length() - 1
        assert ar["goal_slice"][w] == want and 1 <= ar["sweeps"][w] <= K + 1
        check_path(rm.N, K, mask, es, reach, want, ar["path_len"][w], ar["path_node"][w], ar["path_slice"][w])
        reached += want >= 0
    assert reached >= 1
    rm.close()
    # nearest neighbours
    rng = np.random.default_rng(4)
    big = a["lb"] + (a["ub"] - a["lb"]) * np.random.default_rng(3).random((300, a["n"]))
    queries = a["lb"] + (a["ub"] - a["lb"]) * rng.random((40, a["n"]))
    queries[:5] = big[10:15]
    excl = np.where(np.arange(40) < 5, np.arange(10, 50), -1).astype(np.int32)
    bare = Roadmap(a["robot"], big, np.zeros((0, 2), dtype=np.int32), continuous=a["cont"].astype(np.uint8), host=True)
    for k in (1, 8, 64):
        for radius in (np.inf, 3.0):
            for ex in (None, excl):
                assert same(bare.knn(queries, k, radius=radius, exclude=ex, host=True), knn_np(big, queries, a["cont"], k, radius, ex)), (a["name"], k, radius)
    count = bare.knn(queries, 8, radius=3.0, host=True)[2]
    assert count.min() < 8 and count.max() == 8, count                                     # the radius cuts some lists short and not others
    bare.close()
    print(f"  {a['name']}: roadmap create / check / window rule / slices / arrival / knn equal the restatements", flush=True)


def _cpu_audits(a):
    from armour_amd.path_audit import audit, audit_items, audit_moving, audit_self
    from armour_amd.self_check import check, edges_free_host
    from test_moving_audit import compare_moving
    from test_path_audit import CL_TOL, D, _compare, _piece, piece_items
    from test_self_check import audit_self_np, edge_self_free_np, self_check_np, self_clearances
    g, robot = a["g"], a["robot"]
    c = _audit_case(a, 40, 23)
    arrs, kr = c["arrs"], c["kr"]
    total, moving = [0, 0, 0], [0, 0, 0]
    for step, tb_ in ((0.02, None), (0.05, c["tube"])):
        res = audit(robot, c["obs"], c["world"], *arrs[:4], kr, D, arrs[4], arrs[5], tube=tb_, step=step, clearance=True, host=True)
        fast = audit(robot, c["obs"], c["world"], *arrs[:4], kr, D, arrs[4], arrs[5], tube=tb_, step=step, host=True)
        assert np.array_equal(res.verdict, fast.verdict) and np.array_equal(res.t_hit, fast.t_hit, equal_nan=True)
        total = [x + y for x, y in zip(total, _compare(res, g, c["obs"], c["world"], arrs, kr, step, tb_, (a["name"], step)))]
        S = audit_items(robot, *arrs[:4], kr, D, arrs[4], arrs[5], step=step)
        assert np.array_equal(S, [piece_items(g, _piece(arrs, p), kr, D, step)[0].size for p in range(40)])
        res = audit_moving(robot, c["obs"], c["vel"], c["world"], c["t_world"], *arrs[:4], kr, D, arrs[4], arrs[5], tube=tb_, step=step, clearance=True, host=True)
        moving = [x + y for x, y in zip(moving, compare_moving(res, g, c["obs"], c["vel"], c["world"], c["t_world"], arrs, kr, step, tb_, (a["name"], step)))]
    assert min(total[:2]) > 0 and min(moving[:2]) > 0, (total, moving)
    # self-collision: configurations, edges, pieces
    Q = _self_configs(a, 257)
    for pairs, shrink in _self_tables(a)[::-1]:                 # (the defaults last: the checks below go on with them)
        cl, worst, first = self_check_np(g, Q, pairs, shrink)
        full = check(robot, Q, pairs=pairs, shrink=shrink, clearance=True, host=True)
        fast = check(robot, Q, pairs=pairs, shrink=shrink, host=True)
        each = self_clearances(g, Q, pairs, shrink)
        sure = np.abs(each).min(1) > MARGIN
        assert sure.all() and np.abs(full.clearance - cl).max() <= CL_TOL
        assert np.array_equal(full.free, cl > 0) and np.array_equal(fast.free, cl > 0) and np.array_equal(fast.worst_pair, first)
        gap = np.sort(each, axis=1)
        clear_min = gap[:, 1] - gap[:, 0] > MARGIN
        assert np.array_equal(full.worst_pair[clear_min], worst[clear_min])
    _decides(fast.free, "self-check configurations")
    qa = _self_configs(a, 64, 43)
    qb = qa + np.random.default_rng(44).uniform(-0.4, 0.4, qa.shape)
    free = edges_free_host(robot, qa, qb, edge_step=0.05, continuous=a["cont"], pairs=pairs, shrink=shrink)
    for e in range(64):
        want, margin = edge_self_free_np(g, qa[e], qb[e], 0.05, pairs, shrink)
        assert margin > MARGIN and free[e] == want, (a["name"], e)
    _decides(free, "self-check edges")
    res = audit_self(robot, *arrs[:4], kr, D, arrs[4], arrs[5], tube=c["tube"], step=0.02, pairs=pairs, shrink=shrink, clearance=True, host=True)
    for p in range(40):
        vd, th, scl, margin = audit_self_np(g, _piece(arrs, p), kr, D, 0.02, c["tube"][p], pairs, shrink)
        if margin > MARGIN:
            assert res.verdict[p] == vd and ((np.isnan(th) and np.isnan(res.t_hit[p])) or res.t_hit[p] == th), (a["name"], p)
        assert abs(res.clearance[p] - scl) <= CL_TOL
    assert len(set(res.verdict.tolist())) >= 2, np.bincount(res.verdict)
    print(f"  {a['name']}: audits (static {total}, moving {moving}, self {np.bincount(res.verdict, minlength=3).tolist()}) and self-checks equal the restatements", flush=True)


def _cpu_trees(a):
    import test_path_shortcut as tps
    import test_tree_plan as ttp
    from test_tree_moving import plan_moving_np, shortcut_moving_np
    mp = pytest.MonkeyPatch()
    g = a["g"]
    sc = _tree_scene(a)
    plans = _plan(sc, True)
    assert (plans.margin > MARGIN).all(), plans.margin
    for w in range(3):
        ref = ttp.plan_np(g, sc["static"][w], sc["start"], sc["goal"], sc["seed"], a["lb"], a["ub"])
        ttp.assert_equals_restatement(plans, w, ref)
        assert ref["margin"] == np.inf or abs(plans.margin[w] - ref["margin"]) <= 1e-12
    assert list(plans.status) == [1, 1, 2] and plans.iterations[0] >= 1 and len(plans.paths[0]) > 2      # the wall world's trees had to grow
    moving = _plan(sc, True, moving=True)
    assert (moving.margin > MARGIN).all(), moving.margin
    for w in range(2):
        ref = plan_moving_np(mp, g, sc["obs"][w], sc["vel"][w], TREE_WINDOW, sc["start"], sc["goal"], sc["seed"], a["lb"], a["ub"])
        ttp.assert_equals_restatement(moving, w, ref)
        assert abs(moving.margin[w] - ref["margin"]) <= 1e-12
    assert list(moving.status) == [1, 3] and len(moving.paths[0]) > 2, (moving.status, moving.iterations)
    found, short = _shorten(sc, plans, True)
    assert found == [0, 1]
    for i, w in enumerate(found):
        tps.assert_equals_restatement(short, i, tps.shortcut_np(g, sc["static"][w], plans.paths[w], 2))
    assert short.status[1] == 0 and ttp._same_bits(short.paths[1], plans.paths[1])        # the empty world's direct edge stays
    assert 2 < len(short.paths[0]) <= len(plans.paths[0]) and short.length_out[0] < short.length_in[0]
    found, mshort = _shorten(sc, moving, True, moving=True)
    assert found == [0]
    tps.assert_equals_restatement(mshort, 0, shortcut_moving_np(mp, g, sc["obs"][0], sc["vel"][0], TREE_WINDOW, moving.paths[0], 2))
    print(f"  {a['name']}: tree plans (static {plans.status.tolist()} in {plans.iterations.tolist()} iterations, moving {moving.status.tolist()} in "
          f"{moving.iterations.tolist()}) and shortened paths ({len(plans.paths[0])} -> {len(short.paths[0])} points) equal the restatements", flush=True)
    return sc


def _cpu_ik(a, sc):
    import test_ik as tik
    from armour_amd.ik import end_effector
    from test_tree_moving import window_clearance
    g, n = a["g"], a["n"]
    rng = np.random.default_rng(3)
    Q = rng.uniform(np.maximum(a["lb"], -np.pi), np.minimum(a["ub"], np.pi), (40, n))
    for tool in (np.zeros(3), np.array([0.03, -0.02, 0.11])):
        p, jac = end_effector(a["robot"], Q, tool=tool, jacobian=True)
        pe, c = tik.chain_np(g, Q, tool)
        assert p.shape == (40, 3) and jac.shape == (40, 3, n)
        assert np.abs(p - pe).max() <= 1e-13 and np.abs(jac - np.swapaxes(c, 1, 2)).max() <= 1e-13
        assert not tool.any() or np.abs(jac).max(axis=(0, 1)).min() > 1e-3                 # every factor is actuated: no zero column
    ik = _ik_scene(a, sc)

    def against_restatement(host, ref, what):
        assert (host.margin > MARGIN).all(), host.margin
        cl = np.abs(ref["clearance"])
        finite = np.isfinite(np.where(np.isnan(cl), np.inf, cl)).any(axis=1)
        assert np.nanmin(cl) > MARGIN and np.abs(np.nanmin(cl[finite], axis=1) - host.margin[finite]).max() <= 1e-11
        assert np.array_equal(host.status, ref["status"]) and np.array_equal(host.best, ref["best"]), (what, host.status, ref["status"])
        same = (host.iterations == ref["iterations"]) & ((host.flags & 1) == (ref["flags"] & 1))
        assert (~same).mean() <= 0.01, (what, (~same).sum())
        assert np.array_equal(host.flags[same], ref["flags"][same])
        dq, de = np.abs(host.q_all - ref["q_all"])[same].max(), np.abs(host.err - ref["err"])[same].max()
        print(f"    {what}: statuses {host.status.tolist()}, max |dq| = {dq:.3g}, max |derr| = {de:.3g}, items left out {(~same).sum()}", flush=True)
        assert dq <= tik.Q_TOL and de <= tik.ERR_TOL, (what, dq, de)

    for S in (1, 8, 32):
        host = _ik(a, ik, S, True)
        ref = tik.solve_np(g, ik["targets"], ik["q_ref"], ik["obs"], ik["world"], IK_SEEDS, S, a["lb"], a["ub"], tool=ik["tool"])
        against_restatement(host, ref, f"{a['name']} S = {S}")
    assert sorted(set(host.status.tolist())) == [0, 1, 2], host.status
    host = _ik(a, ik, 8, True, moving=True)
    with pytest.MonkeyPatch().context() as m:
        mid_half = window_clearance(ik["vel"][0], *ik["window"])
        m.setattr(tik, "config_clearance", lambda g_, Q_, Z, r=None: mid_half(g_, Q_, Z, r) if np.asarray(Z).size else np.full(np.asarray(Q_).shape[0], np.inf))
        ref = tik.solve_np(g, ik["targets"], ik["q_ref"], ik["moving"], ik["moving_world"], IK_SEEDS, 8, a["lb"], a["ub"], tool=ik["tool"])
    against_restatement(host, ref, f"{a['name']} moving")
    assert host.status[2] == 2 and host.status[3] == 1                                      # the cube is about the point within the window


def _body_cpu_restatements():
    """(runs with ARMOUR_KEY128=1)  every host entry against its numpy restatement on fetch8 and kinova8"""
    _abi()
    for name in NAMES8:
        a = _arm(name)
        assert (a["n"], a["J"]) == {"fetch8": (8, 9), "kinova8": (8, 8)}[name]
        _cpu_roadmap(a)
        _cpu_audits(a)
        _cpu_ik(a, _cpu_trees(a))
    print("planner k128 cpu ok", flush=True)


# ----------------------------------------------------------------------------------------------------------- the dead slot
def _flat_paths(prefix, paths, out):
    out[prefix + "_points"] = np.array([-1 if p is None else len(p) for p in paths], dtype=np.int32)
    out[prefix + "_path"] = np.concatenate([np.zeros((0, 1)) if p is None else p.reshape(-1, 1) for p in paths])


def _host_results(name):
    """Every host entry once on the 7-factor robot `name`, in the ABI of this process -> dict of arrays"""
    from armour_amd.ik import end_effector
    from armour_amd.path_audit import audit, audit_moving, audit_self
    from armour_amd.roadmap import Roadmap
    from armour_amd.self_check import check, edges_free_host
    from test_path_audit import D
    from test_roadmap_slices import search_case
    a = _arm(name)
    robot, out = a["robot"], {}
    sc = _roadmap_scene(a, 48, 5)
    rm = Roadmap(robot, sc["nodes"], sc["edges"], continuous=a["cont"], edge_step=RM_STEP, host=True)
    t0, t1 = np.array(RM_WINDOWS).T
    for key, v in (("static", rm.check_moving(sc["obs"], np.zeros_like(sc["vel"]), 0.0, 0.0, clearance=True, host=True)),
                   ("moving", rm.check_moving(sc["moving"], sc["vel"], t0, t1, clearance=True, host=True))):
        out.update({f"rm_{key}_{k}": v[k] for k in ("node_free", "edge_free", "node_clearance")})
    s, ar, *_ = search_case(rm, sc["moving"], sc["vel"] * 0.5, SLICE_T0, 0.03, 64, 0.25, host=True)
    out.update({f"slices_{k}": s[k] for k in ("node_slices", "edge_slices", "extra_slices", "slice_times")})
    out.update({f"arrival_{k}": ar[k] for k in ("reach", "goal_slice", "path_len", "path_node", "path_slice", "sweeps")})
    queries = a["lb"] + (a["ub"] - a["lb"]) * np.random.default_rng(4).random((40, a["n"]))
    out["knn_index"], out["knn_dist"], out["knn_count"] = rm.knn(queries, 8, radius=3.0, host=True)
    rm.close()
    c = _audit_case(a, 40, 23)
    arrs, kr = c["arrs"], c["kr"]
    pairs, shrink = _self_tables(a)[0]
    for key, res in (("audit", audit(robot, c["obs"], c["world"], *arrs[:4], kr, D, arrs[4], arrs[5], tube=c["tube"], step=0.05, clearance=True, host=True)),
                     ("audit_moving", audit_moving(robot, c["obs"], c["vel"], c["world"], c["t_world"], *arrs[:4], kr, D, arrs[4], arrs[5], tube=c["tube"], step=0.05,
                                                   clearance=True, host=True)),
                     ("audit_self", audit_self(robot, *arrs[:4], kr, D, arrs[4], arrs[5], tube=c["tube"], step=0.02, pairs=pairs, shrink=shrink, clearance=True, host=True))):
        out.update({f"{key}_{k}": getattr(res, k) for k in ("verdict", "t_hit", "clearance")})
    Q = _self_configs(a, 257)
    res = check(robot, Q, pairs=pairs, shrink=shrink, clearance=True, host=True)
    out.update(self_free=res.free, self_worst=res.worst_pair, self_clearance=res.clearance)
    out["self_edges"] = edges_free_host(robot, Q[:64], Q[64:128] * 0.9 + Q[:64] * 0.1, edge_step=0.05, continuous=a["cont"], pairs=pairs, shrink=shrink)
    ts = _tree_scene(a)
    for key, moving in (("tree", False), ("tree_moving", True)):
        plans = _plan(ts, True, moving)
        out.update({f"{key}_{k}": getattr(plans, k) for k in ("status", "iterations", "count", "nodes", "parent", "margin")})
        _flat_paths(key, plans.paths, out)
        _, short = _shorten(ts, plans, True, moving)
        out.update({f"{key}_short_{k}": getattr(short, k) for k in ("status", "first_bad", "passes_done", "length_in", "length_out", "margin")})
        _flat_paths(key + "_short", short.paths, out)
    ik = _ik_scene(a, ts)
    for key, moving in (("ik", False), ("ik_moving", True)):
        res = _ik(a, ik, 8, True, moving)
        out.update({f"{key}_{k}": getattr(res, k) for k in ("status", "best", "q", "q_all", "err", "iterations", "flags", "margin")})
    out["ee_p"], out["ee_jac"] = end_effector(robot, Q[:40], tool=np.array([0.03, -0.02, 0.11]), jacobian=True)
    return out


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _different_fields(got, want):
    return [k for k in want.files if got[k].shape != want[k].shape or got[k].dtype != want[k].dtype or not np.array_equal(_bits(got[k]), _bits(want[k]))]


def _body_cpu_dead_slot(folder):
    """(runs with ARMOUR_KEY128=1)  kinova and fetch through the 8-factor library: every host entry's result equals the shipped library's"""
    _abi()
    for name in NAMES7:
        want = np.load(os.path.join(folder, name + ".npz"))
        got = _host_results(name)
        assert sorted(got) == sorted(want.files)
        bad = _different_fields(got, want)
        print(f"  {name}: {len(want.files)} fields of the host entries, different from the shipped ABI's: {bad}", flush=True)
        assert not bad, (name, bad)
        assert sorted(set(want["tree_status"].tolist()) | set(want["tree_moving_status"].tolist())) == [1, 2, 3]
        assert sorted(set(want["ik_status"].tolist())) == [0, 1, 2]
    print("planner k128 dead slot ok", flush=True)


# ----------------------------------------------------------------------------------------------------------- GPU: device entries against host twins
def _device_roadmap_results(a, sc):
    """the node check and the nearest neighbours of the dead-slot comparison on a device handle -> dict of arrays"""
    from armour_amd.roadmap import Roadmap
    rm = Roadmap(a["robot"], sc["nodes"], sc["edges"], continuous=a["cont"], edge_step=RM_STEP)
    v = rm.check(sc["obs"], clearance=True)
    queries = a["lb"] + (a["ub"] - a["lb"]) * np.random.default_rng(4).random((40, a["n"]))
    index, dist, count = rm.knn(queries, 8, radius=3.0)
    rm.close()
    return dict(node_free=v["node_free"], edge_free=v["edge_free"], node_clearance=v["node_clearance"], knn_index=index, knn_dist=dist, knn_count=count)


def _device_tree_results(a, ts):
    plans = _plan(ts, False)
    out = {k: getattr(plans, k) for k in ("status", "iterations", "count", "nodes", "parent")}
    _flat_paths("tree", plans.paths, out)
    return out


def _same_masks(x, y):
    return np.array_equal(x["node_free"], y["node_free"]) and np.array_equal(x["edge_free"], y["edge_free"])


def _body_gpu_roadmap(shipped):
    """(runs with ARMOUR_KEY128=1)  roadmap.hip, roadmap_slices.hip, roadmap_knn.hip"""
    from armour_amd.roadmap import Roadmap
    from test_path_audit import CL_TOL
    from test_roadmap_knn import same
    from test_roadmap_slices import search_case, some_extras
    _abi()
    t0, t1 = np.array(RM_WINDOWS).T
    for name in NAMES8:
        a = _arm(name)
        sc = _roadmap_scene(a, 300, 3)
        nodes, edges = sc["nodes"], sc["edges"]
        dev = Roadmap(a["robot"], nodes, edges, continuous=a["cont"], edge_step=RM_STEP)
        host = Roadmap(a["robot"], nodes, edges, continuous=a["cont"], edge_step=RM_STEP, host=True)
        assert dev.N == 300 and dev.E == len(edges) > 300
        # node and edge check, static (the host loop at zero velocity is the static rule) and moving
        hs = host.check_moving(sc["obs"], np.zeros_like(sc["vel"]), 0.0, 0.0, clearance=True, host=True)
        ds, fast = dev.check(sc["obs"], clearance=True), dev.check(sc["obs"])
        assert _same_masks(ds, hs) and _same_masks(fast, hs), name
        assert np.abs(ds["node_clearance"] - hs["node_clearance"]).max() <= CL_TOL
        _decides(hs["node_free"], "static nodes"), _decides(hs["edge_free"], "static edges")
        hm = host.check_moving(sc["moving"], sc["vel"], t0, t1, clearance=True, host=True)
        dm, fast = dev.check_moving(sc["moving"], sc["vel"], t0, t1, clearance=True), dev.check_moving(sc["moving"], sc["vel"], t0, t1)
        assert _same_masks(dm, hm) and _same_masks(fast, hm), name
        assert np.abs(dm["node_clearance"] - hm["node_clearance"]).max() <= CL_TOL
        _decides(hm["node_free"], "moving nodes"), _decides(hm["edge_free"], "moving edges")
        # batched joins after the moving check: an edge start -> x is free exactly when the host handle's plan(connect_k = 0) finds the direct edge
        rng = np.random.default_rng(3)
        world = np.array([0, 1, 2, 1], dtype=np.int32)
        starts = nodes[rng.integers(0, 300, 4)] + rng.normal(scale=0.05, size=(4, a["n"]))
        goals = nodes[rng.integers(0, 300, 3)] + rng.normal(scale=0.05, size=(3, a["n"]))
        got = dev.connect_many(world, starts, targets=goals[world], connect_k=6)
        oks = []
        for i, w in enumerate(world):
            assert bool(got["direct"][i]) == (host.plan(int(w), starts[i], goals[w], connect_k=0) is not None), (name, i)
            for c in range(got["count"][i]):
                v = int(got["node"][i, c])
                assert hm["node_free"][w, v]
                ok = host.plan(int(w), starts[i], nodes[v], connect_k=0) is not None
                assert bool(got["edge_ok"][i, c]) == ok, (name, i, c)
                oks.append(ok)
        assert 0 < sum(oks) < len(oks), (name, oks)
        dev.field(goals, connect_k=6)
        many = dev.descend_many(world, starts, connect_k=6)
        for i, w in enumerate(world):
            path, length = dev.descend(int(w), starts[i], connect_k=6)
            assert (path is None) == (many[i][0] is None) and np.float64(length).tobytes() == np.float64(many[i][1]).tobytes(), (name, i)
            assert path is None or np.array_equal(path, many[i][0]), (name, i)
        assert any(p is not None for p, _ in many), name
        # slices and the search on them
        xw, xa, xb = some_extras(nodes, 3)
        for K, dt in ((1, 0.3), (64, 0.03)):
            d = dev.check_slices(sc["moving"], sc["vel"], SLICE_T0, dt, K, extra_world=xw, extra_a=xa, extra_b=xb)
            h = host.check_slices(sc["moving"], sc["vel"], SLICE_T0, dt, K, extra_world=xw, extra_a=xa, extra_b=xb, host=True)
            for fam in ("node_slices", "edge_slices", "extra_slices", "slice_times"):
                assert np.array_equal(d[fam], h[fam]), (name, K, fam)
            full = np.uint64((1 << K) - 1)
            assert (h["edge_slices"] != 0).any() and (h["edge_slices"] != full).any() and (h["node_slices"] != 0).any() and (h["node_slices"] != full).any()
        assert ((h["edge_slices"] != 0) & (h["edge_slices"] != full)).any()
        _, d, *_ = search_case(dev, sc["moving"], sc["vel"] * 0.5, SLICE_T0, 0.03, 64, 0.25, host=False)
        _, h, *_ = search_case(host, sc["moving"], sc["vel"] * 0.5, SLICE_T0, 0.03, 64, 0.25, host=True)
        for key in ("reach", "goal_slice", "path_len", "path_node", "path_slice"):
            assert np.array_equal(d[key], h[key]), (name, key)
        assert (h["goal_slice"] >= 0).any(), h["goal_slice"]
        # nearest neighbours: both launch shapes, k = 1 and the cap, with and without a radius
        for Q in (3, 2048):
            queries = a["lb"] + (a["ub"] - a["lb"]) * np.random.default_rng(Q).random((Q, a["n"]))
            queries[0] = nodes[10]
            for k, radius in ((1, np.inf), (64, 4.0), (64, np.inf)):
                hk = host.knn(queries, k, radius=radius, host=True)
                assert same(dev.knn(queries, k, radius=radius), hk), (name, Q, k, radius)
            cut = host.knn(queries, 64, radius=4.0, host=True)[2]
            assert Q == 3 or (cut.min() < 64 and cut.max() > 0), (cut.min(), cut.max())
        dev.close(), host.close()
        print(f"  {name}: node / edge check, window rule, joins, slices, arrival and knn equal the host twins", flush=True)
    # the dead slot: the Kinova through this library, device against this library's host twin, and (printed) against the shipped ABI's device
    a = _arm("kinova")
    sc = _roadmap_scene(a, 300, 3)
    got = _device_roadmap_results(a, sc)
    host = Roadmap(a["robot"], sc["nodes"], sc["edges"], continuous=a["cont"], edge_step=RM_STEP, host=True)
    hs = host.check_moving(sc["obs"], np.zeros_like(sc["vel"]), 0.0, 0.0, clearance=True, host=True)
    assert _same_masks(got, hs) and np.abs(got["node_clearance"] - hs["node_clearance"]).max() <= CL_TOL
    _decides(hs["node_free"], "kinova static nodes"), _decides(hs["edge_free"], "kinova static edges")
    queries = a["lb"] + (a["ub"] - a["lb"]) * np.random.default_rng(4).random((40, a["n"]))
    assert same((got["knn_index"], got["knn_dist"], got["knn_count"]), host.knn(queries, 8, radius=3.0, host=True))
    host.close()
    print(f"  kinova: device fields different from the shipped ABI's device results: {_different_fields(got, np.load(shipped))}", flush=True)
    print("planner k128 gpu roadmap ok", flush=True)


def _body_gpu_audits():
    """(runs with ARMOUR_KEY128=1)  path_audit.hip and self_check.hip"""
    from armour_amd.path_audit import audit, audit_moving, audit_self
    from armour_amd.roadmap import Roadmap, uniform_roadmap
    from armour_amd.self_check import check, edges_free_host
    from test_path_audit import CL_TOL, D
    from test_self_check import self_check_np
    _abi()

    def same(dev, host, what):
        assert np.array_equal(dev.verdict, host.verdict) and np.array_equal(dev.t_hit, host.t_hit, equal_nan=True), (what, dev.verdict, host.verdict)
        assert dev.clearance is None or np.abs(dev.clearance - host.clearance).max() <= CL_TOL, what
        share = np.bincount(host.verdict, minlength=3) / host.verdict.size
        print(f"    {what}: verdicts {np.bincount(host.verdict, minlength=3).tolist()}", flush=True)
        assert (share >= 0.1).sum() >= 2, (what, share)

    for name in NAMES8:
        a = _arm(name)
        robot = a["robot"]
        c = _audit_case(a, 6, {"fetch8": 23, "kinova8": 23}[name])
        arrs, kr = c["arrs"], c["kr"]
        pairs, shrink = _self_tables(a)[0]
        for clearance in (True, False):
            kw = dict(tube=c["tube"], step=0.02, clearance=clearance)
            same(audit(robot, c["obs"], c["world"], *arrs[:4], kr, D, arrs[4], arrs[5], **kw),
                 audit(robot, c["obs"], c["world"], *arrs[:4], kr, D, arrs[4], arrs[5], host=True, **kw), (name, "static audit"))
            same(audit_moving(robot, c["obs"], c["vel"], c["world"], c["t_world"], *arrs[:4], kr, D, arrs[4], arrs[5], **kw),
                 audit_moving(robot, c["obs"], c["vel"], c["world"], c["t_world"], *arrs[:4], kr, D, arrs[4], arrs[5], host=True, **kw), (name, "moving audit"))
            same(audit_self(robot, *arrs[:4], kr, D, arrs[4], arrs[5], pairs=pairs, shrink=shrink, **kw),
                 audit_self(robot, *arrs[:4], kr, D, arrs[4], arrs[5], pairs=pairs, shrink=shrink, host=True, **kw), (name, "self audit"))
        Q = _self_configs(a, 257)
        for pairs, shrink in _self_tables(a)[::-1]:                 # (the defaults last: the checks below go on with them)
            cl, _, _ = self_check_np(a["g"], Q, pairs, shrink)
            for N in (1, 256, 257):
                dev, host = check(robot, Q[:N], pairs=pairs, shrink=shrink), check(robot, Q[:N], pairs=pairs, shrink=shrink, host=True)
                assert np.array_equal(dev.free, host.free) and np.array_equal(dev.worst_pair, host.worst_pair), (name, N)
                devc, hostc = check(robot, Q[:N], pairs=pairs, shrink=shrink, clearance=True), check(robot, Q[:N], pairs=pairs, shrink=shrink, clearance=True, host=True)
                assert np.array_equal(devc.free, hostc.free) and np.array_equal(devc.worst_pair, hostc.worst_pair), (name, N)
                assert np.abs(devc.clearance - cl[:N]).max() <= CL_TOL, (name, N)
        _decides(host.free, "self-check configurations")
        nodes, edges = uniform_roadmap(257, 6.0, 1, 5, a["lb"], a["ub"], a["cont"])
        edges = edges[:64]
        rm = Roadmap(robot, Q, edges, continuous=a["cont"], edge_step=0.05)
        s1 = rm.check_self(pairs=pairs, shrink=shrink, clearance=True)
        assert np.array_equal(s1["node_free"], hostc.free) and np.abs(s1["node_clearance"] - hostc.clearance).max() <= CL_TOL
        want = edges_free_host(robot, Q[edges[:, 0]], Q[edges[:, 1]], edge_step=0.05, continuous=a["cont"], pairs=pairs, shrink=shrink)
        assert len(edges) == 64 and np.array_equal(s1["edge_free"], want)
        _decides(want, "self-check edges")
        rm.close()
        print(f"  {name}: static, moving and self audits, self-checks of configurations and edges equal the host twins", flush=True)
    print("planner k128 gpu audits ok", flush=True)


def _body_gpu_trees(shipped):
    """(runs with ARMOUR_KEY128=1)  tree_plan.hip and path_shortcut.hip"""
    from test_path_shortcut_gpu import assert_same
    from test_tree_plan import assert_same_plans
    _abi()
    statuses = set()
    for name in NAMES8 + ("kinova",):
        a = _arm(name)
        sc = _tree_scene(a)
        for moving, W in ((False, 3), (True, 2)):
            host = _plan(sc, True, moving)
            assert (host.margin > MARGIN).all(), (name, host.margin)
            dev = _plan(sc, False, moving)
            for w in range(W):
                assert_same_plans(dev, w, host, w)
            assert dev.ms > 0.0 and dev.margin is None and len(host.paths[0]) > 2
            statuses |= set(host.status.tolist())
            found, hshort = _shorten(sc, host, True, moving)
            assert (hshort.margin > MARGIN).all(), (name, hshort.margin)
            _, dshort = _shorten(sc, dev, False, moving)
            assert_same(dshort, hshort, range(len(found)))
            assert dshort.ms > 0.0 and (hshort.passes_done == 2).all() and hshort.length_out[0] < hshort.length_in[0]
            print(f"  {name}{' moving' if moving else ''}: statuses {host.status.tolist()}, iterations {host.iterations.tolist()}, nodes {host.count.tolist()}, "
                  f"shortened {[len(host.paths[w]) for w in found]} -> {[len(p) for p in hshort.paths]} points: device equals host twin", flush=True)
        if name == "kinova":
            print(f"  kinova: device fields different from the shipped ABI's device results: {_different_fields(_device_tree_results(a, sc), np.load(shipped))}", flush=True)
    assert len(statuses) >= 3, statuses
    print("planner k128 gpu trees ok", flush=True)


def _body_gpu_ik():
    """(runs with ARMOUR_KEY128=1)  ik.hip"""
    from test_ik_gpu import assert_device_equals_twin
    _abi()
    for name in NAMES8:
        a = _arm(name)
        ik = _ik_scene(a, _tree_scene(a))
        for S, moving in ((1, False), (8, False), (200, False), (8, True)):
            host = _ik(a, ik, S, True, moving)
            assert (host.margin > MARGIN).all(), (name, S, host.margin)
            dev = _ik(a, ik, S, False, moving)
            assert_device_equals_twin(dev, host, f"{name} S = {S}{' moving' if moving else ''}", q_tol=K128_Q_TOL, err_tol=K128_ERR_TOL)
            assert S == 1 or sorted(set(host.status.tolist())) == [0, 1, 2], (name, S, host.status)
    print("planner k128 gpu ik ok", flush=True)


# ----------------------------------------------------------------------------------------------------------- the pytest functions
def _run_k128(call):
    env = dict(os.environ, ARMOUR_KEY128="1")
    env.pop("ARMOUR_HIP_LIB", None)
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_planner_k128 as t; t.%s" % (ROOT, os.path.join(ROOT, "tests"), call)
    return subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)


def _passed(r, last):
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith(last), r.stdout[-3000:] + r.stderr[-3000:]


def test_host_entries_equal_their_restatements_on_eight_factor_arms():
    _passed(_run_k128("_body_cpu_restatements()"), "planner k128 cpu ok")


def test_seven_factor_robots_in_the_eight_factor_library_equal_the_shipped_library(tmp_path):
    assert _lib.MAXF == 7
    for name in NAMES7:
        np.savez(str(tmp_path / (name + ".npz")), **_host_results(name))
    _passed(_run_k128("_body_cpu_dead_slot(%r)" % str(tmp_path)), "planner k128 dead slot ok")


@pytest.mark.gpu
def test_device_roadmap_slices_and_knn_equal_the_host_twins(tmp_path):
    a = _arm("kinova")
    path = str(tmp_path / "kinova_device.npz")
    np.savez(path, **_device_roadmap_results(a, _roadmap_scene(a, 300, 3)))
    _passed(_run_k128("_body_gpu_roadmap(%r)" % path), "planner k128 gpu roadmap ok")


@pytest.mark.gpu
def test_device_audits_and_self_checks_equal_the_host_twins():
    _passed(_run_k128("_body_gpu_audits()"), "planner k128 gpu audits ok")


@pytest.mark.gpu
def test_device_tree_plans_and_shortened_paths_equal_the_host_twins(tmp_path):
    a = _arm("kinova")
    path = str(tmp_path / "kinova_device.npz")
    np.savez(path, **_device_tree_results(a, _tree_scene(a)))
    _passed(_run_k128("_body_gpu_trees(%r)" % path), "planner k128 gpu trees ok")


@pytest.mark.gpu
def test_device_inverse_kinematics_equals_the_host_twin():
    _passed(_run_k128("_body_gpu_ik()"), "planner k128 gpu ik ok")
