"""Roadmap high-level planner (include/armour_hip.h armour_roadmap_*, armour_amd/roadmap.py).

The node and edge rules are restated below in numpy, in the library's order of operations (so that node clearances agree to rounding
of sin / cos), and the restatement is itself checked against an independent membership LP.  CPU tests: the restatement, the soundness
of the displacement bound rho, the sampler and the waypoint rule.  GPU tests: the device verdicts against the restatement, against the
reach-set pipeline, batched against one-by-one, and planning around a wall."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

DEGENERATE = 1e-18


# ----------------------------------------------------------------------------------------------------------- numpy restatement
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def matmul3(A, B):
    out = np.empty(np.broadcast_shapes(A.shape, B.shape))
    for i in range(3):
        for j in range(3):
            out[..., i, j] = (A[..., i, 0] * B[..., 0, j] + A[..., i, 1] * B[..., 1, j]) + A[..., i, 2] * B[..., 2, j]
    return out


def geometry(robot):
    """The robot as the rule reads it (plain arrays, so that a preset from the other ABI can be passed as a dict)."""
    from armour_amd.robot_geometry import rpy_matrix
    J, n = robot["J"], robot["n"]
    rots = np.array(robot["rots"][:3 * J]).reshape(J, 3)
    g = dict(J=J, n=n, axes=np.array(robot["axes"][:J]), T0=np.stack([rpy_matrix(*r) for r in rots]),
             trans=np.array(robot["trans"][:3 * J]).reshape(J, 3), c=np.array(robot["center"][:3 * J]).reshape(J, 3),
             h=np.array(robot["half"][:3 * J]).reshape(J, 3), cont=np.array(robot["continuous"][:n]).astype(bool))
    rho = np.zeros((n, J))
    for j in range(n):
        for l in range(j, J):
            acc = 0.0
            for i in range(j + 1, l + 1):
                acc += np.sqrt(dot3(g["trans"][i], g["trans"][i]))
            rho[j, l] = acc + np.sqrt(dot3(g["c"][l], g["c"][l])) + np.sqrt(dot3(g["h"][l], g["h"][l]))
    g["rho"] = rho
    return g


def robot_dict(r):
    return dict(J=r.num_joints, n=r.num_factors, axes=list(r.axes), rots=list(r.rots), trans=list(r.trans),
                center=list(r.link_zonotope_center), half=list(r.link_zonotope_generators), continuous=list(r.continuous))


def link_boxes(g, Q):
    """Q [K,n] -> link frame origins p [K,J,3], rotations R [K,J,3,3], box centres x [K,J,3]."""
    Q = np.asarray(Q, dtype=np.float64)
    K = Q.shape[0]
    R = np.broadcast_to(np.eye(3), (K, 3, 3)).copy()
    p = np.zeros((K, 3))
    P, Rs, X = [], [], []
    for l in range(g["J"]):
        t = np.stack([(R[:, i, 0] * g["trans"][l, 0] + R[:, i, 1] * g["trans"][l, 1]) + R[:, i, 2] * g["trans"][l, 2] for i in range(3)], -1)
        p = p + t
        A = matmul3(R, g["T0"][l])
        ax = int(g["axes"][l])
        if ax != 0 and l < g["n"]:
            c, s = np.cos(Q[:, l]), np.sin(Q[:, l]) * (1.0 if ax > 0 else -1.0)
            Rot = np.zeros((K, 3, 3))
            e = abs(ax) - 1
            i1, i2 = (e + 1) % 3, (e + 2) % 3
            Rot[:, e, e] = 1.0
            Rot[:, i1, i1], Rot[:, i1, i2], Rot[:, i2, i1], Rot[:, i2, i2] = c, -s, s, c
            R = matmul3(A, Rot)
        else:
            R = A
        x = p + np.stack([(R[:, i, 0] * g["c"][l, 0] + R[:, i, 1] * g["c"][l, 1]) + R[:, i, 2] * g["c"][l, 2] for i in range(3)], -1)
        P.append(p.copy()), Rs.append(R.copy()), X.append(x)
    return np.stack(P, 1), np.stack(Rs, 1), np.stack(X, 1)


def pair_clearance(x, U, s, Z):
    """Clearance of boxes (centre x [...,3], unit axes U [...,3(k),3], half-sizes s [...,3]) against obstacles Z [O,12]: [..., O]."""
    Z = np.asarray(Z, dtype=np.float64).reshape(-1, 12)
    x, U, s = x[..., None, :], U[..., None, :, :], s[..., None, :]
    c, G = Z[:, 0:3], [Z[:, 3:6], Z[:, 6:9], Z[:, 9:12]]
    d = x - c
    vals = []
    for a, b, rest in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):     # obstacle x obstacle
        m = cross3(G[a], G[b])
        m2 = dot3(m, m)
        ok = ~(m2 <= DEGENERATE * (dot3(G[a], G[a]) * dot3(G[b], G[b])))
        nrm = np.where(ok, np.sqrt(m2), 1.0)
        num = np.abs(dot3(m, d)) - (np.abs(dot3(m, G[rest])) + ((s[..., 0] * np.abs(dot3(m, U[..., 0, :])) + s[..., 1] * np.abs(dot3(m, U[..., 1, :])))
                                                               + s[..., 2] * np.abs(dot3(m, U[..., 2, :]))))
        vals.append(np.where(ok, num / nrm, -np.inf))
    for k in range(3):                                         # link x link
        u = U[..., k, :]
        vals.append(np.abs(dot3(u, d)) - (((np.abs(dot3(u, G[0])) + np.abs(dot3(u, G[1]))) + np.abs(dot3(u, G[2]))) + s[..., k]))
    for a in range(3):                                         # obstacle x link
        a1, a2 = [i for i in range(3) if i != a]
        for k in range(3):
            k1, k2 = [i for i in range(3) if i != k]
            m = cross3(G[a], U[..., k, :])
            m2 = dot3(m, m)
            ok = ~(m2 <= DEGENERATE * dot3(G[a], G[a]))
            num = np.abs(dot3(m, d)) - ((np.abs(dot3(m, G[a1])) + np.abs(dot3(m, G[a2])))
                                        + (s[..., k1] * np.abs(dot3(m, U[..., k1, :])) + s[..., k2] * np.abs(dot3(m, U[..., k2, :]))))
            vals.append(np.where(ok, num / np.where(ok, np.sqrt(m2), 1.0), -np.inf))
    return np.max(np.stack(vals, -1), -1)


def config_clearance(g, Q, Z, r=None):
    """Node clearance [K] of configurations Q [K,n] (r [K,J]: enlargement of every half-size, the edge rule's)."""
    if np.asarray(Z).size == 0:
        return np.full(np.asarray(Q).shape[0], np.inf)
    _, R, x = link_boxes(g, Q)
    U = np.swapaxes(R, -1, -2)            # U[..., k, :] = column k of R
    s = np.broadcast_to(g["h"], x.shape).copy()
    if r is not None:
        s = s + r[..., None]
    return pair_clearance(x, U, s, Z).min(axis=(1, 2))


def wrap(d):
    return d - 2 * np.pi * np.floor((d + np.pi) / (2 * np.pi))


def edge_samples(g, a, b, edge_step):
    """The edge rule's sub-segment midpoints [S,n] and enlargements [S,J] of the edge a -> b."""
    D = np.where(g["cont"], wrap(b - a), b - a)
    S = max(1, int(np.ceil(np.abs(D).max() / edge_step)))
    t = (2 * np.arange(S) + 1).astype(np.float64) / float(2 * S)
    q = a + t[:, None] * D
    r = np.zeros(g["J"])
    for l in range(g["J"]):
        acc = 0.0
        for j in range(min(l + 1, g["n"])):
            acc = acc + g["rho"][j, l] * abs(D[j])
        r[l] = acc / float(2 * S)
    return q, np.broadcast_to(r, (S, g["J"])).copy()


def edge_free_np(g, a, b, Z, edge_step):
    """(free, smallest sub-segment clearance) of one edge by the edge rule."""
    q, r = edge_samples(g, a, b, edge_step)
    cl = config_clearance(g, q, Z, r).min()
    return cl > 0, cl


# ----------------------------------------------------------------------------------------------------------- helpers
def _kinova8_robot():
    """The Kinova with an eighth revolute joint and link (tests/test_key128.py): J = n = 8, no fixed joint."""
    from armour_amd import planner
    from test_key128 import make_eight_factor_arm
    return make_eight_factor_arm(planner.kinova_robot())


def _robot(name):
    """The preset `name`.  "fetch8" (n = 8, J = 9) and "kinova8" (n = J = 8) exist in the 8-factor ABI only (ARMOUR_KEY128=1)."""
    from armour_amd import _lib, planner
    presets = {"kinova": planner.kinova_robot, "gripper": planner.kinova_gripper_robot, "fetch": planner.fetch_robot}
    if _lib.MAXF == 8:
        presets.update(fetch8=planner.fetch8_robot, kinova8=_kinova8_robot)
    return presets[name]()


def _fetch8_dict():
    """The 8-factor preset lives in the 128-bit-key library (another ABI): read it in a child process."""
    code = ("import json; from armour_amd import planner; from tests.test_roadmap import robot_dict; "
            "print(json.dumps(robot_dict(planner.fetch8_robot())))")
    env = dict(os.environ, ARMOUR_KEY128="1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout.strip().splitlines()[-1])


def _limits(robot):
    n = robot.num_factors
    cont = np.array(robot.continuous[:n]).astype(bool)
    lb = np.where(cont, -np.pi, np.array(robot.state_limits_lb[:n]))
    ub = np.where(cont, np.pi, np.array(robot.state_limits_ub[:n]))
    return lb, ub, cont


def _random_box_pair(rng):
    """(link centre, R, h, obstacle Z) with a random rotation and a general (skewed) obstacle zonotope."""
    from armour_amd.robot_geometry import rpy_matrix
    R = rpy_matrix(*rng.uniform(-np.pi, np.pi, 3))
    h = rng.uniform(0.02, 0.3, 3)
    Z = np.zeros(12)
    Z[3:12] = (rng.normal(size=9) * 0.15)
    if rng.random() < 0.5:                                   # axis-aligned boxes, as the worlds hold
        Z[3:12] = 0.0
        Z[3], Z[7], Z[11] = rng.uniform(0.02, 0.3, 3)
    x = rng.normal(size=3) * 0.45
    return x, R, h, Z


# ----------------------------------------------------------------------------------------------------------- CPU
def test_numpy_rule_agrees_with_membership_lp():
    """The 15-plane rule separates a box from an obstacle exactly when c_link - c_obs is NOT in Z([G_obs, R diag(h)])."""
    from scipy.optimize import linprog
    rng = np.random.default_rng(7)
    checked = sep = 0
    for _ in range(200):
        x, R, h, Z = _random_box_pair(rng)
        cl = pair_clearance(x, R.T, h, Z[None])[0]
        if abs(cl) < 1e-7:
            continue
        G = np.concatenate([Z[3:12].reshape(3, 3).T, R * h], axis=1)       # 3 x 6
        lp = linprog(np.zeros(6), A_eq=G, b_eq=x - Z[0:3], bounds=[(-1, 1)] * 6, method="highs")
        assert lp.status in (0, 2), lp.message
        inside = lp.status == 0
        assert inside == (cl <= 0), (cl, lp.status)
        checked += 1
        sep += cl > 0
    assert checked >= 190 and 20 <= sep <= checked - 20, (checked, sep)


@pytest.mark.parametrize("name", ["kinova", "gripper", "fetch", "fetch8"])
def test_rho_bounds_the_displacement_inside_a_sub_segment(name):
    """Every corner of link l, anywhere on a sub-segment, stays within r_l of where it is at the sub-segment's midpoint."""
    rd = _fetch8_dict() if name == "fetch8" else robot_dict(_robot(name))
    g = geometry(rd)
    rng = np.random.default_rng(11)
    n, J = g["n"], g["J"]
    corners = np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)], dtype=np.float64)
    worst = 0.0
    for _ in range(40):
        a = rng.uniform(-np.pi, np.pi, n)
        b = a + rng.uniform(-0.6, 0.6, n)
        step = rng.choice([0.05, 0.2, 1.0])
        qm, r = edge_samples(g, a, b, step)
        S = qm.shape[0]
        D = np.where(g["cont"], wrap(b - a), b - a)
        for s in rng.choice(S, size=min(S, 3), replace=False):
            t = (s + rng.random(60)) / S                          # dense points of sub-segment s
            Qs = a + t[:, None] * D
            Pm, Rm, _ = link_boxes(g, qm[s:s + 1])
            Pq, Rq, _ = link_boxes(g, Qs)
            for l in range(J):
                pts_m = Pm[0, l] + (Rm[0, l] @ (g["c"][l] + corners * g["h"][l]).T).T              # [8,3]
                pts_q = Pq[:, l, None, :] + np.einsum("kij,cj->kci", Rq[:, l], g["c"][l] + corners * g["h"][l])
                disp = np.linalg.norm(pts_q - pts_m[None], axis=-1).max()
                assert disp <= r[s, l] * (1 + 1e-12) + 1e-15, (name, l, disp, r[s, l])
                worst = max(worst, disp / max(r[s, l], 1e-300))
    assert worst > 0.05, worst    # the bound is not vacuous


def test_uniform_roadmap_properties():
    from armour_amd.roadmap import uniform_roadmap, wrapped_diff
    from armour_amd.worlds import STATE_LB, STATE_UB
    cont = np.abs(STATE_LB) >= 1000.0
    lb, ub = np.where(cont, -np.pi, STATE_LB), np.where(cont, np.pi, STATE_UB)
    n1, e1 = uniform_roadmap(600, 1.6, 6, 3, lb, ub, cont)
    n2, e2 = uniform_roadmap(600, 1.6, 6, 3, lb, ub, cont)
    assert np.array_equal(n1, n2) and np.array_equal(e1, e2)
    n3, _ = uniform_roadmap(600, 1.6, 6, 4, lb, ub, cont)
    assert not np.array_equal(n1, n3)
    assert n1.shape == (600, 7) and np.all(n1 >= lb) and np.all(n1 <= ub)
    assert e1.shape[0] > 100 and e1.dtype == np.int32 and np.all(e1[:, 0] < e1[:, 1])
    d = wrapped_diff(n1[e1[:, 0]], n1[e1[:, 1]], cont)
    assert np.sqrt((d * d).sum(-1)).max() <= 1.6
    assert len(np.unique(e1, axis=0)) == len(e1)


def test_waypoint_on_a_two_point_path_is_the_straight_line_rule():
    from armour_amd.roadmap import waypoint_along
    from armour_amd.scenes import CONTINUOUS, straight_line_waypoint
    rng = np.random.default_rng(5)
    for _ in range(50):
        q, goal = rng.uniform(-3, 3, 7), rng.uniform(-3, 3, 7)
        for la in (0.1, 1.0, 50.0):
            w = waypoint_along([q, goal], q, la, CONTINUOUS)
            assert np.abs(w - straight_line_waypoint(q, goal, la)).max() <= 1e-15


def test_create_refuses_bad_arguments_before_touching_a_device():
    from armour_amd import _lib
    from armour_amd.roadmap import Roadmap
    r = _robot("kinova")
    nodes = np.zeros((3, 7))
    with pytest.raises(_lib.ArmourError) as ei:
        Roadmap(r, nodes, [[0, 3]])
    assert ei.value.code == _lib.EINVAL
    with pytest.raises(_lib.ArmourError) as ei:
        Roadmap(r, nodes, [[0, 1]], edge_step=0.0)
    assert ei.value.code == _lib.EINVAL
    with pytest.raises(ValueError):
        Roadmap(r, np.zeros((3, 6)), [[0, 1]], continuous=np.zeros(6))


# ----------------------------------------------------------------------------------------------------------- GPU
def _reference_obstacles():
    from armour_amd.scenes import as_batch, reference_worlds
    return as_batch(reference_worlds())


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", ["kinova", "gripper", "fetch"])
def test_node_parity_on_the_reference_worlds(name):
    from armour_amd.roadmap import Roadmap
    robot = _robot(name)
    g = geometry(robot_dict(robot))
    lb, ub, cont = _limits(robot)
    rng = np.random.default_rng(21)
    nodes = lb + (ub - lb) * rng.random((2000, robot.num_factors))
    batch = _reference_obstacles()
    obs = batch["obstacles"]
    rm = Roadmap(robot, nodes, np.zeros((0, 2)), continuous=cont)
    v = rm.check(obs, clearance=True)
    v2 = rm.check(obs)
    assert np.array_equal(v["node_free"], v2["node_free"])           # the early-exit verdict is the clearance's sign
    assert np.array_equal(v["node_free"], v["node_clearance"] > 0)
    n_free = n_col = 0
    for w in range(obs.shape[0]):
        cl = config_clearance(g, nodes, obs[w])
        dev = v["node_clearance"][w]
        assert np.abs(dev - cl).max() <= 1e-12, (name, w, np.abs(dev - cl).max())
        sure = np.abs(cl) > 1e-9
        assert np.array_equal(v["node_free"][w][sure], (cl > 0)[sure]), (name, w)
        n_free += int((cl > 0).sum())
        n_col += int((cl <= 0).sum())
    assert n_free > 0 and n_col > 0, (n_free, n_col)


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_edge_parity_and_soundness():
    from armour_amd.roadmap import Roadmap, uniform_roadmap
    robot = _robot("kinova")
    g = geometry(robot_dict(robot))
    lb, ub, cont = _limits(robot)
    nodes, edges = uniform_roadmap(600, 2.0, 4, 1, lb, ub, cont)
    step = 0.1
    obs = _reference_obstacles()["obstacles"][::11][:10]
    rm = Roadmap(robot, nodes, edges, continuous=cont, edge_step=step)
    assert rm.E == len(edges) > 200
    v = rm.check(obs)
    rng = np.random.default_rng(3)
    n_free_edges = 0
    for w in range(obs.shape[0]):
        ef, nf = v["edge_free"][w], v["node_free"][w]
        assert np.all(nf[edges[ef, 0]]) and np.all(nf[edges[ef, 1]])      # a free edge has free endpoints
        for e, (a, b) in enumerate(edges):
            free, cl = edge_free_np(g, nodes[a], nodes[b], obs[w], step)
            if abs(cl) > 1e-9:
                assert bool(ef[e]) == free, (w, e, cl)
        free_idx = np.flatnonzero(ef)
        n_free_edges += free_idx.size
        for e in free_idx:                                                  # 200 dense samples of every free edge
            a, b = nodes[edges[e, 0]], nodes[edges[e, 1]]
            t = np.sort(rng.random(200))
            Q = a + t[:, None] * np.where(cont, wrap(b - a), b - a)
            assert config_clearance(g, Q, obs[w]).min() > 0, (w, e)
    assert n_free_edges > 100, n_free_edges


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_stationary_reach_set_agrees_with_the_node_check():
    """At rest, k = 0 is the stationary trajectory, so ARMOUR's reach set of every time step contains the static link boxes at q0:
    wherever every collision row of k = 0 is strictly satisfied, the node check at q0 says free."""
    from armour_amd._lib import ArmourLimits
    from armour_amd.planner import ArmourNLP, desired_trajectory
    from armour_amd.roadmap import Roadmap
    batch = _reference_obstacles()
    q0, obs = batch["q0"], batch["obstacles"]
    B, n = q0.shape
    for b in (0, 50, B - 1):
        for t in np.linspace(0.0, 1.0, 11):
            q, qd, _ = desired_trajectory(q0[b], np.zeros(n), np.zeros(n), np.zeros(n), t)
            assert np.abs(q - q0[b]).max() <= 1e-14 and np.abs(qd).max() <= 1e-14, (b, t)   # stationary up to rounding
    T = 20
    nlp = ArmourNLP(T=T, limits=ArmourLimits(max_batch=B, max_obstacles=obs.shape[1]))
    nlp.set_parameters(q0, np.zeros((B, n)), np.zeros((B, n)), batch["q_des"], obs)
    gv, _ = nlp.eval_g_jac(np.zeros((B, n)))
    J, O = nlp.J, obs.shape[1]
    col = gv[:, n * T:n * T + J * T * O]
    satisfied = np.all(col < -1e-9, axis=1)
    robot = nlp.robot
    rm = Roadmap(robot, q0, np.zeros((0, 2)))
    v = rm.check(obs)
    node = v["node_free"][np.arange(B), np.arange(B)]
    assert satisfied.sum() > 10, satisfied.sum()
    assert np.all(node[satisfied]), np.flatnonzero(satisfied & ~node)


def _wall_world(g):
    """A start / goal pair of the Kinova whose straight segment hits a wall, and a hand-placed free detour chain.  The wall is a thin
    box through the end of the forearm at the segment's middle; the detour folds the elbow, swings the base and unfolds."""
    start = np.zeros(g["n"])                                   # (an arm with more factors than the Kinova: its further joints at zero)
    start[:7] = [0.0, 0.6, 0.0, 1.2, 0.0, 0.6, 0.0]
    goal = start.copy()
    goal[0] = 2.0
    mid = 0.5 * (start + goal)
    _, _, x = link_boxes(g, mid[None])
    c = x[0, 5]
    wall = np.array([c[0], c[1], c[2], 0.06, 0, 0, 0, 0.06, 0, 0, 0, 0.12])
    folded = start.copy()
    folded[1], folded[3] = -0.3, 2.4
    chain = [start + (folded - start) * f for f in (0.5, 1.0)]
    for f in (0.25, 0.5, 0.75, 1.0):
        q = folded.copy()
        q[0] = start[0] + (goal[0] - start[0]) * f
        chain.append(q)
    end = chain[-1]
    chain.append(end + (goal - end) * 0.5)
    return start, goal, wall, chain


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plan_detours_around_a_wall_and_goes_straight_in_an_empty_world():
    from armour_amd import _lib
    from armour_amd.roadmap import Roadmap, RoadmapHLP, uniform_roadmap
    from armour_amd.scenes import FAR_BOX, straight_line_waypoint
    robot = _robot("kinova")
    g = geometry(robot_dict(robot))
    lb, ub, cont = _limits(robot)
    step = 0.05
    start, goal, wall, chain = _wall_world(g)
    assert not edge_free_np(g, start, goal, wall[None], step)[0]          # the straight segment collides
    for a, b in zip([start] + chain, chain + [goal]):
        assert edge_free_np(g, a, b, wall[None], step)[0]                 # the detour is free by the rule
    rnd, redges = uniform_roadmap(300, 2.0, 4, 2, lb, ub, cont)
    nodes = np.vstack([rnd, np.array(chain)])
    k0 = len(rnd)
    chain_edges = [[k0 + i, k0 + i + 1] for i in range(len(chain) - 1)]
    edges = np.vstack([redges, np.array(chain_edges, dtype=np.int32)])
    rm = Roadmap(robot, nodes, edges, continuous=cont, edge_step=step)
    with pytest.raises(_lib.ArmourError) as ei:
        rm.plan(0, start, goal)
    assert ei.value.code == _lib.ESTATE
    with pytest.raises(_lib.ArmourError) as ei:
        _lib.check(rm.L.armour_roadmap_check(rm.h, -1, 0, None, None, None, None, None))
    assert ei.value.code == _lib.EINVAL
    worlds = np.stack([wall[None], FAR_BOX[None]])
    v = rm.check(worlds)
    path = rm.plan(0, start, goal, connect_k=4)
    assert path is not None and len(path) > 2
    assert np.array_equal(path[0], start) and np.array_equal(path[-1], goal)
    for a, b in zip(path[:-1], path[1:]):
        assert edge_free_np(g, a, b, wall[None], step)[0]
    hlp = RoadmapHLP(rm, goal, world=0, connect_k=4)
    w1 = hlp.get_waypoint(start, 0.1)
    d = np.where(cont, wrap(path[1] - start), path[1] - start)
    assert np.abs(w1 - (start + 0.1 * d / np.linalg.norm(d))).max() <= 1e-12         # steps along the path's first edge
    assert np.abs(w1 - straight_line_waypoint(start, goal, 0.1)).max() > 1e-3         # not the straight-line rule
    # the empty world (a far box only): the direct two-point path, and the straight-line rule's waypoint
    direct = rm.plan(1, start, goal)
    assert direct.shape == (2, 7) and np.array_equal(direct[0], start) and np.array_equal(direct[1], goal)
    assert np.abs(RoadmapHLP(rm, goal, world=1).get_waypoint(start, 0.3) - straight_line_waypoint(start, goal, 0.3)).max() <= 1e-15
    assert v["node_free"][1].all() and v["edge_free"][1].all()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_batch_of_worlds_equals_one_by_one():
    from armour_amd.roadmap import Roadmap, uniform_roadmap
    robot = _robot("gripper")
    lb, ub, cont = _limits(robot)
    nodes, edges = uniform_roadmap(800, 2.5, 4, 9, lb, ub, cont)
    obs = _reference_obstacles()["obstacles"][:16]
    rm = Roadmap(robot, nodes, edges, continuous=cont, edge_step=0.1)
    v = rm.check(obs, clearance=True)
    for w in range(16):
        one = rm.check(obs[w:w + 1], clearance=True)
        assert np.array_equal(one["node_free"][0], v["node_free"][w])
        assert np.array_equal(one["edge_free"][0], v["edge_free"][w])
        assert np.array_equal(one["node_clearance"][0], v["node_clearance"][w])
    assert v["edge_free"].any() and not v["edge_free"].all()
