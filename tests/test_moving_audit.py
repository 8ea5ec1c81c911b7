"""Path audit against obstacles in linear motion (include/armour_hip.h armour_path_audit_moving, armour_amd.path_audit.audit_moving): the host twin.

The moving rule is restated below in numpy on top of the static audit's restatement (tests/test_path_audit.py) and the roadmap's node rule
(tests/test_roadmap.py): for item (p, s) and obstacle o, with tau = t_world[p] + t_s, the pair test of link box l against obstacle o at its pose
of world time 0 with the box centre x - v_o tau; the tube test enlarges every half-size by r_l + |v_o| half besides.  CPU tests: the library's
host audit against the restatement, the soundness of verdicts 0 and 1 by dense sampling in time, zero velocity against the static host audit."""
import numpy as np
import pytest

from test_path_audit import CL_TOL, D, K_RANGE, _piece, _worlds, piece_items, q_des, random_pieces
from test_roadmap import _robot, config_clearance, geometry, link_boxes, pair_clearance, robot_dict


# ----------------------------------------------------------------------------------------------------------- numpy restatement
def velocity_norm(V):
    return np.sqrt((V[..., 0] * V[..., 0] + V[..., 1] * V[..., 1]) + V[..., 2] * V[..., 2])


def config_clearance_moving(g, Q, Z, V, tau, r=None, half=0.0):
    """Clearance [K] of configurations Q [K,n] against obstacles Z [O,12] with velocities V [O,3] at their poses of world times tau [K]:
    per obstacle the node rule's pair test with the box centres x - v tau and the half-sizes h + (r + |v| half) (r [K,J] or None: zeros)."""
    Z = np.asarray(Z, dtype=np.float64).reshape(-1, 12)
    K = np.asarray(Q).shape[0]
    if Z.size == 0:
        return np.full(K, np.inf)
    _, R, x = link_boxes(g, Q)
    U = np.swapaxes(R, -1, -2)
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (K,))
    rr = np.zeros((K, g["J"])) if r is None else r
    nv = velocity_norm(V)
    out = np.full(K, np.inf)
    for o in range(Z.shape[0]):
        xs = x - V[o][None, None, :] * tau[:, None, None]
        grow = rr + nv[o] * half
        s = np.broadcast_to(g["h"], x.shape) + grow[..., None]
        out = np.minimum(out, pair_clearance(xs, U, s, Z[o:o + 1])[..., 0].min(axis=1))
    return out


def audit_moving_np(g, Z, V, t_world, piece, k_range, dur, step, tube=None):
    """(verdict, t_hit, clearance, margin) of one piece by the moving rule (tests/test_path_audit.py audit_np with moving obstacles)."""
    t, q, r = piece_items(g, piece, k_range, dur, step, tube)
    half = (piece[5] - piece[4]) / float(2 * t.size)
    tau = t_world + t
    sample = config_clearance_moving(g, q, Z, V, tau)
    tube_cl = config_clearance_moving(g, q, Z, V, tau, r, half)
    hit = sample <= 0
    margin = min(np.abs(sample).min(), np.abs(tube_cl).min())
    if hit.any():
        return 1, t[np.argmax(hit)], sample.min(), margin
    return (0 if np.all(tube_cl > 0) else 2), np.nan, sample.min(), margin


# ----------------------------------------------------------------------------------------------------------- helpers
def random_motion(rng, obs, lo=0.2, hi=1.0):
    """velocity [W,O,3]: random directions, speeds of lo..hi m/s"""
    v = rng.normal(size=obs.shape[:2] + (3,))
    return v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.uniform(lo, hi, obs.shape[:2] + (1,))


def compare_moving(res, g, obs, vel, world, t_world, arrs, k_range, step, tube, tag):
    """A library result against the restatement, piece by piece; returns the verdict counts."""
    counts = [0, 0, 0]
    for p in range(len(world)):
        v, th, cl, margin = audit_moving_np(g, obs[world[p]], vel[world[p]], t_world[p], _piece(arrs, p), k_range, D, step, None if tube is None else tube[p])
        if margin > 1e-9:          # (a decisive quantity within rounding of zero may fall either way)
            assert res.verdict[p] == v, (tag, p, res.verdict[p], v)
            assert (np.isnan(th) and np.isnan(res.t_hit[p])) or res.t_hit[p] == th, (tag, p, res.t_hit[p], th)
        if res.clearance is not None:
            assert abs(res.clearance[p] - cl) <= CL_TOL, (tag, p, res.clearance[p], cl)
        counts[v] += 1
    return counts


# ----------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name", ["kinova", "fetch"])
def test_host_audit_equals_the_restatement(name):
    from armour_amd.path_audit import audit_moving
    robot = _robot(name)
    g = geometry(robot_dict(robot))
    n = g["n"]
    obs = _worlds()[::9]
    rng = np.random.default_rng(31)
    vel = random_motion(rng, obs)
    P = 80
    arrs = random_pieces(robot, rng, P, still=0.3)
    world = rng.integers(0, obs.shape[0], P).astype(np.int32)
    t_world = rng.uniform(-1.0, 2.0, P)
    tube = rng.choice([0.0, 0.01], (P, 1)) * rng.random((P, n))
    total = [0, 0, 0]
    for step, tb_ in ((0.02, None), (0.05, tube)):
        res = audit_moving(robot, obs, vel, world, t_world, *arrs[:4], K_RANGE[:n], D, arrs[4], arrs[5], tube=tb_, step=step, clearance=True, host=True)
        fast = audit_moving(robot, obs, vel, world, t_world, *arrs[:4], K_RANGE[:n], D, arrs[4], arrs[5], tube=tb_, step=step, host=True)
        assert np.array_equal(res.verdict, fast.verdict) and np.array_equal(res.t_hit, fast.t_hit, equal_nan=True)   # early exit changes nothing
        counts = compare_moving(res, g, obs, vel, world, t_world, arrs, K_RANGE[:n], step, tb_, (name, step))
        total = [a + b for a, b in zip(total, counts)]
    print(f"{name}: proved free / proved hit / undecided = {total}")
    assert min(total) > 0, total


@pytest.mark.parametrize("name", ["kinova", "fetch"])
def test_verdicts_are_sound_by_sampling(name):
    """Verdict 0 of the host audit: at 200 dense times of the window the arm, with every joint moved by a random offset within the tube, is free
    of every obstacle at its pose of that time.  Verdict 1: the plan's configuration at t_hit collides with an obstacle at its pose of then."""
    from armour_amd.path_audit import audit_moving
    robot = _robot(name)
    g = geometry(robot_dict(robot))
    n = g["n"]
    kr = K_RANGE[:n]
    obs = _worlds()
    rng = np.random.default_rng(37)
    vel = random_motion(rng, obs)
    P = 100
    arrs = random_pieces(robot, rng, P, still=0.3)
    world = rng.integers(0, obs.shape[0], P).astype(np.int32)
    t_world = rng.uniform(-1.0, 2.0, P)
    tube = rng.choice([0.0, 0.005, 0.02], (P, 1)) * rng.random((P, n))
    res = audit_moving(robot, obs, vel, world, t_world, *arrs[:4], kr, D, arrs[4], arrs[5], tube=tube, step=0.02, host=True)
    counts = np.bincount(res.verdict, minlength=3)
    for p in range(P):
        q0, qd0, qdd0, k, ta, tb = _piece(arrs, p)
        Z, V = obs[world[p]], vel[world[p]]
        if res.verdict[p] == 0:
            t = np.concatenate([[ta, tb], ta + (tb - ta) * rng.random(198)])
            Q = q_des(q0[None], (qd0 * D)[None], (qdd0 * D * D)[None], (kr * k)[None], (t / D)[:, None])
            assert config_clearance_moving(g, Q, Z, V, t_world[p] + t).min() > 0, (name, p)
            assert config_clearance_moving(g, Q + tube[p] * rng.uniform(-1, 1, Q.shape), Z, V, t_world[p] + t).min() > 0, (name, p)
        elif res.verdict[p] == 1:
            th = res.t_hit[p]
            Q = q_des(q0, qd0 * D, qdd0 * D * D, kr * k, th / D)[None]
            Zt = Z.copy()
            Zt[:, 0:3] += V * (t_world[p] + th)       # the obstacles themselves moved, not the box
            assert ta <= th <= tb and config_clearance(g, Q, Zt)[0] <= 1e-12, (name, p)
    print(f"{name}: proved free / proved hit / undecided = {counts.tolist()}")
    assert counts[0] >= 10 and counts[1] >= 10, counts


@pytest.mark.parametrize("name", ["kinova", "fetch"])
def test_zero_velocity_is_the_static_audit_bit_for_bit(name):
    from armour_amd.path_audit import audit, audit_moving
    robot = _robot(name)
    n = robot.num_factors
    obs = _worlds()[::9]
    rng = np.random.default_rng(41)
    P = 60
    arrs = random_pieces(robot, rng, P, still=0.3)
    world = rng.integers(0, obs.shape[0], P).astype(np.int32)
    tube = rng.choice([0.0, 0.01], (P, 1)) * rng.random((P, n))
    ref = audit(robot, obs, world, *arrs[:4], K_RANGE[:n], D, arrs[4], arrs[5], tube=tube, step=0.02, clearance=True, host=True)
    assert len(set(ref.verdict.tolist())) == 3
    for t_world in (0.0, rng.uniform(-5.0, 5.0, P)):
        res = audit_moving(robot, obs, np.zeros(obs.shape[:2] + (3,)), world, t_world, *arrs[:4], K_RANGE[:n], D, arrs[4], arrs[5], tube=tube, step=0.02,
                           clearance=True, host=True)
        assert np.array_equal(res.verdict, ref.verdict) and np.array_equal(res.t_hit, ref.t_hit, equal_nan=True)
        assert np.array_equal(res.clearance, ref.clearance)


def test_moving_audit_refuses_bad_arguments_before_touching_a_device():
    from armour_amd._lib import ArmourError
    from armour_amd.path_audit import audit_moving
    robot = _robot("kinova")
    box = np.array([[0.5, 0.0, 0.5, 0.1, 0, 0, 0, 0.1, 0, 0, 0, 0.1]])
    z = np.zeros((1, 7))
    ok = dict(obstacles=box, velocity=np.zeros((1, 3)), world_of_piece=0, t_world=0.0)
    for host in (True, False):
        for bad in (dict(velocity=np.array([[0.0, np.nan, 0.0]])), dict(t_world=np.inf), dict(world_of_piece=1)):
            a = {**ok, **bad}
            with pytest.raises(ArmourError):
                audit_moving(robot, a["obstacles"], a["velocity"], a["world_of_piece"], a["t_world"], z, z, z, z, K_RANGE, D, 0.0, 0.5, host=host)
