"""Path audit against moving obstacles on the device (armour_path_audit_moving) against its host twin, and the two halves of the moving-world
safety claim against each other: a plan that the moving half-space tables call collision-free is never a proved hit of the moving audit."""
import numpy as np
import pytest

from test_moving_audit import random_motion
from test_path_audit import CL_TOL, D, K_RANGE, _worlds, random_pieces
from test_roadmap import _robot

pytestmark = pytest.mark.gpu

W, P, STEP = 4, 64, 0.02


def _case(name="kinova", seed=51):
    robot = _robot(name)
    n = robot.num_factors
    rng = np.random.default_rng(seed)
    obs = _worlds()[:: 9][:W]
    vel = random_motion(rng, obs)
    arrs = random_pieces(robot, rng, P, still=0.3)
    world = rng.integers(0, W, P).astype(np.int32)
    t_world = rng.uniform(-1.0, 2.0, P)
    tube = rng.choice([0.0, 0.01], (P, 1)) * rng.random((P, n))
    return robot, obs, vel, world, t_world, arrs, K_RANGE[:n], tube


def _same(a, b, bitwise=False):
    assert np.array_equal(a.verdict, b.verdict) and np.array_equal(a.t_hit, b.t_hit, equal_nan=True)
    if a.clearance is not None:
        assert np.array_equal(a.clearance, b.clearance) if bitwise else np.abs(a.clearance - b.clearance).max() <= CL_TOL


@pytest.mark.parametrize("clearance", [False, True])
def test_device_audit_equals_the_host_twin(clearance):
    from armour_amd.path_audit import audit_moving
    robot, obs, vel, world, t_world, arrs, kr, tube = _case()
    kw = dict(tube=tube, step=STEP, clearance=clearance)
    dev = audit_moving(robot, obs, vel, world, t_world, *arrs[:4], kr, D, arrs[4], arrs[5], **kw)
    host = audit_moving(robot, obs, vel, world, t_world, *arrs[:4], kr, D, arrs[4], arrs[5], host=True, **kw)
    assert len(set(host.verdict.tolist())) == 3, np.bincount(host.verdict)
    _same(dev, host)
    assert dev.ms > 0


def test_four_worlds_in_one_call_equal_four_calls():
    from armour_amd.path_audit import audit_moving
    robot, obs, vel, world, t_world, arrs, kr, tube = _case()
    all_ = audit_moving(robot, obs, vel, world, t_world, *arrs[:4], kr, D, arrs[4], arrs[5], tube=tube, step=STEP, clearance=True)
    for w in range(W):
        m = world == w
        assert m.any()
        one = audit_moving(robot, obs[w], vel[w], 0, t_world[m], *[a[m] for a in arrs[:4]], kr, D, arrs[4][m], arrs[5][m], tube=tube[m], step=STEP, clearance=True)
        assert np.array_equal(one.verdict, all_.verdict[m]) and np.array_equal(one.t_hit, all_.t_hit[m], equal_nan=True)
        assert np.array_equal(one.clearance, all_.clearance[m])


def test_zero_velocity_is_the_static_device_audit_bit_for_bit():
    from armour_amd.path_audit import audit, audit_moving
    robot, obs, vel, world, t_world, arrs, kr, tube = _case()
    for clearance in (False, True):
        kw = dict(tube=tube, step=STEP, clearance=clearance)
        st = audit(robot, obs, world, *arrs[:4], kr, D, arrs[4], arrs[5], **kw)
        mv = audit_moving(robot, obs, np.zeros_like(vel), world, t_world, *arrs[:4], kr, D, arrs[4], arrs[5], **kw)
        _same(mv, st, bitwise=True)


# ---- the two halves: moving tables and moving audit.  Worlds HALVES_SEEDS (armour_amd.worlds.random_problem, 3 boxes), the boxes' velocities and
# the 16 fixed k per world below were picked with the per-frame CPU oracle (T = 16) and the host audit alone so that the three counts asserted
# at the end of the test hold for the reference arithmetic: of the 64 (world, k) pairs 25 are collision-feasible (11, 12, 0 and 2 per world), 39
# are not, and 8 of those (world 2) are proved hits; no collision row of the oracle is within 1.6e-4 of zero and no sample clearance of the host
# audit within 1e-4.
HALVES_T = 16
HALVES_SEEDS = (0, 10, 5, 7)
HALVES_T_WORLD = (1.7, 1.7, 0.0, -0.8)


def halves_worlds():
    """[(problem dict, velocity [O,3], t_world, frames [T,O,12], k [16,7])] of the four worlds"""
    from armour_amd.worlds import moving_frames, random_k, random_problem
    out = []
    for seed, tw in zip(HALVES_SEEDS, HALVES_T_WORLD):
        p = random_problem(seed, 3)
        vel = random_motion(np.random.default_rng(2000 + seed), p["obstacles"][None])[0]
        out.append((p, vel, tw, moving_frames(p["obstacles"], vel, HALVES_T, duration=D, t_world=tw), random_k(seed, 16)))
    return out


def collision_rows(g, O=3, T=HALVES_T, J=7, n=7):
    return g[..., n * T:n * T + J * T * O]


def test_the_two_halves_agree():
    """Every (world, k) whose collision rows are all <= 0 on the moving tables has a verdict 0 or 2 of audit_moving for the piece [0, duration]
    (tube None), never 1: the tables' frame t covers the obstacle over plan interval t, the reach set covers the link there, and a proved hit is
    the nominal link box meeting the obstacle at one time of that interval."""
    from armour_amd.path_audit import audit_moving
    from armour_amd.planner import ArmourNLP, kinova_robot
    ws = halves_worlds()
    robot = kinova_robot()
    feasible, verdict = [], []
    for p, vel, tw, frames, ks in ws:
        nlp = ArmourNLP(T=HALVES_T).set_parameters_moving(p["q0"], p["qd0"], p["qdd0"], p["q_des"], frames)
        kr, dur = np.array(nlp.params.k_range[:7]), nlp.params.duration
        assert dur == D
        feasible += [bool(np.all(collision_rows(nlp.eval_g(k)[0]) <= 0)) for k in ks]
        S = len(ks)
        res = audit_moving(robot, p["obstacles"], vel, 0, tw, np.tile(p["q0"], (S, 1)), np.tile(p["qd0"], (S, 1)), np.tile(p["qdd0"], (S, 1)), ks, kr, dur,
                           0.0, dur, tube=None, step=STEP)
        verdict += res.verdict.tolist()
    feasible, verdict = np.array(feasible), np.array(verdict)
    assert not np.any(feasible & (verdict == 1)), np.nonzero(feasible & (verdict == 1))[0]
    assert feasible.sum() >= 16 and (~feasible).sum() >= 4 and np.any(~feasible & (verdict == 1)), (feasible.sum(), np.bincount(verdict, minlength=3))
