"""Per-interval obstacle frames (armour_amd.worlds.moving_frames) and the argument rules of armour_set_problems_moving.

moving_frames is host arithmetic and is tested without a device.  The setter's refusals need a handle, and armour_create needs a device (the
library has no CPU path), so that test is marked gpu."""
import numpy as np
import pytest

from armour_amd.worlds import moving_frames, random_problem

T, O = 8, 3


def _motion(seed, obstacles):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(obstacles.shape[0], 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.2, 1.0, (obstacles.shape[0], 1))


def _corners(Z):
    """the 8 corners [8,3] of an axis-aligned box zonotope Z [12]"""
    h = np.array([Z[3], Z[7], Z[11]])
    sg = np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], dtype=np.float64)
    return Z[0:3] + sg * np.abs(h)


@pytest.mark.parametrize("duration,t_world", [(1.0, 0.0), (1.0, 0.7), (2.5, -1.3)])
def test_frames_cover_the_moving_box_corner_by_corner(duration, t_world):
    obs = random_problem(3, O)["obstacles"]
    vel = _motion(4, obs)
    fr = moving_frames(obs, vel, T, duration=duration, t_world=t_world)
    assert fr.shape == (T, O, 12)
    dl = duration / T
    for t in range(T):
        for o in range(O):
            lo, hi = _corners(fr[t, o]).min(0), _corners(fr[t, o]).max(0)
            for tau in np.linspace(t * dl, (t + 1) * dl, 41):          # dense plan times of interval t, both ends included
                Z = obs[o].copy()
                Z[0:3] = Z[0:3] + vel[o] * (t_world + tau)
                c = _corners(Z)
                slack = np.minimum(c - lo, hi - c).min()
                assert slack >= -1e-14, (t, o, tau, slack)               # (rounding of the two centres: a few ulp of coordinates of size ~1)
    # the cover is the tight one: at an interval's ends a corner touches the frame's face
    for o in range(O):
        Z = obs[o].copy()
        Z[0:3] = Z[0:3] + vel[o] * t_world
        assert np.abs(np.minimum(_corners(Z) - _corners(fr[0, o]).min(0), _corners(fr[0, o]).max(0) - _corners(Z)).min()) <= 1e-14


def test_zero_velocity_returns_the_static_obstacle_in_every_frame():
    obs = random_problem(5, O)["obstacles"]
    fr = moving_frames(obs, np.zeros((O, 3)), T, duration=1.0, t_world=3.7)
    for t in range(T):
        assert np.array_equal(fr[t], obs)
    # one obstacle at rest among moving ones keeps its zonotope too
    vel = _motion(6, obs)
    vel[1] = 0.0
    fr = moving_frames(obs, vel, T)
    assert all(np.array_equal(fr[t, 1], obs[1]) for t in range(T)) and not np.array_equal(fr[0, 0], obs[0])


def test_a_rotated_generator_block_raises():
    obs = random_problem(7, O)["obstacles"]
    q, _ = np.linalg.qr(np.random.default_rng(8).normal(size=(3, 3)))
    rot = obs.copy()
    rot[1, 3:] = (rot[1, 3:].reshape(3, 3) @ q.T).ravel()
    with pytest.raises(ValueError):
        moving_frames(rot, np.zeros((O, 3)), T)
    with pytest.raises(ValueError):
        moving_frames(obs, np.zeros((O + 1, 3)), T)


@pytest.mark.gpu
def test_the_setter_follows_the_argument_rules_of_the_static_one():
    """A null pointer with O > 0 and non-finite entries are refused and the handle stays usable.  ArmourLimits.max_obstacles means what it means
    to armour_set_problems ("any value allowed": a first capacity, the handle grows past it), so O = max_obstacles + 1 gets the static setter's
    answer."""
    from armour_amd import _lib
    from armour_amd._lib import ArmourError, ArmourLimits, _dp
    from armour_amd.planner import ArmourNLP
    p = random_problem(9, O)
    fr = moving_frames(p["obstacles"], _motion(10, p["obstacles"]), T)
    nlp = ArmourNLP(T=T, limits=ArmourLimits(max_batch=1, max_obstacles=O))
    L = _lib.load()
    st = [np.ascontiguousarray(p[k].reshape(1, 7)) for k in ("q0", "qd0", "qdd0", "q_des")]
    assert L.armour_set_problems_moving(nlp.h, 1, O, *[_dp(a) for a in st], None) < 0
    assert b"null" in L.armour_last_error()
    bad = fr.copy()
    bad[T - 1, O - 1, 11] = np.nan
    with pytest.raises(ArmourError, match="non-finite"):
        nlp.set_parameters_moving(p["q0"], p["qd0"], p["qdd0"], p["q_des"], bad)
    with pytest.raises(ValueError):
        nlp.set_parameters_moving(p["q0"], p["qd0"], p["qdd0"], p["q_des"], fr[: T - 1])
    g = nlp.set_parameters_moving(p["q0"], p["qd0"], p["qdd0"], p["q_des"], fr).eval_g(np.zeros(7))
    assert np.all(np.isfinite(g))
    # too many obstacles: whatever the static setter answers
    many = random_problem(11, O + 1)["obstacles"]

    def status(call):
        try:
            call()
            return 0
        except ArmourError as e:
            return e.code
    s_static = status(lambda: nlp.set_parameters(p["q0"], p["qd0"], p["qdd0"], p["q_des"], many))
    s_moving = status(lambda: nlp.set_parameters_moving(p["q0"], p["qd0"], p["qdd0"], p["q_des"], moving_frames(many, np.zeros((O + 1, 3)), T)))
    assert s_static == s_moving
    g2 = nlp.set_parameters_moving(p["q0"], p["qd0"], p["qdd0"], p["q_des"], fr).eval_g(np.zeros(7))
    assert np.array_equal(g, g2)
