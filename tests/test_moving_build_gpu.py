"""Reach-set build against moving obstacles (include/armour_hip.h armour_set_problems_moving, ArmourNLP.set_parameters_moving): the half-space
rows of plan interval t are built from obstacle frame t.

The reference for every row (l, t, .) is the STATIC build (this library's, bit for bit, and the CPU oracle's, within the tolerances of
tests/test_p1_parity.py) of a world whose obstacles are frame t: Kinova without gripper, T = 8 (the smallest even T with a first, a last and
interior frames), O = 3, frames from armour_amd.worlds.moving_frames with speeds of 0.2 .. 1.0 m/s."""
import functools

import numpy as np
import pytest

from test_batch_api import _reference_records
from test_p1_parity import C_TOL, G_TOL, J_TOL

pytestmark = pytest.mark.gpu

T, O, J, N = 8, 3, 7, 7
SEED = 40                 # first world of the batches below (seeds SEED .. SEED + 8); min_margin() > 1e-9 holds for every one (asserted)


def _limits(B, o=O):
    from armour_amd._lib import ArmourLimits
    return ArmourLimits(max_batch=B, max_obstacles=o)


def _velocity(seed):
    """[O,3] of world `seed`: random directions, 0.2 .. 1.0 m/s (per world, so that world b is the same in every batch size)"""
    rng = np.random.default_rng(1000 + seed)
    v = rng.normal(size=(O, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.uniform(0.2, 1.0, (O, 1))


@functools.lru_cache(maxsize=None)
def _batch(B):
    """B worlds with moving obstacles: dict(q0 .. q_des [B,7], obstacles [B,O,12], velocity [B,O,3], frames [B,T,O,12])"""
    from armour_amd.worlds import moving_frames, random_batch
    bp = random_batch(SEED, B, O)
    bp["velocity"] = np.stack([_velocity(SEED + b) for b in range(B)])
    bp["frames"] = np.stack([moving_frames(bp["obstacles"][b], bp["velocity"][b], T) for b in range(B)])
    return bp


def _state(bp):
    return bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"]


def _moving(bp, B):
    from armour_amd.planner import ArmourNLP
    return ArmourNLP(T=T, limits=_limits(B)).set_parameters_moving(*_state(bp), bp["frames"])


@functools.lru_cache(maxsize=None)
def _frame_oracles(b):
    """the CPU oracle of world b of _batch(9) with frame t as its static obstacles, for every t"""
    from oracle.cpu_oracle import Oracle
    bp = _batch(9)
    return [Oracle(T=T).set_problem(bp["q0"][b], bp["qd0"][b], bp["qdd0"][b], bp["q_des"][b], bp["frames"][b, t]) for t in range(T)]


def _collision(g):
    """the collision rows of g [..., m] as [..., J, T, O] (O from m = nT + JTO + 4n)"""
    o = (g.shape[-1] - N * T - 4 * N) // (J * T)
    return g[..., N * T:N * T + J * T * o].reshape(g.shape[:-1] + (J, T, o))


def _collision_jac(jac):
    o = (jac.shape[-2] - N * T - 4 * N) // (J * T)
    return jac[..., N * T:N * T + J * T * o, :].reshape(jac.shape[:-2] + (J, T, o, N))


@pytest.mark.parametrize("B", [1, 9])
def test_frame_by_frame_against_the_static_build(B):
    """hyperplanes() rows (l, t, .) of the moving handle = those of a static handle whose obstacles are frame t: A and delta bit for bit; d bit
    for bit at B = 1 and within C_TOL at B = 9 (as the issue of this feature states it; both sides rebuild the full table with the same kernel
    code, so it is bit for bit there too).  pz / torque radius / link generators do not read obstacles: bit for bit."""
    from armour_amd.planner import ArmourNLP
    bp = _batch(B)
    mv = _moving(bp, B)
    A, d, dl = mv.hyperplanes()
    st = ArmourNLP(T=T, limits=_limits(B))
    for t in range(T):
        st.set_parameters(*_state(bp), bp["frames"][:, t])
        A1, d1, dl1 = st.hyperplanes()                       # [B, T, J, O, 36(, 3)]
        assert np.array_equal(A[:, t], A1[:, t]) and np.array_equal(dl[:, t], dl1[:, t]), (B, t)
        if B == 1:
            assert np.array_equal(d[:, t], d1[:, t]), t
        else:
            assert np.abs(d[:, t] - d1[:, t]).max() <= C_TOL, t
    assert np.array_equal(mv.torque_radius(), st.torque_radius()) and np.array_equal(mv.link_generators(), st.link_generators())
    for b in sorted({0, B - 1}):
        for which, i, t in (("link", 0, 0), ("link", J - 1, T - 1), ("torque", 3, T // 2), ("torque", N - 1, 1)):
            for x, y in zip(mv.pz(which, i, t, b=b), st.pz(which, i, t, b=b)):
                assert np.array_equal(x, y), (b, which, i, t)


@pytest.mark.parametrize("B", [1, 9])
def test_against_the_cpu_oracle_frame_by_frame(B):
    from armour_amd.worlds import random_k
    bp = _batch(B)
    mv = _moving(bp, B)
    A, d, dl = mv.hyperplanes()
    ks = random_k(77, 2 * B).reshape(2, B, N)
    gj = [mv.eval_g_jac(ks[i]) for i in range(2)]
    row0, Q = N * T, J * T * O
    for b in sorted({0, B - 1}):
        orc = _frame_oracles(b)                              # (world b of the 9-world batch is world b of the 1-world batch: same seeds)
        for t, o in enumerate(orc):
            assert o.min_margin() > 1e-9
            Ao, do, dlo = o.hyperplanes()                    # [T, J, O, 36(, 3)]
            assert np.abs(A[b, t] - Ao[t]).max() <= C_TOL and np.abs(d[b, t] - do[t]).max() <= C_TOL and np.abs(dl[b, t] - dlo[t]).max() <= C_TOL
        for i in range(2):
            g, jac = gj[i][0][b], gj[i][1][b]
            ref = [o.eval_g_jac(ks[i, b]) for o in orc]
            for t in range(T):
                assert np.abs(_collision(g)[:, t] - _collision(ref[t][0])[:, t]).max() <= G_TOL, (b, i, t)
                assert np.abs(_collision_jac(jac)[:, t] - _collision_jac(ref[t][1])[:, t]).max() <= J_TOL, (b, i, t)
            other = np.r_[0:row0, row0 + Q:g.size]           # torque and limit rows: obstacles do not enter them
            assert np.abs(g[other] - ref[0][0][other]).max() <= G_TOL and np.abs(jac[other] - ref[0][1][other]).max() <= J_TOL


def test_zero_velocity_is_the_static_build():
    from armour_amd.planner import ArmourNLP
    from armour_amd.worlds import random_k
    for B in (1, 9):
        bp = _batch(B)
        still = np.repeat(bp["obstacles"][:, None], T, axis=1)
        mv = ArmourNLP(T=T, limits=_limits(B)).set_parameters_moving(*_state(bp), still)
        st = ArmourNLP(T=T, limits=_limits(B)).set_parameters(*_state(bp), bp["obstacles"])
        ks = random_k(78, B)
        (g, jac), (g1, jac1) = mv.eval_g_jac(ks), st.eval_g_jac(ks)
        if B == 1:
            assert np.array_equal(g, g1) and np.array_equal(jac, jac1)
            assert np.array_equal(mv.plane_skip(), st.plane_skip()) and np.array_equal(mv.prune_margin(), st.prune_margin())
            (r, c, _), (r1, c1, _) = mv.row_relevance(), st.row_relevance()
            assert np.array_equal(r, r1) and np.array_equal(c, c1)
        else:                                                # the static side recomputes d from the centres
            assert np.abs(g - g1).max() <= G_TOL and np.abs(jac - jac1).max() <= J_TOL
            assert np.array_equal(mv.plane_skip(), st.plane_skip())


# One obstacle, fixed by hand: a 6 cm cube that starts 0.55 m beside the Kinova's forearm (the arm holds still at SCENE_Q: zero velocity and
# acceleration, k = 0) and flies through it at 1 m/s.  With T = 8 its frame t covers y in [y0 - 0.03 - t / 8 - 1 / 8, y0 + 0.03 - t / 8].
SCENE_Q = np.array([0.0, 0.6, 0.0, 1.2, 0.0, 0.4, 0.0])
SCENE_BOX = np.array([[0.0, 0.0, 0.0, 0.03, 0, 0, 0, 0.03, 0, 0, 0, 0.03]])     # centre filled in by _scene
SCENE_V = np.array([[0.0, -1.0, 0.0]])


def _scene():
    """(obstacle [1,12] at its start pose, frames [T,1,12]): the cube starts 0.55 m in +y of the centre of link 4's box"""
    from armour_amd.planner import kinova_robot
    from armour_amd.worlds import moving_frames
    from test_roadmap import geometry, link_boxes, robot_dict
    x = link_boxes(geometry(robot_dict(kinova_robot())), SCENE_Q[None])[2][0]
    box = SCENE_BOX.copy()
    box[0, 0:3] = x[3] + np.array([0.0, 0.55, 0.0])
    return box, moving_frames(box, SCENE_V, T)


def test_the_feature_is_visible():
    """Static build at the start pose: every collision row <= 0 at k = 0.  Moving build: rows > 0, and exactly where the per-frame oracle has
    them (rows within G_TOL of zero are left out of the comparison)."""
    from armour_amd.planner import ArmourNLP
    from oracle.cpu_oracle import Oracle
    z = np.zeros(N)
    box, frames = _scene()
    k = np.zeros(N)
    st = ArmourNLP(T=T, limits=_limits(1, 1)).set_parameters(SCENE_Q, z, z, SCENE_Q, box)
    assert _collision(st.eval_g(k)[0]).max() < 0
    mv = ArmourNLP(T=T, limits=_limits(1, 1)).set_parameters_moving(SCENE_Q, z, z, SCENE_Q, frames)
    c = _collision(mv.eval_g(k)[0])                          # [J, T, 1]
    ref = np.stack([_collision(Oracle(T=T).set_problem(SCENE_Q, z, z, SCENE_Q, frames[t]).eval_g_jac(k)[0])[:, t] for t in range(T)], axis=1)
    assert np.abs(c - ref).max() <= G_TOL
    sure = np.abs(ref) > 10 * G_TOL
    assert np.array_equal((c > 0)[sure], (ref > 0)[sure])
    hit_t = np.nonzero((ref > 10 * G_TOL).any(axis=(0, 2)))[0]
    assert hit_t.size >= 1 and hit_t.min() >= 2 and (c[:, :2] < 0).all(), hit_t     # clear during the first intervals, crossed later
    assert (c[:, hit_t] > 0).any()


def test_handle_reuse_restores_every_flag():
    """moving, static, moving on one handle, at B = 9 (where the static build stores no d and recomputes it from the centres, and the moving one
    must not): each equals a fresh handle's result bit for bit."""
    from armour_amd.planner import ArmourNLP
    from armour_amd.worlds import random_k
    B = 9
    bp = _batch(B)
    ks = random_k(79, B)
    fresh_mv = _moving(bp, B).eval_g_jac(ks)
    fresh_st = ArmourNLP(T=T, limits=_limits(B)).set_parameters(*_state(bp), bp["obstacles"]).eval_g_jac(ks)
    assert not np.array_equal(fresh_mv[0], fresh_st[0])
    h = ArmourNLP(T=T, limits=_limits(B))
    for kind in ("moving", "static", "moving", "static"):
        if kind == "moving":
            got, want = h.set_parameters_moving(*_state(bp), bp["frames"]).eval_g_jac(ks), fresh_mv
        else:
            got, want = h.set_parameters(*_state(bp), bp["obstacles"]).eval_g_jac(ks), fresh_st
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), kind
    # and the same at B = 1 on a handle that has held the batch
    one = {k: v[:1] for k, v in bp.items()}
    a = h.set_parameters_moving(*_state(one), one["frames"]).eval_g_jac(ks[:1])
    b = _moving(_batch(1), 1).eval_g_jac(ks[:1])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("B", [1, 9])
def test_the_tables_consumers_run_on_a_moving_build(B):
    from armour_amd.planner import sweep_candidates
    from armour_amd.worlds import random_k
    bp = _batch(B)
    mv = _moving(bp, B)
    # eval_violations against the record derived from eval_g_jac on the host
    ks = random_k(80, B)
    g = mv.eval_g_jac(ks)[0]
    rec = mv.eval_violations(ks)
    want = _reference_records(mv, g)                       # (tests/test_batch_api.py: the record from the full g)
    for b in range(B):
        r, e = rec[b], want[b]
        assert r["feasible"] == e["feasible"] and (r["n_outside_slack"] == 0) == e["feasible"], (b, r, e)
        assert r["n_violated"] == e["n_violated"] and r["worst_row"] == e["worst_row"] and r["worst"] == e["worst"], (b, r, e)
        assert abs(r["l1_violation"] - e["l1"]) <= 1e-12 * max(1.0, e["l1"])
    # sweep: its records are eval_violations' of every (problem, candidate)
    cand = sweep_candidates(N, 8)
    sw = mv.sweep(cand)
    for s in (0, 7):
        ev = mv.eval_violations(np.repeat(cand[s][None], B, axis=0))
        for b in range(B):
            assert sw["records"][b, s]["n_violated"] == ev[b]["n_violated"] and bool(sw["records"][b, s]["feasible"]) == ev[b]["feasible"], (b, s)
    # solve: a k reported feasible is feasible by finalize_solution on this handle's own g
    res = mv.solve()
    kopt = np.stack([np.where(np.isfinite(r["k_opt"]), r["k_opt"], 0.0) for r in res])
    feas = mv.finalize_solution(mv.eval_g(kopt))
    for b, r in enumerate(res):
        if r["feasible"]:
            assert feas[b], b
    res2 = mv.solve(k_start=np.clip(kopt, -1.0, 1.0))
    assert len(res2) == B
