"""Moving obstacles in the workspace RRT*, the inverse kinematics and the end-effector HLP on the MI355X (armour_ws_tree_plan_moving,
armour_ik_moving): the device against the host twins -- the host twins are tied to the numpy restatement of the window rule in
test_ws_moving.py.  A comparison is made only where the host twin's `margin` is above 1e-9, asserted first.  The trees hold no
transcendental function and are compared bit for bit on every output.  The inverse kinematics takes sin / cos in its link frames from the
device's library on one side and from libm on the other, so -- as for the static entry -- device against twin is
test_ik_gpu.assert_device_equals_twin: statuses, picks, flags and iteration counts equal, q and err within its DEV_Q_TOL / DEV_ERR_TOL (100 x
the rounding-size differences measured for the static entry, <= 1e-9); device against device (zero velocity against the static entry, a
target alone against the same target in a batch, static after moving) is bit for bit.  Shapes are the small ones of
test_ws_moving.py (250 iterations, 512 nodes, W <= 6; at most 14 targets), chosen to reach every path of the moving instantiations: the
obstacle split with the moving stride (O = 5 and 14 with a rewire radius so small that a round's work list fills under half the block,
O = 1 without a split; the inverse kinematics on both sides of its 128 seeds), the raised dynamic LDS at O = 256, a tree past 256 nodes,
a seeded chain, and a static launch before and after a moving one."""
import numpy as np
import pytest

import test_ws_tree
from test_ik import Q_A, blocking_box, chain_np
from test_ik_gpu import assert_device_equals_twin
from test_tree_plan import _same_bits
from test_trials_moving import GPU_SEED, GPU_WORLDS, seeded_velocities
from test_ws_moving import CHAIN, WINDOWS, _plan, _solve, ik_problem, kinova, moving_worlds
from test_ws_tree import MARGIN, START, _box, assert_same_plans, wall_with_window

SOLVE = dict(tolerance=1e-7, max_iterations=100)      # tests/test_reference_scenes.py
SIX = WINDOWS + ((0.3, 0.9), (2.0, 2.0), (-0.5, 0.0))
IK_KEYS = ("status", "best", "q", "q_all", "err", "iterations", "flags")
NARROW = dict(rewire_radius=0.06)                     # a round's candidates: the nearest node and the few within 6 cm, 10 sub-segments each


@pytest.fixture(scope="module")
def arm():
    return kinova()


def both_plans(obs, vel, windows, seeds, **kw):
    """(device, host twin) of one moving plan_workspace_trees call with trees, compared; the host run's margins are asserted first"""
    host = _plan(obs, vel, windows, seeds, **kw)
    assert (host.margin > MARGIN).all(), host.margin
    dev = _plan(obs, vel, windows, seeds, host=False, **kw)
    for w in range(np.asarray(obs).shape[0]):
        assert_same_plans(dev, w, host, w)
    assert dev.ms > 0.0 and dev.margin is None
    return dev, host


def assert_same_ik(a, b, ta=None, tb=None):
    ta = slice(None) if ta is None else ta
    tb = slice(None) if tb is None else tb
    for k in IK_KEYS:
        assert np.array_equal(getattr(a, k)[ta], getattr(b, k)[tb], equal_nan=True), k


def both_ik(s, targets, q_ref, obs, vel, windows, world, seeds, S):
    host = _solve(s, targets, q_ref, obs, vel, windows, world, seeds, S=S)
    assert (host.margin > MARGIN).all(), host.margin
    dev = _solve(s, targets, q_ref, obs, vel, windows, world, seeds, S=S, host=False)
    assert_device_equals_twin(dev, host, f"S = {S}, O = {np.asarray(obs).shape[-2]}")
    return dev, host


def six_worlds():
    """six moving worlds with different windows and velocities; in the fifth a box sits on the start (and drifts), the sixth has one far box"""
    obs, vel = moving_worlds(3, W=6)
    obs[4, 5] = _box(START, (0.04, 0.04, 0.04))
    vel[4, 5] *= 0.1
    obs[5] = test_ws_tree.FAR
    return obs, vel


@pytest.fixture(scope="module")
def mixed():
    obs, vel = six_worlds()
    dev, host = both_plans(obs, vel, SIX, [1, 2, 3, 4, 5, 6])
    return dict(obs=obs, vel=vel, dev=dev, host=host)


# ----------------------------------------------------------------------------------------------------------- trees
@pytest.mark.gpu
def test_mixed_batch_of_trees_equals_the_host_twin(mixed):
    host = mixed["host"]
    print("status", list(host.status), "count", list(host.count), "rewires", list(host.rewires))
    assert host.status[4] == 2 and (host.count[:4] > 50).all() and (host.rewires[:4] > 0).all() and host.count[5] > 50
    frozen = test_ws_tree._plan(mixed["obs"], [1, 2, 3, 4, 5, 6])
    assert any(frozen.count[w] != host.count[w] or not _same_bits(frozen.nodes[w], host.nodes[w]) for w in range(4))      # the motion shows


@pytest.mark.gpu
def test_zero_velocity_on_the_device_is_the_static_device_entry(arm):
    from armour_amd.ik import solve_ik
    obs, _ = moving_worlds(3)
    zero = np.zeros(obs.shape[:2] + (3,))
    static = test_ws_tree._plan(obs, [1, 2, 3], host=False, init=[CHAIN] * 3)
    targets, q_ref, world, seeds = ik_problem(arm)
    static_ik = solve_ik(arm["robot"], targets, q_ref, obs, world, seeds, S=32, details=True)
    for windows in (((0.0, 0.0),) * 3, ((-3.0, 4.0), (0.25, 0.25), (7.0, 11.5))):
        moving = _plan(obs, zero, windows, [1, 2, 3], host=False, init=[CHAIN] * 3)
        for w in range(3):
            assert_same_plans(moving, w, static, w)
        assert_same_ik(_solve(arm, targets, q_ref, obs, zero, windows, world, seeds, S=32, host=False), static_ik)


@pytest.mark.gpu
@pytest.mark.parametrize("O", [1, 5, 14])
def test_the_obstacle_split_offsets_by_the_moving_stride(O):
    """O staged obstacles and a near set of a few nodes: a round's work list is T = some tens of sub-segments, 2 T <= 256, so with O = 5 and
    O = 14 each item's obstacles are split over G = min(O, 256 / T) > 1 lanes whose slices begin at o0 * RM_MOV_STRIDE; with O = 1 there is
    no split.  A kernel that offset by the static stride would read another obstacle's numbers exactly here."""
    wall = wall_with_window()
    obs, vel = moving_worlds(5, extra=max(O - 5, 0), wall=wall[:min(O, 5)])
    assert obs.shape[1] == O
    dev, host = both_plans(obs, vel, WINDOWS, [1, 2, 3], **NARROW)
    print("O", O, "status", list(host.status), "count", list(host.count), "rewires", list(host.rewires))
    assert (host.count > 50).all()
    frozen = test_ws_tree._plan(obs, [1, 2, 3], **NARROW)
    if O > 1:
        assert any(frozen.count[w] != host.count[w] or not _same_bits(frozen.nodes[w], host.nodes[w]) for w in range(3))   # a verdict differs


@pytest.mark.gpu
def test_the_cap_of_256_obstacles_takes_the_raised_dynamic_lds(arm):
    """O = 256: 62 KB of staged obstacles, above the 48 KB a block has without asking -- once per entry."""
    from armour_amd.scenes import pad_obstacles
    obs = pad_obstacles(wall_with_window(), 256)[None]
    vel = np.zeros((1, 256, 3))
    vel[0, :, 1] = 0.02
    vel[0, 5:, 2] = 0.3                                                                 # the far boxes move, away from the workspace
    dev, host = both_plans(obs, vel, [(0.0, 0.5)], [1], max_iterations=120)
    assert host.count[0] > 50
    targets, q_ref, world, seeds = ik_problem(arm, W=1, per=2)
    both_ik(arm, targets, q_ref, obs, vel, [(0.0, 0.5)], world, seeds, 32)


@pytest.mark.gpu
def test_a_seeded_chain_with_a_blocked_edge_and_a_tree_past_256_nodes():
    obs, vel = moving_worlds(3)
    dev, host = both_plans(obs, vel, WINDOWS, [1, 2, 3], init=[CHAIN] * 3, max_iterations=60)
    assert (host.chain_kept < len(CHAIN)).all() and (host.chain_kept > 0).any()
    dev, host = both_plans(obs[:1], vel[:1], WINDOWS[:1], [1], max_iterations=450)
    assert host.count[0] > 256


@pytest.mark.gpu
def test_a_world_does_not_depend_on_the_other_worlds_of_its_launch(mixed):
    for w in (0, 1, 3):
        one = _plan(mixed["obs"][w:w + 1], mixed["vel"][w:w + 1], [SIX[w]], [w + 1], host=False)
        assert_same_plans(mixed["dev"], w, one, 0)


@pytest.mark.gpu
def test_static_then_moving_then_static_in_one_process(arm):
    from armour_amd.ik import solve_ik
    obs, vel = moving_worlds(3)
    targets, q_ref, world, seeds = ik_problem(arm)

    def static():
        return test_ws_tree._plan(obs, [1, 2, 3], host=False), solve_ik(arm["robot"], targets, q_ref, obs, world, seeds, S=32, details=True)
    before = static()
    moving = _plan(obs, vel, WINDOWS, [1, 2, 3], host=False)
    _solve(arm, targets, q_ref, obs, vel, WINDOWS, world, seeds, S=32, host=False)
    after = static()
    assert any(moving.count[w] != before[0].count[w] or not _same_bits(moving.nodes[w], before[0].nodes[w]) for w in range(3))
    for w in range(3):
        assert_same_plans(before[0], w, after[0], w)
    assert_same_ik(before[1], after[1])


# ----------------------------------------------------------------------------------------------------------- inverse kinematics
@pytest.fixture(scope="module")
def fourteen(arm):
    """14 targets in four moving worlds, S = 32, two of them in world -1, one under a box that arrives within its window"""
    obs, vel = moving_worlds(3, W=4)
    targets, q_ref, world, seeds = ik_problem(arm, W=4, per=3, seed=9)
    targets, q_ref = np.vstack([targets, targets[:1]]), np.vstack([q_ref, q_ref[:1]])
    world, seeds = np.concatenate([world, [-1]]), np.concatenate([seeds, seeds[:1] + 50])
    windows = SIX[:4]
    dev, host = both_ik(arm, targets, q_ref, obs, vel, windows, world, seeds, 32)
    return dict(obs=obs, vel=vel, targets=targets, q_ref=q_ref, world=world, seeds=seeds, windows=windows, dev=dev, host=host)


@pytest.mark.gpu
def test_mixed_batch_of_targets_equals_the_host_twin(arm, fourteen):
    from armour_amd.ik import solve_ik
    f = fourteen
    host = f["host"]
    print("status", list(host.status), "best", list(host.best))
    assert len(host.status) == 14 and (host.status == 1).any() and ((host.flags & 3) == 1).any() and (f["world"] == -1).sum() == 2
    frozen = solve_ik(arm["robot"], f["targets"], f["q_ref"], f["obs"], f["world"], f["seeds"], S=32, host=True, details=True)
    assert not np.array_equal(frozen.flags, host.flags)                                  # the motion shows in a verdict
    for t in (0, 5, 12, 13):                                                             # a target does not depend on the others of its launch
        one = _solve(arm, f["targets"][t:t + 1], f["q_ref"][t:t + 1], f["obs"], f["vel"], f["windows"], f["world"][t:t + 1], f["seeds"][t:t + 1], S=32, host=False)
        assert_same_ik(f["dev"], one, slice(t, t + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("O", [1, 5, 14])
@pytest.mark.parametrize("S", [1, 32, 128, 256])
def test_the_split_of_the_free_test_on_both_sides_of_its_threshold(arm, S, O):
    """Up to 128 seeds an item's obstacles are split over G = min(O, 256 / S) lanes, the slice of a lane beginning at rule.from(o0); above,
    a lane tests all O.  O = 1 has no split."""
    wall = wall_with_window()
    obs, vel = moving_worlds(5, extra=max(O - 5, 0), wall=wall[:min(O, 5)])
    targets, q_ref, world, seeds = ik_problem(arm, per=1, seed=4)
    dev, host = both_ik(arm, targets, q_ref, obs, vel, WINDOWS, world, seeds, S)
    assert (host.flags & 1).any()


@pytest.mark.gpu
def test_a_box_arriving_on_the_pick_on_the_device(arm):
    p_a = chain_np(arm["g"], Q_A[None], np.zeros(3))[0][0]
    box = blocking_box(arm["g"], p_a)
    box[0:3] += np.array([0.0, 0.0, 2.0])
    vel = np.array([[[0.0, 0.0, -1.0]]])
    dev, host = both_ik(arm, np.stack([p_a] * 2), Q_A, np.stack([box[None]] * 2), np.concatenate([vel] * 2), [(0.0, 0.5), (1.9, 2.1)], [0, 1], [3, 3], 8)
    assert host.status[0] == 1 and host.best[0] == 0 and (host.status[1] == 2 or host.best[1] != 0)


# ----------------------------------------------------------------------------------------------------------- the HLP
@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_trials_in_moving_worlds_record_the_host_twins_waypoints_and_no_proved_hit():
    """Two reference worlds with the 0.05 - 0.2 m/s velocities of test_trials_moving.py under moving_workspace_hlps on the device.  Every
    recorded waypoint is the host twins' for the recorded q0 and world time: the tree and the workspace waypoint of the twin, then the twin's
    inverse kinematics, whose device run differs by the rounding of sin / cos (test_ik_gpu.py's DEV_Q_TOL, as in test_ws_tree_gpu.py; so the
    records are re-derived one by one from the device run's own q0 instead of running a second trial, which that rounding would drive apart).
    And -- the end-to-end claim, which rests on the solver's tables, not on the planner -- no `plan` or `brake` piece is a proved hit."""
    from armour_amd import ik, scenes
    from armour_amd.planner import default_params, kinova_robot
    from armour_amd.tree_planner import call_seed
    from armour_amd.trials import run_trials
    from armour_amd.ws_planner import moving_workspace_hlps, plan_workspace_trees, waypoint_along_points, workspace_box
    from test_ik_gpu import DEV_Q_TOL
    robot = kinova_robot()
    all_ws = scenes.reference_worlds()
    idx = GPU_WORLDS[:2]
    ws = [all_ws[i] for i in idx]
    vel = seeded_velocities(ws, idx, GPU_SEED)
    opts = dict(max_iterations=150, max_nodes=256)
    make = moving_workspace_hlps(ws, robot, vel, seed=5, ik_options=dict(S=8), **opts)
    res = run_trials(ws, hlp=make, velocities=vel, T=64, solve_options=SOLVE, max_iterations=4)
    O = max(np.asarray(p["obstacles"]).reshape(-1, 12).shape[0] for _, p in ws)
    lb, ub = workspace_box(robot)
    horizon = default_params(1).duration
    records = from_ik = 0
    for i, w in enumerate(res["worlds"]):
        goal = np.asarray(ws[i][1]["goal"], dtype=np.float64)
        obs = scenes.pad_obstacles(np.asarray(ws[i][1]["obstacles"], dtype=np.float64).reshape(-1, 12), O)[None]
        v = np.concatenate([np.asarray(vel[i]).reshape(-1, 3), np.zeros((O - len(vel[i]), 3))])[None]
        for c, r in enumerate(w["records"]):
            window = dict(velocity=v, t_from=r["t_world"], t_to=r["t_world"] + horizon)
            z = ik.end_effector(robot, r["q0"])
            own = plan_workspace_trees(obs, [z], [ik.end_effector(robot, goal)], [call_seed(5, i, c)], lb, ub, host=True, **opts, **window)
            assert own.margin[0] > MARGIN
            point = z if own.paths[0] is None else waypoint_along_points(own.paths[0], z, 0.1)
            sol = ik.solve_ik(robot, point[None], 0.5 * (r["q0"] + goal), obs, [0], [call_seed(5, i, c)], S=8, host=True, **window)
            assert sol.margin[0] > MARGIN
            found = own.paths[0] is not None and sol.status[0] == ik.FOUND
            assert np.abs(r["q_des"] - (sol.q[0] if found else goal)).max() <= DEV_Q_TOL, (w["name"], c)
            records += 1
            from_ik += found
    assert records >= 4 and from_ik >= 2, (records, from_ik)
    assert sum(h.fallbacks for h in make.hlps.values()) == records - from_ik
    recs = [(w, r) for w in res["worlds"] for r in w["records"]]
    print({k: v for k, v in res["summary"].items() if "_ms" not in k}, [w["outcome"] for w in res["worlds"]],
          [(h.calls, h.fallbacks) for h in make.hlps.values()], "hlp_ms", [round(b["hlp_ms"], 2) for b in res["batches"]])
    bad = [(w["name"], r["iteration"], r["executed"], r["t_hit"]) for w, r in recs if r["executed"] in ("plan", "brake") and r["audit_verdict"] == 1]
    assert not bad, bad
    assert make.last_ms > 0.0 and all("hlp_ms" in b for b in res["batches"])
