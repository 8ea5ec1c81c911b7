"""Batched inverse kinematics for workspace goals, device half: armour_ik on the MI355X against its host twin armour_ik_host.

The two run the same functions; only sin / cos in the link frames differ.  That moves a configuration by rounding -- an item's q and err
are compared to a measured tolerance -- and can change a discrete outcome only where an error is within rounding of `tol` or a clearance
within rounding of zero: every comparison first asserts that the host twin's `margin` is above 1e-9 and then demands equal statuses and
picks, and equal flags and iteration counts on all but at most 1 % of the items (measured: on all).  The host twin is held to the numpy restatement of the
rule in test_ik.py.  The shapes are the smallest at which each part of the kernel can go wrong: one seed, seeds across a wave, the free
test shared by 14 and by 2 lanes and not shared, all four waves in the pick, no obstacles and more obstacles than the worlds hold."""
import numpy as np
import pytest

from test_ik import MARGIN, Q_A, _setup, blocking_box, chain_np
from test_tree_plan import box_at_link

# |q(device) - q(host twin)| and |err(device) - err(host twin)| over the converged items of every test below, measured once on one MI355X:
# the largest seen is 8.3e-15 (the tool test) and 4.5e-16 (the gripper arm), with no flag and no iteration count different anywhere.  The
# tolerance is 100 x that, as headroom for other builds of the device's sin / cos; it has to stay <= 1e-9, else something other than
# rounding is at work.
# Items that did NOT converge are compared by flags and iteration count only.  At a target out of reach the iteration chatters about the
# stretched arm and is chaotic: in the numpy restatement alone a relative 4e-16 perturbation of the start points grows to 1.4e-8 after 25
# steps and to 1.2 rad after 100, and the device's items of the mixed batch's unreachable target end up to 1.2 rad (err: 0.045 m) from the
# twin's after their 200 steps -- each a faithful run of the rule with its own sin / cos.  Such a q is no solution and nobody reads it.
DEV_SEEN_Q, DEV_SEEN_ERR = 8.3e-15, 4.5e-16
DEV_Q_TOL, DEV_ERR_TOL = 100 * DEV_SEEN_Q, 100 * DEV_SEEN_ERR
assert DEV_Q_TOL <= 1e-9 and DEV_ERR_TOL <= 1e-9


@pytest.fixture(scope="module")
def kinova():
    return _setup("kinova")


@pytest.fixture(scope="module")
def scenes14():
    """the reference's worlds, padded to one obstacle count (14), with the end effector of every goal as the target"""
    from armour_amd import scenes
    ws = scenes.reference_worlds()
    O = max(p["obstacles"].shape[0] for _, p in ws)
    g = _setup("kinova")["g"]
    goals = np.stack([p["goal"] for _, p in ws])
    return dict(worlds=ws, obs=np.stack([scenes.pad_obstacles(p["obstacles"], O) for _, p in ws]), starts=np.stack([p["q0"] for _, p in ws]),
                targets=chain_np(g, goals, np.zeros(3))[0], O=O)


def both(robot, targets, q_ref, obstacles, world, seeds, **kw):
    """(device, host twin) of one solve_ik call with details; the host run's margins are asserted first"""
    from armour_amd.ik import solve_ik
    host = solve_ik(robot, targets, q_ref, obstacles, world, seeds, host=True, details=True, **kw)
    assert (host.margin > MARGIN).all(), host.margin
    return solve_ik(robot, targets, q_ref, obstacles, world, seeds, details=True, **kw), host


def assert_device_equals_twin(dev, host, what="", q_tol=None, err_tol=None):
    """(q_tol / err_tol: a caller's own measured tolerances, for arms measured elsewhere; default: this file's)"""
    q_tol, err_tol = DEV_Q_TOL if q_tol is None else q_tol, DEV_ERR_TOL if err_tol is None else err_tol
    assert np.array_equal(dev.status, host.status) and np.array_equal(dev.best, host.best), (what, dev.status, host.status, dev.best, host.best)
    same = (dev.iterations == host.iterations) & ((dev.flags & 1) == (host.flags & 1))
    assert (~same).mean() <= 0.01, (what, (~same).sum())
    assert np.array_equal(dev.flags[same], host.flags[same]), what
    conv = same & ((host.flags & 1) == 1)                                       # (items that did not converge: see DEV_Q_TOL)
    dq, de = (np.abs(dev.q_all - host.q_all)[conv].max(), np.abs(dev.err - host.err)[conv].max()) if conv.any() else (0.0, 0.0)
    found = host.status == 1
    db = np.abs(dev.q[found] - host.q[found]).max() if found.any() else 0.0
    print(f"device against the host twin {what}: max |dq| = {dq:.3g}, max |derr| = {de:.3g}, max |dq_best| = {db:.3g}, items left out {(~same).sum()} of {same.size}, converged {conv.sum()}")
    assert dq <= q_tol and de <= err_tol and db <= q_tol, (what, dq, de, db)
    assert np.array_equal(np.isnan(dev.q), np.isnan(host.q))                   # a row without a pick is left as it was on both sides
    for t in np.flatnonzero(found):
        assert np.array_equal(dev.q[t], dev.q_all[t, dev.best[t]])
    assert dev.ms > 0.0 and dev.margin is None


@pytest.mark.gpu
def test_mixed_batch_equals_the_host_twin(kinova, scenes14):
    """N = 6 in one launch: three reference worlds, a target out of reach, a target inside a box, a target without a world."""
    from armour_amd.scenes import FAR_BOX
    s, r = kinova, scenes14
    p_a = chain_np(s["g"], Q_A[None], np.zeros(3))[0][0]
    pick = [3, 55, 104]
    obs = np.concatenate([r["obs"][pick], np.stack([np.vstack([blocking_box(s["g"], p_a)[None], np.tile(FAR_BOX, (r["O"] - 1, 1))])])])
    targets = np.vstack([r["targets"][pick], [[3.0, 0.0, 0.0]], [p_a], [p_a]])
    q_ref = np.vstack([r["starts"][pick], [Q_A], [np.zeros(7)], [np.zeros(7)]])
    dev, host = both(s["robot"], targets, q_ref, obs, [0, 1, 2, 0, 3, -1], np.arange(6) + 7, S=32)
    assert list(host.status) == [1, 1, 1, 0, 2, 1]
    assert_device_equals_twin(dev, host, "mixed batch")


@pytest.mark.gpu
@pytest.mark.parametrize("S,O", [(1, 14), (8, 14), (65, 14), (128, 3), (200, 14), (256, 14), (32, 0), (32, 64)])
def test_seed_and_obstacle_counts_equal_the_host_twin(kinova, scenes14, S, O):
    """S = 1; S = 8 with O = 14 (14 lanes per item); S = 65 (across a wave); S = 128 with O = 3 (2 lanes per item); S = 200 (a lane per
    item); S = 256 (all four waves in the pick); O = 0; O = 64 (LDS staging beyond the worlds' own 14)."""
    from armour_amd import scenes
    s, r = kinova, scenes14
    pick = [3, 104]
    if O == 0:
        obs = np.zeros((2, 0, 12))
    elif O <= r["O"]:
        obs = r["obs"][pick][:, :O]
    else:
        obs = np.stack([scenes.pad_obstacles(r["obs"][w], O) for w in pick])
    dev, host = both(s["robot"], r["targets"][pick], r["starts"][pick], obs, [0, 1], [10, 111], S=S)
    assert (host.flags & 1).any() and host.flags.shape == (2, S)
    if O == 0:
        assert np.array_equal((host.flags & 1) == 1, (host.flags & 2) == 2)
    assert_device_equals_twin(dev, host, f"S = {S}, O = {O}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fetch", "gripper"])
def test_other_arms_equal_the_host_twin(name):
    """Fetch (J = 9, mixed and negative axes, fixed joints) and the gripper arm (J = 8, a fixed last joint), with a box in the way of some solutions."""
    s = _setup(name)
    g, n = s["g"], s["g"]["n"]
    rng = np.random.default_rng(8)
    lo, hi = np.maximum(s["lb"], -np.pi), np.minimum(s["ub"], np.pi)
    goals = rng.uniform(0.5 * lo, 0.5 * hi, (3, n))
    q_ref = rng.uniform(0.25 * lo, 0.25 * hi, (3, n))
    obs = np.stack([box_at_link(g, 0.5 * (a + b), link=3)[None] for a, b in zip(goals, q_ref)])
    dev, host = both(s["robot"], chain_np(g, goals, np.zeros(3))[0], q_ref, obs, [0, 1, 2], [1, 2, 3], S=24)
    assert (host.status == 1).any() and ((host.flags & 3) == 1).any()          # some solutions are blocked
    assert_device_equals_twin(dev, host, name)


@pytest.mark.gpu
def test_a_tool_point_equals_the_host_twin(kinova, scenes14):
    s, r = kinova, scenes14
    tool = np.array([0.03, -0.02, 0.11])
    pick = [20, 21, 105]
    goals = np.stack([r["worlds"][w][1]["goal"] for w in pick])
    targets = chain_np(s["g"], goals, tool)[0]
    dev, host = both(s["robot"], targets, r["starts"][pick], r["obs"][pick], [0, 1, 2], [5, 6, 7], S=16, tool=tool)
    assert (host.status == 1).all()
    assert np.linalg.norm(chain_np(s["g"], dev.q, tool)[0] - targets, axis=1).max() <= 1e-9 + 1e-13
    assert_device_equals_twin(dev, host, "tool")


@pytest.mark.gpu
def test_a_target_does_not_depend_on_the_other_targets_of_the_launch(kinova, scenes14):
    """The first 16 reference worlds in one launch and in 16 launches: device against device, so the bits must match."""
    from armour_amd.ik import solve_ik
    s, r = kinova, scenes14
    seeds = np.arange(16, dtype=np.uint64) + 3
    batch = solve_ik(s["robot"], r["targets"][:16], r["starts"][:16], r["obs"][:16], np.arange(16), seeds, S=32, details=True)
    for t in range(16):
        one = solve_ik(s["robot"], r["targets"][t:t + 1], r["starts"][t:t + 1], r["obs"][t:t + 1], [0], seeds[t:t + 1], S=32, details=True)
        for k in ("status", "best", "q", "q_all", "err", "iterations", "flags"):
            assert np.array_equal(getattr(batch, k)[t:t + 1], getattr(one, k), equal_nan=True), (t, k)
    assert (batch.status == 1).all() and (batch.flags & 1).mean() > 0.9


@pytest.mark.gpu
def test_workspace_goals_feed_the_tree_planner(kinova, scenes14):
    """with_workspace_goals on eight reference worlds, then ONE plan_trees call from the starts to the returned goals: the statuses are
    those of the same call with the goals of the host twin's inverse kinematics."""
    from armour_amd.ik import with_workspace_goals
    from armour_amd.tree_planner import plan_trees
    s, r = kinova, scenes14
    worlds = r["worlds"][:8]
    plans, goals = {}, {}
    for host in (False, True):
        new = with_workspace_goals(worlds, s["robot"], r["targets"][:8], on_fail="raise", seed=5, host=host)
        goals[host] = np.stack([p["goal"] for _, p in new])
        assert not any(np.array_equal(p["goal"], q["goal"]) for (_, p), (_, q) in zip(new, worlds))
        plans[host] = plan_trees(s["robot"], r["obs"][:8], r["starts"][:8], goals[host], np.arange(8) + 1, step=0.5, edge_step=0.05, max_iterations=400, max_nodes=512)
    assert np.abs(goals[False] - goals[True]).max() <= DEV_Q_TOL
    assert np.array_equal(plans[False].status, plans[True].status) and (plans[False].status == 1).sum() >= 6
