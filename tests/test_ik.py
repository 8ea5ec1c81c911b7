"""Batched inverse kinematics for workspace goals, CPU half (include/armour_hip.h armour_ik / armour_ik_host / armour_ik_end_effector_host,
armour_amd/ik.py).

The rule -- end-effector point, position Jacobian, start points, the damped least-squares step with its Cholesky solve, the free test and the
pick -- is restated below in numpy from the header's text, on top of the frames and the node rule of test_roadmap.py and the counter hash of
test_tree_plan.py.  The restatement and the library's host twin run the same operations in the same order; only sin / cos come from
different libraries, so discrete outcomes (flags, iteration counts, the pick) must be equal wherever no clearance is within rounding of
zero (every comparison first asserts the twin's `margin`), and configurations agree to a measured tolerance.  What a user relies on is
asserted independently of both: a found configuration reaches its target, respects the joint limits and is free by the node rule.
The device is compared to the host twin in test_ik_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from test_roadmap import _limits, _robot, config_clearance, cross3, geometry, link_boxes, robot_dict
from test_tree_plan import u, wrapped_sq

LAM, E_MAX, TOL, MAX_IT = 0.05, 0.1, 1e-9, 200
MARGIN = 1e-9
# The tolerance on q and err.  Measured, host twin against the restatement over the 3424 items of the reference's worlds (S = 32, seeds
# 7 + w): max |dq| = 0 and max |derr| = 0 -- numpy and the C library take sin / cos from the same libm here -- with every flag and iteration
# count equal.  100 x 0 would leave no room for another libm, which is what the factor is for, so the tolerance is 100 x the response of the
# restatement to a rounding-size perturbation of its start points (relative 4e-16, random signs): max |dq| = 3.2e-13 (|derr| 4.6e-16), no
# flag or iteration count changed.  It has to stay <= 1e-9, else something other than rounding is at work.
Q_TOL = ERR_TOL = 3.2e-11
assert Q_TOL <= 1e-9


# ----------------------------------------------------------------------------------------------------------- numpy restatement
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def chain_np(g, Q, tool):
    """Q [K,n] -> the end-effector points [K,3] and the Jacobian's columns c [K,n,3] (c[:, j] = a_j x (p - o_j), zero for a joint that is not actuated)."""
    Q = np.asarray(Q, dtype=np.float64)
    P, R, _ = link_boxes(g, Q)
    Rl = R[:, -1]
    pe = P[:, -1] + np.stack([(Rl[:, i, 0] * tool[0] + Rl[:, i, 1] * tool[1]) + Rl[:, i, 2] * tool[2] for i in range(3)], -1)
    c = np.zeros((Q.shape[0], g["n"], 3))
    for j in range(g["n"]):
        ax = int(g["axes"][j]) if j < g["J"] else 0
        if ax != 0:
            a = (1.0 if ax > 0 else -1.0) * R[:, j, :, abs(ax) - 1]
            c[:, j] = cross3(a, pe - P[:, j])
    return pe, c


def clip_np(g, q, lb, ub):
    return np.where(g["cont"], q, np.minimum(np.maximum(q, lb), ub))


def starts_np(g, q_ref, seed, S, lb, ub):
    n = g["n"]
    q = np.stack([np.asarray(q_ref, dtype=np.float64)] + [np.array([lb[j] + u(int(seed), s, j) * (ub[j] - lb[j]) for j in range(n)]) for s in range(1, S)])
    return clip_np(g, q, lb, ub)


def iterate_np(g, targets, q0, lb, ub, tool, lam=LAM, e_max=E_MAX, tol=TOL, max_it=MAX_IT):
    """K items at once: targets [K,3], start points q0 [K,n] -> q [K,n], err [K], iterations [K], converged [K]."""
    q = np.array(q0, dtype=np.float64)
    K, n = q.shape
    err, its, conv = np.zeros(K), np.zeros(K, dtype=np.int32), np.zeros(K, dtype=bool)
    live = np.arange(K)
    l2 = lam * lam
    for k in range(max_it + 1):
        pe, c = chain_np(g, q[live], tool)
        e = targets[live] - pe
        er = np.sqrt(dot3(e, e))
        err[live], its[live] = er, k
        done = er <= tol
        conv[live[done]] = True
        if k == max_it:
            break
        live, e, er, c = live[~done], e[~done], er[~done], c[~done]
        if live.size == 0:
            break
        big = er > e_max
        sc = np.where(big, e_max / np.where(big, er, 1.0), 1.0)
        e = np.where(big[:, None], e * sc[:, None], e)
        A = np.zeros((live.size, 3, 3))
        for j in range(n):
            for i in range(3):
                for m in range(i + 1):
                    A[:, i, m] = A[:, i, m] + c[:, j, i] * c[:, j, m]
        for i in range(3):
            A[:, i, i] = A[:, i, i] + l2
        L00 = np.sqrt(A[:, 0, 0]); L10 = A[:, 1, 0] / L00; L20 = A[:, 2, 0] / L00
        L11 = np.sqrt(A[:, 1, 1] - L10 * L10); L21 = (A[:, 2, 1] - L20 * L10) / L11
        L22 = np.sqrt((A[:, 2, 2] - L20 * L20) - L21 * L21)
        z0 = e[:, 0] / L00; z1 = (e[:, 1] - L10 * z0) / L11; z2 = ((e[:, 2] - L20 * z0) - L21 * z1) / L22
        y2 = z2 / L22; y1 = (z1 - L21 * y2) / L11; y0 = ((z0 - L10 * y1) - L20 * y2) / L00
        y = np.stack([y0, y1, y2], -1)
        step = np.stack([dot3(c[:, j], y) for j in range(n)], -1)
        q[live] = clip_np(g, q[live] + step, lb, ub)
    return q, err, its, conv


def pick_np(g, q_ref, q, flags):
    """best of one target: the argmin of (acc, s) over the items with both bits, -1 with none"""
    keys = [(wrapped_sq(g, q_ref, q[s]), s) for s in range(len(flags)) if flags[s] == 3]
    return min(keys)[1] if keys else -1


def solve_np(g, targets, q_ref, obstacles, world, seeds, S, lb, ub, tool=np.zeros(3), **kw):
    """The header's run of N targets -> dict(status, best, q_all, err, iterations, flags, clearance [N,S] (nan where not converged))."""
    N, n = len(targets), g["n"]
    q0 = np.concatenate([starts_np(g, q_ref[t], seeds[t], S, lb, ub) for t in range(N)])
    q, err, its, conv = iterate_np(g, np.repeat(np.asarray(targets, dtype=np.float64), S, axis=0), q0, lb, ub, tool, **kw)
    q, err, its, conv = q.reshape(N, S, n), err.reshape(N, S), its.reshape(N, S), conv.reshape(N, S)
    cl = np.full((N, S), np.nan)
    for t in range(N):
        if conv[t].any():
            cl[t, conv[t]] = config_clearance(g, q[t, conv[t]], obstacles[world[t]] if world[t] >= 0 else np.zeros((0, 12)))
    flags = conv.astype(np.int32) + 2 * (conv & (np.nan_to_num(cl, nan=-1.0) > 0))
    best = np.array([pick_np(g, q_ref[t], q[t], flags[t]) for t in range(N)])
    status = np.where(best >= 0, 1, np.where(conv.any(axis=1), 2, 0))
    return dict(status=status, best=best, q_all=q, err=err, iterations=its, flags=flags, clearance=cl)


# ----------------------------------------------------------------------------------------------------------- fixtures
def _setup(name):
    robot = _robot(name)
    g = geometry(robot_dict(robot))
    lb, ub, _ = _limits(robot)
    return dict(robot=robot, g=g, lb=lb, ub=ub)


@pytest.fixture(scope="module")
def kinova():
    return _setup("kinova")


@pytest.fixture(scope="module")
def reference(kinova):
    """The reference's 107 worlds: target = the end effector of the scene's goal configuration, q_ref = the start, S = 32, seeds 7 + w;
    the host twin's answer with details and the restatement's, computed once."""
    from armour_amd import scenes
    from armour_amd.ik import solve_ik
    ws = scenes.reference_worlds()
    O = max(p["obstacles"].shape[0] for _, p in ws)
    obs = np.stack([scenes.pad_obstacles(p["obstacles"], O) for _, p in ws])
    starts, goals = np.stack([p["q0"] for _, p in ws]), np.stack([p["goal"] for _, p in ws])
    targets = chain_np(kinova["g"], goals, np.zeros(3))[0]
    seeds = np.arange(len(ws), dtype=np.uint64) + 7
    world = np.arange(len(ws))
    host = solve_ik(kinova["robot"], targets, starts, obs, world, seeds, S=32, host=True, details=True)
    ref = solve_np(kinova["g"], targets, starts, obs, world, seeds, 32, kinova["lb"], kinova["ub"])
    return dict(obs=obs, starts=starts, goals=goals, targets=targets, seeds=seeds, world=world, host=host, ref=ref)


# ----------------------------------------------------------------------------------------------------------- end effector, Jacobian
@pytest.mark.parametrize("name", ["kinova", "gripper", "fetch"])
def test_end_effector_and_jacobian(name):
    """Kinova; the gripper arm (J = 8, a fixed last joint); Fetch (J = 9, mixed axes, fixed joints): the library's point and Jacobian against
    the restatement, and the Jacobian against central differences of the restatement's point."""
    from armour_amd.ik import end_effector
    s = _setup(name)
    g, n = s["g"], s["g"]["n"]
    rng = np.random.default_rng(3)
    Q = rng.uniform(np.maximum(s["lb"], -np.pi), np.minimum(s["ub"], np.pi), (40, n))
    for tool in (np.zeros(3), np.array([0.03, -0.02, 0.11])):
        p, jac = end_effector(s["robot"], Q, tool=tool, jacobian=True)
        pe, c = chain_np(g, Q, tool)
        assert p.shape == (40, 3) and jac.shape == (40, 3, n)
        assert np.abs(p - pe).max() <= 1e-13 and np.abs(jac - np.swapaxes(c, 1, 2)).max() <= 1e-13      # a few ulp of sin / cos on lengths below 2 m
        h = 1e-6
        for j in range(n):
            d = np.zeros(n)
            d[j] = h
            fd = (chain_np(g, Q + d, tool)[0] - chain_np(g, Q - d, tool)[0]) / (2 * h)
            assert np.abs(jac[:, :, j] - fd).max() <= 1e-8, (name, j)      # truncation h^2 |p'''| / 6 ~ 3e-13, rounding 1e-16 / h ~ 1e-10
        if tool.any():                                                       # (with tool = 0 a last joint that turns about the point itself has a zero column)
            assert np.abs(jac).max(axis=(0, 1)).min() > 1e-3                # every factor of these arms is actuated: no zero column
    assert np.array_equal(end_effector(s["robot"], Q[0]), end_effector(s["robot"], Q[:1])[0])
    last = link_boxes(g, Q)[0][:, -1]
    assert np.abs(end_effector(s["robot"], Q) - last).max() <= 1e-13         # tool = 0: the origin of the last link frame


# ----------------------------------------------------------------------------------------------------------- the reference's worlds
def test_found_configurations_reach_their_targets_inside_the_limits_and_free(kinova, reference):
    g, r = kinova["g"], reference
    host = r["host"]
    assert (host.margin > MARGIN).all(), host.margin.min()
    assert (host.status == 1).all()                                           # FOUND for all 107
    conv = (host.flags & 1) == 1
    assert conv.mean() >= 0.95, conv.mean()
    assert not ((host.flags & 2) == 2)[~conv].any()                           # bit 1 is 0 when the item is not converged
    pe = chain_np(g, host.q, np.zeros(3))[0]
    assert np.linalg.norm(pe - r["targets"], axis=1).max() <= TOL + 1e-13     # tol, plus rounding between two sin / cos
    fixed = ~g["cont"]
    assert (host.q[:, fixed] >= kinova["lb"][fixed]).all() and (host.q[:, fixed] <= kinova["ub"][fixed]).all()
    for w in range(len(host.status)):
        assert config_clearance(g, host.q[w][None], r["obs"][w])[0] > 0, w
        assert host.best[w] == pick_np(g, r["starts"][w], host.q_all[w], host.flags[w]), w
        assert np.array_equal(host.q[w], host.q_all[w, host.best[w]])
    assert (host.best == 0).sum() >= 80 and (host.best > 0).any()             # mostly the start point's own solution, but not always


def test_host_twin_equals_the_restatement(kinova, reference):
    host, ref = reference["host"], reference["ref"]
    assert (host.margin > MARGIN).all()
    cl = np.abs(ref["clearance"])
    assert np.nanmin(cl) > MARGIN and np.abs(np.nanmin(cl, axis=1) - host.margin).max() <= 1e-11
    assert np.array_equal(host.status, ref["status"]) and np.array_equal(host.best, ref["best"])
    same = (host.iterations == ref["iterations"]) & ((host.flags & 1) == (ref["flags"] & 1))
    assert (~same).mean() <= 0.01, (~same).sum()                              # (measured: every item is the same)
    assert np.array_equal(host.flags[same], ref["flags"][same])
    dq, de = np.abs(host.q_all - ref["q_all"])[same].max(), np.abs(host.err - ref["err"])[same].max()
    print(f"host twin against the restatement: max |dq| = {dq:.3g}, max |derr| = {de:.3g}, items left out {(~same).sum()}")
    assert dq <= Q_TOL and de <= ERR_TOL, (dq, de)       # measured 0 and 0; the tolerance is 100 x 3.2e-13, a rounding-size perturbation's response (above)


# ----------------------------------------------------------------------------------------------------------- statuses
def _solve(s, targets, q_ref, **kw):
    from armour_amd.ik import solve_ik
    opts = dict(S=8, host=True, details=True)
    opts.update(kw)
    return solve_ik(s["robot"], targets, q_ref, **opts)


Q_A = np.array([0.3, 0.6, -0.2, 1.2, 0.1, 0.6, 0.0])


def blocking_box(g, p):
    """a cube about the point p that holds the whole last link that has a box (the last link itself on the Kinova arms; the Fetch presets end
    in links without one), wherever it points, when the last frame's origin is at p"""
    l = max(i for i in range(g["J"]) if np.any(g["h"][i] != 0.0))
    r = np.sqrt(dot3(g["c"][l], g["c"][l])) + np.sqrt(dot3(g["h"][l], g["h"][l])) + 0.01
    for i in range(l + 1, g["J"]):
        r = r + np.sqrt(dot3(g["trans"][i], g["trans"][i]))
    return np.array([p[0], p[1], p[2], r, 0, 0, 0, r, 0, 0, 0, r])


def test_statuses(kinova):
    s = kinova
    g = s["g"]
    p_a = chain_np(g, Q_A[None], np.zeros(3))[0][0]
    far = _solve(s, [[3.0, 0.0, 0.0]], Q_A, max_iterations=50)
    assert far.status[0] == 0 and far.best[0] == -1 and (far.iterations == 50).all() and not far.flags.any() and np.isnan(far.q).all()
    assert far.margin[0] == np.inf
    blocked = _solve(s, [p_a], np.zeros(7), obstacles=blocking_box(g, p_a)[None])
    assert blocked.status[0] == 2 and blocked.best[0] == -1 and np.isnan(blocked.q).all()        # the row still holds what it was filled with
    assert (blocked.flags & 1).sum() >= 4 and not (blocked.flags & 2).any() and blocked.margin[0] > MARGIN
    for kw in (dict(obstacles=blocking_box(g, p_a)[None], world=[-1]), dict(obstacles=np.zeros((1, 0, 12))), dict()):
        res = _solve(s, [p_a], np.zeros(7), **kw)
        assert res.status[0] == 1 and (res.flags & 1).sum() >= 4 and np.array_equal((res.flags & 1) == 1, (res.flags & 2) == 2), kw
        assert res.margin[0] == np.inf
    on = _solve(s, [p_a], Q_A, max_iterations=0)
    assert on.status[0] == 1 and on.best[0] == 0 and on.iterations[0, 0] == 0 and on.flags[0, 0] == 3 and np.array_equal(on.q[0], Q_A)
    assert not on.iterations.any() and not on.flags[0, 1:].any()


def test_joint_limits_clip_and_pin(kinova):
    """Every joint but joint 1 is pinned (lb = ub), so the end effector moves on one arc and a target on it is reached by one value of
    joint 1 alone."""
    s = kinova
    g = s["g"]
    lb, ub = Q_A.copy(), Q_A.copy()
    lb[1], ub[1] = -0.5, 0.5
    at = lambda x: chain_np(g, np.where(np.arange(7) == 1, x, Q_A)[None], np.zeros(3))[0][0]
    start = np.where(np.arange(7) == 1, 0.2, Q_A)
    kw = dict(lb=lb, ub=ub, continuous=np.zeros(7), S=4)
    res = _solve(s, [at(0.5)], start, **kw)                                   # the target is reached with joint 1 at its bound
    assert res.status[0] == 1 and res.best[0] == 0
    assert 0.5 - 1e-8 <= res.q[0, 1] <= 0.5 and np.array_equal(np.delete(res.q[0], 1), np.delete(Q_A, 1))
    q1 = res.q_all[0, :, 1]
    assert (q1 >= -0.5).all() and (q1 <= 0.5).all() and (np.delete(res.q_all[0], 1, axis=1) == np.delete(Q_A, 1)).all()
    beyond = _solve(s, [at(0.7)], start, max_iterations=30, **kw)             # the target lies past the bound: the joint stops AT the bound
    assert beyond.status[0] == 0 and (beyond.iterations == 30).all() and beyond.q_all[0, 0, 1] == 0.5
    outside = _solve(s, [at(0.5)], np.where(np.arange(7) == 1, 0.9, Q_A), **kw)   # a start point outside the box is clipped first
    assert outside.status[0] == 1 and outside.iterations[0, 0] == 0 and outside.q[0, 1] == 0.5
    ref = solve_np(dict(g, cont=np.zeros(7, dtype=bool)), np.array([at(0.5)]), start[None], np.zeros((0, 0, 12)), [-1], [0], 4, lb, ub)
    assert np.array_equal(res.iterations, ref["iterations"]) and np.abs(res.q_all - ref["q_all"]).max() <= Q_TOL


# ----------------------------------------------------------------------------------------------------------- the C ABI
def _raw(s, host, N=1, S=4, W=1, O=1, **kw):
    """armour_ik(_host) itself, every argument replaceable -> (rc, status, best, q_best)"""
    from armour_amd import _lib
    from armour_amd.scenes import FAR_BOX
    L = _lib.load()
    n, rows = s["robot"].num_factors, max(N, 1)
    a = dict(lb=s["lb"], ub=s["ub"], tool=np.zeros(3), obstacles=np.tile(FAR_BOX, (max(W, 1), max(O, 1), 1)), world=np.zeros(rows, dtype=np.int32),
             targets=np.tile([0.4, 0.1, 0.6], (rows, 1)), q_ref=np.tile(Q_A, (rows, 1)), lam=LAM, e_max=E_MAX, tol=TOL, max_iterations=20)
    a.update(kw)
    f64 = lambda k: np.ascontiguousarray(a[k], dtype=np.float64)
    lb, ub, tool, obstacles, targets, q_ref = (f64(k) for k in ("lb", "ub", "tool", "obstacles", "targets", "q_ref"))
    world = np.ascontiguousarray(a["world"], dtype=np.int32)
    seeds = np.arange(1, rows + 1, dtype=np.uint64)
    status, best, q_best = np.zeros(rows, dtype=np.int32), np.zeros(rows, dtype=np.int32), np.full((rows, n), -7.0)
    i32, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    fn = L.armour_ik_host if host else L.armour_ik
    rc = fn(C.byref(s["robot"]), None, lb.ctypes.data_as(dp), ub.ctypes.data_as(dp), tool.ctypes.data_as(dp), N, S, W, O, obstacles.ctypes.data_as(dp),
            world.ctypes.data_as(i32), targets.ctypes.data_as(dp), q_ref.ctypes.data_as(dp), seeds.ctypes.data_as(C.POINTER(C.c_uint64)), float(a["lam"]),
            float(a["e_max"]), float(a["tol"]), int(a["max_iterations"]), status.ctypes.data_as(i32), best.ctypes.data_as(i32), q_best.ctypes.data_as(dp),
            None, None, None, None, None)
    return rc, status, best, q_best


def _with(x, j, v):
    x = np.array(x, dtype=np.float64)
    x.flat[j] = v
    return x


@pytest.mark.parametrize("host", [False, True])
def test_bad_arguments_are_refused_before_a_device_is_touched(kinova, host):
    """The device entry too answers EINVAL, not EDEVICE, on a machine without a device: the checks come first."""
    from armour_amd import _lib
    s = kinova
    bad = [dict(S=0), dict(S=_lib.IK_MAX_SEEDS + 1), dict(N=-1), dict(max_iterations=-1), dict(max_iterations=_lib.IK_MAX_ITERATIONS + 1)]
    bad += [{k: v} for k in ("lam", "e_max", "tol") for v in (0.0, -0.1, np.nan, np.inf)]
    bad += [dict(lb=_with(s["lb"], 1, s["ub"][1] + 0.1)), dict(lb=_with(s["lb"], 2, -np.inf)), dict(ub=_with(s["ub"], 3, np.inf)), dict(ub=_with(s["ub"], 0, np.nan)),
            dict(targets=[[0.4, np.nan, 0.6]]), dict(targets=[[np.inf, 0.1, 0.6]]), dict(q_ref=_with(Q_A[None], 4, np.nan)), dict(tool=[0.0, np.inf, 0.0]),
            dict(obstacles=_with(np.zeros((1, 1, 12)), 5, np.nan)), dict(W=-1), dict(O=257, obstacles=np.zeros((1, 257, 12))), dict(world=[-2]), dict(world=[1]),
            dict(W=2, world=[2])]
    for kw in bad:
        rc, _, _, _ = _raw(s, host, **kw)
        assert rc == _lib.EINVAL, kw
    rc, _, _, _ = _raw(s, host, N=0)                     # no target: a success that does nothing, with or without a device
    assert rc == _lib.OK
    if host:
        rc, status, best, q_best = _raw(s, True, targets=[[3.0, 0.0, 0.0]])
        assert rc == _lib.OK and status[0] == 0 and best[0] == -1 and (q_best == -7.0).all()      # no pick: the row is not written


def test_a_batch_equals_its_targets_one_by_one_and_one_seed_is_enough(kinova, reference):
    from armour_amd.ik import solve_ik
    s, r = kinova, reference
    pick = [0, 17, 101, 106]
    world = np.array([0, 1, 2, -1])
    obs, targets, starts, seeds = r["obs"][pick[:3]], r["targets"][pick], r["starts"][pick], r["seeds"][pick]
    for S in (1, 6):
        batch = solve_ik(s["robot"], targets, starts, obs, world, seeds, S=S, host=True, details=True)
        for t in range(4):
            one = solve_ik(s["robot"], targets[t:t + 1], starts[t:t + 1], obs, world[t:t + 1], seeds[t:t + 1], S=S, host=True, details=True)
            for k in ("status", "best", "q", "q_all", "err", "iterations", "flags", "margin"):
                assert np.array_equal(getattr(batch, k)[t:t + 1], getattr(one, k), equal_nan=True), (S, t, k)
        assert batch.flags.shape == (4, S) and (batch.flags & 1).any()
    assert np.array_equal(batch.q_all[:, 0], solve_ik(s["robot"], targets, starts, obs, world, seeds, S=1, host=True, details=True).q_all[:, 0])   # item 0 starts at q_ref


# ----------------------------------------------------------------------------------------------------------- the Python helpers
def test_workspace_goals_for_worlds(kinova, reference):
    from armour_amd import scenes
    from armour_amd.ik import goal_configurations, solve_ik, with_workspace_goals
    from armour_amd.tree_planner import call_seed
    s, r = kinova, reference
    worlds = scenes.reference_worlds()[:4]
    ee = r["targets"][:4].copy()
    goals, status = goal_configurations(worlds, s["robot"], ee, seed=11, host=True, S=8)
    own = solve_ik(s["robot"], ee, r["starts"][:4], r["obs"][:4], np.arange(4), [call_seed(11, i, 0) for i in range(4)], S=8, host=True)
    assert np.array_equal(goals, own.q) and np.array_equal(status, own.status) and (status == 1).all()
    new = with_workspace_goals(worlds, s["robot"], ee, seed=11, host=True, S=8)
    for (name, p), (name2, p2), gq in zip(worlds, new, goals):
        assert name == name2 and np.array_equal(p2["goal"], gq) and p2 is not p and np.array_equal(p2["q0"], p["q0"])
        assert np.array_equal(p2["q_des"], scenes.straight_line_waypoint(p["q0"], gq, p["lookahead"]))
        assert np.abs(chain_np(s["g"], p2["goal"][None], np.zeros(3))[0][0] - chain_np(s["g"], p["goal"][None], np.zeros(3))[0][0]).max() <= 2 * TOL
    ee[2] = [3.0, 0.0, 0.0]                                                    # out of reach
    kept = with_workspace_goals(worlds, s["robot"], ee, on_fail="keep", seed=11, host=True, S=8, max_iterations=40)
    assert np.array_equal(kept[2][1]["goal"], worlds[2][1]["goal"]) and np.array_equal(kept[2][1]["q_des"], worlds[2][1]["q_des"])
    with pytest.raises(RuntimeError):
        with_workspace_goals(worlds, s["robot"], ee, on_fail="raise", seed=11, host=True, S=8, max_iterations=40)
    with pytest.raises(ValueError):
        with_workspace_goals(worlds, s["robot"], ee, on_fail="drop", host=True)
