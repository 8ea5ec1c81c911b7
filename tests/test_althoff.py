"""The Althoff robust input (armour_althoff_controller, ARMOUR_TRACK_CTL_ALTHOFF) and the two-controller study
(tracking.compare_robust_controller(..., controllers=("robust", "althoff"))): kinova_controller_ALTHOFF.cpp, robust_controller.cpp:112-128,
kinova_compare_robust_controller.m and its _summary.m.

The restatement is numpy on top of the CPU oracle as it is: oracle.cpu_oracle.robust_controller returns tau, tau_interval and inside, none of
which depend on alpha or V_max; from them bound_i = max(|lo_i - tau_i|, |hi_i - tau_i|), v = -(kappa_t |bound| + phi_t) r, u = tau - v
(althoff_restatement).  Rollouts reuse test_tracking.host_track unchanged: it imports robust_controller at call time, so it runs with
controller="robust" while oracle.cpu_oracle.robust_controller is replaced by the Althoff restatement (_althoff_in_the_oracle) -- the same RK4,
monitors and limit bookkeeping, no second copy.

Tolerances: the controller at 1e-12 max(1, |ref|), tests/test_controller.py's derived figure (same operation order; the device rounds the
interval difference phi outward by an ulp, which the restatement does not: 1e-16 relative); tracking at test_tracking._compare's 1e-9 with
status, steps, flags, t_end and first_violation_t exact; flags only where every node is >= 1e-6 from the limit.

Seen on one MI355X: the largest |device - restatement| of the tracking rollouts, with and without the torque limit, is 7.3e-15.

Not covered: status 1 under the Althoff mode -- the interval model encloses the nominal one by construction, as for the robust mode.
"""
import contextlib
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from armour_amd import _lib
from test_tracking import N_J, _compare, _plans, _reference, _robot, _same_bits, _start_inside, _wrap, host_track, with_limits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_RANGE = np.full(N_J, np.pi / 48)
KP = (28.1037, 28.1037)   # KSI/uarmtd_robust_CBF_LLC.m:11
MARGIN = 1e-6
FIELDS = ("status", "steps", "limit_flags", "t_end", "q", "qd", "max_pos_error", "max_vel_error", "max_V", "max_robust_input", "max_torque_ratio",
          "first_violation_t", "trace")


def althoff_restatement(robust_controller, Kr, Kp, Ki, q, qd, q_des, qd_des, qdd_des, eps, robot, e_acc=0.0):
    """RobustController::update, ALTHOFF method, for one state from the oracle's nominal torque and interval torque."""
    n = robot.num_factors
    out = robust_controller(Kr, 1.0, 1.0, 0.0, q, qd, q_des, qd_des, qdd_des, eps=eps, robot=robot)   # (alpha, V_max: tau and its interval do not depend on them)
    tau, ti = out["tau"], out["tau_interval"]
    bound = np.maximum(np.abs(ti[:, 0] - tau), np.abs(ti[:, 1] - tau))
    kr = np.broadcast_to(np.asarray(Kr, dtype=np.float64).ravel(), (n,))
    r = (np.asarray(qd_des) - np.asarray(qd)) + kr * _wrap(np.asarray(q_des, dtype=np.float64) - np.asarray(q, dtype=np.float64))
    phi_t, kappa_t = Kp[0] + Ki[0] * e_acc, Kp[1] + Ki[1] * e_acc
    v = -(kappa_t * np.linalg.norm(bound) + phi_t) * r
    return dict(u=tau - v, tau=tau, v=v, inside=out["inside"], r=r, bound=bound)


@contextlib.contextmanager
def _althoff_in_the_oracle(Kp=KP):
    """oracle.cpu_oracle.robust_controller replaced by the Althoff restatement (e_acc = 0, as armour_track runs it) for host_track."""
    from oracle import cpu_oracle
    orig = cpu_oracle.robust_controller

    def patched(Kr, alpha, V_max, r_thr, q, qd, q_des, qd_des, qdd_des, eps=0.03, robot=None):
        return althoff_restatement(orig, Kr, Kp, (0.0, 0.0), q, qd, q_des, qd_des, qdd_des, eps, robot)

    cpu_oracle.robust_controller = patched
    try:
        yield
    finally:
        cpu_oracle.robust_controller = orig


def host_track_althoff(*a, Kp=KP, **kw):
    with _althoff_in_the_oracle(Kp):
        return host_track(*a, controller="robust", **kw)


def _simulate(*a, **kw):
    from armour_amd.tracking import simulate_tracking
    return simulate_tracking(*a, **kw)


def _bit_equal(a, b, lane_a, lane_b, fields=FIELDS):
    for name in fields:
        x, y = getattr(a, name), getattr(b, name)
        if x is None and y is None:
            continue
        assert np.array_equal(np.asarray(x[lane_a]), np.asarray(y[lane_b]), equal_nan=True), (name, lane_a, lane_b)


# ------------------------------------------------------------------------------------------------ CPU
def test_entries_check_their_arguments():
    """The symbol, every bad argument before the device, the device error without one; the tracking mode's id, its gain's place in the
    options and the ids that stay refused."""
    L = _lib.load()
    rb = _robot()
    n, B = rb.num_factors, 3
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    rng = np.random.default_rng(41)
    good = dict(q=rng.uniform(-3, 3, (B, n)), qd=rng.uniform(-1, 1, (B, n)), q_des=rng.uniform(-3, 3, (B, n)), qd_des=rng.uniform(-1, 1, (B, n)),
                qdd_des=rng.uniform(-2, 2, (B, n)), Kr=np.full(n, 10.0), Kp=np.array(KP), Ki=np.array([4.0, 4.0]), e_acc=np.zeros(B),
                u=np.zeros((B, n)), tau=np.zeros((B, n)), v=np.zeros((B, n)))

    def call(eps=0.03, B=B, robot=rb, **over):
        a = {**good, **over}
        a = {key: (None if val is None else np.ascontiguousarray(val)) for key, val in a.items()}
        return L.armour_althoff_controller(None if robot is None else C.byref(robot), eps, dp(a["Kr"]), dp(a["Kp"]), dp(a["Ki"]), dp(a["e_acc"]), B,
                                           dp(a["q"]), dp(a["qd"]), dp(a["q_des"]), dp(a["qd_des"]), dp(a["qdd_des"]), dp(a["u"]), dp(a["tau"]), dp(a["v"]))

    assert call(robot=None) == _lib.EINVAL
    for name in good:
        if name != "e_acc":
            assert call(**{name: None}) == _lib.EINVAL, name
    assert call(B=0) == _lib.EINVAL and call(B=-1) == _lib.EINVAL
    for bad in (math.nan, math.inf, -math.inf):
        for name in ("q", "qd", "q_des", "qd_des", "qdd_des"):
            for where in ((0, 0), (B - 1, n - 1)):
                arr = good[name].copy()
                arr[where] = bad
                assert call(**{name: arr}) == _lib.EINVAL, (name, where, bad)
        for name, where in (("Kr", n - 1), ("Kp", 0), ("Kp", 1), ("Ki", 0), ("Ki", 1), ("e_acc", B - 1)):
            arr = good[name].copy()
            arr[where] = bad
            assert call(**{name: arr}) == _lib.EINVAL, (name, bad)
        assert call(eps=bad) == _lib.EINVAL, bad
    assert call(eps=-0.01) == _lib.EINVAL
    expected = _lib.OK if L.armour_device_available() else _lib.EDEVICE
    assert call() == expected and call(e_acc=None) == expected

    # tracking: mode 4
    assert _lib.TRACK_CTL_ALTHOFF == 4
    assert C.sizeof(_lib.ArmourTrackOptions) == 16 + 8 * (_lib.MAXF + 12)
    assert _lib.ArmourTrackOptions.althoff_Kp.offset == 16 + 8 * (_lib.MAXF + 8) and _lib.ArmourTrackOptions.reserved.offset == 16 + 8 * (_lib.MAXF + 10)
    opt = _lib.ArmourTrackOptions()
    L.armour_track_options_default(C.byref(rb), C.byref(opt))
    raw = (C.c_double * (_lib.MAXF + 12)).from_buffer_copy(bytes(opt)[16:])   # the doubles as the library wrote them: Kr | 8 constants | 4 that were reserved
    assert list(raw[_lib.MAXF + 8:]) == [28.1037, 28.1037, 0.0, 0.0] and list(opt.althoff_Kp) == [28.1037, 28.1037]
    z, kr = np.zeros(n), np.full(n, np.pi / 48)
    res = (_lib.ArmourTrackResult * 1)()

    def track(**fields):
        o = _lib.ArmourTrackOptions()
        L.armour_track_options_default(C.byref(rb), C.byref(o))
        o.t1, o.duration = 0.01, 1.0
        for key, val in fields.items():
            if key == "kp0":
                o.althoff_Kp[0] = val
            else:
                setattr(o, key, val)
        return L.armour_track(C.byref(rb), C.byref(o), 1, dp(z), dp(z), dp(z), dp(z), dp(kr), None, None, None, res, None, None)

    assert track(controller=4) == expected
    assert track(controller=4, kp0=math.nan) == _lib.EINVAL and track(controller=4, kp0=math.inf) == _lib.EINVAL
    assert track(controller=0, kp0=math.nan) == expected   # ignored by the other modes
    assert track(controller=3) == _lib.EINVAL and track(controller=5) == _lib.EINVAL and track(controller=7) == _lib.EINVAL
    assert L.armour_track_auto_steps(4) >= 1
    assert L.armour_track_auto_steps(3) == _lib.EINVAL and L.armour_track_auto_steps(7) == _lib.EINVAL
    from armour_amd.tracking import CONTROLLERS
    assert CONTROLLERS["althoff"] == 4


def test_restatement_stays_on_the_reference_on_the_nominal_plant():
    """True plant = nominal model, start on the reference: r = 0, so v = 0 and the closed loop is the nominal controller's -- q = q_des is its
    solution.  The bounds are test_restatement_tracks_exactly_under_the_nominal_controller's."""
    rb = _robot()
    rng = np.random.default_rng(5)
    q0, qd0, qdd0, k = _plans(rng, 1)
    out = host_track_althoff(rb, q0[0], qd0[0], qdd0[0], k[0], K_RANGE, 1.0, t1=0.5)
    assert out["status"] == 0 and out["steps"] == 500
    assert out["max_pos_error"] <= 1e-10 and out["max_vel_error"] <= 1e-9
    assert out["max_robust_input"] <= 1e-6   # (v = -(gain) r with r at rounding level)


def test_restatement_v_opposes_r_and_grows_with_the_uncertainty():
    from oracle.cpu_oracle import robust_controller
    import test_controller as tc
    rb = tc._oracle_robot("kinova")
    q, qd, q_des, qd_des, qdd_des = tc._states(7, 20)
    for s in range(20):
        norms = []
        for eps in (0.0, 0.03, 0.3):
            out = althoff_restatement(robust_controller, tc.KR, KP, (4.0, 4.0), q[s], qd[s], q_des[s], qd_des[s], qdd_des[s], eps, rb)
            r, v = out["r"], out["v"]
            assert out["inside"] and np.linalg.norm(r) > 0
            assert v @ r <= -(1 - 1e-12) * np.linalg.norm(v) * np.linalg.norm(r)   # anti-parallel
            assert np.array_equal(out["u"], out["tau"] - v)
            norms.append(np.linalg.norm(v))
        assert norms[0] >= KP[0] * np.linalg.norm(r) * (1 - 1e-12) and norms[0] < norms[1] < norms[2], norms


# ------------------------------------------------------------------------------------------------ GPU: the controller
def _controller_states(seed, B, n):
    """test_controller._wide_states (errors 1e-5 .. 1e-1, whole-turn shifts, the last 4 about 150 rad away) with rows 1-4 moved to
    q_des - q = +-pi -+ 1e-9 / +-pi +- 1e-9 (both sides of the wrap's edge) and row 5 on the reference exactly."""
    import test_controller as tc
    q, qd, q_des, qd_des, qdd_des = tc._wide_states(seed, B, n, far=4 if B > 8 else 0)
    if B > 8:
        for row, (sign, off) in zip((1, 2, 3, 4), ((1, -1e-9), (1, 1e-9), (-1, 1e-9), (-1, -1e-9))):
            q_des[row] = q[row] + sign * np.pi + off
        q_des[5], qd_des[5] = q[5], qd[5]
    return q, qd, q_des, qd_des, qdd_des


def _assert_controller_matches(got, refs, what):
    import test_controller as tc
    u, tau, v = got
    for s, ref in enumerate(refs):
        assert ref["inside"], (what, s)
        for mine, key in ((u[s], "u"), (tau[s], "tau"), (v[s], "v")):
            assert tc._close(mine, ref[key]), (what, s, key, np.abs(mine - ref[key]).max(), np.abs(ref[key]).max())


def _controller_parity(rb_dev, rb_ref, eps, seed, B=65):
    from armour_amd.controller import kinova_controller, kinova_controller_althoff
    from oracle.cpu_oracle import robust_controller
    n = rb_ref.num_factors
    rng = np.random.default_rng(seed)
    Kr = rng.uniform(5, 20, n)
    arrs = _controller_states(seed + 1, B, n)
    rows = lambda s: [a[s] for a in arrs]
    what = (n, eps)
    # e_acc = NULL, and explicit zeros: the same bits
    got = kinova_controller_althoff(Kr, KP, (4.0, 4.0), 1e-5, *arrs, eps=eps, robot=rb_dev)
    zeros = kinova_controller_althoff(Kr, KP, (4.0, 4.0), 1e-5, *arrs, eps=eps, robot=rb_dev, e_acc=np.zeros(B))
    assert all(_same_bits(a, b) for a, b in zip(got, zeros))
    refs = [althoff_restatement(robust_controller, Kr, KP, (4.0, 4.0), *rows(s), eps, rb_ref) for s in range(B)]
    _assert_controller_matches(got, refs, what)
    u, tau, v = got
    assert not v[5].any() and _same_bits(u[5], tau[5])   # on the reference: r = 0, v = 0 exactly, u = tau to the bit
    assert all(v[s].any() for s in range(B) if s != 5)
    # the wrap's two regimes were met: errors next to +-pi on both sides, and ~150 rad away
    diff = arrs[2] - arrs[0]
    assert np.abs(np.abs(diff[1:5]) - np.pi).max() < 2e-9 and np.abs(diff[-4:]).min() > 140
    # tau is the ARMOUR method's nominal pass
    tau_robust = kinova_controller(Kr, 1.0, 1e-2, 1e-10, *arrs, eps=eps, robot=rb_dev)[1]
    assert _same_bits(tau, tau_robust)
    # a non-zero accumulated error acts through Ki
    e_acc = rng.uniform(0.01, 0.1, B)
    got_e = kinova_controller_althoff(Kr, KP, (4.0, 4.0), 1e-5, *arrs, eps=eps, robot=rb_dev, e_acc=e_acc)
    refs_e = [althoff_restatement(robust_controller, Kr, KP, (4.0, 4.0), *rows(s), eps, rb_ref, e_acc=e_acc[s]) for s in range(B)]
    _assert_controller_matches(got_e, refs_e, what + ("e_acc",))
    assert _same_bits(got_e[1], tau) and np.abs(got_e[2] - v).max() > 1e-3
    # B = 1 in the single-state call shape: the MEX's
    one = kinova_controller_althoff(Kr, KP, (4.0, 4.0), 1e-5, *rows(0), eps=eps, robot=rb_dev)
    assert all(o.shape == (n,) and _same_bits(o, g[0]) for o, g in zip(one, got))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("eps", [0.0, 0.03, 0.3])
def test_device_controller_equals_the_restatement(eps):
    import test_controller as tc
    _controller_parity(tc._device_robot("kinova"), tc._oracle_robot("kinova"), eps, 800 + int(100 * eps))


@pytest.mark.gpu
def test_device_controller_equals_the_restatement_on_the_fetch():
    """Mixed joint axes."""
    import test_controller as tc
    _controller_parity(tc._device_robot("fetch"), tc._oracle_robot("fetch"), 0.03, 850)


# ------------------------------------------------------------------------------------------------ GPU: tracking
@functools.lru_cache(maxsize=None)
def _runs():
    """Six rollouts of 60 steps at 1e-3 under the Althoff restatement: uncertain plants, starts off the reference, every node kept."""
    from armour_amd.tracking import plant_samples
    rb = _robot()
    rng = np.random.default_rng(71)
    B, D = 6, 1.0
    q0, qd0, qdd0, k = _plans(rng, B)
    sm, sI = plant_samples(rb, B, rb.mass_uncertainty, rng)
    z0 = _start_inside(rb, rng, q0, qd0, qdd0, k, K_RANGE, D, sm, sI)
    kw = dict(t1=0.06, dt=1e-3, record_every=7)
    host = [host_track_althoff(rb, q0[b], qd0[b], qdd0[b], k[b], K_RANGE, D, sm=sm[b], sI=sI[b], z0=z0[b], **kw) for b in range(B)]
    assert all(h["status"] == 0 and h["steps"] == 60 and h["limit_flags"] == 0 and h["max_robust_input"] > 1e-3 for h in host)
    return dict(args=(q0, qd0, qdd0, k, K_RANGE, D), kw=dict(kw, controller="althoff", z0=z0, mass_scale=sm, inertia_scale=sI), host=host)


@pytest.mark.gpu
def test_device_tracking_equals_the_restatement():
    setup = _runs()
    dev = _simulate(_robot(), *setup["args"], **setup["kw"])
    assert np.all(dev.steps == 60) and dev.trace.shape == (6, 9, 3, N_J)
    worst = _compare(dev, setup["host"])
    print(f"tracking, althoff: worst {worst:.2e}")
    # the mode is its own: the robust controller on the same rollouts gives another input
    robust = _simulate(_robot(), *setup["args"], **{**setup["kw"], "controller": "robust"})
    assert not np.array_equal(robust.max_robust_input, dev.max_robust_input)
    # althoff_Kp reaches the kernel: the default is the reference's pair, another pair moves the result
    same = _simulate(_robot(), *setup["args"], althoff_Kp=KP, **setup["kw"])
    _bit_equal(same, dev, slice(None), slice(None))
    other = _simulate(_robot(), *setup["args"], althoff_Kp=(10.0, 28.1037), **setup["kw"])
    assert not np.array_equal(other.q, dev.q)


def _torque_limit():
    """A torque limit half-way between two nodes' |u| of rollout 0's restatement: (robot, runs monitored again under it)."""
    import test_tracking_edges as te
    host = _runs()["host"]
    u = np.array([nd[3] for nd in host[0]["nodes"]])
    for cand in te._crossings(u, (22, 38), range(N_J)):
        rb = te._limited_robot(torque=cand)
        runs = [with_limits(h, rb) for h in host]
        if min(r["margins"]["torque"] for r in runs) >= MARGIN and runs[0]["limit_flags"] == _lib.TRACK_LIMIT_TORQUE:
            return rb, runs, cand
    raise AssertionError("no joint of rollout 0 crosses a limit with every node 1e-6 away")


@pytest.mark.gpu
def test_device_torque_limit_under_the_althoff_mode():
    setup = _runs()
    rb, runs, (joint, node, limit) = _torque_limit()
    assert min(min(r["margins"].values()) for r in runs) >= MARGIN
    assert runs[0]["first_violation_t"] == runs[0]["nodes"][node][0] and 0 < node < 60
    dev = _simulate(rb, *setup["args"], **setup["kw"])
    worst = _compare(dev, runs)   # (flags and first_violation_t exactly)
    assert dev.limit_flags[0] == _lib.TRACK_LIMIT_TORQUE and _same_bits(dev.first_violation_t[0], runs[0]["first_violation_t"])
    print(f"torque limit {limit:.6g} on joint {joint} at node {node}: flags {list(dev.limit_flags)}, worst {worst:.2e}")


def _edge_setup(B, seed, steps):
    from armour_amd.tracking import plant_samples
    rb = _robot()
    rng = np.random.default_rng(seed)
    q0, qd0, qdd0, k = _plans(rng, B)
    sm, sI = plant_samples(rb, B, rb.mass_uncertainty, rng)
    z0 = np.concatenate([q0 + rng.uniform(-5e-3, 5e-3, (B, N_J)), qd0 + rng.uniform(-5e-3, 5e-3, (B, N_J))], axis=1)
    kw = dict(t1=steps * 1e-3, dt=1e-3, controller="althoff", record_every=1)
    return lambda s, **more: _simulate(rb, q0[s], qd0[s], qdd0[s], k[s], K_RANGE, 1.0, z0=z0[s], mass_scale=sm[s], inertia_scale=sI[s], **{**kw, **more})


@pytest.mark.gpu
def test_a_rollout_is_independent_of_its_batch_and_of_the_chunking():
    N = 8
    sim = _edge_setup(130, 81, N)
    full = sim(slice(0, 130))
    assert np.all(full.steps == N) and np.all(full.status == 0)
    _bit_equal(full, sim(slice(37, 38)), 37, 0)
    runs = [sim(slice(0, 3), steps_per_launch=S) for S in (1, 7, N + 1)]
    for r in runs:
        _bit_equal(r, full, slice(None), slice(0, 3))


@pytest.mark.gpu
def test_block_edges_under_the_althoff_mode():
    sim = _edge_setup(65, 82, 5)
    alone = {lane: sim(slice(lane, lane + 1)) for lane in (0, 62, 63, 64)}
    for B in (63, 64, 65):
        full = sim(slice(0, B))
        assert np.all(full.steps == 5) and np.all(full.status == 0)
        for lane in (lane for lane in alone if lane < B):
            _bit_equal(full, alone[lane], lane, 0)


# ------------------------------------------------------------------------------------------------ GPU: the 8-factor ABI
def _k128_states(n):
    return np.random.default_rng(900 + n).uniform(5, 20, n), _controller_states(910 + n, 65, n)


def _body_k128_gpu(kinova_default_abi):
    """(runs with ARMOUR_KEY128=1)  controller parity on fetch8, 8 of 8 slots; the Kinova's outputs against the 7-factor library's bits"""
    from armour_amd import planner
    from armour_amd.controller import kinova_controller_althoff
    from oracle.cpu_oracle import robust_controller
    assert _lib.MAXF == 8 and _lib.load().armour_abi_max_factors() == 8
    rb = planner.fetch8_robot()
    assert rb.num_factors == 8
    Kr, arrs = _k128_states(8)
    got = kinova_controller_althoff(Kr, KP, (4.0, 4.0), 1e-5, *arrs, eps=0.03, robot=rb)
    refs = [althoff_restatement(robust_controller, Kr, KP, (4.0, 4.0), *[a[s] for a in arrs], 0.03, rb) for s in range(65)]
    _assert_controller_matches(got, refs, ("k128", "fetch8"))
    assert not got[2][5].any() and _same_bits(got[0][5], got[1][5])
    print("controller, fetch8 (8 of 8): 65 states at 1e-12", flush=True)
    Kr, arrs = _k128_states(7)
    got = kinova_controller_althoff(Kr, KP, (4.0, 4.0), 1e-5, *arrs, eps=0.03, robot=planner.kinova_robot())
    ref = np.load(kinova_default_abi)
    assert all(_same_bits(g, ref[name]) for g, name in zip(got, ("u", "tau", "v")))
    print("kinova bits equal across ABIs", flush=True)
    print("althoff k128 gpu ok", flush=True)


@pytest.mark.gpu
def test_eight_factor_abi_on_the_device(tmp_path):
    from armour_amd.controller import kinova_controller_althoff
    Kr, arrs = _k128_states(7)
    u, tau, v = kinova_controller_althoff(Kr, KP, (4.0, 4.0), 1e-5, *arrs, eps=0.03, robot=_robot())
    path = str(tmp_path / "kinova_default_abi.npz")
    np.savez(path, u=u, tau=tau, v=v)
    env = dict(os.environ, ARMOUR_KEY128="1")
    env.pop("ARMOUR_HIP_LIB", None)
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_althoff as t; t._body_k128_gpu(%r)" % (ROOT, os.path.join(ROOT, "tests"), path)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "althoff k128 gpu ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout)


# ------------------------------------------------------------------------------------------------ GPU: the study
@pytest.mark.gpu
def test_two_controller_study():
    from armour_amd.tracking import compare_robust_controller
    from oracle.cpu_oracle import robust_controller
    rb = _robot()
    kw = dict(levels=(0.0, 0.1), samples=4, seed=3, T=0.25)
    out = compare_robust_controller(controllers=("robust", "althoff"), **kw)
    assert out["controllers"] == ("robust", "althoff")
    assert out["per_joint_max_v"].shape == (2, 2, 4, N_J) and out["per_joint_median_max_v"].shape == (2, 2, N_J)
    assert np.all(np.isfinite(out["per_joint_max_v"])) and np.all(np.isfinite(out["per_joint_median_max_v"]))
    assert np.array_equal(out["per_joint_median_max_v"], np.median(out["per_joint_max_v"], axis=2))
    assert out["max_v"].shape == (2, 2, 4) and out["status"].shape == (2, 2, 4) and np.all(out["status"] == 0)
    # both controllers ran on the same z0 and reference; each trace is every 10th node of 250
    for li, level in enumerate(kw["levels"]):
        plan, runs = out["plans"][li], out["result"][li]
        assert all(r.trace.shape == (4, 26, 3, N_J) and np.all(r.steps == 250) for r in runs)
        assert np.array_equal(runs[0].trace[:, 0, :2], runs[1].trace[:, 0, :2]) and np.array_equal(runs[0].trace[:, 0, 0], plan["z0"][:, :N_J])
        # one sample per controller: the per-joint maxima from the returned trace with the oracle restatements
        for ci, sample in ((0, 1), (1, 2)):
            vs = []
            for j in range(26):
                qr, qdr, qddr = _reference(plan["q0"][sample], plan["qd0"][sample], plan["qdd0"][sample], plan["k"][sample], plan["k_range"], 0.25, 0.25 if j == 25 else (10 * j) * (0.25 / 250))
                q, qd = runs[ci].trace[sample, j, 0], runs[ci].trace[sample, j, 1]
                if ci == 0:
                    vs.append(robust_controller(rb.K, rb.alpha, rb.V_m, 0.0, q, qd, qr, qdr, qddr, eps=level, robot=rb)["v"])
                else:
                    vs.append(althoff_restatement(robust_controller, rb.K, KP, (0.0, 0.0), q, qd, qr, qdr, qddr, level, rb)["v"])
            ref = np.abs(np.array(vs)).max(axis=0)
            got = out["per_joint_max_v"][li, ci, sample]
            assert np.all(np.abs(got - ref) <= 1e-9 * np.maximum(1.0, ref)), (level, ci, got, ref)
    # the robust half is the default call's run, bit for bit
    default = compare_robust_controller(**kw)
    assert set(default) == {"levels", "median_max_v", "max_v", "status", "result"}
    assert _same_bits(default["max_v"], out["max_v"][:, 0]) and _same_bits(default["median_max_v"], out["median_max_v"][:, 0])
    for li in range(2):
        for name in ("q", "qd", "max_V", "max_pos_error", "max_vel_error", "max_torque_ratio"):
            assert _same_bits(getattr(default["result"][li], name), getattr(out["result"][li][0], name)), name
