"""The tracking controller: kinova_controller(Kr, alpha, V_max, r_thr, q, qd, q_des, qd_des, qdd_des, eps).

The reference records no outputs of its controller (parity unpinned), so the CPU restatement (oracle/controller_oracle.cpp)
is pinned by invariants -- an independent formulation of the same dynamics, interval enclosure, the control-barrier
logic -- and the device implementation is then compared with it.

Robots: the oracle is held against the independent formulation on the Kinova, the gripper preset, the Fetch (mixed signed axes) and a
damped Kinova, and the device against the oracle on the same four.  The controller models the ACTUATED chain (num_factors joints): the
fixed bodies behind it (the gripper preset's 1.72 kg eighth body, the Fetch's last two) are not in its model, on either side.
Not covered: the stop path "nominal torque outside the interval torque" (ARMOUR_ESTATE) -- no input found that reaches it, so no test
here runs it; and nothing larger than 64 pi goes through the angle wrap ON THE DEVICE (termination beyond is shown on the host build of
the same header, test_angle_wrap_*)."""
import ctypes as C
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT
from test_oracle_invariants import robot_arrays, rot_rpy, scalar_rnea

KR, ALPHA, V_MAX, R_THR = 10.0, 1.0, 1e-2, 1e-10   # gains of kinova_src/kinova_simulator_interfaces/uarmtd_robust_CBF_MEX_LLC.m defaults


def _states(seed, count):
    rng = np.random.default_rng(seed)
    q = rng.uniform(-np.pi, np.pi, (count, 7))
    qd = rng.uniform(-1, 1, (count, 7))
    q_des = q + rng.uniform(-0.02, 0.02, (count, 7))
    qd_des = qd + rng.uniform(-0.05, 0.05, (count, 7))
    qdd_des = rng.uniform(-2, 2, (count, 7))
    return q, qd, q_des, qd_des, qdd_des


def test_spatial_passivity_rnea_equals_the_planners_vector_formulation():
    """The controller's Featherstone-style passRNEA (CoM frames, twists) and the planner's 3-vector passivity RNEA
    (RT/Dynamics.cu:83-181, written out in numpy in test_oracle_invariants.scalar_rnea) are two formulations of
    M(q) qdd_a + C(q, qd) qd_a + g(q): their torques must agree for arbitrary (q, qd, qd_a, qdd_a)."""
    from oracle.cpu_oracle import pass_rnea_scaled
    rb = robot_arrays()
    rng = np.random.default_rng(1)
    for _ in range(20):
        q, qd, qda, qdda = rng.uniform(-np.pi, np.pi, 7), rng.uniform(-2, 2, 7), rng.uniform(-2, 2, 7), rng.uniform(-3, 3, 7)
        tau = pass_rnea_scaled(np.zeros(7), np.zeros(7), q, qd, qda, qdda)
        assert np.abs(tau - scalar_rnea(rb, q, qd, qda, qdda)).max() <= 1e-10


def test_interval_rnea_encloses_every_model_in_the_uncertainty_set():
    from oracle.cpu_oracle import pass_rnea_scaled, robust_controller
    eps = 0.03
    q, qd, q_des, qd_des, qdd_des = _states(2, 6)
    rng = np.random.default_rng(3)
    for s in range(6):
        out = robust_controller(KR, ALPHA, V_MAX, R_THR, q[s], qd[s], q_des[s], qd_des[s], qdd_des[s], eps=eps)
        lo, hi = out["tau_interval"][:, 0], out["tau_interval"][:, 1]
        assert out["inside"] and np.all(lo <= out["tau"]) and np.all(out["tau"] <= hi) and np.all(hi - lo > 0)
        # the reference inputs of the RNEA calls (robust_controller.cpp:70-80)
        e = (q_des[s] - q[s] + np.pi) % (2 * np.pi) - np.pi
        qa_d, qa_dd = qd_des[s] + KR * e, qdd_des[s] + KR * (qd_des[s] - qd[s])
        for _ in range(25):
            corner = rng.random() < 0.5
            s_m = eps * (rng.choice([-1.0, 1.0], 7) if corner else rng.uniform(-1, 1, 7))
            s_I = eps * (rng.choice([-1.0, 1.0], 7) if corner else rng.uniform(-1, 1, 7))
            tau = pass_rnea_scaled(s_m, s_I, q[s], qd[s], qa_d, qa_dd)
            assert np.all(tau >= lo - 1e-12) and np.all(tau <= hi + 1e-12)


def test_robust_input_logic():
    """v = 0 when the tracking error r vanishes; otherwise v is anti-parallel to r with the gain of robust_controller.cpp:150-163,
    u = tau - v, and a larger uncertainty never shrinks the gain."""
    from oracle.cpu_oracle import robust_controller
    q, qd, q_des, qd_des, qdd_des = _states(4, 4)
    out0 = robust_controller(KR, ALPHA, V_MAX, R_THR, q[0], qd[0], q[0], qd[0], qdd_des[0])
    assert not out0["v"].any() and np.array_equal(out0["u"], out0["tau"])
    for s in range(4):
        e = (q_des[s] - q[s] + np.pi) % (2 * np.pi) - np.pi
        r = (qd_des[s] - qd[s]) + KR * e
        small = robust_controller(KR, ALPHA, V_MAX, R_THR, q[s], qd[s], q_des[s], qd_des[s], qdd_des[s], eps=0.01)
        big = robust_controller(KR, ALPHA, V_MAX, R_THR, q[s], qd[s], q_des[s], qd_des[s], qdd_des[s], eps=0.10)
        for out in (small, big):
            assert np.abs(out["u"] - (out["tau"] - out["v"])).max() == 0.0
            lam = np.linalg.norm(out["v"])
            assert np.abs(out["v"] + lam * r / np.linalg.norm(r)).max() <= 1e-12 * max(1.0, lam)
        assert np.linalg.norm(big["v"]) >= np.linalg.norm(small["v"]) - 1e-12


@pytest.mark.gpu
def test_device_controller_matches_the_cpu_restatement():
    """One device thread per state against the CPU restatement: same operation order, same outward rounding -> agreement
    to the last bits (1e-12 relative asserted); single-state call = the MEX shape."""
    from armour_amd.controller import kinova_controller
    from oracle.cpu_oracle import robust_controller
    B = 200
    q, qd, q_des, qd_des, qdd_des = _states(7, B)
    q_des[5], qd_des[5] = q[5], qd[5]                         # r = 0: no robust input
    u, tau, v = kinova_controller(KR, ALPHA, V_MAX, R_THR, q, qd, q_des, qd_des, qdd_des, eps=0.03)
    for s in list(range(0, B, 17)) + [5]:
        ref = robust_controller(KR, ALPHA, V_MAX, R_THR, q[s], qd[s], q_des[s], qd_des[s], qdd_des[s], eps=0.03)
        for got, key in ((u[s], "u"), (tau[s], "tau"), (v[s], "v")):
            assert np.abs(got - ref[key]).max() <= 1e-12 * max(1.0, np.abs(ref[key]).max())
    assert not v[5].any()
    u1, tau1, v1 = kinova_controller(KR, ALPHA, V_MAX, R_THR, q[3], qd[3], q_des[3], qd_des[3], qdd_des[3])
    assert np.array_equal(u1, u[3]) and np.array_equal(tau1, tau[3]) and np.array_equal(v1, v[3])


@pytest.mark.gpu
def test_latency_and_throughput_kernels_agree_bit_for_bit():
    """Few states run the three RNEA passes of an update on three waves (controller.hip, the latency kernel), many run one lane per state:
    the same states give the same bits either way, with and without a robust input."""
    from armour_amd.controller import kinova_controller
    B = 64 * 256 + 1000                                       # past the latency kernel's limit
    q, qd, q_des, qd_des, qdd_des = _states(11, B)
    q_des[70], qd_des[70] = q[70], qd[70]                     # r = 0: the third pass is skipped
    bulk = kinova_controller(KR, ALPHA, V_MAX, R_THR, q, qd, q_des, qd_des, qdd_des, eps=0.03)
    for lo, hi in ((0, 1), (64, 130), (16000, 16200)):
        few = kinova_controller(KR, ALPHA, V_MAX, R_THR, q[lo:hi], qd[lo:hi], q_des[lo:hi], qd_des[lo:hi], qdd_des[lo:hi], eps=0.03)
        for a, b in zip(few, bulk):
            assert np.array_equal(np.asarray(a).reshape(hi - lo, 7), b[lo:hi])
    assert not bulk[2][70].any()


@pytest.mark.gpu
def test_controller_kernel_choice_is_an_api_call_and_changes_no_bit():
    """armour_controller_set_kernel (round 4: it was the environment variable ARMOUR_CTL_SPLIT): the same 300 states through the one-lane-per-state
    kernel (0), the four-wave latency kernel (1) and the automatic choice (-1) -- identical outputs; values outside -1..1 are refused."""
    from armour_amd import _lib
    from armour_amd.controller import kinova_controller
    L = _lib.load()
    q, qd, q_des, qd_des, qdd_des = _states(23, 300)
    got = []
    try:
        for which in (0, 1, -1):
            _lib.check(L.armour_controller_set_kernel(which))
            got.append(kinova_controller(KR, ALPHA, V_MAX, R_THR, q, qd, q_des, qd_des, qdd_des, eps=0.03))
        assert L.armour_controller_set_kernel(2) < 0
    finally:
        L.armour_controller_set_kernel(-1)
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# The angle wrap (controller_core.h clamp_angle, the oracle's wrap): bounded for every double
# ---------------------------------------------------------------------------------------------------------------------------------
WRAP_LOOP_MAX = 64 * math.pi   # up to here the wrap is the reference's loop (robust_controller.hpp:11-16), at most 32 steps


def _loop_wrap(x):
    """The reference's loop as it stands -- only ever called with |x| <= 64 pi here."""
    assert abs(x) <= WRAP_LOOP_MAX
    while x >= math.pi:
        x -= 2 * math.pi
    while x < -math.pi:
        x += 2 * math.pi
    return x


def _wrap_inputs():
    pi = math.pi
    edges = [pi, -pi, math.nextafter(pi, 4), math.nextafter(pi, 0), math.nextafter(-pi, -4), math.nextafter(-pi, 0), 3 * pi, -3 * pi, 0.0, -0.0,
             WRAP_LOOP_MAX, -WRAP_LOOP_MAX, math.nextafter(WRAP_LOOP_MAX, 0), math.nextafter(-WRAP_LOOP_MAX, 0)]
    small = np.concatenate([edges, np.random.default_rng(31).uniform(-WRAP_LOOP_MAX, WRAP_LOOP_MAX, 2000)])
    decades = [10.0 ** e for e in range(3, 301)]
    large = np.array([math.nextafter(WRAP_LOOP_MAX, 1e3), 250.0, 1e3 * pi] + decades + [-d for d in decades] + [sys.float_info.max, -sys.float_info.max])
    special = np.array([math.inf, -math.inf, math.nan])
    return small, large, special


def _check_wrap(small, large, special, got_small, got_large, got_special):
    """The three properties asked of the wrap; returns the worst error above 64 pi in ulp of |x|."""
    mpmath = pytest.importorskip("mpmath")
    want = np.array([_loop_wrap(float(x)) for x in small])
    assert np.array_equal(got_small.view(np.uint64), want.view(np.uint64)), "below 64 pi the wrap must be the loop, bit for bit"
    assert np.all(got_large >= -math.pi) and np.all(got_large < math.pi)
    mpmath.mp.dps = 50   # (1e300 has 301 digits before the point: the quotient below is exact integer arithmetic on mpf values of enough precision)
    worst = 0.0
    with mpmath.workprec(1200):
        two_pi = 2 * mpmath.pi
        for x, g in zip(large, got_large):
            d = (mpmath.mpf(float(x)) - mpmath.mpf(float(g))) / two_pi
            d = abs(d - mpmath.nint(d)) * two_pi                      # distance on the circle between x and the result
            worst = max(worst, float(d / mpmath.mpf(math.ulp(abs(float(x))))))
    assert np.all(np.isnan(got_special))
    return worst


# Bound above 64 pi, derived: the reduction is fmod(x, fl(2 pi)), which is exact, so the only error against x mod 2 pi is
# k * |fl(2 pi) - 2 pi| with k <= |x| / (2 pi): |x| * 3.9e-17 <= 0.36 ulp(|x|) (ulp(|x|) >= |x| * 2^-53), plus one rounding of the final
# +- 2 pi step (<= 4.5e-16, under 0.01 ulp of any |x| > 64 pi).  Asserted: 0.5 ulp(|x|).  Measured worst case: 0.345 ulp (product header
# and oracle alike).
WRAP_ULP_BOUND = 0.5


def test_angle_wrap_of_the_product_header_terminates_and_keeps_its_bits(tmp_path):
    """ctl::clamp_angle of armour_amd/csrc/controller_core.h itself, compiled for the host and run in a child process under a timeout (the loop
    form never returns for |x| >~ 1e16 or inf, and takes ~1.6e9 steps at 1e10): bit-identical to the loop up to 64 pi, x mod 2 pi in
    [-pi, pi) to WRAP_ULP_BOUND beyond, NaN for inf and NaN."""
    exe = tmp_path / "clamp_angle_probe"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
           os.path.join(ROOT, "tests", "stubs", "clamp_angle_probe.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    small, large, special = _wrap_inputs()
    x = np.concatenate([small, large, special])
    r = subprocess.run([str(exe)], input=x.tobytes(), capture_output=True, timeout=5)   # (the timeout is the point: do not remove it)
    assert r.returncode == 0
    got = np.frombuffer(r.stdout, dtype=np.float64)
    assert got.size == x.size
    worst = _check_wrap(small, large, special, got[:small.size], got[small.size:small.size + large.size], got[small.size + large.size:])
    print(f"clamp_angle above 64 pi: worst error {worst:.3f} ulp(|x|)")
    assert worst <= WRAP_ULP_BOUND


_ORACLE_WRAP_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from oracle.cpu_oracle import robust_controller
x = np.load(sys.argv[2])
out = np.zeros((x.size, 7))
z = np.zeros(7)
for i, xi in enumerate(x):
    q_des = z.copy()
    q_des[int(sys.argv[4])] = xi
    out[i] = robust_controller(10.0, 1.0, 1e-2, 1e-10, z, z, q_des, z, z, eps=0.03)["u"]
np.save(sys.argv[3], out)
"""


def test_angle_wrap_of_the_oracle_terminates_and_agrees(tmp_path):
    """The oracle's wrap has no entry of its own: robust_controller with q = 0 and q_des = x on one joint has q_des - q = x exactly, and its
    output must be the output for q_des = wrap(x) bit for bit, wrap(x) being this module's statement of the rule (loop up to 64 pi, fmod
    first beyond; the product header is held to the same properties above).  In a child process under a timeout, as above."""
    small, large, special = _wrap_inputs()
    small, large = np.concatenate([small[:14], small[14::10]]), np.concatenate([large[:3], large[3::7], large[-2:]])
    x = np.concatenate([small, large, special])
    joint = 1
    np.save(tmp_path / "x.npy", x)
    r = subprocess.run([sys.executable, "-c", _ORACLE_WRAP_CHILD, ROOT, str(tmp_path / "x.npy"), str(tmp_path / "u.npy"), str(joint)],
                       capture_output=True, text=True, timeout=60)   # (the timeout is the point: do not remove it)
    assert r.returncode == 0, r.stderr
    got = np.load(tmp_path / "u.npy")
    from oracle.cpu_oracle import robust_controller
    z = np.zeros(7)

    def rule(v):
        if not abs(v) <= WRAP_LOOP_MAX:
            v = math.fmod(v, 2 * math.pi)
        return _loop_wrap(v)

    wrapped = np.array([rule(float(v)) for v in x[:small.size + large.size]])
    worst = _check_wrap(small, large, special, wrapped[:small.size], wrapped[small.size:], np.full(3, np.nan))   # the rule itself has the properties
    assert worst <= WRAP_ULP_BOUND
    for i, w in enumerate(wrapped):
        q_des = z.copy()
        q_des[joint] = w
        ref = robust_controller(10.0, 1.0, 1e-2, 1e-10, z, z, q_des, z, z, eps=0.03)["u"]
        assert np.array_equal(got[i], ref), (x[i], w)
    assert np.all(np.isnan(got[small.size + large.size:, joint]))


def test_controller_entry_refuses_non_finite_arguments_before_the_device():
    """armour_robust_controller: a non-finite state, gain or constant, or a negative / non-finite model uncertainty, is ARMOUR_EINVAL -- and
    that before the first HIP call, so without a device too; a good call without a device is the device error."""
    from armour_amd import _lib
    from armour_amd.planner import kinova_robot
    L = _lib.load()
    rb = kinova_robot()
    n, B = rb.num_factors, 3
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    q, qd, q_des, qd_des, qdd_des = _states(41, B)
    out = [np.zeros((B, n)) for _ in range(3)]

    def call(eps=0.03, alpha=ALPHA, V_max=V_MAX, thr=R_THR, Kr=None, **arrays):
        kr = np.full(n, KR) if Kr is None else Kr
        a = [np.ascontiguousarray(arrays.get(name, val)) for name, val in (("q", q), ("qd", qd), ("q_des", q_des), ("qd_des", qd_des), ("qdd_des", qdd_des))]
        return L.armour_robust_controller(C.byref(rb), eps, dp(kr), alpha, V_max, thr, B, *[dp(x) for x in a], *[dp(o) for o in out])

    for bad in (math.nan, math.inf, -math.inf):
        for name, val in (("q", q), ("qd", qd), ("q_des", q_des), ("qd_des", qd_des), ("qdd_des", qdd_des)):
            for where in ((0, 0), (B - 1, n - 1)):
                arr = val.copy()
                arr[where] = bad
                assert call(**{name: arr}) == _lib.EINVAL, (name, where, bad)
        kr = np.full(n, KR)
        kr[n - 1] = bad
        assert call(Kr=kr) == _lib.EINVAL, ("Kr", bad)
        for name in ("eps", "alpha", "V_max", "thr"):
            assert call(**{name: bad}) == _lib.EINVAL, (name, bad)
    assert call(eps=-0.01) == _lib.EINVAL
    assert call() == (_lib.OK if L.armour_device_available() else _lib.EDEVICE)


# ---------------------------------------------------------------------------------------------------------------------------------
# More than one robot: mixed signed axes, damping, another armature
# ---------------------------------------------------------------------------------------------------------------------------------
ROBOTS = ("kinova", "gripper", "fetch", "damped")


def _make_robot(name, source):
    """`source`: oracle.cpu_oracle (the oracle's own tables) or armour_amd.planner (the product's) -- the same constants twice
    (tests/test_robot_constants.py).  "damped": a Kinova with damping drawn from [0.1, 2] and half the armature."""
    rb = {"kinova": source.kinova_robot, "gripper": source.kinova_gripper_robot, "fetch": source.fetch_robot, "damped": source.kinova_robot}[name]()
    if name == "damped":
        damping = np.random.default_rng(99).uniform(0.1, 2.0, rb.num_factors)
        for i in range(rb.num_factors):
            rb.damping[i] = damping[i]
            rb.armature[i] = 0.5 * rb.armature[i]
    return rb


def _oracle_robot(name):
    from oracle import cpu_oracle
    return _make_robot(name, cpu_oracle)


def _device_robot(name):
    from armour_amd import planner
    return _make_robot(name, planner)


def _axis_rotation(a, angle):
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def vector_rnea(rb, q, qd, qda, qdda):
    """test_oracle_invariants.scalar_rnea (the planner's 3-vector passivity RNEA, RT/Dynamics.cu:83-181) for joints about any signed
    coordinate axis (axes[i] in +-1..3) and with the joint damping damping[i] * qd[i], over the actuated chain of an ArmourRobot."""
    J = rb.num_factors
    trans = np.array(rb.trans)[:3 * (J + 1)].reshape(J + 1, 3)
    rots, com = np.array(rb.rots)[:3 * J].reshape(J, 3), np.array(rb.com)[:3 * J].reshape(J, 3)
    inertia, mass = np.array(rb.inertia)[:9 * J].reshape(J, 3, 3), np.array(rb.mass)[:J]
    axis = [np.sign(rb.axes[i]) * np.eye(3)[abs(rb.axes[i]) - 1] for i in range(J)]
    R = [rot_rpy(*rots[i]) @ _axis_rotation(axis[i], q[i]) for i in range(J)] + [np.eye(3)]
    w = np.zeros(3); wdot = np.zeros(3); waux = np.zeros(3); lacc = np.array([0, 0, rb.gravity])
    F, N = [], []
    for i in range(J):
        Rt = R[i].T
        lacc = Rt @ (lacc + np.cross(wdot, trans[i]) + np.cross(w, np.cross(waux, trans[i])))
        w = Rt @ w + qd[i] * axis[i]
        waux = Rt @ waux
        wdot = Rt @ wdot + np.cross(waux, qd[i] * axis[i]) + qdda[i] * axis[i]
        waux = waux + qda[i] * axis[i]
        F.append(mass[i] * (lacc + np.cross(wdot, com[i]) + np.cross(w, np.cross(waux, com[i]))))
        N.append(inertia[i] @ wdot + np.cross(waux, inertia[i] @ w))
    f = np.zeros(3); n = np.zeros(3); u = np.zeros(J)
    for i in range(J - 1, -1, -1):
        n = N[i] + R[i + 1] @ n + np.cross(com[i], F[i]) + np.cross(trans[i + 1], R[i + 1] @ f)
        f = R[i + 1] @ f + F[i]
        u[i] = n @ axis[i] + rb.armature[i] * qdda[i] + rb.damping[i] * qd[i]
    return u


@pytest.mark.parametrize("name", ROBOTS)
def test_spatial_passivity_rnea_equals_the_vector_formulation_on_every_robot(name):
    """The comparison of test_spatial_passivity_rnea_equals_the_planners_vector_formulation, same 1e-10, where the joints are not all about
    +z (the Fetch: 3, 2, 1, 2, 1, 2, 1) and where damping and armature differ from the Kinova's.  On the Kinova the generalised formulation
    is also held to the one it generalises."""
    from oracle.cpu_oracle import pass_rnea_scaled
    rb = _oracle_robot(name)
    n = rb.num_factors
    assert (name == "fetch") == (len({rb.axes[i] for i in range(n)}) > 1)
    rng = np.random.default_rng(5)
    for _ in range(20):
        q, qd, qda, qdda = rng.uniform(-np.pi, np.pi, n), rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(-3, 3, n)
        ref = vector_rnea(rb, q, qd, qda, qdda)
        tau = pass_rnea_scaled(np.zeros(n), np.zeros(n), q, qd, qda, qdda, robot=rb)
        assert np.abs(tau - ref).max() <= 1e-10
        if name == "kinova":
            assert np.abs(ref - scalar_rnea(robot_arrays(), q, qd, qda, qdda)).max() <= 1e-12
    if name == "damped":   # the damping term is there at all: it moves the torque by damping * qd exactly as stated
        plain = _oracle_robot("damped")
        for i in range(n):
            plain.damping[i] = 0.0
        diff = pass_rnea_scaled(np.zeros(n), np.zeros(n), q, qd, qda, qdda, robot=rb) - pass_rnea_scaled(np.zeros(n), np.zeros(n), q, qd, qda, qdda, robot=plain)
        assert np.abs(diff - np.array(rb.damping[:n]) * qd).max() <= 1e-12 and np.abs(diff).max() > 1e-3


def test_interval_rnea_encloses_every_model_in_the_uncertainty_set_on_the_fetch():
    """test_interval_rnea_encloses_every_model_in_the_uncertainty_set with mixed joint axes."""
    from oracle.cpu_oracle import pass_rnea_scaled, robust_controller
    rb = _oracle_robot("fetch")
    eps = 0.03
    q, qd, q_des, qd_des, qdd_des = _states(2, 6)
    rng = np.random.default_rng(3)
    for s in range(6):
        out = robust_controller(KR, ALPHA, V_MAX, R_THR, q[s], qd[s], q_des[s], qd_des[s], qdd_des[s], eps=eps, robot=rb)
        lo, hi = out["tau_interval"][:, 0], out["tau_interval"][:, 1]
        assert out["inside"] and np.all(lo <= out["tau"]) and np.all(out["tau"] <= hi) and np.all(hi - lo > 0)
        e = (q_des[s] - q[s] + np.pi) % (2 * np.pi) - np.pi
        qa_d, qa_dd = qd_des[s] + KR * e, qdd_des[s] + KR * (qd_des[s] - qd[s])
        for _ in range(25):
            corner = rng.random() < 0.5
            s_m = eps * (rng.choice([-1.0, 1.0], 7) if corner else rng.uniform(-1, 1, 7))
            s_I = eps * (rng.choice([-1.0, 1.0], 7) if corner else rng.uniform(-1, 1, 7))
            tau = pass_rnea_scaled(s_m, s_I, q[s], qd[s], qa_d, qa_dd, robot=rb)
            assert np.all(tau >= lo - 1e-12) and np.all(tau <= hi + 1e-12)


# ---------------------------------------------------------------------------------------------------------------------------------
# The device against the oracle off the Kinova defaults
# ---------------------------------------------------------------------------------------------------------------------------------
def _wide_states(seed, count, n=7, far=0):
    """Errors from 1e-5 to 1e-1 rad (one scale per state), every third state with q_des moved by whole turns, -2..2 of them per joint, so that
    the wrap wraps, differently per lane; the last `far` states with q_des - q of about +-150 rad (24 turns; below 64 pi = 201 by design)."""
    rng = np.random.default_rng(seed)
    q, qd = rng.uniform(-np.pi, np.pi, (count, n)), rng.uniform(-1, 1, (count, n))
    s = 10.0 ** rng.uniform(-5, -1, (count, 1))
    q_des = q + s * rng.uniform(-1, 1, (count, n))
    qd_des = qd + 2 * s * rng.uniform(-1, 1, (count, n))
    qdd_des = rng.uniform(-2, 2, (count, n))
    q_des[::3] += 2 * np.pi * rng.integers(-2, 3, (len(range(0, count, 3)), n))
    if far:
        q_des[count - far:] = q[count - far:] + rng.choice([-1.0, 1.0], (far, n)) * (150 + rng.uniform(-1, 1, (far, n)))
    assert np.abs(q_des - q).max() < WRAP_LOOP_MAX
    return q, qd, q_des, qd_des, qdd_des


def _close(got, ref):
    """The module's rule, derived and not measured: same operation order, outward rounding by one ulp on both sides, only sin / cos differ by
    an ulp between the device and libm."""
    return np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def _assert_matches_oracle(got, rows, ref_of, what):
    u, tau, v = got
    for s in rows:
        ref = ref_of(s)
        assert ref["inside"], (what, s)
        for mine, key in ((u[s], "u"), (tau[s], "tau"), (v[s], "v")):
            assert _close(mine, ref[key]), (what, s, key, np.abs(mine - ref[key]).max(), np.abs(ref[key]).max())


def _through_both_kernels(call):
    """call() through the one-lane-per-state kernel and through the four-wave kernel: the same bits; returns them."""
    from armour_amd import _lib
    L = _lib.load()
    got = []
    try:
        for which in (0, 1):
            _lib.check(L.armour_controller_set_kernel(which))
            got.append(call())
    finally:
        L.armour_controller_set_kernel(-1)
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    return got[0]


LAMBDA_MARGIN = 1e-9   # relative to the two terms lambda is the difference of: 10^6 ulp -- far more than the two sides' last-bit differences can move it


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROBOTS)
def test_device_matches_the_oracle_on_every_robot_gain_and_uncertainty(name):
    """robot x eps in {0, 0.03, 0.10} x V_max in {1e-2, the robot's V_m} x alpha in {1, 10}, a per-joint Kr from [5, 20], 300 states of
    _wide_states plus 4 about 150 rad away: u, tau, v of EVERY state against the oracle at 1e-12, both kernels bit for bit.  Which side of
    lambda = max(0, .) a state is on is decided by the oracle, with LAMBDA_MARGIN to spare: there v is exactly zero (u = tau to the bit),
    or not zero, on the device; at most 1 % of states may lie inside the margin, and each side holds at least 5 % of a robot's states (on the
    oracle every cell has 15 % .. 85 % on each side except the Fetch at V_max = 1e-7 with eps > 0, which is always above)."""
    import itertools
    from armour_amd.controller import kinova_controller
    from oracle.cpu_oracle import robust_controller
    rb_dev, rb_ref = _device_robot(name), _oracle_robot(name)
    n, B = rb_ref.num_factors, 304
    sides, skipped = [0, 0], 0
    cells = list(itertools.product((0.0, 0.03, 0.10), sorted({1e-2, rb_ref.V_m}), (1.0, 10.0)))
    for ci, (eps, V_max, alpha) in enumerate(cells):
        what = (name, eps, V_max, alpha)
        Kr = np.random.default_rng(500 + ci).uniform(5, 20, n)
        q, qd, q_des, qd_des, qdd_des = _wide_states(600 + 16 * ROBOTS.index(name) + ci, B, n, far=4)
        u, tau, v = _through_both_kernels(lambda: kinova_controller(Kr, alpha, V_max, R_THR, q, qd, q_des, qd_des, qdd_des, eps=eps, robot=rb_dev))
        refs = [robust_controller(Kr, alpha, V_max, R_THR, q[s], qd[s], q_des[s], qd_des[s], qdd_des[s], eps=eps, robot=rb_ref) for s in range(B)]
        _assert_matches_oracle((u, tau, v), range(B), lambda s: refs[s], what)
        for s, ref in enumerate(refs):
            assert ref["r_norm"] > R_THR
            if ref["lambda_raw"] < -LAMBDA_MARGIN * ref["lambda_scale"]:
                sides[0] += 1
                assert not v[s].any() and np.array_equal(u[s], tau[s]), (what, s)
            elif ref["lambda_raw"] > LAMBDA_MARGIN * ref["lambda_scale"]:
                sides[1] += 1
                assert v[s].any(), (what, s)
            else:
                skipped += 1
    total = B * len(cells)
    print(f"{name}: lambda = 0 for {sides[0]}, > 0 for {sides[1]}, within the margin {skipped} of {total} states")
    assert skipped <= 0.01 * total and min(sides) >= 0.05 * total


@pytest.mark.gpu
def test_threshold_on_the_robust_input_with_blocks_below_above_and_mixed():
    """r_norm_threshold = 1e-3 with states on both sides of it, laid out for the four-wave kernel's 16-state blocks: block 0 entirely below
    (its M r wave has nothing to do and wave 0 reads M r slots nobody wrote), block 1 entirely above, block 2 alternating, block 3 partial and
    mixed.  Below (by the oracle's |r|, 1e-9 relative clear of the threshold) v is exactly zero and u = tau; everything against the oracle."""
    from armour_amd.controller import kinova_controller
    from oracle.cpu_oracle import robust_controller
    thr, eps, alpha = 1e-3, 0.03, 1.0
    rb_dev, rb_ref = _device_robot("fetch"), _oracle_robot("fetch")
    n = rb_ref.num_factors
    Kr = np.random.default_rng(70).uniform(5, 20, n)
    pool = _wide_states(71, 400, n)
    ref_of = lambda arrs, s: robust_controller(Kr, alpha, V_MAX, thr, *[a[s] for a in arrs], eps=eps, robot=rb_ref)
    r_norm = np.array([ref_of(pool, s)["r_norm"] for s in range(400)])
    near = np.abs(r_norm - thr) <= 1e-9 * thr
    assert near.sum() <= 4                                    # at most 1 % of states are left out of the exact assertion (none, in fact)
    below, above = list(np.flatnonzero((r_norm < thr) & ~near)), list(np.flatnonzero((r_norm > thr) & ~near))
    assert len(below) >= 27 and len(above) >= 27
    order = below[:16] + above[:16] + [x for pair in zip(below[16:24], above[16:24]) for x in pair] + [above[24], below[24], below[25], above[25], below[26]]
    arrs = [a[order] for a in pool]
    B = len(order)
    assert B == 53 and B % 16 != 0
    got = _through_both_kernels(lambda: kinova_controller(Kr, alpha, V_MAX, thr, *arrs, eps=eps, robot=rb_dev))
    _assert_matches_oracle(got, range(B), lambda s: ref_of(arrs, s), "threshold")
    u, tau, v = got
    is_below = r_norm[order] < thr
    assert is_below[:16].all() and not is_below[16:32].any() and is_below[32:48].sum() == 8
    for s in range(B):
        if is_below[s]:
            assert not v[s].any() and np.array_equal(u[s], tau[s]), s
    # above the threshold the input is not switched off: the oracle has a non-zero v in some of those states, and the device agrees with it above
    assert sum(ref_of(arrs, s)["v"].any() for s in range(B) if not is_below[s]) >= 4
    assert all(v[s].any() == ref_of(arrs, s)["v"].any() for s in range(B) if not is_below[s] and abs(ref_of(arrs, s)["lambda_raw"]) > LAMBDA_MARGIN * ref_of(arrs, s)["lambda_scale"])


@pytest.mark.gpu
def test_block_edges_of_both_kernels_are_prefixes_of_one_run():
    """B = 1, 15, 16, 17, 4096, 4097 on the automatic choice (the four-wave kernel up to 4096 states, then the one-lane kernel) and 1, 63, 64,
    65 with the one-lane kernel forced: each a prefix of one 4097-state array and equal to the same rows of the full run bit for bit; the
    first, the last and every 97th row against the oracle."""
    from armour_amd import _lib
    from armour_amd.controller import kinova_controller
    from oracle.cpu_oracle import robust_controller
    L = _lib.load()
    rb_dev, rb_ref = _device_robot("fetch"), _oracle_robot("fetch")
    n, B = rb_ref.num_factors, 4097
    eps, alpha = 0.10, 10.0
    Kr = np.random.default_rng(80).uniform(5, 20, n)
    arrs = _wide_states(81, B, n, far=4)
    run = lambda count: kinova_controller(Kr, alpha, V_MAX, R_THR, *[a[:count] for a in arrs], eps=eps, robot=rb_dev)
    full = run(B)
    rows = sorted(set(range(0, B, 97)) | {B - 1})
    _assert_matches_oracle(full, rows, lambda s: robust_controller(Kr, alpha, V_MAX, R_THR, *[a[s] for a in arrs], eps=eps, robot=rb_ref), "sizes")
    for count in (1, 15, 16, 17, 4096, 4097):
        for a, b in zip(run(count), full):
            assert np.array_equal(a, b[:count]), count
    try:
        _lib.check(L.armour_controller_set_kernel(0))
        for count in (1, 63, 64, 65):
            for a, b in zip(run(count), full):
                assert np.array_equal(a, b[:count]), count
    finally:
        L.armour_controller_set_kernel(-1)


@pytest.mark.gpu
def test_unstaged_copy_path_and_buffers_that_grew():
    """Calls of more than 2^20 input doubles copy each array from the caller's (pageable) memory and read the status word back on its own:
    the largest B that is still staged and the first that is not, on one array -- common rows bit-identical, 50 rows (the last among them)
    against the oracle -- and then B = 1 in the same thread, served by the buffers the big call grew."""
    from armour_amd.controller import kinova_controller
    from oracle.cpu_oracle import robust_controller
    rb_dev, rb_ref = _device_robot("kinova"), _oracle_robot("kinova")
    n = rb_ref.num_factors
    B_staged = (1 << 20) // (5 * n)                           # 5 * B * n <= 2^20 (controller.hip kStagedDoubles)
    B = B_staged + 1
    assert 5 * B_staged * n <= 1 << 20 < 5 * B * n
    eps, alpha = 0.03, 1.0
    Kr = np.random.default_rng(90).uniform(5, 20, n)
    arrs = _wide_states(91, B, n, far=4)
    run = lambda count: kinova_controller(Kr, alpha, V_MAX, R_THR, *[a[:count] for a in arrs], eps=eps, robot=rb_dev)
    staged, unstaged = run(B_staged), run(B)
    for a, b in zip(staged, unstaged):
        assert np.array_equal(a, b[:B_staged])
    rows = sorted(set(np.linspace(0, B - 1, 50).astype(int)))
    assert rows[-1] == B - 1
    _assert_matches_oracle(unstaged, rows, lambda s: robust_controller(Kr, alpha, V_MAX, R_THR, *[a[s] for a in arrs], eps=eps, robot=rb_ref), "unstaged")
    for a, b in zip(run(1), unstaged):
        assert np.array_equal(a, b[:1])


@pytest.mark.gpu
def test_cached_models_follow_every_change_of_robot_and_constants():
    """The entry keeps the prepared models per host thread and rebuilds them when the robot or a constant changes: a chain of calls on the same
    32 states that changes one thing at a time -- eps, the last entry of Kr alone, alpha, V_max, the threshold, the robot (Kinova -> Fetch ->
    Kinova) -- each against the oracle, back at the first setting the first result bit for bit, and again from a fresh thread (its own cache)."""
    from armour_amd.controller import kinova_controller
    from oracle.cpu_oracle import robust_controller
    n = 7
    arrs = _wide_states(95, 32, n)
    Kr0 = np.random.default_rng(96).uniform(5, 20, n)
    Kr1 = Kr0.copy()
    Kr1[n - 1] += 1.0
    first = dict(robot="kinova", eps=0.03, Kr=Kr0, alpha=1.0, V_max=1e-2, thr=1e-10)
    chain = [first]
    for change in (dict(eps=0.10), dict(Kr=Kr1), dict(alpha=10.0), dict(V_max=1e-7), dict(thr=1e-3), dict(robot="fetch"), dict(robot="kinova")):
        chain.append(dict(chain[-1], **change))
    chain.append(first)

    def device(c):
        return kinova_controller(c["Kr"], c["alpha"], c["V_max"], c["thr"], *arrs, eps=c["eps"], robot=_device_robot(c["robot"]))

    results = []
    for i, c in enumerate(chain):
        results.append(device(c))
        rb_ref = _oracle_robot(c["robot"])
        _assert_matches_oracle(results[-1], range(32), lambda s: robust_controller(c["Kr"], c["alpha"], c["V_max"], c["thr"], *[a[s] for a in arrs], eps=c["eps"], robot=rb_ref), ("chain", i))
        if 0 < i < len(chain) - 1:   # every link of the chain changes the answer, so a stale model would show
            assert any(not np.array_equal(a, b) for a, b in zip(results[-1], results[-2])), i
    for a, b in zip(results[-1], results[0]):
        assert np.array_equal(a, b)
    other = []
    t = threading.Thread(target=lambda: other.append(device(first)))
    t.start()
    t.join()
    assert len(other) == 1
    for a, b in zip(other[0], results[0]):
        assert np.array_equal(a, b)
