"""Closed-loop tracking (armour_track, armour_amd/tracking.py): the plan executed by an arm with uncertain masses and inertias under the
tracking controller -- uarmtd_agent.dynamics + integrator with the LLC in the right-hand side (KSI/uarmtd_agent.m:280-293, :360-405).

The device is checked against a host restatement written here: the same RK4 and node rule, the controller of the CPU oracle
(oracle.cpu_oracle.robust_controller), the plant's M columns and bias from oracle.cpu_oracle.pass_rnea_scaled.  The restatement is
itself held by two invariants (exact tracking under the nominal controller, fourth-order energy convergence of the passive plant).
The limit monitors are a function of the nodes alone (limit_monitors; with_limits monitors a finished run again under other limits) and
report how far every node stayed from every limit; _compare holds the device to the restatement, flags and times exactly.  The verdict
paths -- limits, stops, ragged grids, block edges, the 8-factor ABI -- are in test_tracking_edges.py."""
import ctypes as C
import math

import numpy as np
import pytest

from armour_amd import _lib

N_J = 7


def _robot():
    from armour_amd.planner import kinova_robot
    return kinova_robot()


def _wrap(x):
    """clamp_angle's rule (controller_core.h): the reference's loop up to 64 pi, fmod first beyond, NaN for inf / NaN -- bounded for every double."""
    x = np.array(x, dtype=np.float64)
    for i in range(x.size):
        r = float(x.flat[i])
        if not abs(r) <= 64 * math.pi:
            r = math.fmod(r, 2 * math.pi) if math.isfinite(r) else math.nan
        while r >= math.pi:
            r -= 2 * math.pi
        while r < -math.pi:
            r += 2 * math.pi
        x.flat[i] = r
    return x


def _reference(q0, qd0, qdd0, k, k_range, D, t):
    L = _lib.load()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    n = q0.size
    q, qd, qdd = np.zeros(n), np.zeros(n), np.zeros(n)
    args = [np.ascontiguousarray(a, dtype=np.float64) for a in (q0, qd0, qdd0, k_range)]
    kk = np.ascontiguousarray(k, dtype=np.float64)
    assert L.armour_desired_trajectory(n, dp(args[0]), dp(args[1]), dp(args[2]), dp(args[3]), float(D), dp(kk), float(t), dp(q), dp(qd), dp(qdd)) == 0
    return q, qd, qdd


def _limits(rb, n):
    return (np.array(rb.state_limits_lb[:n]), np.array(rb.state_limits_ub[:n]), np.array(rb.speed_limits[:n]), np.array(rb.torque_limits[:n]))


def limit_monitors(nodes, lb, ub, speed, torque):
    """The kernel's limit monitors over a rollout's nodes [(t, q, qd, u), ...], joint by joint as tracking.hip has them: the torque ratio only
    for joints whose limit is above 0 (a limit <= 0 contributes no ratio and still flags), each flag from two one-sided comparisons (a NaN
    crosses nothing), maxima by fmax (a NaN candidate is ignored), first_violation_t the first flagged node's t.  The monitors read the
    state and change none of it, so the same nodes can be monitored again under other limits (with_limits).
    margins: per quantity the smallest distance, over nodes and joints, between the monitored value and a limit -- a flag asserted on the
    device is only as sure as this distance is large against the parity tolerance."""
    out = dict(limit_flags=0, first_violation_t=np.nan, max_torque_ratio=0.0)
    margins = dict(torque=np.inf, position=np.inf, speed=np.inf)
    for t, q, qd, u in nodes:
        flags = 0
        for i in range(len(q)):
            if torque[i] > 0:
                out["max_torque_ratio"] = float(np.fmax(out["max_torque_ratio"], abs(u[i]) / torque[i]))
            if u[i] > torque[i] or u[i] < -torque[i]:
                flags |= _lib.TRACK_LIMIT_TORQUE
            if q[i] < lb[i] or q[i] > ub[i]:
                flags |= _lib.TRACK_LIMIT_POSITION
            if qd[i] > speed[i] or qd[i] < -speed[i]:
                flags |= _lib.TRACK_LIMIT_SPEED
        with np.errstate(invalid="ignore"):
            margins["torque"] = float(np.fmin(margins["torque"], np.fmin.reduce(np.abs(np.abs(u) - torque))))
            margins["position"] = float(np.fmin(margins["position"], np.fmin.reduce(np.fmin(np.abs(q - lb), np.abs(q - ub)))))
            margins["speed"] = float(np.fmin(margins["speed"], np.fmin.reduce(np.abs(np.abs(qd) - speed))))
        if flags and out["limit_flags"] == 0:
            out["first_violation_t"] = t
        out["limit_flags"] |= flags
    out["margins"] = margins
    return out


def with_limits(run, rb):
    """A host_track result monitored again under the limits of `rb` (every other field is the run's own)."""
    return {**run, **limit_monitors(run["nodes"], *_limits(rb, len(run["q"])))}


def host_track(rb, q0, qd0, qdd0, k, k_range, D, t0=0.0, t1=None, dt=1e-3, controller="robust", z0=None, sm=None, sI=None, Kr=None, alpha=None,
               V_max=None, r_thr=0.0, eps=None, record_every=0):
    """One rollout of armour_track restated on the host (numpy + the CPU oracle).  Besides the fields of ArmourTrackResult: trace, nodes
    (t, q, qd, u of every node reached), N, h and margins (limit_monitors)."""
    from oracle.cpu_oracle import pass_rnea_scaled, robust_controller
    n = rb.num_factors
    t1 = D if t1 is None else t1
    Kr = np.full(n, rb.K) if Kr is None else np.broadcast_to(np.asarray(Kr, dtype=np.float64), (n,))
    alpha = rb.alpha if alpha is None else alpha
    V_max = rb.V_m if V_max is None else V_max
    eps = rb.mass_uncertainty if eps is None else eps
    sm = np.zeros(n) if sm is None else np.asarray(sm, dtype=np.float64)
    sI = np.zeros(n) if sI is None else np.asarray(sI, dtype=np.float64)
    N = int(np.ceil((t1 - t0) / dt - 1e-9))
    h = (t1 - t0) / N
    zeros = np.zeros(n)

    def rhs(t, q, qd):
        qr, qdr, qddr = _reference(q0, qd0, qdd0, k, k_range, D, t)
        ok, v = True, np.zeros(n)
        if controller == "robust":
            out = robust_controller(Kr, alpha, V_max, r_thr, q, qd, qr, qdr, qddr, eps=eps, robot=rb)
            u, v, ok = out["u"], out["v"], out["inside"]
        elif controller == "nominal":
            e = _wrap(qr - q)
            u = pass_rnea_scaled(zeros, zeros, q, qd, qdr + Kr * e, qddr + Kr * (qdr - qd), True, rb)
        else:
            u = np.zeros(n)
        M = np.stack([pass_rnea_scaled(sm, sI, q, zeros, zeros, np.eye(n)[j], False, rb) for j in range(n)], axis=1)
        hb = pass_rnea_scaled(sm, sI, q, qd, qd, zeros, True, rb)
        r = (qdr - qd) + Kr * _wrap(qr - q)
        return np.linalg.solve(M, u - hb), u, v, qr, qdr, 0.5 * r @ M @ r, ok

    q, qd = _reference(q0, qd0, qdd0, k, k_range, D, t0)[:2]
    if z0 is not None:
        q, qd = np.array(z0[:n], dtype=np.float64), np.array(z0[n:], dtype=np.float64)
    res = dict(status=0, steps=0, max_pos_error=0.0, max_vel_error=0.0, max_V=0.0, max_robust_input=0.0, t_end=t0, N=N, h=h)
    trace = np.full((N // record_every + 1, 3, n), np.nan) if record_every else None
    nodes = []
    fmax = lambda name, cand: float(np.fmax(res[name], np.fmax.reduce(np.atleast_1d(cand))))   # fmax: a NaN candidate is ignored
    with np.errstate(all="ignore"):   # (a non-finite state is ordinary arithmetic here, as on the device)
        for s in range(N + 1):
            t = t1 if s == N else t0 + s * h
            kqd, u, v, qr, qdr, V, ok = rhs(t, q, qd)
            res["max_pos_error"] = fmax("max_pos_error", np.abs(_wrap(qr - q)))
            res["max_vel_error"] = fmax("max_vel_error", np.abs(qdr - qd))
            res["max_robust_input"] = fmax("max_robust_input", np.abs(v))
            res["max_V"] = fmax("max_V", V)
            nodes.append((t, q.copy(), qd.copy(), u.copy()))
            res["t_end"] = t
            if record_every and s % record_every == 0:
                trace[s // record_every] = (q, qd, u)
            if not ok:
                res["status"] = 1
                break
            if s == N:
                break
            kq, acc_q, acc_qd = qd.copy(), qd.copy(), kqd.copy()
            for stg in (1, 2, 3):
                ch = h if stg == 3 else 0.5 * h
                zq, zqd = q + ch * kq, qd + ch * kqd
                kqd, _, _, _, _, _, ok = rhs(t + ch, zq, zqd)
                if not ok:
                    break
                w = 1.0 if stg == 3 else 2.0
                kq = zqd
                acc_q, acc_qd = acc_q + w * kq, acc_qd + w * kqd
            if not ok:
                res["status"] = 1
                break
            nq, nqd = q + (h / 6) * acc_q, qd + (h / 6) * acc_qd
            if not (np.all(np.isfinite(nq)) and np.all(np.isfinite(nqd))):
                res["status"] = 2   # the state stays at the last finite node, steps unchanged
                break
            q, qd = nq, nqd
            res["steps"] = s + 1
    res["q"], res["qd"], res["trace"], res["nodes"] = q, qd, trace, nodes
    res.update(limit_monitors(nodes, *_limits(rb, n)))
    return res


def _plans(rng, B, n=N_J):
    q0 = rng.uniform(-1.5, 1.5, (B, n))
    qd0 = rng.uniform(-0.5, 0.5, (B, n))
    qdd0 = rng.uniform(-1.0, 1.0, (B, n))
    k = rng.uniform(-1, 1, (B, n))
    return q0, qd0, qdd0, k


def _start_inside(rb, rng, q0, qd0, qdd0, k, k_range, D, sm, sI, frac=0.5):
    """Actual start states near the reference's: V_true(0) <= frac V_max and every |position error| <= frac qe."""
    from oracle.cpu_oracle import pass_rnea_scaled
    from armour_amd.tracking import ultimate_bound
    n = rb.num_factors
    _, qe, _ = ultimate_bound(rb)
    z0 = np.zeros((q0.shape[0], 2 * n))
    for b in range(q0.shape[0]):
        qr, qdr, _ = _reference(q0[b], qd0[b], qdd0[b], k[b], k_range, D, 0.0)
        e = rng.uniform(-1, 1, n) * frac * qe
        de = rng.normal(size=n) * 0.01
        r = de + rb.K * e
        M = np.stack([pass_rnea_scaled(sm[b], sI[b], qr - e, np.zeros(n), np.zeros(n), np.eye(n)[j], False, rb) for j in range(n)], axis=1)
        V = 0.5 * r @ M @ r
        if V > frac * rb.V_m:   # shrink the whole error: V scales with the square
            sc = np.sqrt(frac * rb.V_m / V) * 0.99
            e, de = e * sc, de * sc
        z0[b] = np.concatenate([qr - e, qdr - de])
    return z0


# ------------------------------------------------------------------------------------------------ CPU
def test_entry_checks_its_arguments():
    L = _lib.load()
    rb = _robot()
    n = rb.num_factors
    z = np.zeros(n)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    kr = np.full(n, np.pi / 48)
    res = (_lib.ArmourTrackResult * 1)()

    def call(B=1, **fields):
        opt = _lib.ArmourTrackOptions()
        L.armour_track_options_default(C.byref(rb), C.byref(opt))
        opt.t1, opt.duration = 0.01, 1.0
        for key, val in fields.items():
            setattr(opt, key, val)
        return L.armour_track(C.byref(rb), C.byref(opt), B, dp(z), dp(z), dp(z), dp(z), dp(kr), None, None, None, res, None, None)

    opt = _lib.ArmourTrackOptions()
    L.armour_track_options_default(C.byref(rb), C.byref(opt))
    assert (opt.controller, opt.dt, opt.r_norm_threshold) == (_lib.TRACK_CTL_ROBUST, 1e-3, 0.0)
    assert list(opt.Kr[:n]) == [rb.K] * n and opt.alpha == rb.alpha and opt.V_max == rb.V_m and opt.model_uncertainty == rb.mass_uncertainty
    for bad in (dict(dt=0.0), dict(dt=-1e-3), dict(t0=0.5, t1=0.5), dict(t0=0.5, t1=0.4), dict(t1=1.5), dict(controller=3), dict(controller=-1),
                dict(t0=-0.1), dict(record_every=-1), dict(steps_per_launch=-2)):
        assert call(**bad) == _lib.EINVAL, bad
    assert call(B=0) == _lib.EINVAL
    assert L.armour_track_auto_steps(_lib.TRACK_CTL_ROBUST) >= 1 and L.armour_track_auto_steps(7) == _lib.EINVAL


def test_entry_needs_a_device():
    L = _lib.load()
    if L.armour_device_available():
        pytest.skip("a GPU is visible here")
    from armour_amd.tracking import simulate_tracking
    with pytest.raises(_lib.ArmourError) as ei:
        simulate_tracking(_robot(), np.zeros(N_J), np.zeros(N_J), np.zeros(N_J), np.zeros(N_J), np.pi / 48, 1.0, t1=0.01)
    assert ei.value.code == _lib.EDEVICE


def test_restatement_tracks_exactly_under_the_nominal_controller():
    """True plant = nominal model, start on the reference: the passivity controller's closed loop has q = q_des as its solution."""
    rb = _robot()
    rng = np.random.default_rng(5)
    q0, qd0, qdd0, k = _plans(rng, 1)
    out = host_track(rb, q0[0], qd0[0], qdd0[0], k[0], np.full(N_J, np.pi / 48), 1.0, t1=0.5, controller="nominal")
    assert out["status"] == 0 and out["steps"] == 500
    assert out["max_pos_error"] <= 1e-10 and out["max_vel_error"] <= 1e-9


def test_restatement_is_fourth_order_on_the_passive_plant():
    """u = 0, no gravity, no damping: the kinetic energy 1/2 qd' M qd is conserved; RK4's drift falls by ~2^4 when dt halves."""
    from oracle.cpu_oracle import pass_rnea_scaled
    rb = _robot()
    rb.gravity = 0.0
    n = rb.num_factors
    rng = np.random.default_rng(6)
    q0 = rng.uniform(-1, 1, n)
    z0 = np.concatenate([q0, rng.uniform(-2, 2, n)])

    def energy(q, qd):
        M = np.stack([pass_rnea_scaled(np.zeros(n), np.zeros(n), q, np.zeros(n), np.zeros(n), np.eye(n)[j], False, rb) for j in range(n)], axis=1)
        return 0.5 * qd @ M @ qd

    E0 = energy(z0[:n], z0[n:])
    drift = []
    for dt in (0.04, 0.02, 0.01):
        out = host_track(rb, q0, np.zeros(n), np.zeros(n), np.zeros(n), np.ones(n), 1.0, dt=dt, controller="none", z0=z0)
        assert out["status"] == 0
        drift.append(abs(energy(out["q"], out["qd"]) - E0))
    ratios = [drift[0] / drift[1], drift[1] / drift[2]]
    assert all(10 <= r <= 24 for r in ratios), (drift, ratios)


# ------------------------------------------------------------------------------------------------ GPU
def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _compare(dev, host_runs, tol=1e-9, lanes=None):
    """Device lane lanes[i] (default i) against host_runs[i]; returns the largest |device - restatement| over states, maxima and trace."""
    worst = 0.0
    for i, h in enumerate(host_runs):
        b = i if lanes is None else lanes[i]
        assert dev.status[b] == h["status"] and dev.steps[b] == h["steps"] and dev.limit_flags[b] == h["limit_flags"], \
            (b, dev.status[b], h["status"], dev.steps[b], h["steps"], dev.limit_flags[b], h["limit_flags"])
        assert _same_bits(dev.t_end[b], h["t_end"]), (b, dev.t_end[b], h["t_end"])
        assert _same_bits(dev.first_violation_t[b], h["first_violation_t"]) or (np.isnan(dev.first_violation_t[b]) and np.isnan(h["first_violation_t"])), \
            (b, dev.first_violation_t[b], h["first_violation_t"])
        assert np.abs(dev.q[b] - h["q"]).max() <= tol and np.abs(dev.qd[b] - h["qd"]).max() <= tol, b
        worst = max(worst, np.abs(dev.q[b] - h["q"]).max(), np.abs(dev.qd[b] - h["qd"]).max())
        for name in ("max_pos_error", "max_vel_error", "max_V", "max_robust_input", "max_torque_ratio"):
            d, r = getattr(dev, name)[b], h[name]
            assert np.isnan(d) == np.isnan(r), (b, name, d, r)
            if np.isinf(r) or np.isinf(d):   # equal infinities are equal
                assert d == r, (b, name, d, r)
            elif not np.isnan(r):
                assert abs(d - r) <= tol * max(abs(r), 1e-300) or abs(d - r) <= 1e-15, (b, name, d, r)
                worst = max(worst, abs(d - r))
        if h["trace"] is not None:
            dt_, ht = dev.trace[b], h["trace"]
            assert np.array_equal(np.isnan(dt_), np.isnan(ht)), b
            inf = np.isinf(ht) | np.isinf(dt_)
            assert np.array_equal(dt_[inf], ht[inf]), b
            fin = np.isfinite(ht)
            if fin.any():
                diff = np.abs(dt_[fin] - ht[fin]).max()
                assert diff <= tol * max(1.0, np.abs(ht[fin]).max()), (b, diff)
                worst = max(worst, diff)
    return float(worst)


@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["robust", "nominal", "none"])
def test_device_equals_the_host_restatement(controller):
    from armour_amd.tracking import plant_samples, simulate_tracking
    rb = _robot()
    rng = np.random.default_rng(11)
    B, eps, kr, D = 16, 0.05, np.full(N_J, np.pi / 48), 1.0
    q0, qd0, qdd0, k = _plans(rng, B)
    sm, sI = plant_samples(rb, B, eps, rng)
    z0 = _start_inside(rb, rng, q0, qd0, qdd0, k, kr, D, sm, sI)
    kw = dict(t1=0.2, dt=1e-3, controller=controller, z0=z0)
    dev = simulate_tracking(rb, q0, qd0, qdd0, k, kr, D, mass_scale=sm, inertia_scale=sI, model_uncertainty=eps, record_every=1, **kw)
    host = [host_track(rb, q0[b], qd0[b], qdd0[b], k[b], kr, D, sm=sm[b], sI=sI[b], eps=eps, record_every=1, **{**kw, "z0": z0[b]}) for b in range(B)]
    assert np.all(dev.steps == 200)
    _compare(dev, host)


@pytest.mark.gpu
def test_the_ultimate_bound_holds_on_uncertain_plants():
    """1024 rollouts, true masses / inertias anywhere within +-model_uncertainty, starts inside the bound, the whole plan.
    tau: the continuous-time guarantee (V <= V_max, |e| <= qe, |de| <= qde) seen through RK4 at dt = 1e-3 and its node sampling.  The
    host restatement's dt-halving study on rollouts of this kind (tools/track_bench.py --tau-study, profiles/track_tau_study.txt) changes
    every maximum by < 1e-10 relative between dt = 1e-3 and 5e-4; tau = 1e-4 is six orders of magnitude above that discretisation effect
    and still far below any real excursion past the bound."""
    from armour_amd.tracking import plant_samples, simulate_tracking, ultimate_bound
    rb = _robot()
    rng = np.random.default_rng(12)
    B, kr, D, tau = 1024, np.full(N_J, np.pi / 48), 1.0, 1e-4
    q0, qd0, qdd0, k = _plans(rng, B)
    sm, sI = plant_samples(rb, B, rb.mass_uncertainty, rng)
    z0 = _start_inside(rb, rng, q0, qd0, qdd0, k, kr, D, sm, sI)
    res = simulate_tracking(rb, q0, qd0, qdd0, k, kr, D, z0=z0, mass_scale=sm, inertia_scale=sI)
    ub, qe, qde = ultimate_bound(rb)
    bad = np.flatnonzero((res.status != 0) | (res.max_V > rb.V_m * (1 + tau)) | (res.max_pos_error > qe * (1 + tau)) | (res.max_vel_error > qde * (1 + tau)))
    assert bad.size == 0, [(int(b), int(res.status[b]), res.max_V[b], res.max_pos_error[b], res.max_vel_error[b]) for b in bad[:5]]
    assert np.all(res.steps == 1000)


@pytest.mark.gpu
def test_planned_trajectories_are_tracked_inside_the_bound():
    """ARMOUR's end-to-end promise: every feasible plan of the 107 reference worlds, executed on 8 plants within the robot's
    mass_uncertainty by its own controller, stays within qe of the plan and within every torque / position / speed limit."""
    from armour_amd.planner import ArmourNLP
    from armour_amd.scenes import as_batch, reference_worlds
    from armour_amd.tracking import simulate_plans, ultimate_bound
    bp = as_batch(reference_worlds())
    nlp = ArmourNLP(T=100).set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], bp["obstacles"])
    sols = nlp.solve(tolerance=1e-7, max_iterations=100)
    out = simulate_plans(nlp, sols, samples=8, rng=np.random.default_rng(13))
    assert len(out["problems"]) + len(out["skipped"]) == 107 and len(out["problems"]) >= 50
    res = out["result"]
    _, qe, _ = ultimate_bound(nlp.robot)
    bad = np.flatnonzero((res.status != 0) | (res.limit_flags != 0) | (res.max_pos_error > qe))
    assert bad.size == 0, [(out["problems"][b // 8], int(res.status[b]), int(res.limit_flags[b]), res.max_pos_error[b], res.max_torque_ratio[b]) for b in bad[:5]]


@pytest.mark.gpu
def test_rollouts_are_independent_of_batch_and_chunking():
    from armour_amd.tracking import plant_samples, simulate_tracking
    rb = _robot()
    rng = np.random.default_rng(14)
    B, kr, D = 1024, np.full(N_J, np.pi / 48), 1.0
    q0, qd0, qdd0, k = _plans(rng, B)
    sm, sI = plant_samples(rb, B, rb.mass_uncertainty, rng)
    z0 = np.concatenate([q0 + rng.uniform(-5e-3, 5e-3, (B, N_J)), qd0 + rng.uniform(-5e-3, 5e-3, (B, N_J))], axis=1)
    kw = dict(t1=0.1, record_every=5)
    full = simulate_tracking(rb, q0, qd0, qdd0, k, kr, D, z0=z0, mass_scale=sm, inertia_scale=sI, **kw)
    s = slice(37, 38)
    one = simulate_tracking(rb, q0[s], qd0[s], qdd0[s], k[s], kr, D, z0=z0[s], mass_scale=sm[s], inertia_scale=sI[s], **kw)
    for name in ("q", "qd", "max_pos_error", "max_vel_error", "max_V", "max_robust_input", "max_torque_ratio", "trace", "status", "steps"):
        assert np.array_equal(getattr(full, name)[37], getattr(one, name)[0]), name
    s = slice(0, 16)
    runs = [simulate_tracking(rb, q0[s], qd0[s], qdd0[s], k[s], kr, D, z0=z0[s], mass_scale=sm[s], inertia_scale=sI[s], steps_per_launch=S, **kw)
            for S in (1, 7, 0)]
    for r in runs[1:]:
        for name in ("q", "qd", "max_pos_error", "max_vel_error", "max_V", "max_robust_input", "max_torque_ratio", "trace", "steps", "t_end"):
            assert np.array_equal(getattr(r, name), getattr(runs[0], name), equal_nan=True), name
    assert np.array_equal(runs[0].trace[:, -1, 0], runs[0].q) and np.array_equal(runs[0].trace[:, -1, 1], runs[0].qd)
    assert np.all(runs[0].t_end == 0.1)


@pytest.mark.gpu
def test_reference_controller_study_runs():
    from armour_amd.tracking import compare_robust_controller
    out = compare_robust_controller(levels=(0.0, 0.1), samples=8, seed=3)
    assert out["max_v"].shape == (2, 8) and out["status"].shape == (2, 8) and out["median_max_v"].shape == (2,)
    assert np.all(np.isfinite(out["max_v"])) and np.all(np.isfinite(out["median_max_v"]))
    for res in out["result"]:
        assert np.all(np.isin(res.status, (0, 1, 2)))
        ok = res.status == 0
        assert np.all(res.steps[ok] == 2500) and np.all(np.isfinite(res.q)) and np.all(np.isfinite(res.max_V))
