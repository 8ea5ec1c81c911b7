// armour_track: the closed loop of the reference's simulator -- an arm whose masses and inertias lie anywhere in the uncertainty
// interval, driven by the tracking controller along the planner's Bezier reference -- for a BATCH of rollouts on the device.
//
// Replaces uarmtd_agent.integrator + uarmtd_agent.dynamics with the LLC in the right-hand side (KSI/uarmtd_agent.m:280-293, :360-405;
// KSI/uarmtd_robust_CBF_LLC.m:160-175): ode15s there, fixed-step classical RK4 here.  One lane per rollout; the controller's nominal
// and interval models are built on the host once per call (controller_models.h, the same code as armour_robust_controller) and
// staged in LDS; the controller update is controller_core.h's robust_update, the plant is the nominal model with the rollout's
// scales in passivity-RNEA form (M by n unit-acceleration passes and a Cholesky factorisation, the bias by one pass with gravity).
//
// A robust update is ~10^4 dependent interval operations, four per RK4 step: a 2.5 s rollout at dt = 1e-3 is seconds of lane time.
// So the state lives in device memory (the ArmourTrackResult records themselves) and each launch advances every live rollout by at
// most `steps` steps; the host enqueues launches until every rollout has passed its last node.  A step reads nothing but its own
// rollout's state: the bits do not depend on the chunking.
#include <cmath>
#include <cstring>
#include <vector>

#include "bezier.h"
#include "common.h"
#include "controller_core.h"
#include "controller_models.h"

namespace {

using namespace ctl;
constexpr int MF = ARMOUR_MAX_FACTORS;

struct TrackArgs {
    Model<double> md;
    Model<Itv> imd;
    double Kr[MF];
    double alpha, V_max, r_norm_threshold;
    double lb[MF], ub[MF], speed[MF], torque[MF];
    double t0, t1, h, duration;
    int32_t N, controller, record_every, n_records;
};
// per rollout: the Bezier coefficients as armour_desired_trajectory forms them, and the plant's scales
struct TrackIn {
    double q0[MF], a[MF], b[MF], ka[MF];   // a = qd0 D, b = qdd0 D^2, ka = k_range k
    double sm[MF], sI[MF];
};

CTL_HD CTL_FLATTEN void reference(const TrackIn& in, int n, double D, double t, double* q, double* qd, double* qdd) {
    const double s = t / D;   // armour_desired_trajectory (api.hip)
    for (int i = 0; i < n; i++) {
        q[i] = bez::q_des(in.q0[i], in.a[i], in.b[i], in.ka[i], s);
        qd[i] = bez::qd_des(in.q0[i], in.a[i], in.b[i], in.ka[i], s) / D;
        qdd[i] = bez::qdd_des(in.q0[i], in.a[i], in.b[i], in.ka[i], s) / (D * D);
    }
}

// One evaluation of the closed loop at (t, q, qd): the reference, the controller's u and v, the plant's qdd and V_true = 1/2 r' M_true r.
// Returns false when the robust update finds the nominal torque outside the interval torque.
CTL_HD CTL_FLATTEN bool closed_loop(const TrackArgs& a, const Model<double>& mt, const TrackIn& in, double t, const double* q, const double* qd,
                                    double* qdd, double* u, double* v, double* qr, double* qdr, double* V) {
    const int n = a.md.n;
    double qddr[MF];
    reference(in, n, a.duration, t, qr, qdr, qddr);
    bool ok = true;
    if (a.controller == ARMOUR_TRACK_CTL_ROBUST) {
        double tau[MF];
        ok = robust_update(a.md, a.imd, a.Kr, a.alpha, a.V_max, a.r_norm_threshold, q, qd, qr, qdr, qddr, u, tau, v);
    } else if (a.controller == ARMOUR_TRACK_CTL_NOMINAL) {   // KSI/uarmtd_nominal_passivity_LLC.m: u = tau, the nominal passivity RNEA
        double qa_d[MF], qa_dd[MF], r[MF];
        (void)robust_prepare(n, a.Kr, q, qd, qr, qdr, qddr, qa_d, qa_dd, r);
        pass_rnea<double>(a.md, q, qd, qa_d, qa_dd, false, true, u);
        for (int i = 0; i < n; i++) v[i] = 0.0;
    } else {
        for (int i = 0; i < n; i++) { u[i] = 0.0; v[i] = 0.0; }
    }
    // the plant: M_true (armature on the diagonal through transI) column by column, h_true = C qd + g + damping qd
    KinStore<double> k;
    rnea_kinematics(mt, q, k);
    double M[MF * MF], e[MF], zero[MF], col[MF], hb[MF];
    for (int i = 0; i < n; i++) zero[i] = 0.0;
#pragma unroll 1
    for (int j = 0; j < n; j++) {
        for (int i = 0; i < n; i++) e[i] = i == j ? 1.0 : 0.0;
        rnea_dynamics(mt, k, zero, zero, e, false, false, col);
        for (int i = 0; i < n; i++) M[i * MF + j] = col[i];
    }
    rnea_dynamics(mt, k, qd, qd, zero, false, true, hb);
    // V_true before M is overwritten by its factor
    double r[MF];
    for (int i = 0; i < n; i++) r[i] = (qdr[i] - qd[i]) + a.Kr[i] * clamp_angle(qr[i] - q[i]);
    double Vt = 0.0;
    for (int i = 0; i < n; i++) {
        double Mr = 0.0;
        for (int j = 0; j < n; j++) Mr += M[i * MF + j] * r[j];
        Vt += r[i] * Mr;
    }
    *V = 0.5 * Vt;
    // Cholesky M = L L' on the lower triangle, then L y = u - h, L' qdd = y
    for (int j = 0; j < n; j++) {
        double d = M[j * MF + j];
        for (int p = 0; p < j; p++) d -= M[j * MF + p] * M[j * MF + p];
        d = sqrt(d);
        M[j * MF + j] = d;
        for (int i = j + 1; i < n; i++) {
            double s = M[i * MF + j];
            for (int p = 0; p < j; p++) s -= M[i * MF + p] * M[j * MF + p];
            M[i * MF + j] = s / d;
        }
    }
    for (int i = 0; i < n; i++) {
        double s = u[i] - hb[i];
        for (int p = 0; p < i; p++) s -= M[i * MF + p] * qdd[p];
        qdd[i] = s / M[i * MF + i];
    }
    for (int i = n - 1; i >= 0; i--) {
        double s = qdd[i];
        for (int p = i + 1; p < n; p++) s -= M[p * MF + i] * qdd[p];
        qdd[i] = s / M[i * MF + i];
    }
    return ok;
}

__global__ __launch_bounds__(64) void armour_track_kernel(const TrackArgs* __restrict__ ap, int B, const TrackIn* __restrict__ inputs,
                                                          ArmourTrackResult* __restrict__ state, double* __restrict__ trace, int steps) {
    // the models go to LDS as in the controller's kernels: every lane reads them on a chain of ~10^4 dependent operations
    __shared__ TrackArgs sa;
    static_assert(sizeof(TrackArgs) % sizeof(double) == 0, "TrackArgs is copied as doubles");
    for (unsigned i2 = threadIdx.x; i2 < sizeof(TrackArgs) / sizeof(double); i2 += blockDim.x)
        reinterpret_cast<double*>(&sa)[i2] = reinterpret_cast<const double*>(ap)[i2];
    __syncthreads();
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const TrackArgs& a = sa;
    ArmourTrackResult R = state[b];
    if (R.reserved) return;   // (reserved = 1: this rollout has passed its last node or stopped)
    const TrackIn in = inputs[b];
    const int n = a.md.n;
    Model<double> mt = a.md;   // the true plant: masses and CoM-frame inertias scaled (oracle_pass_rnea_scaled's convention)
    for (int i = 0; i < n; i++) {
        mt.I[i].m = mt.I[i].m * (1 + in.sm[i]);
        for (int e = 0; e < 9; e++) mt.I[i].I_bar.a[e] = mt.I[i].I_bar.a[e] * (1 + in.sI[i]);
    }
    const double h = a.h;
#pragma unroll 1
    for (int it = 0; it < steps; it++) {
        const int s = R.steps;
        const double t = s == a.N ? a.t1 : a.t0 + s * h;
        double kq[MF], kqd[MF], u[MF], v[MF], qr[MF], qdr[MF], V;
        bool ok = closed_loop(a, mt, in, t, R.q, R.qd, kqd, u, v, qr, qdr, &V);
        // the node's monitors, from the first stage
        int flags = 0;
        for (int i = 0; i < n; i++) {
            R.max_pos_error = fmax(R.max_pos_error, fabs(clamp_angle(qr[i] - R.q[i])));
            R.max_vel_error = fmax(R.max_vel_error, fabs(qdr[i] - R.qd[i]));
            R.max_robust_input = fmax(R.max_robust_input, fabs(v[i]));
            if (a.torque[i] > 0) R.max_torque_ratio = fmax(R.max_torque_ratio, fabs(u[i]) / a.torque[i]);
            if (u[i] > a.torque[i] || u[i] < -a.torque[i]) flags |= ARMOUR_TRACK_LIMIT_TORQUE;
            if (R.q[i] < a.lb[i] || R.q[i] > a.ub[i]) flags |= ARMOUR_TRACK_LIMIT_POSITION;
            if (R.qd[i] > a.speed[i] || R.qd[i] < -a.speed[i]) flags |= ARMOUR_TRACK_LIMIT_SPEED;
        }
        R.max_V = fmax(R.max_V, V);
        if (flags && R.limit_flags == 0) R.first_violation_t = t;
        R.limit_flags |= flags;
        R.t_end = t;
        if (trace && a.record_every && s % a.record_every == 0) {
            double* row = trace + ((size_t)b * a.n_records + s / a.record_every) * 3 * n;
            for (int i = 0; i < n; i++) { row[i] = R.q[i]; row[n + i] = R.qd[i]; row[2 * n + i] = u[i]; }
        }
        if (!ok) { R.status = 1; R.reserved = 1; break; }
        if (s == a.N) { R.reserved = 1; break; }
        // stages 2-4 of classical RK4; acc = k1 + 2 k2 + 2 k3 + k4
        double accq[MF], accqd[MF], zq[MF], zqd[MF];
        for (int i = 0; i < n; i++) { kq[i] = R.qd[i]; accq[i] = kq[i]; accqd[i] = kqd[i]; }
#pragma unroll 1
        for (int stg = 1; stg < 4 && ok; stg++) {
            const double ch = stg == 3 ? h : 0.5 * h;
            for (int i = 0; i < n; i++) { zq[i] = R.q[i] + ch * kq[i]; zqd[i] = R.qd[i] + ch * kqd[i]; }
            double Vs, us[MF], vs[MF], qrs[MF], qdrs[MF];
            ok = closed_loop(a, mt, in, t + ch, zq, zqd, kqd, us, vs, qrs, qdrs, &Vs);
            const double w = stg == 3 ? 1.0 : 2.0;
            for (int i = 0; i < n; i++) { kq[i] = zqd[i]; accq[i] = accq[i] + w * kq[i]; accqd[i] = accqd[i] + w * kqd[i]; }
        }
        if (!ok) { R.status = 1; R.reserved = 1; break; }
        const double h6 = h / 6;
        bool finite = true;
        for (int i = 0; i < n; i++) {
            zq[i] = R.q[i] + h6 * accq[i];
            zqd[i] = R.qd[i] + h6 * accqd[i];
            finite = finite && fabs(zq[i]) < INFINITY && fabs(zqd[i]) < INFINITY;
        }
        if (!finite) { R.status = 2; R.reserved = 1; break; }
        for (int i = 0; i < n; i++) { R.q[i] = zq[i]; R.qd[i] = zqd[i]; }
        R.steps = s + 1;
    }
    state[b] = R;
}

// Device time of one RK4 step, measured on the MI355X (tools/track_bench.py, profiles/track_bench.json "per_step_ms": 64 lanes, 60 steps
// at 20 per launch): robust 4.29 ms -- four robust updates plus the plant --, no controller 0.77 ms (the plant alone; the nominal
// controller adds one double pass per stage).  Lanes run side by side, so this holds from B = 1 to thousands (the same JSON: a whole 2.5 s rollout
// takes 10.88 s at B = 1 and 11.27 s at B = 4096, 4.35 / 4.51 ms per step).  Automatic steps per launch aim at kLaunchTargetMs of device time per launch:
// 3 robust steps (12.9 ms), 19 plant steps (14.7 ms).
constexpr double kStepMsRobust = 4.3;
constexpr double kStepMsPlant = 0.77;
constexpr double kLaunchTargetMs = 15.0;

}  // namespace

extern "C" void armour_track_options_default(const ArmourRobot* robot, ArmourTrackOptions* opt) {
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->controller = ARMOUR_TRACK_CTL_ROBUST;
    if (robot) {   // KSI/uarmtd_robust_CBF_LLC.m:6-9 with the robot's constants
        for (int i = 0; i < ARMOUR_MAX_FACTORS; i++) opt->Kr[i] = robot->K;
        opt->alpha = robot->alpha;
        opt->V_max = robot->V_m;
        opt->model_uncertainty = robot->mass_uncertainty;
    }
    opt->r_norm_threshold = 0.0;
    opt->dt = 1e-3;
    opt->t0 = 0.0;
    opt->t1 = 1.0;
    opt->duration = 1.0;
}

extern "C" int armour_track(const ArmourRobot* robot, const ArmourTrackOptions* opt, int32_t B, const double* q0, const double* qd0, const double* qdd0,
                            const double* k, const double* k_range, const double* z0, const double* mass_scale, const double* inertia_scale,
                            ArmourTrackResult* results, double* trace, double* ms) {
    // ---- arguments, before the device is touched
    if (!robot || !opt || !q0 || !qd0 || !qdd0 || !k || !k_range || !results || B < 1) { armour_set_error("armour_track: null or empty argument"); return ARMOUR_EINVAL; }
    const int n = robot->num_factors;
    if (n < 1 || n > MF) { armour_set_error("armour_track: num_factors out of range"); return ARMOUR_EINVAL; }
    if (opt->controller < ARMOUR_TRACK_CTL_ROBUST || opt->controller > ARMOUR_TRACK_CTL_NONE) { armour_set_error("armour_track: unknown controller %d", opt->controller); return ARMOUR_EINVAL; }
    if (!(opt->dt > 0) || !std::isfinite(opt->dt) || !(opt->t0 >= 0) || !(opt->t1 > opt->t0) || !(opt->t1 <= opt->duration) || !std::isfinite(opt->duration)) {
        armour_set_error("armour_track: need dt > 0 and 0 <= t0 < t1 <= duration");
        return ARMOUR_EINVAL;
    }
    if (opt->record_every < 0 || opt->steps_per_launch < 0) { armour_set_error("armour_track: record_every and steps_per_launch must be >= 0"); return ARMOUR_EINVAL; }
    const double steps_real = std::ceil((opt->t1 - opt->t0) / opt->dt - 1e-9);
    if (!(steps_real >= 1) || steps_real > 1e8) { armour_set_error("armour_track: (t1 - t0) / dt gives %g steps", steps_real); return ARMOUR_EINVAL; }
    const int N = (int)steps_real;
    if (!finite_all(opt->Kr, n) || !std::isfinite(opt->alpha) || !std::isfinite(opt->V_max) || !std::isfinite(opt->r_norm_threshold) ||
        !(opt->model_uncertainty >= 0) || !std::isfinite(opt->model_uncertainty)) {
        armour_set_error("armour_track: non-finite controller constant");
        return ARMOUR_EINVAL;
    }
    const size_t bn = (size_t)B * n;
    if (!finite_all(q0, bn) || !finite_all(qd0, bn) || !finite_all(qdd0, bn) || !finite_all(k, bn) || !finite_all(k_range, n) ||
        (z0 && !finite_all(z0, 2 * bn)) || (mass_scale && !finite_all(mass_scale, bn)) || (inertia_scale && !finite_all(inertia_scale, bn))) {
        armour_set_error("armour_track: non-finite input");
        return ARMOUR_EINVAL;
    }
    std::vector<TrackArgs> args(1);
    TrackArgs& ta = args[0];
    memset(&ta, 0, sizeof(ta));
    if (build_models(*robot, opt->model_uncertainty, ta.md, ta.imd) != 0) { armour_set_error("armour_track: unsupported robot model (joint axes / count)"); return ARMOUR_EINVAL; }
    for (int i = 0; i < n; i++) {
        ta.Kr[i] = opt->Kr[i];
        ta.lb[i] = robot->state_limits_lb[i]; ta.ub[i] = robot->state_limits_ub[i];
        ta.speed[i] = robot->speed_limits[i]; ta.torque[i] = robot->torque_limits[i];
    }
    ta.alpha = opt->alpha; ta.V_max = opt->V_max; ta.r_norm_threshold = opt->r_norm_threshold;
    ta.t0 = opt->t0; ta.t1 = opt->t1; ta.h = (opt->t1 - opt->t0) / N; ta.duration = opt->duration;
    ta.N = N; ta.controller = opt->controller;
    const bool want_trace = trace && opt->record_every > 0;
    ta.record_every = want_trace ? opt->record_every : 0;
    ta.n_records = want_trace ? N / opt->record_every + 1 : 0;
    std::vector<TrackIn> ins(B);
    std::vector<ArmourTrackResult> st(B);
    const double D = opt->duration;
    for (int b = 0; b < B; b++) {
        TrackIn& in = ins[b];
        memset(&in, 0, sizeof(in));
        for (int i = 0; i < n; i++) {
            const size_t x = (size_t)b * n + i;
            in.q0[i] = q0[x]; in.a[i] = qd0[x] * D; in.b[i] = qdd0[x] * D * D; in.ka[i] = k_range[i] * k[x];
            in.sm[i] = mass_scale ? mass_scale[x] : 0.0;
            in.sI[i] = inertia_scale ? inertia_scale[x] : 0.0;
        }
        ArmourTrackResult& r = st[b];
        memset(&r, 0, sizeof(r));
        r.first_violation_t = NAN;
        double qr[MF], qdr[MF], qddr[MF];
        reference(in, n, D, opt->t0, qr, qdr, qddr);
        for (int i = 0; i < n; i++) {
            r.q[i] = z0 ? z0[(size_t)b * 2 * n + i] : qr[i];
            r.qd[i] = z0 ? z0[(size_t)b * 2 * n + n + i] : qdr[i];
        }
        r.t_end = opt->t0;
    }
    int S = opt->steps_per_launch;
    if (S == 0) {
        const double per_step = opt->controller == ARMOUR_TRACK_CTL_ROBUST ? kStepMsRobust : kStepMsPlant;
        S = (int)std::fmax(1.0, std::floor(kLaunchTargetMs / per_step));
    }
    const size_t trace_doubles = want_trace ? (size_t)B * ta.n_records * 3 * n : 0;
    // ---- the device
    if (!armour_device_available()) { armour_set_error("armour_track: no HIP device visible (there is no CPU path)"); return ARMOUR_EDEVICE; }
    DevStream stream;
    EventPair ev;
    DevBuf<TrackArgs> d_args;
    DevBuf<TrackIn> d_in;
    DevBuf<ArmourTrackResult> d_st;
    DevBuf<double> d_trace;
    ARMOUR_TRY(stream.create());
    ARMOUR_TRY(d_args.reserve(1));
    ARMOUR_TRY(d_in.reserve(B));
    ARMOUR_TRY(d_st.reserve(B));
    if (trace_doubles) ARMOUR_TRY(d_trace.reserve(trace_doubles));
    HIPCHK(hipMemcpyAsync(d_args, &ta, sizeof(TrackArgs), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_in, ins.data(), sizeof(TrackIn) * B, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_st, st.data(), sizeof(ArmourTrackResult) * B, hipMemcpyHostToDevice, stream));
    if (trace_doubles) HIPCHK(hipMemsetAsync(d_trace, 0xff, trace_doubles * sizeof(double), stream));   // all-ones bytes: NaN for nodes never reached
    // every rollout needs N steps and one pass at its last node: ceil((N + 1) / S) launches; rollouts that stop early return at once
    const long long launches = ((long long)N + S) / S;
    ARMOUR_TRY(ev.record_start(stream));
    for (long long l = 0; l < launches; l++) {
        hipLaunchKernelGGL(armour_track_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, d_args, B, d_in, d_st, d_trace, S);
        HIPCHK(hipGetLastError());
    }
    ARMOUR_TRY(ev.record_stop(stream));
    HIPCHK(hipMemcpyAsync(st.data(), d_st, sizeof(ArmourTrackResult) * B, hipMemcpyDeviceToHost, stream));
    if (trace_doubles) HIPCHK(hipMemcpyAsync(trace, d_trace, trace_doubles * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (ms) ARMOUR_TRY(ev.elapsed_ms(ms));
    for (int b = 0; b < B; b++) {   // every rollout has passed its last node or stopped: the launches above are enough by construction
        if (!st[b].reserved) { armour_set_error("armour_track: rollout %d did not finish", b); return ARMOUR_ESTATE; }
        st[b].reserved = 0;
    }
    memcpy(results, st.data(), sizeof(ArmourTrackResult) * B);
    return ARMOUR_OK;
}

// the number of steps per launch armour_track picks for a controller when steps_per_launch = 0 (tools/track_bench.py records it)
extern "C" int armour_track_auto_steps(int32_t controller) {
    if (controller < ARMOUR_TRACK_CTL_ROBUST || controller > ARMOUR_TRACK_CTL_NONE) return ARMOUR_EINVAL;
    const double per_step = controller == ARMOUR_TRACK_CTL_ROBUST ? kStepMsRobust : kStepMsPlant;
    return (int)std::fmax(1.0, std::floor(kLaunchTargetMs / per_step));
}
