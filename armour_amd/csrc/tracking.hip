// armour_track: the closed loop of the reference's simulator -- an arm whose masses and inertias lie anywhere in the uncertainty
// interval, driven by the tracking controller along the planner's Bezier reference -- for a BATCH of rollouts on the device.
//
// Replaces uarmtd_agent.integrator + uarmtd_agent.dynamics with the LLC in the right-hand side (KSI/uarmtd_agent.m:280-293, :360-405;
// KSI/uarmtd_robust_CBF_LLC.m:160-175): ode15s there, fixed-step classical RK4 here.  One lane per rollout; the controller's nominal
// and interval models are built on the host once per call (controller_models.h, the same code as armour_robust_controller) and
// staged in LDS; the controller update is controller_core.h's robust_update (or althoff_update: ARMOUR_TRACK_CTL_ALTHOFF, the second
// controller of kinova_compare_robust_controller.m, whose kernel is tracking_althoff.hip; the steps are tracking_steps.h), the plant is the nominal model with the rollout's
// scales in passivity-RNEA form (M by n unit-acceleration passes and a Cholesky factorisation, the bias by one pass with gravity).
//
// A robust update is ~10^4 dependent interval operations, four per RK4 step: a 2.5 s rollout at dt = 1e-3 is seconds of lane time.
// So the state lives in device memory (the ArmourTrackResult records themselves) and each launch advances every live rollout by at
// most `steps` steps; the host enqueues launches until every rollout has passed its last node.  A step reads nothing but its own
// rollout's state: the bits do not depend on the chunking.
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "controller_models.h"
#include "tracking_steps.h"

namespace {

using namespace ctl;
using namespace trk;

__global__ __launch_bounds__(64) void armour_track_kernel(const TrackArgs* __restrict__ ap, int B, const TrackIn* __restrict__ inputs,
                                                          ArmourTrackResult* __restrict__ state, double* __restrict__ trace, int steps) {
    track_steps<false>(ap, B, inputs, state, trace, steps);
}

// Device time of one RK4 step, measured on the MI355X (tools/track_bench.py, profiles/track_bench.json "per_step_ms": 64 lanes, 60 steps
// at 20 per launch): robust 4.32 ms -- four robust updates plus the plant --, no controller 0.78 ms (the plant alone; the nominal
// controller adds one double pass per stage), Althoff 3.17 ms (the robust update without the interval M r pass).  Lanes run side by side, so this
// holds from B = 1 to thousands (the same JSON: a whole 2.5 s rollout takes 11.09 s at B = 1 and 11.26 s at B = 4096, 4.43 / 4.51 ms per step).
// Automatic steps per launch aim at kLaunchTargetMs of device time per launch: 3 robust steps (12.9 ms), 19 plant steps (14.7 ms), 4 steps of
// the Althoff mode (12.8 ms).
constexpr double kStepMsRobust = 4.3;
constexpr double kStepMsAlthoff = 3.2;
constexpr double kStepMsPlant = 0.77;
constexpr double kLaunchTargetMs = 15.0;

// ARMOUR_TRACK_CTL_*: 0, 1, 2 and 4 (3 is unassigned, include/armour_hip.h)
bool known_controller(int32_t c) { return (c >= ARMOUR_TRACK_CTL_ROBUST && c <= ARMOUR_TRACK_CTL_NONE) || c == ARMOUR_TRACK_CTL_ALTHOFF; }
int auto_steps(int32_t c) {
    const double per_step = c == ARMOUR_TRACK_CTL_ROBUST ? kStepMsRobust : c == ARMOUR_TRACK_CTL_ALTHOFF ? kStepMsAlthoff : kStepMsPlant;
    return (int)std::fmax(1.0, std::floor(kLaunchTargetMs / per_step));
}

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
    opt->althoff_Kp[0] = opt->althoff_Kp[1] = 28.1037;   // KSI/uarmtd_robust_CBF_LLC.m:11
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
    if (!known_controller(opt->controller)) { armour_set_error("armour_track: unknown controller %d", opt->controller); return ARMOUR_EINVAL; }
    const bool althoff = opt->controller == ARMOUR_TRACK_CTL_ALTHOFF;
    if (althoff && !finite_all(opt->althoff_Kp, 2)) { armour_set_error("armour_track: non-finite althoff_Kp"); return ARMOUR_EINVAL; }
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
    if (althoff) { ta.althoff_Kp[0] = opt->althoff_Kp[0]; ta.althoff_Kp[1] = opt->althoff_Kp[1]; }
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
    if (S == 0) S = auto_steps(opt->controller);
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
        if (althoff) track_althoff_launch(stream, d_args, B, d_in, d_st, d_trace, S);
        else hipLaunchKernelGGL(armour_track_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, d_args, B, d_in, d_st, d_trace, S);
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
    if (!known_controller(controller)) return ARMOUR_EINVAL;
    return auto_steps(controller);
}
