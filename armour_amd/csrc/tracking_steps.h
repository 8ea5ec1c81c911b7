// The tracking simulator's device code: what a launch reads (TrackArgs, TrackIn), one evaluation of the closed loop and the RK4 steps
// of one launch -- shared by tracking.hip (the kernel of the robust, nominal and passive modes, and the host entry) and tracking_althoff.hip
// (the kernel of ARMOUR_TRACK_CTL_ALTHOFF).  Two units on purpose: with both kernels in one object the compiler builds the first differently
// (10384 B of scratch per lane instead of 7696 B, same source), so the existing modes' kernel stays alone in tracking.o, as it was.
#pragma once
#include "bezier.h"
#include "common.h"
#include "controller_core.h"

namespace trk {

using namespace ctl;
constexpr int MF = ARMOUR_MAX_FACTORS;

struct TrackArgs {
    Model<double> md;
    Model<Itv> imd;
    double Kr[MF];
    double alpha, V_max, r_norm_threshold;
    double althoff_Kp[2];
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
// kAlthoff: the instantiation of ARMOUR_TRACK_CTL_ALTHOFF alone (tracking_althoff.hip) -- the other three modes' kernel does not hold the
// branch.  e_acc = 0 at every stage, as in the reference's runs (controller_core.h).
template <bool kAlthoff>
CTL_HD CTL_FLATTEN bool closed_loop(const TrackArgs& a, const Model<double>& mt, const TrackIn& in, double t, const double* q, const double* qd,
                                    double* qdd, double* u, double* v, double* qr, double* qdr, double* V) {
    const int n = a.md.n;
    double qddr[MF];
    reference(in, n, a.duration, t, qr, qdr, qddr);
    bool ok = true;
    if (kAlthoff) {
        const double Ki[2] = {0.0, 0.0};
        double tau[MF];
        ok = althoff_update(a.md, a.imd, a.Kr, a.althoff_Kp, Ki, 0.0, q, qd, qr, qdr, qddr, u, tau, v);
    } else if (a.controller == ARMOUR_TRACK_CTL_ROBUST) {
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

template <bool kAlthoff>
__device__ CTL_FLATTEN void track_steps(const TrackArgs* __restrict__ ap, int B, const TrackIn* __restrict__ inputs, ArmourTrackResult* __restrict__ state,
                                        double* __restrict__ trace, int steps) {
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
        bool ok = closed_loop<kAlthoff>(a, mt, in, t, R.q, R.qd, kqd, u, v, qr, qdr, &V);
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
            ok = closed_loop<kAlthoff>(a, mt, in, t + ch, zq, zqd, kqd, us, vs, qrs, qdrs, &Vs);
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
// launches armour_track_althoff_kernel (tracking_althoff.hip) on `stream`: `steps` steps for each of B rollouts
void track_althoff_launch(hipStream_t stream, const TrackArgs* args, int B, const TrackIn* inputs, ArmourTrackResult* state, double* trace, int steps);

}  // namespace trk
