// The pieces of the path audit (include/armour_hip.h, armour_path_audit*): the plans as the rule reads them, the speed bound, the
// sub-intervals of a piece and the configuration at a sub-interval's midpoint.  Shared by path_audit.hip and self_check.hip.
#pragma once
#include "bezier.h"
#include "common.h"
#include "roadmap_geometry.h"

namespace rmgeo {

// The plans as the rule reads them, piece-major [P][n] (device copies of the caller's arrays), and the windows.
struct PaPieces {
    const double *q0, *qd0, *qdd0, *k, *ta, *tb, *tube;   // tube may be null: zeros
    double k_range[ARMOUR_MAX_FACTORS];
    double duration, step;
};

// v_j = max_i |5 (P_{i+1,j} - P_{i,j})| / duration over the control points P0 = q0, P1 = q0 + a/5, P2 = q0 + 2a/5 + b/20, P3 = P4 = P5 = q0 + k_range k
// (a = qd0 duration, b = qdd0 duration^2, as armour_desired_trajectory forms them): a bound of |qd_j| on the whole curve.
__host__ __device__ inline double speed_bound(double q0, double qd0, double qdd0, double ka, double D) {
    const double a = qd0 * D, b = qdd0 * D * D;
    const double P1 = q0 + a / 5, P2 = q0 + (2 * a) / 5 + b / 20, P3 = q0 + ka;
    return fmax(fmax(fabs(5 * (P1 - q0)), fabs(5 * (P2 - P1))), fabs(5 * (P3 - P2))) / D;
}

// S of piece p: max(1, ceil(max_j v_j (tb - ta) / step))
__host__ __device__ inline double piece_intervals(const RmRobot& rb, const PaPieces& pc, int64_t p) {
    const double w = pc.tb[p] - pc.ta[p];
    double mx = 0.0;
    for (int j = 0; j < rb.n; j++) {
        const size_t x = (size_t)p * rb.n + j;
        mx = fmax(mx, speed_bound(pc.q0[x], pc.qd0[x], pc.qdd0[x], pc.k_range[j] * pc.k[x], pc.duration) * w);
    }
    const double S = ceil(mx / pc.step);
    return S < 1.0 ? 1.0 : S;
}

// Sub-interval s of S of piece p: its midpoint time, the configuration there and how far every joint of a configuration within the tube
// can be from it inside the sub-interval, dev_j = v_j (tb - ta) / (2S) + e_j.
__host__ __device__ inline double piece_point(const RmRobot& rb, const PaPieces& pc, int64_t p, int64_t s, int64_t S, double (&q)[ARMOUR_MAX_FACTORS],
                                              double (&dev)[ARMOUR_MAX_FACTORS]) {
    const double ta = pc.ta[p], w = pc.tb[p] - ta, D = pc.duration;
    const double t = ta + ((double)(2 * s + 1) * w) / (double)(2 * S);
    const double half = w / (double)(2 * S), u = t / D;
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) {
        if (j < rb.n) {
            const size_t x = (size_t)p * rb.n + j;
            const double q0 = pc.q0[x], qd0 = pc.qd0[x], qdd0 = pc.qdd0[x], ka = pc.k_range[j] * pc.k[x];
            q[j] = bez::q_des(q0, qd0 * D, qdd0 * D * D, ka, u);
            dev[j] = speed_bound(q0, qd0, qdd0, ka, D) * half + (pc.tube ? pc.tube[x] : 0.0);
        } else {
            q[j] = 0.0;
            dev[j] = 0.0;
        }
    }
    return t;
}

// The same with the per-link enlargement of the world audit's tube test, r_l = sum over actuated j <= l of rho_{j,l} dev_j.
__host__ __device__ inline double piece_sample(const RmRobot& rb, const PaPieces& pc, int64_t p, int64_t s, int64_t S, double (&q)[ARMOUR_MAX_FACTORS],
                                               double (&r)[ARMOUR_MAX_JOINTS]) {
    double dev[ARMOUR_MAX_FACTORS];
    const double t = piece_point(rb, pc, p, s, S, q, dev);
#pragma unroll
    for (int l = 0; l < ARMOUR_MAX_JOINTS; l++) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < ARMOUR_MAX_FACTORS && j <= l; j++) acc = j < rb.n ? acc + rb.rho[j][l] * dev[j] : acc;
        r[l] = acc;
    }
    return t;
}

}  // namespace rmgeo
