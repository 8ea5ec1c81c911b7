// The pieces of the path audit (include/armour_hip.h, armour_path_audit*): the plans as the rule reads them, the speed bound, the
// sub-intervals of a piece, the configuration at a sub-interval's midpoint and what an audit's work item does around its free-test (decode,
// the three-state decision, the record).  Shared by path_audit.hip and self_check.hip; the host side of an audit is in audit_host.h.
#pragma once
#include <cstdint>

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

constexpr int32_t PA_NO_HIT = INT32_MAX;      // first_hit[p] before any sample test collided

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

// Work item `item` of an audit kernel: sub-interval *s of the *S of piece *p = item_piece[item].  False when the item is settled already:
// in verdict mode (full = false) an item behind a recorded hit of its piece can change neither the minimum nor the verdict.
__device__ inline bool audit_item(int64_t item, const int32_t* __restrict__ item_piece, const int64_t* __restrict__ piece_off, const int32_t* first_hit,
                                  bool full, int* p, int64_t* s, int64_t* S) {
    *p = item_piece[item];
    *s = item - piece_off[*p];
    *S = piece_off[*p + 1] - piece_off[*p];
    return full || !((int64_t)__atomic_load_n(&first_hit[*p], __ATOMIC_RELAXED) < *s);
}

// The state of an item from its two free-tests: 0 the tube test separates, 1 the sample test collides, 2 neither.  sample_free(full) is the
// test with the boxes as they are (full: without an early exit, leaving its clearance), tube_free() the test with the enlarged boxes.
// full: sample first, then tube; otherwise tube first and the sample test only for an item the tube test does not settle.
template <class Tube, class Sample>
__host__ __device__ inline int audit_state(bool full, const Tube& tube_free, const Sample& sample_free) {
    if (full) {
        if (!sample_free(true)) return 1;
        return tube_free() ? 0 : 2;
    }
    if (tube_free()) return 0;   // enlarged boxes separated: the boxes themselves are
    return sample_free(false) ? 2 : 1;
}

// The record of an item's state in its piece's merge words (first_hit holds PA_NO_HIT and undecided 0 before the first item): a colliding
// item lowers first_hit to its sub-interval (an integer minimum, atomic on the device), an undecided one stores 1 (every writer writes 1).
__host__ __device__ inline void audit_record(int state, int64_t s, int32_t* first_hit, uint8_t* undecided) {
    if (state == 1) {
#ifdef __HIP_DEVICE_COMPILE__
        atomicMin(first_hit, (int32_t)s);
#else
        if ((int32_t)s < *first_hit) *first_hit = (int32_t)s;
#endif
    } else if (state == 2) {
        *undecided = 1;
    }
}

}  // namespace rmgeo
