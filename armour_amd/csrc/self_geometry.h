// The self-collision pair rule (include/armour_hip.h, "self-collision checks"): the 15-axis separation test of two link boxes and the rule
// for one configuration, one first link at a time, written once as __host__ __device__ code.  Shared by the kernels of self_check.hip, their
// host twins and the host-checked edges of armour_roadmap_plan; tests/test_self_check.py restates it in numpy.
#pragma once
#include "roadmap_geometry.h"

namespace rmgeo {

// Box a (centre xa, unit axes ua[k], half-sizes sa) against box b.  full = false: true as soon as one axis separates (numerator > 0).
// full = true: *value = the pair's clearance, no early exit.  The box whose axis is the normal contributes its own half-size on that axis
// (the axes are orthonormal), and a cross product's two parents contribute nothing, as in pair_separated.
__host__ __device__ inline bool box_pair_separated(const double* xa, const double (*ua)[3], const double* sa, const double* xb, const double (*ub)[3],
                                                   const double* sb, bool full, double* value) {
    const double d[3] = {xb[0] - xa[0], xb[1] - xa[1], xb[2] - xa[2]};
    double best = -INFINITY;
    // the face normals of a
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double num = fabs(dot3(ua[k], d)) - (sa[k] + ((sb[0] * fabs(dot3(ua[k], ub[0])) + sb[1] * fabs(dot3(ua[k], ub[1]))) + sb[2] * fabs(dot3(ua[k], ub[2]))));
        if (!full) {
            if (num > 0.0) return true;
        } else {
            best = fmax(best, num);
        }
    }
    // the face normals of b
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double num = fabs(dot3(ub[k], d)) - (((sa[0] * fabs(dot3(ub[k], ua[0])) + sa[1] * fabs(dot3(ub[k], ua[1]))) + sa[2] * fabs(dot3(ub[k], ua[2]))) + sb[k]);
        if (!full) {
            if (num > 0.0) return true;
        } else {
            best = fmax(best, num);
        }
    }
    // edge of a x edge of b
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int i1 = i == 0 ? 1 : 0, i2 = i == 2 ? 1 : 2;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            double m[3];
            cross3(ua[i], ub[k], m);
            const double m2 = dot3(m, m);
            if (m2 <= RM_DEGENERATE) continue;
            const int k1 = k == 0 ? 1 : 0, k2 = k == 2 ? 1 : 2;
            const double num = fabs(dot3(m, d)) - ((sa[i1] * fabs(dot3(m, ua[i1])) + sa[i2] * fabs(dot3(m, ua[i2]))) + (sb[k1] * fabs(dot3(m, ub[k1])) + sb[k2] * fabs(dot3(m, ub[k2]))));
            if (!full) {
                if (num > 0.0) return true;
            } else {
                best = fmax(best, num / sqrt(m2));
            }
        }
    }
    if (full) *value = best;
    return best > 0.0;
}

// The rule for the pairs (a, b) of ONE first link a at configuration q, with joint j free to move delta[j] about q[j] (all zero: the exact
// test).  on[b] != 0 lists pair (a, b) (row a of the effective table: a < b, both links with a half-size), shrink[b] its shrink (row a;
// shrink may be null: zeros).  q is consumed (shifted).  The chain runs once; box a is kept when the chain passes it, and every listed b
// is tested as the chain reaches it, so no array is indexed by a lane's own value (no scratch memory).
// full = false: returns false at the first colliding pair, *which = its b (-1 when the row is free).
// full = true: *clearance = min over the row's pairs (+inf for an empty row), *which = the b of the first minimum (-1 for an empty row).
__host__ __device__ inline bool self_row_free(const RmRobot& rb, int a, double (&q)[ARMOUR_MAX_FACTORS], const double (&delta)[ARMOUR_MAX_FACTORS],
                                              const uint8_t* on, const double* shrink, bool full, double* clearance, int* which) {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
    double xa[3] = {0, 0, 0}, ua[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, sa[3] = {0, 0, 0};
    double cl = INFINITY;
    int wb = -1;
    bool free_ = true;
    for (int l = 0; l < rb.J; l++) {
        link_frame(rb, l, q[0], R, p);
#pragma unroll
        for (int j = 0; j + 1 < ARMOUR_MAX_FACTORS; j++) q[j] = q[j + 1];
        if (l < a) continue;
        double x[3], u[3][3];
        link_box(rb, l, R, p, x, u);
        if (l == a) {
            for (int i = 0; i < 3; i++) {
                xa[i] = x[i];
                sa[i] = rb.h[l][i];
                for (int k = 0; k < 3; k++) ua[i][k] = u[i][k];
            }
            continue;
        }
        if (!on[l]) continue;
        // r_ab = sum over actuated j in a+1..l of rho_{j,l} delta_j, left to right
        double r = 0.0;
#pragma unroll
        for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) r = (j > a && j <= l && j < rb.n) ? r + rb.rho[j][l] * delta[j] : r;
        const double sh = shrink ? shrink[l] : 0.0;
        double sb[3];
        for (int k = 0; k < 3; k++) sb[k] = fmax(rb.h[l][k] - sh, 0.0) + r;
        double v;
        const bool sep = box_pair_separated(xa, ua, sa, x, u, sb, full, &v);
        if (!full) {
            if (!sep) { *which = l; return false; }
        } else {
            if (v < cl) { cl = v; wb = l; }
            free_ = free_ && sep;
        }
    }
    if (full) *clearance = cl;
    *which = wb;
    return free_;
}

// The pair table as the rule reads it: on[a][b] = 1 iff the pair is tested (a < b, listed, both links with a non-zero half-size),
// shrink [J][J] (zeros without one); rows = 1 + the last first link with a pair (the a's worth a work item).
struct SelfTable {
    int J = 0, rows = 0;
    uint8_t on[ARMOUR_MAX_JOINTS * ARMOUR_MAX_JOINTS];
    double shrink[ARMOUR_MAX_JOINTS * ARMOUR_MAX_JOINTS];
};

inline bool link_has_size(const RmRobot& rb, int l) { return rb.h[l][0] != 0.0 || rb.h[l][1] != 0.0 || rb.h[l][2] != 0.0; }

// pairs [J][J] (null: every b - a >= 2), shrink [J][J] (null: zeros); only a < b is read
inline void fill_self_table(const RmRobot& rb, const uint8_t* pairs, const double* shrink, SelfTable* tb) {
    const int J = rb.J;
    tb->J = J;
    tb->rows = 0;
    std::memset(tb->on, 0, sizeof(tb->on));
    std::memset(tb->shrink, 0, sizeof(tb->shrink));
    for (int a = 0; a < J; a++)
        for (int b = a + 1; b < J; b++) {
            const bool listed = pairs ? pairs[a * J + b] != 0 : b - a >= 2;
            if (!listed || !link_has_size(rb, a) || !link_has_size(rb, b)) continue;
            tb->on[a * J + b] = 1;
            tb->shrink[a * J + b] = shrink ? shrink[a * J + b] : 0.0;
            tb->rows = a + 1;
        }
}

// One configuration on the host: every row in turn.  full = false: *worst = a J + b of the first colliding pair (-1: free).
// full = true: *clearance = min over rows, *worst = the pair of the first minimum (-1 with no pair).
inline bool self_config_free(const RmRobot& rb, const SelfTable& tb, const double* qin, const double (&delta)[ARMOUR_MAX_FACTORS], bool full, double* clearance,
                             int* worst) {
    double cl = INFINITY;
    int wp = -1;
    bool free_ = true;
    for (int a = 0; a < tb.rows; a++) {
        double q[ARMOUR_MAX_FACTORS], v = INFINITY;
        int b = -1;
        for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q[j] = j < rb.n ? qin[j] : 0.0;
        const bool ok = self_row_free(rb, a, q, delta, tb.on + a * tb.J, tb.shrink + a * tb.J, full, &v, &b);
        if (!full) {
            if (!ok) { if (worst) *worst = a * tb.J + b; return false; }
        } else {
            if (b >= 0 && v < cl) { cl = v; wp = a * tb.J + b; }
            free_ = free_ && ok;
        }
    }
    if (full && clearance) *clearance = cl;
    if (worst) *worst = wp;
    return free_;
}

// Sub-segment s of S of the edge a -> b: midpoint configuration and how far every joint is from it inside the sub-segment.
__host__ __device__ inline void self_edge_sample(const RmRobot& rb, const double* a, const double* b, int64_t s, int64_t S, double (&q)[ARMOUR_MAX_FACTORS],
                                                 double (&delta)[ARMOUR_MAX_FACTORS]) {
    const double t = (double)(2 * s + 1) / (double)(2 * S);
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) {
        const double D = j < rb.n ? (rb.cont[j] ? wrap_diff(a[j], b[j]) : b[j] - a[j]) : 0.0;
        q[j] = j < rb.n ? a[j] + t * D : 0.0;
        delta[j] = fabs(D) / (double)(2 * S);
    }
}

// S of the edge a -> b: max(1, ceil(max_j |D_j| / edge_step)), the roadmap's
__host__ __device__ inline int64_t edge_segments(const RmRobot& rb, const double* a, const double* b, double edge_step) {
    double mx = 0.0;
    for (int j = 0; j < rb.n; j++) mx = fmax(mx, fabs(rb.cont[j] ? wrap_diff(a[j], b[j]) : b[j] - a[j]));
    const double S = ceil(mx / edge_step);
    return S < 1.0 ? 1 : (int64_t)S;
}

// the self edge rule on the host: every sub-segment's midpoint with box b of every listed pair enlarged by r_ab
inline bool self_edge_free(const RmRobot& rb, const SelfTable& tb, double edge_step, const double* a, const double* b) {
    const int64_t S = edge_segments(rb, a, b, edge_step);
    double q[ARMOUR_MAX_FACTORS], delta[ARMOUR_MAX_FACTORS];
    for (int64_t s = 0; s < S; s++) {
        self_edge_sample(rb, a, b, s, S, q, delta);
        if (!self_config_free(rb, tb, q, delta, false, nullptr, nullptr)) return false;
    }
    return true;
}

}  // namespace rmgeo
