// The roadmap's node rule (include/armour_hip.h, "roadmap high-level planner"): forward kinematics of the link boxes and the 15-plane
// separation test of a link box and an obstacle, written once as __host__ __device__ code.  Shared by the roadmap check (roadmap.hip) and
// the path audit (path_audit.hip), so that both judge a configuration by the same arithmetic; tests/test_roadmap.py restates it in numpy.
#pragma once
#include <cmath>
#include <cstring>

#include "common.h"

namespace rmgeo {

constexpr int RM_OBS_STRIDE = 27;             // doubles per staged obstacle: Z[12], then 3 x {m[3], |m.g_rest|, |m|} of the obstacle pairs
constexpr double RM_DEGENERATE = 1e-18;       // a normal m = a x b is skipped when |m|^2 <= RM_DEGENERATE |a|^2 |b|^2
constexpr double RM_PI = 3.141592653589793;
constexpr double RM_TWO_PI = 6.283185307179586;

// The robot as the rule reads it: frames, link boxes and the displacement bounds rho (passed by value as a kernel argument, ~2.3 KB).
struct RmRobot {
    int J, n;
    int axis[ARMOUR_MAX_JOINTS];                      // signed 1..3, 0 = fixed
    int cont[ARMOUR_MAX_FACTORS];
    double T0[ARMOUR_MAX_JOINTS][9];                  // rpy(rots_l), row-major
    double trans[ARMOUR_MAX_JOINTS][3];
    double c[ARMOUR_MAX_JOINTS][3], h[ARMOUR_MAX_JOINTS][3];
    double rho[ARMOUR_MAX_FACTORS][ARMOUR_MAX_JOINTS];  // rho[j][l], j actuated, l >= j (0 otherwise)
};

__host__ __device__ inline double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__host__ __device__ inline void cross3(const double* a, const double* b, double* m) {
    m[0] = a[1] * b[2] - a[2] * b[1];
    m[1] = a[2] * b[0] - a[0] * b[2];
    m[2] = a[0] * b[1] - a[1] * b[0];
}
// C = A B (3x3 row-major), sums left to right -- the order tests/test_roadmap.py restates
__host__ __device__ inline void matmul3(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
__host__ __device__ inline double wrap_diff(double a, double b) {
    const double d = b - a;
    return d - RM_TWO_PI * floor((d + RM_PI) / RM_TWO_PI);
}

// Obstacle-only part of the rule: the three obstacle x obstacle normals (unnormalised), their |m . g_rest| and |m| (|m| = 0: skipped).
__host__ __device__ inline void obstacle_normals(const double* Z, double* out /* [15] */) {
    const double* g[3] = {Z + 3, Z + 6, Z + 9};
    const int pa[3] = {0, 0, 1}, pb[3] = {1, 2, 2}, rest[3] = {2, 1, 0};
    for (int p = 0; p < 3; p++) {
        double* o = out + 5 * p;
        cross3(g[pa[p]], g[pb[p]], o);
        const double m2 = dot3(o, o);
        if (m2 <= RM_DEGENERATE * (dot3(g[pa[p]], g[pa[p]]) * dot3(g[pb[p]], g[pb[p]]))) {
            o[0] = o[1] = o[2] = o[3] = o[4] = 0.0;
        } else {
            o[3] = fabs(dot3(o, g[rest[p]]));
            o[4] = sqrt(m2);
        }
    }
}

// `count` obstacles as the kernels stage them in LDS, on the host: staged[o][RM_OBS_STRIDE] = Z[12], then the obstacle's normals
inline void stage_obstacles(const double* obstacles, size_t count, double* staged) {
    for (size_t o = 0; o < count; o++) {
        std::memcpy(staged + o * RM_OBS_STRIDE, obstacles + o * ARMOUR_OBS_DOUBLES, ARMOUR_OBS_DOUBLES * sizeof(double));
        obstacle_normals(obstacles + o * ARMOUR_OBS_DOUBLES, staged + o * RM_OBS_STRIDE + ARMOUR_OBS_DOUBLES);
    }
}

// stage_obstacles on the device: a block of BLOCK lanes stages its world's O obstacles Zw into LDS, s_obs [O][RM_OBS_STRIDE], and meets at the barrier
template <int BLOCK>
__device__ inline void stage_obstacles_lds(const double* __restrict__ Zw, int O, double* s_obs) {
    for (int i = threadIdx.x; i < O * ARMOUR_OBS_DOUBLES; i += BLOCK)
        s_obs[(i / ARMOUR_OBS_DOUBLES) * RM_OBS_STRIDE + i % ARMOUR_OBS_DOUBLES] = Zw[i];
    for (int o = threadIdx.x; o < O; o += BLOCK) obstacle_normals(Zw + (size_t)o * ARMOUR_OBS_DOUBLES, s_obs + (size_t)o * RM_OBS_STRIDE + 12);
    __syncthreads();
}

// One link box (centre x, unit axes u[k] = column k of R, half-sizes s) against one staged obstacle.  full = false: true as soon as
// one plane separates (value > 0; the sign of the numerator is the sign of the value).  full = true: *value = the pair's clearance.
__host__ __device__ inline bool pair_separated(const double* x, const double (*u)[3], const double* s, const double* ob, bool full,
                                               double* value) {
    const double* Z = ob;
    const double* g[3] = {Z + 3, Z + 6, Z + 9};
    double d[3] = {x[0] - Z[0], x[1] - Z[1], x[2] - Z[2]};
    double best = -INFINITY;
    // obstacle x obstacle
#pragma unroll
    for (int p = 0; p < 3; p++) {
        const double* m = ob + 12 + 5 * p;
        if (m[4] == 0.0) continue;
        const double num = fabs(dot3(m, d)) - (m[3] + ((s[0] * fabs(dot3(m, u[0])) + s[1] * fabs(dot3(m, u[1]))) + s[2] * fabs(dot3(m, u[2]))));
        if (!full) {
            if (num > 0.0) return true;
        } else {
            best = fmax(best, num / m[4]);
        }
    }
    // link x link: the normal is the third axis
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double num = fabs(dot3(u[k], d)) - (((fabs(dot3(u[k], g[0])) + fabs(dot3(u[k], g[1]))) + fabs(dot3(u[k], g[2]))) + s[k]);
        if (!full) {
            if (num > 0.0) return true;
        } else {
            best = fmax(best, num);
        }
    }
    // obstacle x link
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double ga2 = dot3(g[a], g[a]);
        const int a1 = a == 0 ? 1 : 0, a2 = a == 2 ? 1 : 2;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            double m[3];
            cross3(g[a], u[k], m);
            const double m2 = dot3(m, m);
            if (m2 <= RM_DEGENERATE * ga2) continue;
            const int k1 = k == 0 ? 1 : 0, k2 = k == 2 ? 1 : 2;
            const double num = fabs(dot3(m, d)) - ((fabs(dot3(m, g[a1])) + fabs(dot3(m, g[a2]))) + (s[k1] * fabs(dot3(m, u[k1])) + s[k2] * fabs(dot3(m, u[k2]))));
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

// One step along the chain: R, p = the frame of link l - 1 on entry, of link l on return; ql = the angle of joint l (read only when it is actuated).
__host__ __device__ inline void link_frame(const RmRobot& rb, int l, double ql, double* R, double* p) {
    double t[3], A[9];
    for (int i = 0; i < 3; i++) t[i] = (R[3 * i] * rb.trans[l][0] + R[3 * i + 1] * rb.trans[l][1]) + R[3 * i + 2] * rb.trans[l][2];
    for (int i = 0; i < 3; i++) p[i] = p[i] + t[i];
    matmul3(R, rb.T0[l], A);
    const int ax = rb.axis[l];
    if (ax != 0 && l < rb.n) {
        const double c = cos(ql), sn = ax > 0 ? sin(ql) : -sin(ql);
        const int e = ax > 0 ? ax : -ax;
        // Rot about x / y / z: {1,0,0; 0,c,-s; 0,s,c}, {c,0,s; 0,1,0; -s,0,c}, {c,-s,0; s,c,0; 0,0,1}
        const double Q[9] = {e == 1 ? 1.0 : c,          e == 3 ? -sn : 0.0,       e == 2 ? sn : 0.0,
                             e == 3 ? sn : 0.0,         e == 2 ? 1.0 : c,         e == 1 ? -sn : 0.0,
                             e == 2 ? -sn : 0.0,        e == 1 ? sn : 0.0,        e == 3 ? 1.0 : c};
        matmul3(A, Q, R);
    } else {
        for (int i = 0; i < 9; i++) R[i] = A[i];
    }
}

// Link l's box in the frame R, p of link l: centre x and unit axes u[k] = column k of R (the half-sizes are the caller's)
__host__ __device__ inline void link_box(const RmRobot& rb, int l, const double* R, const double* p, double* x, double (*u)[3]) {
    for (int i = 0; i < 3; i++) x[i] = p[i] + ((R[3 * i] * rb.c[l][0] + R[3 * i + 1] * rb.c[l][1]) + R[3 * i + 2] * rb.c[l][2]);
    for (int k = 0; k < 3; k++) {
        u[k][0] = R[k]; u[k][1] = R[3 + k]; u[k][2] = R[6 + k];
    }
}

// The rule for one configuration q with per-link enlargement r[l] (all zero for a node) against O staged obstacles (stride
// RM_OBS_STRIDE); q and r are consumed (shifted).  full = false: returns at the first colliding pair.  full = true: *clearance = min over pairs of the pair clearance.
__host__ __device__ inline bool config_free(const RmRobot& rb, double (&q)[ARMOUR_MAX_FACTORS], double (&r)[ARMOUR_MAX_JOINTS], const double* obs, int O, bool full,
                                            double* clearance) {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
    double cl = INFINITY;
    bool free_ = true;
    for (int l = 0; l < rb.J; l++) {
        link_frame(rb, l, q[0], R, p);
        double x[3], u[3][3], s[3];
        const double rl = r[0];
        // shift q and r down one joint: link l always reads entry 0, so neither array is indexed at run time (no scratch memory)
#pragma unroll
        for (int j = 0; j + 1 < ARMOUR_MAX_FACTORS; j++) q[j] = q[j + 1];
#pragma unroll
        for (int j = 0; j + 1 < ARMOUR_MAX_JOINTS; j++) r[j] = r[j + 1];
        link_box(rb, l, R, p, x, u);
        for (int k = 0; k < 3; k++) s[k] = rb.h[l][k] + rl;
        for (int o = 0; o < O; o++) {
            double v;
            const bool sep = pair_separated(x, u, s, obs + (size_t)o * RM_OBS_STRIDE, full, &v);
            if (!full) {
                if (!sep) return false;
            } else {
                cl = fmin(cl, v);
                free_ = free_ && sep;
            }
        }
    }
    if (full) *clearance = cl;
    return free_;
}

// ---- obstacles in linear motion (include/armour_hip.h, armour_path_audit_moving).  New names beside the static rule: pair_separated,
// config_free and stage_obstacles* above are what the static audit and the roadmap compile, untouched.
constexpr int RM_MOV_STRIDE = RM_OBS_STRIDE + 4;   // doubles per staged moving obstacle: the static 27 (pose at world time 0), then v[3], |v|_2

__host__ __device__ inline double velocity_norm(const double* v) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

// stage_obstacles for moving obstacles on the host: staged[o][RM_MOV_STRIDE] from obstacles [count][12] and velocity [count][3]
inline void stage_obstacles_moving(const double* obstacles, const double* velocity, size_t count, double* staged) {
    for (size_t o = 0; o < count; o++) {
        double* st = staged + o * RM_MOV_STRIDE;
        std::memcpy(st, obstacles + o * ARMOUR_OBS_DOUBLES, ARMOUR_OBS_DOUBLES * sizeof(double));
        obstacle_normals(obstacles + o * ARMOUR_OBS_DOUBLES, st + ARMOUR_OBS_DOUBLES);
        for (int i = 0; i < 3; i++) st[RM_OBS_STRIDE + i] = velocity[3 * o + i];
        st[RM_OBS_STRIDE + 3] = velocity_norm(velocity + 3 * o);
    }
}

// the same on the device: a block of BLOCK lanes stages its world's O obstacles Zw and velocities Vw into LDS, s_obs [O][RM_MOV_STRIDE], and meets at the barrier
template <int BLOCK>
__device__ inline void stage_obstacles_moving_lds(const double* __restrict__ Zw, const double* __restrict__ Vw, int O, double* s_obs) {
    for (int i = threadIdx.x; i < O * ARMOUR_OBS_DOUBLES; i += BLOCK)
        s_obs[(i / ARMOUR_OBS_DOUBLES) * RM_MOV_STRIDE + i % ARMOUR_OBS_DOUBLES] = Zw[i];
    for (int o = threadIdx.x; o < O; o += BLOCK) {
        double* st = s_obs + (size_t)o * RM_MOV_STRIDE;
        obstacle_normals(Zw + (size_t)o * ARMOUR_OBS_DOUBLES, st + 12);
        const double* v = Vw + (size_t)o * 3;
        st[RM_OBS_STRIDE] = v[0]; st[RM_OBS_STRIDE + 1] = v[1]; st[RM_OBS_STRIDE + 2] = v[2];
        st[RM_OBS_STRIDE + 3] = velocity_norm(v);
    }
    __syncthreads();
}

// config_free against obstacles staged with stride RM_MOV_STRIDE, each at its pose of world time tau: the pair test of link box l and
// obstacle o with the box centre x - v_o tau (A meets B + d exactly when A - d meets B) and every half-size h_l + (r_l + |v_o| half).
// half = 0 with r = 0 is the sample test; the tube test passes the sub-interval's half width, over which the obstacle leaves its
// midpoint pose by at most |v_o| half.  q and r are consumed as config_free consumes them.
__host__ __device__ inline bool config_free_moving(const RmRobot& rb, double (&q)[ARMOUR_MAX_FACTORS], double (&r)[ARMOUR_MAX_JOINTS], const double* obs, int O,
                                                   double tau, double half, bool full, double* clearance) {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
    double cl = INFINITY;
    bool free_ = true;
    for (int l = 0; l < rb.J; l++) {
        link_frame(rb, l, q[0], R, p);
        double x[3], u[3][3];
        const double rl = r[0];
#pragma unroll
        for (int j = 0; j + 1 < ARMOUR_MAX_FACTORS; j++) q[j] = q[j + 1];
#pragma unroll
        for (int j = 0; j + 1 < ARMOUR_MAX_JOINTS; j++) r[j] = r[j + 1];
        link_box(rb, l, R, p, x, u);
        for (int o = 0; o < O; o++) {
            const double* ob = obs + (size_t)o * RM_MOV_STRIDE;
            const double* v = ob + RM_OBS_STRIDE;
            const double grow = rl + v[3] * half;
            double xs[3], s[3], val;
            for (int i = 0; i < 3; i++) xs[i] = x[i] - v[i] * tau;
            for (int k = 0; k < 3; k++) s[k] = rb.h[l][k] + grow;
            const bool sep = pair_separated(xs, u, s, ob, full, &val);
            if (!full) {
                if (!sep) return false;
            } else {
                cl = fmin(cl, val);
                free_ = free_ && sep;
            }
        }
    }
    if (full) *clearance = cl;
    return free_;
}

inline void fill_rm_robot(const ArmourRobot* robot, const uint8_t* continuous, RmRobot* rb) {
    std::memset(rb, 0, sizeof(*rb));
    rb->J = robot->num_joints;
    rb->n = robot->num_factors;
    for (int l = 0; l < rb->J; l++) {
        rb->axis[l] = robot->axes[l];
        // rpy(roll, pitch, yaw), the product of armour_amd/robot_geometry.py rpy_matrix
        const double cr = cos(robot->rots[3 * l]), sr = sin(robot->rots[3 * l]), cp = cos(robot->rots[3 * l + 1]), sp = sin(robot->rots[3 * l + 1]),
                     cy = cos(robot->rots[3 * l + 2]), sy = sin(robot->rots[3 * l + 2]);
        const double T0[9] = {cp * cy, -cp * sy, sp,
                              cr * sy + cy * sp * sr, cr * cy - sp * sr * sy, -cp * sr,
                              sr * sy - cr * cy * sp, cy * sr + cr * sp * sy, cp * cr};
        std::memcpy(rb->T0[l], T0, sizeof(T0));
        for (int i = 0; i < 3; i++) {
            rb->trans[l][i] = robot->trans[3 * l + i];
            rb->c[l][i] = robot->link_zonotope_center[3 * l + i];
            rb->h[l][i] = robot->link_zonotope_generators[3 * l + i];
        }
    }
    for (int j = 0; j < rb->n; j++) rb->cont[j] = continuous ? (continuous[j] != 0) : (robot->continuous[j] != 0);
    for (int j = 0; j < rb->n; j++)
        for (int l = j; l < rb->J; l++) {
            double acc = 0.0;
            for (int i = j + 1; i <= l; i++) acc += std::sqrt(dot3(rb->trans[i], rb->trans[i]));
            rb->rho[j][l] = acc + std::sqrt(dot3(rb->c[l], rb->c[l])) + std::sqrt(dot3(rb->h[l], rb->h[l]));
        }
}

}  // namespace rmgeo
