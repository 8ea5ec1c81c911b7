// What the tree planner (tree_plan.hip) and the path shortener (path_shortcut.hip) share, one copy: the block shape, the scalar steps of the
// tree planner's rule that both apply to an edge a -> b (the wrapped joint difference, S of a prefix, one sub-segment's verdict, the node rule,
// the cut point), and the host twins' prefix with its margin.  include/armour_hip.h states the rule; everything here is the roadmap's
// geometry (roadmap_handle.h) called the same way by a kernel's lanes and by a host loop.
// The block shape and the counter hash u(seed, i, j) are also what the inverse kinematics (ik.hip) takes from here.
// The block-cooperative steps of the per-world kernels are here too (below): first / any lane with a flag, inclusive scan, argmin in the
// order key_less, the obstacle split and the owner of a work item.  path_shortcut.hip and ik.hip take all they need from here; tree_plan.hip
// takes block_first and ws_tree.hip block_any / block_scan / block_argmin, and each of the two keeps the rest inline, where the shared form
// measured slower.  The argument rules and the staging loop of all four kernels' host entries are here as well.
// The tree planner and the shortener judge by the static rule or, in their moving entries, by the window rule: both reach
// the rule and the stride of a staged obstacle through Rule<MOVING> below and nowhere else.  So do the inverse kinematics (its free test is
// Rule::config) and the workspace trees (ws_tree.hip), whose test of an axis-aligned box against one staged obstacle is Rule::box
// (DESIGN.md 4.16c).
#pragma once
#include <climits>
#include <cmath>
#include <vector>

#include "common.h"
#include "roadmap_handle.h"

namespace treeblk {

using namespace rmgeo;

constexpr int TP_BLOCK = 256;                 // four waves; a block is one world (its obstacles are staged in LDS)
constexpr int TP_WAVES = TP_BLOCK / 64;
constexpr int TP_NONE = INT_MAX;              // "no sub-segment collides" / the index of "no node"

// u(seed, i, j) of the header (the tree planner's samples, the inverse kinematics' start points): a splitmix64 finaliser of the counter, 53 bits -> [0, 1)
__host__ __device__ inline double tree_u(uint64_t seed, uint64_t i, uint64_t j) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (((i << 8) | j) + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1p-53;
}
__host__ __device__ inline double joint_diff(const RmRobot& rb, int j, double a, double b) { return rb.cont[j] ? wrap_diff(a, b) : b - a; }
// joint j of the point that ends the free prefix of m of S sub-segments of the edge a -> b
__host__ __device__ inline double cut_joint(const RmRobot& rb, int j, double a, double b, int m, int S) { return a + ((double)m / (double)S) * joint_diff(rb, j, a, b); }

// S of the edge a -> b as a prefix walks it (the argument checks keep every edge of a run below the cap; the clamp bounds the loop regardless)
__host__ __device__ inline int prefix_segments(const RmRobot& rb, const double* a, const double* b, double edge_step) {
    const int64_t S = edge_segments(rb, a, b, edge_step);
    return S > ARMOUR_TREE_MAX_SEGMENTS ? ARMOUR_TREE_MAX_SEGMENTS : (int)S;
}
// The rule a step judges a configuration by, with the staged obstacles it judges it against: the ONE place from which the two kernels and the
// two host twins reach config_free / config_free_moving and the stride of a staged obstacle.  Rule<false>: the static rule (stride
// RM_OBS_STRIDE).  Rule<true>: the window rule of armour_roadmap_check_moving (stride RM_MOV_STRIDE) with the world's mid and half.
// from(o0) is the view of the obstacles o0, o0 + 1, ...: what the obstacle split hands a lane.
// box(x, h, o, ...): the workspace trees' test, the axis-aligned box (centre x, axes e_0 e_1 e_2, half-sizes h) against staged obstacle o of
// the view, pair_separated's verdict or (full) clearance.  Rule<true>: the box over the world's window, centre x - v_o mid and every
// half-size h_i + |v_o| half -- the obstacle leaves its mid pose by at most |v_o| half in the 2-norm, which the growth along every axis
// covers; v = 0 leaves x and h as they are, bit for bit.
template <bool MOVING>
struct Rule;
__host__ __device__ inline bool box_separated(const double* x, const double* h, const double* ob, bool full, double* value) {
    const double E[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    return pair_separated(x, E, h, ob, full, value);
}
template <>
struct Rule<false> {
    static constexpr int STRIDE = RM_OBS_STRIDE;
    const double* obs;
    __host__ __device__ Rule from(int o0) const { return Rule{obs + (size_t)o0 * STRIDE}; }
    __host__ __device__ bool config(const RmRobot& rb, double (&q)[ARMOUR_MAX_FACTORS], double (&r)[ARMOUR_MAX_JOINTS], int O, bool full, double* clearance) const {
        return config_free(rb, q, r, obs, O, full, clearance);
    }
    __host__ __device__ bool box(const double (&x)[3], const double (&h)[3], int o, bool full, double* value) const {
        return box_separated(x, h, obs + (size_t)o * STRIDE, full, value);
    }
};
template <>
struct Rule<true> {
    static constexpr int STRIDE = RM_MOV_STRIDE;
    const double* obs;
    double mid, half;
    __host__ __device__ Rule from(int o0) const { return Rule{obs + (size_t)o0 * STRIDE, mid, half}; }
    __host__ __device__ bool config(const RmRobot& rb, double (&q)[ARMOUR_MAX_FACTORS], double (&r)[ARMOUR_MAX_JOINTS], int O, bool full, double* clearance) const {
        return config_free_moving(rb, q, r, obs, O, mid, half, full, clearance);
    }
    __host__ __device__ bool box(const double (&x)[3], const double (&h)[3], int o, bool full, double* value) const {
        const double* ob = obs + (size_t)o * STRIDE;
        const double* v = ob + RM_OBS_STRIDE;
        const double grow = v[3] * half;
        double xs[3], s[3];
        for (int i = 0; i < 3; i++) xs[i] = x[i] - v[i] * mid;
        for (int i = 0; i < 3; i++) s[i] = h[i] + grow;
        return box_separated(xs, s, ob, full, value);
    }
};
// what a moving kernel reads besides the static one's arguments (device pointers): velocity [W][O][3], mid / half [W]
struct MovingArgs {
    const double *velocity, *mid, *half;
};

// sub-segment s of S of the edge a -> b against O staged obstacles: the edge rule's enlarged test, verdict mode
template <class R>
__host__ __device__ inline bool segment_free(const RmRobot& rb, const double* a, const double* b, int s, int S, const R& rule, int O) {
    double q[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS];
    edge_sample(rb, a, b, s, S, q, r);
    return rule.config(rb, q, r, O, false, nullptr);
}
template <class R>
__host__ __device__ inline bool node_free(const RmRobot& rb, const double* x, const R& rule, int O) {
    double q[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS];
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q[j] = j < rb.n ? x[j] : 0.0;
#pragma unroll
    for (int l = 0; l < ARMOUR_MAX_JOINTS; l++) r[l] = 0.0;
    return rule.config(rb, q, r, O, false, nullptr);
}

// ---- the block's cooperative steps: TP_BLOCK lanes, ordered by __syncthreads() alone.  Every result is the same in all lanes.
// The per-wave words a step goes through.  Every step is: each wave's lane writes its word, BARRIER, every lane folds the TP_WAVES words,
// and a second barrier after the fold releases the words, so that the next step of any kind may write them at once.  block_argmin alone
// has a form without the second barrier (RELEASE = false), for a caller that names the barrier every lane reaches before the keys are
// written again.
struct BlockWords { int w[TP_WAVES]; };                          // first, any, scan
struct BlockKeys { double d[TP_WAVES]; int v[TP_WAVES]; };      // argmin (a kernel without an argmin has no such words)

// the smallest lane with `flag`, TP_NONE when there is none
__device__ inline int block_first(BlockWords& bw, bool flag) {
    const int t = threadIdx.x;
    const unsigned long long mask = __ballot(flag);
    if ((t & 63) == 0) bw.w[t >> 6] = mask ? (t & ~63) + __ffsll((long long)mask) - 1 : TP_NONE;
    __syncthreads();
    int f = bw.w[0];
#pragma unroll
    for (int w = 1; w < TP_WAVES; w++) f = bw.w[w] < f ? bw.w[w] : f;
    __syncthreads();
    return f;
}
// whether any lane has `flag`: the first step with less output (an OR of the waves' words)
__device__ inline bool block_any(BlockWords& bw, bool flag) {
    const int t = threadIdx.x;
    const unsigned long long mask = __ballot(flag);
    if ((t & 63) == 0) bw.w[t >> 6] = mask != 0ull;
    __syncthreads();
    int r = 0;
#pragma unroll
    for (int w = 0; w < TP_WAVES; w++) r |= bw.w[w];
    __syncthreads();
    return r != 0;
}
// inclusive sum of v over lanes 0 .. t; *total = the block's sum
__device__ inline int block_scan(BlockWords& bw, int v, int* total) {
    const int t = threadIdx.x;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if ((t & 63) >= o) x += y;
    }
    if ((t & 63) == 63) bw.w[t >> 6] = x;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < TP_WAVES; w++) {
        base += w < (t >> 6) ? bw.w[w] : 0;
        tot += bw.w[w];
    }
    __syncthreads();
    *total = tot;
    return base + x;
}
// the smallest (d, v) of the lanes' keys in the order key_less; a lane without a key passes (INFINITY, TP_NONE)
template <bool RELEASE = true>
__device__ inline void block_argmin(BlockKeys& bk, double* d, int* v) {
    const int t = threadIdx.x;
    double bd = *d;
    int bv = *v;
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o);
        const int ov = __shfl_xor(bv, o);
        if (key_less(od, ov, bd, bv)) { bd = od; bv = ov; }
    }
    if ((t & 63) == 0) { bk.d[t >> 6] = bd; bk.v[t >> 6] = bv; }
    __syncthreads();
    bd = bk.d[0]; bv = bk.v[0];
#pragma unroll
    for (int w = 1; w < TP_WAVES; w++)
        if (key_less(bk.d[w], bk.v[w], bd, bv)) { bd = bk.d[w]; bv = bk.v[w]; }
    if (RELEASE) __syncthreads();
    *d = bd;
    *v = bv;
}

// The obstacle split.  `items` >= 1 work items (sub-segments, seeds) are to be tested against O staged obstacles by TP_BLOCK lanes.  When the
// caller allows it and the items fill at most half the block, each item gets G = min(O, TP_BLOCK / items) lanes instead of one, lane t being
// lane g = t % G of item t / G and testing the obstacles [o0, o1) = [g O / G, (g + 1) O / G).  Sound because an item is free iff it is free
// of every obstacle: the intervals of an item's G lanes partition [0, O), so the OR of their hits is the item's verdict, and the longest
// lane's work shrinks from O obstacles to ceil(O / G).  Lanes stay in ascending order of item, so the first lane with a hit names the first
// item with one.  per = TP_BLOCK / G items are taken at a time, by the lanes t < per * G.
struct ObstacleSplit { int G, per, o0, o1; };
__host__ __device__ inline ObstacleSplit obstacle_split(int items, int O, bool allowed, int t) {
    int G = 1;
    if (allowed && 2 * items <= TP_BLOCK && O > 1) G = TP_BLOCK / items < O ? TP_BLOCK / items : O;
    const int per = TP_BLOCK / G, g = t % G, o0 = (g * O) / G, o1 = ((g + 1) * O) / G;
    return ObstacleSplit{G, per, o0, o1};
}
// The owner of work item `item` among n <= TP_BLOCK candidates whose items are numbered in candidate order, end[k] = one past the last item
// of candidate k (ascending; equal neighbours = a candidate without items): the number of ends <= item, which is the first k with
// end[k] > item, and n when there is none.  Nine rounds halve [0, 256] to nothing; the count bounds the loop regardless of end[].
__host__ __device__ inline int item_owner(const int* end, int n, int item) {
    int lo = 0, hi = n;
    for (int it = 0; it < 9 && lo < hi; it++) {
        const int mid = (lo + hi) >> 1;
        if (end[mid] <= item) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- the host twins' steps: the same functions in a loop.  margin (may be null): min |clearance| over the checks that decide.
template <class R>
struct HostWorld {
    const RmRobot& rb;
    R rule;
    int O;
    double edge_step;
    double* margin;

    void note(double (&q)[ARMOUR_MAX_FACTORS], double (&r)[ARMOUR_MAX_JOINTS]) const {
        double cl;
        rule.config(rb, q, r, O, true, &cl);
        *margin = std::fmin(*margin, std::fabs(cl));
    }
    bool node(const double* x) const {
        if (margin) {
            double q[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS] = {};
            for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q[j] = j < rb.n ? x[j] : 0.0;
            note(q, r);
        }
        return node_free(rb, x, rule, O);
    }
    int prefix(const double* a, const double* b, int* S_out) const {
        const int S = prefix_segments(rb, a, b, edge_step);
        *S_out = S;
        for (int s = 0; s < S; s++) {
            if (margin) {
                double q[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS];
                edge_sample(rb, a, b, s, S, q, r);
                note(q, r);
            }
            if (!segment_free(rb, a, b, s, S, rule, O)) return s;
        }
        return S;
    }
};

// ---- the host entries' shared argument rules and staging loop
// No edge of a run is longer, joint by joint, than pi (a wrapped joint) or extent[j], the caller's bound on the spread of joint j over every
// point a run can hold: that many sub-segments must fit the cap.
inline int check_joint_spans(const char* who, const RmRobot& rb, const double* extent, double edge_step) {
    for (int j = 0; j < rb.n; j++) {
        const double span = rb.cont[j] ? RM_PI : extent[j];
        if (!(std::ceil(span / edge_step) <= (double)ARMOUR_TREE_MAX_SEGMENTS)) {
            armour_set_error("%s: joint %d spans %g, more than %d sub-segments of edge_step %g", who, j, span, ARMOUR_TREE_MAX_SEGMENTS, edge_step);
            return ARMOUR_ECAPACITY;
        }
    }
    return ARMOUR_OK;
}
// the motion of a moving entry as the caller passed it: velocity [W][O][3], t_from / t_to [W] (an entry hands a null Motion* for a static call)
struct Motion {
    const double *velocity, *t_from, *t_to;
};
// The refusals that the moving entries add to those of their static forms, before a device is touched (armour_roadmap_check_moving's); fills
// mid / half [W], the two numbers per world that the rule reads, for the kernel and the host twin alike
inline int check_windows(const char* who, int32_t W, int32_t O, const Motion& mv, std::vector<double>* mid, std::vector<double>* half) {
    const double *velocity = mv.velocity, *t_from = mv.t_from, *t_to = mv.t_to;
    if ((W > 0 && O > 0 && !velocity) || (W > 0 && (!t_from || !t_to))) { armour_set_error("%s: null velocity or window", who); return ARMOUR_EINVAL; }
    if (!finite_all(velocity, (size_t)W * O * 3) || !finite_all(t_from, (size_t)W) || !finite_all(t_to, (size_t)W)) {
        armour_set_error("%s: a velocity or a window is not finite", who);
        return ARMOUR_EINVAL;
    }
    mid->resize((size_t)W);
    half->resize((size_t)W);
    for (int32_t w = 0; w < W; w++) {
        if (t_from[w] > t_to[w]) { armour_set_error("%s: world %d: t_from = %g > t_to = %g", who, w, t_from[w], t_to[w]); return ARMOUR_EINVAL; }
        (*mid)[w] = 0.5 * (t_from[w] + t_to[w]);
        (*half)[w] = 0.5 * (t_to[w] - t_from[w]);
    }
    return ARMOUR_OK;
}
// The dynamic LDS of a launch against what the device grants a block: above 48 KB a kernel has it once it asks, above the device's limit
// (with the kernel's static LDS beside it) the entry refuses instead of launching
inline int grant_dynamic_lds(const char* who, const void* kernel, size_t lds) {
    if (lds <= 48 * 1024) return ARMOUR_OK;
    int dev = 0, limit = 0;
    hipFuncAttributes fa{};
    HIPCHK(hipGetDevice(&dev));
    HIPCHK(hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    HIPCHK(hipFuncGetAttributes(&fa, kernel));
    if (lds + fa.sharedSizeBytes > (size_t)limit) {
        armour_set_error("%s: %zu B of dynamic LDS beside %zu B static, the device grants a block %d B", who, lds, (size_t)fa.sharedSizeBytes, limit);
        return ARMOUR_ECAPACITY;
    }
    HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return ARMOUR_OK;
}
// Item i of `count` (a world, or a target in world world[i]; -1: no obstacles) with its world's obstacles staged as the kernels stage them:
// run(i, the rule over the staged obstacles, their number).  MOVING: velocity [W][O][3], mid / half [W] of check_windows.
template <bool MOVING = false, class F>
inline void for_each_staged(int32_t count, int32_t O, const double* obstacles, const int32_t* world, F&& run, const double* velocity = nullptr,
                            const double* mid = nullptr, const double* half = nullptr) {
    std::vector<double> obs((size_t)O * Rule<MOVING>::STRIDE);
    for (int32_t i = 0; i < count; i++) {
        const int32_t w = world ? world[i] : i;
        Rule<MOVING> rule{obs.data()};
        if constexpr (MOVING) {
            if (w >= 0) stage_obstacles_moving(obstacles + (size_t)w * O * ARMOUR_OBS_DOUBLES, velocity + (size_t)w * O * 3, (size_t)O, obs.data());
            rule.mid = w >= 0 ? mid[w] : 0.0;
            rule.half = w >= 0 ? half[w] : 0.0;
        } else {
            if (w >= 0) stage_obstacles(obstacles + (size_t)w * O * ARMOUR_OBS_DOUBLES, (size_t)O, obs.data());
        }
        run(i, rule, w < 0 ? 0 : O);
    }
}

}  // namespace treeblk
