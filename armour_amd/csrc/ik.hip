// Batched collision-aware inverse kinematics for workspace goals (include/armour_hip.h, armour_ik): N targets x S seeds in ONE launch, a
// block per target.  An item (target, seed) is a damped least-squares iteration on the end-effector point; a converged item is judged by the
// node rule (armour_ik_moving: the window rule, through tree_block.h's Rule<MOVING>) against its target's world, and the free item nearest to q_ref is picked.  Everything geometric is the roadmap's, reused as it
// stands (link_frame, config_free, wrapped_sq, key_less, the staged obstacles) and the start points come from the tree planner's counter
// hash; what is new -- the end-effector point with its Jacobian, the step and the pick -- is written once below as __host__ __device__ code,
// run by the kernel's lanes and by armour_ik_host's loop.
//
// Nothing but __syncthreads() orders the block, every barrier is reached on values all lanes hold alike, and every loop is bounded by
// max_iterations, J, O or S.  No per-lane array is indexed at run time: the chain is unrolled over ARMOUR_MAX_JOINTS with static indices, so
// the seven origins and axes of the Jacobian stay in registers (ik.resources.txt beside the object: 0 B of scratch).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "roadmap_handle.h"
#include "tree_block.h"

using namespace treeblk;   // the block shape, the counter hash (and, through it, rmgeo)

namespace {

constexpr int IK_SPLIT_SEEDS = TP_BLOCK / 2;   // up to this many seeds an item's free test is split over several lanes

// What a target's run reads besides the robot: by value in the kernel's arguments (pointers: the device's; the host twin passes its own)
struct IkArgs {
    double lb[ARMOUR_MAX_FACTORS], ub[ARMOUR_MAX_FACTORS];
    double tool[3];
    double lambda, e_max, tol;
    int32_t S, O, max_iterations;
    const double *obstacles, *targets, *q_ref;
    const int32_t* world;
    const uint64_t* seeds;
    int32_t *status, *best, *iterations, *flags;
    double *q_best, *q, *err;
};
// an entry's arguments as it was given them: the kernel's, and what only check_args reads (it copies the box to lb / ub and the tool point)
struct IkCall : IkArgs {
    const double *box_lb, *box_ub, *tool_in;
    int32_t N, W;
};

// The chain at q: pe = the end-effector point; o[j] / a[j] = the origin of frame j and the signed world axis of joint j (zero for a joint
// that is not actuated).  Unrolled over the compiled maximum, so q, o and a are indexed by constants.
__host__ __device__ inline void ik_chain(const RmRobot& rb, const double (&q)[ARMOUR_MAX_FACTORS], const double* tool, double* pe, double (&o)[ARMOUR_MAX_FACTORS][3],
                                         double (&a)[ARMOUR_MAX_FACTORS][3]) {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
#pragma unroll
    for (int l = 0; l < ARMOUR_MAX_JOINTS; l++) {
        if (l < rb.J) link_frame(rb, l, l < ARMOUR_MAX_FACTORS ? q[l < ARMOUR_MAX_FACTORS ? l : 0] : 0.0, R, p);
        if (l < ARMOUR_MAX_FACTORS) {
            const int j = l < ARMOUR_MAX_FACTORS ? l : 0;                      // (both selects: no constant index past the arrays once unrolled)
            const int ax = rb.axis[j];
            const bool on = j < rb.J && j < rb.n && ax != 0;
            const int e = ax > 0 ? ax : -ax;
            const double sg = ax > 0 ? 1.0 : -1.0;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                o[j][i] = p[i];
                const double col = e == 1 ? R[3 * i] : (e == 2 ? R[3 * i + 1] : R[3 * i + 2]);
                a[j][i] = on ? sg * col : 0.0;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 3; i++) pe[i] = p[i] + ((R[3 * i] * tool[0] + R[3 * i + 1] * tool[1]) + R[3 * i + 2] * tool[2]);
}

// Column j of the position Jacobian: a_j x (pe - o_j)
__host__ __device__ inline void ik_columns(const double* pe, const double (&o)[ARMOUR_MAX_FACTORS][3], const double (&a)[ARMOUR_MAX_FACTORS][3],
                                           double (&c)[ARMOUR_MAX_FACTORS][3]) {
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) {
        const double d[3] = {pe[0] - o[j][0], pe[1] - o[j][1], pe[2] - o[j][2]};
        cross3(a[j], d, c[j]);
    }
}

__host__ __device__ inline double ik_clip(const RmRobot& rb, const IkArgs& ar, int j, double x) { return rb.cont[j] ? x : fmin(fmax(x, ar.lb[j]), ar.ub[j]); }

// The start point of item (t, s): q_ref for s = 0, else the counter hash's point of the box; non-continuous joints clipped
__host__ __device__ inline void ik_start(const RmRobot& rb, const IkArgs& ar, const double* q_ref, uint64_t seed, int s, double (&q)[ARMOUR_MAX_FACTORS]) {
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) {
        const double x = s == 0 ? (j < rb.n ? q_ref[j < rb.n ? j : 0] : 0.0) : ar.lb[j] + tree_u(seed, (uint64_t)s, (uint64_t)j) * (ar.ub[j] - ar.lb[j]);
        q[j] = j < rb.n ? ik_clip(rb, ar, j, x) : 0.0;
    }
}

// The iteration of the header from the start point in q.  Returns converged; q, *err and *iterations are the item's outputs.
__host__ __device__ inline bool ik_iterate(const RmRobot& rb, const IkArgs& ar, const double* target, double (&q)[ARMOUR_MAX_FACTORS], double* err_out, int* iterations) {
    const double l2 = ar.lambda * ar.lambda;
    for (int k = 0;; k++) {
        double pe[3], o[ARMOUR_MAX_FACTORS][3], a[ARMOUR_MAX_FACTORS][3], c[ARMOUR_MAX_FACTORS][3];
        ik_chain(rb, q, ar.tool, pe, o, a);
        double e[3] = {target[0] - pe[0], target[1] - pe[1], target[2] - pe[2]};
        const double err = sqrt(dot3(e, e));
        *err_out = err;
        *iterations = k;
        if (err <= ar.tol) return true;
        if (k >= ar.max_iterations) return false;
        if (err > ar.e_max) {
            const double sc = ar.e_max / err;
            e[0] = e[0] * sc; e[1] = e[1] * sc; e[2] = e[2] * sc;
        }
        ik_columns(pe, o, a, c);
        // A = J J^T + lambda^2 I, the lower triangle, columns summed in index order from 0
        double A00 = 0.0, A10 = 0.0, A11 = 0.0, A20 = 0.0, A21 = 0.0, A22 = 0.0;
#pragma unroll
        for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) {
            A00 = A00 + c[j][0] * c[j][0];
            A10 = A10 + c[j][1] * c[j][0];
            A11 = A11 + c[j][1] * c[j][1];
            A20 = A20 + c[j][2] * c[j][0];
            A21 = A21 + c[j][2] * c[j][1];
            A22 = A22 + c[j][2] * c[j][2];
        }
        A00 = A00 + l2; A11 = A11 + l2; A22 = A22 + l2;
        // A = L L^T, L z = e, L^T y = z
        const double L00 = sqrt(A00), L10 = A10 / L00, L20 = A20 / L00;
        const double L11 = sqrt(A11 - L10 * L10), L21 = (A21 - L20 * L10) / L11;
        const double L22 = sqrt((A22 - L20 * L20) - L21 * L21);
        const double z0 = e[0] / L00, z1 = (e[1] - L10 * z0) / L11, z2 = ((e[2] - L20 * z0) - L21 * z1) / L22;
        double y[3];
        y[2] = z2 / L22;
        y[1] = (z1 - L21 * y[2]) / L11;
        y[0] = ((z0 - L10 * y[1]) - L20 * y[2]) / L00;
#pragma unroll
        for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q[j] = j < rb.n ? ik_clip(rb, ar, j, q[j] + dot3(c[j], y)) : 0.0;
    }
}

// The node rule at q against the `count` staged obstacles of the rule's view (tree_block.h, Rule<MOVING>: the static rule, or the window rule
// of the target's world): verdict mode, no enlargement (q is copied: the rule consumes its arguments).  clearance (host twin's margin): the
// full form.
template <class R>
__host__ __device__ inline bool ik_free(const RmRobot& rb, const double (&q)[ARMOUR_MAX_FACTORS], const R& rule, int count, double* clearance = nullptr) {
    double x[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS];
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) x[j] = q[j];
#pragma unroll
    for (int l = 0; l < ARMOUR_MAX_JOINTS; l++) r[l] = 0.0;
    return rule.config(rb, x, r, count, clearance != nullptr, clearance);
}

struct IkShared {
    double q[ARMOUR_MAX_FACTORS][IK_SPLIT_SEEDS];   // joint j of item s, for the lanes that share the item's free test
    BlockKeys keys;
    BlockWords some;                                // per wave: some lane's item converged
    uint8_t conv[TP_BLOCK], hit[TP_BLOCK];
};

// grid N, dynamic LDS [O][Rule<MOVING>::STRIDE] doubles.  MOVING (armour_ik_moving): the window rule of the target's world -- mv.velocity
// [W][O][3], mv.mid / mv.half [W], read only for world >= 0.  The static instantiation reads nothing of mv.
template <bool MOVING>
__global__ __launch_bounds__(TP_BLOCK) void ik_kernel(RmRobot rb, IkArgs ar, MovingArgs mv) {
    extern __shared__ double s_obs[];   // [O][RM_OBS_STRIDE], MOVING: [O][RM_MOV_STRIDE]
    __shared__ IkShared sh;
    const int tg = blockIdx.x, t = threadIdx.x, n = rb.n, S = ar.S;
    const int w = ar.world[tg];
    const int O = w < 0 ? 0 : ar.O;                        // world -1: no obstacles (and no window)
    Rule<MOVING> rule{s_obs};
    if constexpr (MOVING) {
        rule.mid = w < 0 ? 0.0 : mv.mid[w < 0 ? 0 : w];
        rule.half = w < 0 ? 0.0 : mv.half[w < 0 ? 0 : w];
        stage_obstacles_moving_lds<TP_BLOCK>(ar.obstacles + (size_t)(w < 0 ? 0 : w) * ar.O * ARMOUR_OBS_DOUBLES, mv.velocity + (size_t)(w < 0 ? 0 : w) * ar.O * 3, O, s_obs);
    } else {
        stage_obstacles_lds<TP_BLOCK>(ar.obstacles + (size_t)(w < 0 ? 0 : w) * ar.O * ARMOUR_OBS_DOUBLES, O, s_obs);
    }
    const double* q_ref = ar.q_ref + (size_t)tg * n;
    const size_t item = (size_t)tg * S + (t < S ? t : 0);

    // ---- solve: lane s runs item (tg, s)
    double q[ARMOUR_MAX_FACTORS];
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q[j] = 0.0;
    bool conv = false;
    if (t < S) {
        double err;
        int iters;
        ik_start(rb, ar, q_ref, ar.seeds[tg], t, q);
        conv = ik_iterate(rb, ar, ar.targets + (size_t)tg * 3, q, &err, &iters);
        if (ar.err) ar.err[item] = err;
        if (ar.iterations) ar.iterations[item] = iters;
        if (ar.q) {
#pragma unroll
            for (int j = 0; j < ARMOUR_MAX_FACTORS; j++)
                if (j < n) ar.q[item * n + j] = q[j];
        }
        if (S <= IK_SPLIT_SEEDS) {
#pragma unroll
            for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) sh.q[j][t] = q[j];
        }
    }
    sh.conv[t] = conv ? 1 : 0;
    sh.hit[t] = 0;
    __syncthreads();

    // ---- free test of the converged items.  Up to TP_BLOCK / 2 seeds an item's obstacles are split over several lanes (obstacle_split).
    {
        const ObstacleSplit sp = obstacle_split(S, O, true, t);
        const int it = t / sp.G, o0 = sp.o0, o1 = sp.o1;
        if (it < S && sh.conv[it] && o1 > o0) {
            double x[ARMOUR_MAX_FACTORS];
#pragma unroll
            for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) x[j] = S <= IK_SPLIT_SEEDS ? sh.q[j][it] : q[j];   // (above the split: it == t)
            if (!ik_free(rb, x, rule.from(o0), o1 - o0)) sh.hit[it] = 1;                                 // every writer stores the same value
        }
    }
    __syncthreads();
    const bool free_ = conv && !sh.hit[t];
    if (t < S && ar.flags) ar.flags[item] = (conv ? 1 : 0) | (free_ ? 2 : 0);

    // ---- pick: the smallest (acc, s) over the items that are converged and free; the order is total.  The convergence ballot rides on the
    // argmin's barrier: each wave's word is written before it and folded after it.  Neither sh.keys nor sh.some is written again (the
    // kernel ends), so the argmin is not released.
    double bd = INFINITY;
    int bv = TP_NONE;
    if (free_) { bd = wrapped_sq(rb, q_ref, q); bv = t; }
    const unsigned long long any = __ballot(conv);
    if ((t & 63) == 0) sh.some.w[t >> 6] = any ? 1 : 0;
    block_argmin<false>(sh.keys, &bd, &bv);
    int some = 0;
#pragma unroll
    for (int k = 0; k < TP_WAVES; k++) some |= sh.some.w[k];
    if (t == bv) {                                          // the picked item's own lane holds its q
#pragma unroll
        for (int j = 0; j < ARMOUR_MAX_FACTORS; j++)
            if (j < n) ar.q_best[(size_t)tg * n + j] = q[j];
    }
    if (t == 0) {
        ar.best[tg] = bv == TP_NONE ? -1 : bv;
        ar.status[tg] = bv != TP_NONE ? ARMOUR_IK_FOUND : (some ? ARMOUR_IK_ALL_BLOCKED : ARMOUR_IK_NONE_CONVERGED);
    }
}

// target tg of the host twin: the same functions in a loop; rule = the target's world, staged as the kernel stages it, with its rule
template <class R>
void ik_target_host(const RmRobot& rb, const IkArgs& ar, int tg, const R& rule, int O, double* margin) {
    const int n = rb.n, S = ar.S;
    const double* q_ref = ar.q_ref + (size_t)tg * n;
    double bd = INFINITY, m = INFINITY;
    int bv = TP_NONE;
    bool some = false;
    for (int s = 0; s < S; s++) {
        const size_t item = (size_t)tg * S + s;
        double q[ARMOUR_MAX_FACTORS], err;
        int iters;
        ik_start(rb, ar, q_ref, ar.seeds[tg], s, q);
        const bool conv = ik_iterate(rb, ar, ar.targets + (size_t)tg * 3, q, &err, &iters);
        bool free_ = false;
        if (conv) {
            some = true;
            free_ = ik_free(rb, q, rule, O);
            if (margin) {
                double cl;
                ik_free(rb, q, rule, O, &cl);
                m = std::fmin(m, std::fabs(cl));
            }
        }
        if (ar.err) ar.err[item] = err;
        if (ar.iterations) ar.iterations[item] = iters;
        if (ar.flags) ar.flags[item] = (conv ? 1 : 0) | (free_ ? 2 : 0);
        if (ar.q) std::memcpy(ar.q + item * n, q, n * sizeof(double));
        if (free_) {
            const double d = wrapped_sq(rb, q_ref, q);
            if (key_less(d, s, bd, bv)) {
                bd = d; bv = s;
                std::memcpy(ar.q_best + (size_t)tg * n, q, n * sizeof(double));
            }
        }
    }
    ar.best[tg] = bv == TP_NONE ? -1 : bv;
    ar.status[tg] = bv != TP_NONE ? ARMOUR_IK_FOUND : (some ? ARMOUR_IK_ALL_BLOCKED : ARMOUR_IK_NONE_CONVERGED);
    if (margin) *margin = m;
}

// the argument rules of both entries, before a device is touched, on ar as the entry filled it; fills rb and ar.lb / ar.ub / ar.tool
int check_args(const char* who, const ArmourRobot* robot, const uint8_t* continuous, RmRobot* rb, IkCall* ar) {
    const int32_t N = ar->N, S = ar->S, W = ar->W, O = ar->O;
    if (!robot || !ar->box_lb || !ar->box_ub || !ar->tool_in) { armour_set_error("%s: null argument", who); return ARMOUR_EINVAL; }
    ARMOUR_TRY(armour_check_robot_shape(who, robot));
    ARMOUR_TRY(armour_check_world_counts(who, W, O, ar->obstacles));
    const int n = robot->num_factors;
    if (N < 0 || N > ARMOUR_IK_MAX_TARGETS || S < 1 || S > ARMOUR_IK_MAX_SEEDS || ar->max_iterations < 0 || ar->max_iterations > ARMOUR_IK_MAX_ITERATIONS) {
        armour_set_error("%s: N = %d (0..%d), S = %d (1..%d), max_iterations = %d (0..%d)", who, N, ARMOUR_IK_MAX_TARGETS, S, ARMOUR_IK_MAX_SEEDS, ar->max_iterations,
                         ARMOUR_IK_MAX_ITERATIONS);
        return ARMOUR_EINVAL;
    }
    if (N > 0 && (!ar->world || !ar->targets || !ar->q_ref || !ar->seeds || !ar->status || !ar->best || !ar->q_best)) { armour_set_error("%s: null argument", who); return ARMOUR_EINVAL; }
    if (!(ar->lambda > 0.0) || !(ar->e_max > 0.0) || !(ar->tol > 0.0) || !std::isfinite(ar->lambda) || !std::isfinite(ar->e_max) || !std::isfinite(ar->tol)) {
        armour_set_error("%s: lambda = %g, e_max = %g, tol = %g (all must be positive and finite)", who, ar->lambda, ar->e_max, ar->tol);
        return ARMOUR_EINVAL;
    }
    ARMOUR_TRY(armour_check_box(who, "box", "joint", n, ar->box_lb, ar->box_ub));
    if (!finite_all(ar->obstacles, (size_t)W * O * ARMOUR_OBS_DOUBLES) || !finite_all(ar->targets, (size_t)N * 3) || !finite_all(ar->q_ref, (size_t)N * n) || !finite_all(ar->tool_in, 3)) {
        armour_set_error("%s: a target, a reference configuration, the tool point or an obstacle is not finite", who);
        return ARMOUR_EINVAL;
    }
    for (int32_t t = 0; t < N; t++)
        if (ar->world[t] < -1 || ar->world[t] >= W) { armour_set_error("%s: target %d is in world %d (-1..%d)", who, t, ar->world[t], W - 1); return ARMOUR_EINVAL; }
    fill_rm_robot(robot, continuous, rb);
    for (int j = 0; j < n; j++) { ar->lb[j] = ar->box_lb[j]; ar->ub[j] = ar->box_ub[j]; }
    for (int i = 0; i < 3; i++) ar->tool[i] = ar->tool_in[i];
    return ARMOUR_OK;
}

// the host twin of both rules (mv null: the static one)
int solve_on_host(const char* who, const ArmourRobot* robot, const uint8_t* continuous, IkCall& ar, const Motion* mv, double* margin) {
    RmRobot rb;
    ARMOUR_TRY(check_args(who, robot, continuous, &rb, &ar));
    std::vector<double> mid, half;
    if (mv) ARMOUR_TRY(check_windows(who, ar.W, ar.O, *mv, &mid, &half));
    auto target = [&](int32_t t, const auto& rule, int count) { ik_target_host(rb, ar, t, rule, count, margin ? margin + t : nullptr); };
    if (mv) for_each_staged<true>(ar.N, ar.O, ar.obstacles, ar.world, target, mv->velocity, mid.data(), half.data());
    else for_each_staged(ar.N, ar.O, ar.obstacles, ar.world, target);
    return ARMOUR_OK;
}

// the device entry of both rules (mv null: the static one)
int solve_on_device(const char* who, const char* host_form, const ArmourRobot* robot, const uint8_t* continuous, IkCall& ar, const Motion* mv, double* ms) {
    RmRobot rb;
    ARMOUR_TRY(check_args(who, robot, continuous, &rb, &ar));
    std::vector<double> mid, half;
    if (mv) ARMOUR_TRY(check_windows(who, ar.W, ar.O, *mv, &mid, &half));
    const int32_t N = ar.N, S = ar.S, W = ar.W, O = ar.O;
    int32_t *best = ar.best, *iterations = ar.iterations, *flags = ar.flags;
    double *q_best = ar.q_best, *q = ar.q, *err = ar.err;
    if (ms) *ms = 0.0;
    if (N == 0) return ARMOUR_OK;
    if (!armour_device_available()) { armour_set_error("%s: no HIP device visible (%s is the host form)", who, host_form); return ARMOUR_EDEVICE; }
    const int n = rb.n;
    const size_t items = (size_t)N * S;
    DevStream st;
    EventPair ev;
    DevBuf<double> d_obs, d_targets, d_ref, d_qbest, d_q, d_err, d_vel, d_mid, d_half;
    DevBuf<uint64_t> d_seeds;
    DevBuf<int32_t> d_world, d_items;                      // d_items: iterations | flags [N][S] each, either may be absent
    DevColumns<int32_t> out;                               // status | best [N] each
    ARMOUR_TRY(st.create());
    ARMOUR_TRY(d_obs.upload(ar.obstacles, (size_t)W * O * ARMOUR_OBS_DOUBLES, st));
    ARMOUR_TRY(d_targets.upload(ar.targets, (size_t)N * 3, st));
    ARMOUR_TRY(d_ref.upload(ar.q_ref, (size_t)N * n, st));
    ARMOUR_TRY(d_seeds.upload(ar.seeds, (size_t)N, st));
    ARMOUR_TRY(d_world.upload(ar.world, (size_t)N, st));
    MovingArgs dmv{};
    if (mv) {
        ARMOUR_TRY(d_vel.upload(mv->velocity, (size_t)W * O * 3, st));
        ARMOUR_TRY(d_mid.upload(mid.data(), (size_t)W, st));
        ARMOUR_TRY(d_half.upload(half.data(), (size_t)W, st));
        dmv = MovingArgs{d_vel, d_mid, d_half};
    }
    ARMOUR_TRY(d_qbest.reserve((size_t)N * n));
    ARMOUR_TRY(out.reserve(2, (size_t)N));
    if (q) ARMOUR_TRY(d_q.reserve(items * n));
    if (err) ARMOUR_TRY(d_err.reserve(items));
    if (iterations || flags) ARMOUR_TRY(d_items.reserve(2 * items));
    IkArgs dev = ar;                                       // (the kernel's part)
    dev.obstacles = d_obs; dev.targets = d_targets; dev.q_ref = d_ref; dev.seeds = d_seeds; dev.world = d_world;
    dev.status = out.column(0); dev.best = out.column(1); dev.q_best = d_qbest;
    dev.q = q ? d_q.p : nullptr;
    dev.err = err ? d_err.p : nullptr;
    dev.iterations = iterations ? d_items.p : nullptr;
    dev.flags = flags ? d_items + items : nullptr;
    // at the cap of 256 obstacles 54 KB (static) or 62 KB (moving) of dynamic LDS: above 48 KB, which a block may have once it asks
    const size_t lds = (size_t)O * (mv ? Rule<true>::STRIDE : Rule<false>::STRIDE) * sizeof(double);
    const void* kernel = mv ? reinterpret_cast<const void*>(ik_kernel<true>) : reinterpret_cast<const void*>(ik_kernel<false>);
    ARMOUR_TRY(grant_dynamic_lds(who, kernel, lds));
    ARMOUR_TRY(ev.record_start(st));
    if (mv) hipLaunchKernelGGL(ik_kernel<true>, dim3((unsigned)N), dim3(TP_BLOCK), lds, st, rb, dev, dmv);
    else hipLaunchKernelGGL(ik_kernel<false>, dim3((unsigned)N), dim3(TP_BLOCK), lds, st, rb, dev, dmv);
    HIPCHK(hipGetLastError());
    ARMOUR_TRY(ev.record_stop(st));
    ARMOUR_TRY(out.fetch(st));
    if (q) HIPCHK(hipMemcpyAsync(q, d_q, items * n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (err) HIPCHK(hipMemcpyAsync(err, d_err, items * sizeof(double), hipMemcpyDeviceToHost, st));
    if (iterations) HIPCHK(hipMemcpyAsync(iterations, d_items, items * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (flags) HIPCHK(hipMemcpyAsync(flags, d_items + items, items * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ms) ARMOUR_TRY(ev.elapsed_ms(ms));
    out.copy_out(0, ar.status);
    out.copy_out(1, best);
    // only the rows that were written come back (a target without a pick leaves the caller's row as it was)
    for (int32_t t = 0; t < N; t++)
        if (best[t] >= 0) HIPCHK(hipMemcpyAsync(q_best + (size_t)t * n, d_qbest + (size_t)t * n, n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ARMOUR_OK;
}

// an entry's arguments into the call record (the moving entries' three go beside it, in a Motion)
IkCall ik_call(const double* lb, const double* ub, const double* tool, int32_t N, int32_t S, int32_t W, int32_t O, const double* obstacles, const int32_t* world,
               const double* targets, const double* q_ref, const uint64_t* seeds, double lambda, double e_max, double tol, int32_t max_iterations, int32_t* status,
               int32_t* best, double* q_best, double* q, double* err, int32_t* iterations, int32_t* flags) {
    IkCall ar{};
    ar.box_lb = lb; ar.box_ub = ub; ar.tool_in = tool; ar.N = N; ar.S = S; ar.W = W; ar.O = O; ar.obstacles = obstacles; ar.world = world; ar.targets = targets;
    ar.q_ref = q_ref; ar.seeds = seeds; ar.lambda = lambda; ar.e_max = e_max; ar.tol = tol; ar.max_iterations = max_iterations; ar.status = status; ar.best = best;
    ar.q_best = q_best; ar.q = q; ar.err = err; ar.iterations = iterations; ar.flags = flags;
    return ar;
}

}  // namespace

extern "C" int armour_ik_host(const ArmourRobot* robot, const uint8_t* continuous, const double* lb, const double* ub, const double* tool, int32_t N, int32_t S,
                              int32_t W, int32_t O, const double* obstacles, const int32_t* world, const double* targets, const double* q_ref, const uint64_t* seeds,
                              double lambda, double e_max, double tol, int32_t max_iterations, int32_t* status, int32_t* best, double* q_best, double* q, double* err,
                              int32_t* iterations, int32_t* flags, double* margin) {
    IkCall ar = ik_call(lb, ub, tool, N, S, W, O, obstacles, world, targets, q_ref, seeds, lambda, e_max, tol, max_iterations, status, best, q_best, q, err, iterations, flags);
    return solve_on_host("armour_ik_host", robot, continuous, ar, nullptr, margin);
}

extern "C" int armour_ik_moving_host(const ArmourRobot* robot, const uint8_t* continuous, const double* lb, const double* ub, const double* tool, int32_t N, int32_t S,
                                     int32_t W, int32_t O, const double* obstacles, const double* velocity, const double* t_from, const double* t_to,
                                     const int32_t* world, const double* targets, const double* q_ref, const uint64_t* seeds, double lambda, double e_max, double tol,
                                     int32_t max_iterations, int32_t* status, int32_t* best, double* q_best, double* q, double* err, int32_t* iterations, int32_t* flags,
                                     double* margin) {
    IkCall ar = ik_call(lb, ub, tool, N, S, W, O, obstacles, world, targets, q_ref, seeds, lambda, e_max, tol, max_iterations, status, best, q_best, q, err, iterations, flags);
    const Motion mv{velocity, t_from, t_to};
    return solve_on_host("armour_ik_moving_host", robot, continuous, ar, &mv, margin);
}

extern "C" int armour_ik(const ArmourRobot* robot, const uint8_t* continuous, const double* lb, const double* ub, const double* tool, int32_t N, int32_t S, int32_t W,
                         int32_t O, const double* obstacles, const int32_t* world, const double* targets, const double* q_ref, const uint64_t* seeds, double lambda,
                         double e_max, double tol, int32_t max_iterations, int32_t* status, int32_t* best, double* q_best, double* q, double* err,
                         int32_t* iterations, int32_t* flags, double* ms) {
    IkCall ar = ik_call(lb, ub, tool, N, S, W, O, obstacles, world, targets, q_ref, seeds, lambda, e_max, tol, max_iterations, status, best, q_best, q, err, iterations, flags);
    return solve_on_device("armour_ik", "armour_ik_host", robot, continuous, ar, nullptr, ms);
}

extern "C" int armour_ik_moving(const ArmourRobot* robot, const uint8_t* continuous, const double* lb, const double* ub, const double* tool, int32_t N, int32_t S,
                                int32_t W, int32_t O, const double* obstacles, const double* velocity, const double* t_from, const double* t_to, const int32_t* world,
                                const double* targets, const double* q_ref, const uint64_t* seeds, double lambda, double e_max, double tol, int32_t max_iterations,
                                int32_t* status, int32_t* best, double* q_best, double* q, double* err, int32_t* iterations, int32_t* flags, double* ms) {
    IkCall ar = ik_call(lb, ub, tool, N, S, W, O, obstacles, world, targets, q_ref, seeds, lambda, e_max, tol, max_iterations, status, best, q_best, q, err, iterations, flags);
    const Motion mv{velocity, t_from, t_to};
    return solve_on_device("armour_ik_moving", "armour_ik_moving_host", robot, continuous, ar, &mv, ms);
}

extern "C" int armour_ik_end_effector_host(const ArmourRobot* robot, int32_t N, const double* q, const double* tool, double* p, double* jac) {
    const char* who = "armour_ik_end_effector_host";
    if (!robot || !tool || N < 0 || (N > 0 && (!q || !p))) { armour_set_error("%s: null argument or N = %d", who, N); return ARMOUR_EINVAL; }
    ARMOUR_TRY(armour_check_robot_shape(who, robot));
    const int n = robot->num_factors;
    if (!finite_all(q, (size_t)N * n) || !finite_all(tool, 3)) { armour_set_error("%s: a configuration or the tool point is not finite", who); return ARMOUR_EINVAL; }
    RmRobot rb;
    fill_rm_robot(robot, nullptr, &rb);
    for (int32_t i = 0; i < N; i++) {
        double x[ARMOUR_MAX_FACTORS] = {}, pe[3], o[ARMOUR_MAX_FACTORS][3], a[ARMOUR_MAX_FACTORS][3], c[ARMOUR_MAX_FACTORS][3];
        for (int j = 0; j < n; j++) x[j] = q[(size_t)i * n + j];
        ik_chain(rb, x, tool, pe, o, a);
        std::memcpy(p + (size_t)i * 3, pe, sizeof(pe));
        if (jac) {
            ik_columns(pe, o, a, c);
            for (int r = 0; r < 3; r++)
                for (int j = 0; j < n; j++) jac[((size_t)i * 3 + r) * n + j] = c[j][r];
        }
    }
    return ARMOUR_OK;
}
