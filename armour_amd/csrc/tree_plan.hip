// Batched tree planner (include/armour_hip.h, armour_tree_plan): bidirectional RRT-Connect for W worlds in ONE launch, a block per world,
// the whole loop inside the block (armour_tree_plan_moving: the same against obstacles in linear motion, by the window rule; tree_block.h
// Rule<MOVING>).  The rule is the roadmap's, reused as it stands: the node rule (config_free), the edge rule's sub-segments
// (edge_segments / edge_sample) and the wrapped distance (wrapped_sq); what is new here -- the counter hash, the steer and cut steps and the
// order (distance, index) -- is written once below as __host__ __device__ code, run by the kernel's lanes and by armour_tree_plan_host's loop.
//
// Nothing but __syncthreads() orders the block: a tree's nodes live in global memory, written and read by this block alone; every decision
// that steers the loop is taken from values all lanes hold alike, so the barriers are reached by all of them.  The loop is bounded by
// max_iterations, a prefix by ARMOUR_TREE_MAX_SEGMENTS, a nearest scan and a path walk by the tree's count.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "roadmap_handle.h"
#include "tree_block.h"

using namespace treeblk;   // the steps shared with path_shortcut.hip (and, through it, rmgeo)

namespace {

// What a world's run reads besides the robot: by value in the kernel's arguments (pointers: the device's; the host twin passes its own)
struct TreeArgs {
    double lb[ARMOUR_MAX_FACTORS], ub[ARMOUR_MAX_FACTORS];
    double step, edge_step;
    int32_t O, max_iterations, max_nodes, max_points;
    const double *obstacles, *starts, *goals;
    const uint64_t* seeds;
    int32_t *status, *iterations, *points, *count, *parent;
    double *path, *nodes;
};
// an entry's arguments as it was given them: the kernel's, and what only check_args reads (it copies the box to lb / ub)
struct TreeCall : TreeArgs {
    const double *box_lb, *box_ub;
    int32_t W;
};

__host__ __device__ inline double tree_sample(const TreeArgs& a, uint64_t seed, int i, int j) { return a.lb[j] + tree_u(seed, (uint64_t)i, (uint64_t)j) * (a.ub[j] - a.lb[j]); }

// joint j of the steer step: from the nearest node a towards the sample qr, the whole way when dist = sqrt(acc) <= step
__host__ __device__ inline double steer_joint(const RmRobot& rb, int j, double a, double qr, double dist, double step) {
    const double D = joint_diff(rb, j, a, qr);
    return dist <= step ? a + D : a + (step / dist) * D;
}
// ---- the block's cooperative steps.  Every result is the same in all lanes.  The first colliding lane is tree_block.h's block_first; the
// argmin's fold and the obstacle split stay inline: through block_argmin / obstacle_split the kernel measured 0.4 to 0.7 % slower
// (DESIGN.md 4.12d).
struct TreeShared {
    double a[ARMOUR_MAX_FACTORS], b[ARMOUR_MAX_FACTORS];   // the edge a prefix walks; b doubles as the query of a nearest scan
    double red_d[TP_WAVES];
    int red_v[TP_WAVES];
    BlockWords words;
    int flag[2];
};

// argmin over nodes[0 .. cnt) of (wrapped_sq(node, sh.b), index); the caller has put a barrier after the last write of sh.b and of the nodes,
// and reaches one before the next call writes sh.red_*: the barrier that publishes sh.a / sh.b for the prefix, or the one after the sample
__device__ inline void block_nearest(const RmRobot& rb, TreeShared& sh, const double* nodes, int cnt, double* acc, int* index) {
    const int n = rb.n, t = threadIdx.x;
    double q[ARMOUR_MAX_FACTORS];
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q[j] = sh.b[j];
    double bd = INFINITY;
    int bv = TP_NONE;
    for (int v = t; v < cnt; v += TP_BLOCK) {
        const double d = wrapped_sq(rb, nodes + (size_t)v * n, q);
        if (key_less(d, v, bd, bv)) { bd = d; bv = v; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o);
        const int ov = __shfl_xor(bv, o);
        if (key_less(od, ov, bd, bv)) { bd = od; bv = ov; }
    }
    if ((t & 63) == 0) { sh.red_d[t >> 6] = bd; sh.red_v[t >> 6] = bv; }
    __syncthreads();
    bd = sh.red_d[0]; bv = sh.red_v[0];
#pragma unroll
    for (int w = 1; w < TP_WAVES; w++)
        if (key_less(sh.red_d[w], sh.red_v[w], bd, bv)) { bd = sh.red_d[w]; bv = sh.red_v[w]; }
    *acc = bd;
    *index = bv;
}

// prefix(sh.a, sh.b): *S sub-segments, returns m.  Sub-segments are taken in ascending chunks, up to the first chunk with a hit.  An edge of
// at most TP_BLOCK / 2 sub-segments (every extend step; most joins) gives each sub-segment G = min(O, TP_BLOCK / S) lanes, lane g of them
// testing the obstacles [g O / G, (g + 1) O / G): tree_block.h's obstacle_split, which says why it is sound.  Lanes are in ascending order
// of sub-segment, so the first colliding lane names the first colliding sub-segment.  The caller has put a barrier after the last write of
// sh.a / sh.b; on return every lane is past the last read of them, and sh.words is released.  A lane's slice is rule.from(o0): the offset is in
// the stride of the rule's staging.
template <class R>
__device__ inline int block_prefix(const RmRobot& rb, TreeShared& sh, double edge_step, const R& rule, int O, int* S_out) {
    const int t = threadIdx.x;
    const int S = prefix_segments(rb, sh.a, sh.b, edge_step);
    *S_out = S;
    int G = 1;
    if (2 * S <= TP_BLOCK && O > 1) G = TP_BLOCK / S < O ? TP_BLOCK / S : O;
    const int per = TP_BLOCK / G;                           // sub-segments per chunk
    const int g = t % G, o0 = (g * O) / G, o1 = ((g + 1) * O) / G;
    int m = S;
    for (int base = 0; base < S; base += per) {
        const int s = base + t / G;
        const bool hit = t < per * G && s < S && !segment_free(rb, sh.a, sh.b, s, S, rule.from(o0), o1 - o0);
        const int f = block_first(sh.words, hit);           // (released: the next chunk, or the next prefix, may write the words)
        if (f != TP_NONE) { m = base + f / G; break; }
    }
    return m;
}

// grid W, dynamic LDS [O][RM_OBS_STRIDE] doubles.  The trees of world w: nodes [w][2][max_nodes][n], parent [w][2][max_nodes], count [w][2].
// MOVING (armour_tree_plan_moving): the window rule -- dynamic LDS [O][RM_MOV_STRIDE], mv.velocity [W][O][3], mv.mid / mv.half [W], this world's
// two kept in registers.  The static instantiation reads nothing of mv and keeps the static rule's calls as they were.
template <bool MOVING>
__global__ __launch_bounds__(TP_BLOCK) void tree_plan_kernel(RmRobot rb, TreeArgs ar, MovingArgs mv) {
    extern __shared__ double s_obs[];   // [O][RM_OBS_STRIDE], MOVING: [O][RM_MOV_STRIDE]
    __shared__ TreeShared sh;
    const int w = blockIdx.x, t = threadIdx.x, n = rb.n, O = ar.O, cap = ar.max_nodes;
    Rule<MOVING> rule{s_obs};
    if constexpr (MOVING) {
        rule.mid = mv.mid[w];
        rule.half = mv.half[w];
        stage_obstacles_moving_lds<TP_BLOCK>(ar.obstacles + (size_t)w * O * ARMOUR_OBS_DOUBLES, mv.velocity + (size_t)w * O * 3, O, s_obs);
    } else {
        stage_obstacles_lds<TP_BLOCK>(ar.obstacles + (size_t)w * O * ARMOUR_OBS_DOUBLES, O, s_obs);
    }
    const double* start = ar.starts + (size_t)w * n;
    const double* goal = ar.goals + (size_t)w * n;
    const uint64_t seed = ar.seeds[w];
    double* nodes[2] = {ar.nodes + ((size_t)w * 2) * cap * n, ar.nodes + ((size_t)w * 2 + 1) * cap * n};
    int32_t* parent[2] = {ar.parent + ((size_t)w * 2) * cap, ar.parent + ((size_t)w * 2 + 1) * cap};
    int cnt[2] = {0, 0};
    int status = ARMOUR_TREE_NOT_FOUND, iterations = 0, points = 0;

    // the node rule at start and goal (lanes 0 and 1), and the direct edge
    if (t < 2) sh.flag[t] = node_free(rb, t == 0 ? start : goal, rule, O) ? 1 : 0;
    if (t < ARMOUR_MAX_FACTORS) {
        sh.a[t] = t < n ? start[t] : 0.0;
        sh.b[t] = t < n ? goal[t] : 0.0;
    }
    __syncthreads();
    bool run = false;
    if (!sh.flag[0]) {
        status = ARMOUR_TREE_START_BLOCKED;
    } else if (!sh.flag[1]) {
        status = ARMOUR_TREE_GOAL_BLOCKED;
    } else {
        int S;
        const int m = block_prefix(rb, sh, ar.edge_step, rule, O, &S);
        if (m == S) {
            status = ARMOUR_TREE_FOUND;
            points = 2;
            if (ar.path && points <= ar.max_points && t < n) {
                ar.path[((size_t)w * ar.max_points) * n + t] = start[t];
                ar.path[((size_t)w * ar.max_points + 1) * n + t] = goal[t];
            }
        } else {
            run = true;
        }
    }
    if (run) {
        if (t < n) {
            nodes[0][t] = start[t];
            nodes[1][t] = goal[t];
        }
        if (t == 0) parent[0][0] = parent[1][0] = -1;
        cnt[0] = cnt[1] = 1;
        iterations = ar.max_iterations;
        for (int i = 0; i < ar.max_iterations; i++) {
            const int a = i & 1, b = 1 - a;
            if (cnt[a] >= cap || cnt[b] >= cap) { status = ARMOUR_TREE_FULL; iterations = i; break; }
            // ---- sample (into sh.b, the query of the scan)
            if (t < ARMOUR_MAX_FACTORS) sh.b[t] = t < n ? tree_sample(ar, seed, i, t) : 0.0;
            __syncthreads();                                // also: the nodes appended in iteration i - 1 are written
            // ---- nearest in tree a, steer
            double acc;
            int v;
            block_nearest(rb, sh, nodes[a], cnt[a], &acc, &v);
            if (acc == 0.0) continue;
            const double dist = sqrt(acc);
            if (t < ARMOUR_MAX_FACTORS) {                   // lane t alone reads and writes joint t of sh.a / sh.b
                const double x = t < n ? nodes[a][(size_t)v * n + t] : 0.0;
                sh.a[t] = x;
                sh.b[t] = t < n ? steer_joint(rb, t, x, sh.b[t], dist, ar.step) : 0.0;
            }
            __syncthreads();
            // ---- extend: the free prefix of nearest -> qn
            int S;
            int m = block_prefix(rb, sh, ar.edge_step, rule, O, &S);
            if (m == 0) continue;
            if (t < n) {
                if (m < S) sh.b[t] = cut_joint(rb, t, sh.a[t], sh.b[t], m, S);
                nodes[a][(size_t)cnt[a] * n + t] = sh.b[t];
            }
            if (t == 0) parent[a][cnt[a]] = v;
            const int joined_a = cnt[a];
            cnt[a]++;
            __syncthreads();                                // qn is in sh.b and in tree a
            // ---- connect: the other tree's nearest node towards qn
            int vb;
            block_nearest(rb, sh, nodes[b], cnt[b], &acc, &vb);
            if (t < ARMOUR_MAX_FACTORS) sh.a[t] = t < n ? nodes[b][(size_t)vb * n + t] : 0.0;
            __syncthreads();
            m = block_prefix(rb, sh, ar.edge_step, rule, O, &S);
            if (m == S) {
                // joined: the start tree's chain root -> ..., then the goal tree's chain ... -> root.  The walks are bounded by the counts.
                const int join[2] = {a == 0 ? joined_a : vb, a == 0 ? vb : joined_a};
                int len[2];
                for (int k = 0; k < 2; k++) {
                    int d = 0;
                    for (int x = join[k]; x >= 0 && x < cnt[k] && d < cnt[k]; x = parent[k][x]) d++;
                    len[k] = d;
                }
                status = ARMOUR_TREE_FOUND;
                iterations = i + 1;
                points = len[0] + len[1];
                if (ar.path && points <= ar.max_points && t < n) {
                    double* out = ar.path + ((size_t)w * ar.max_points) * n;
                    int pos = len[0] - 1, d = 0;
                    for (int x = join[0]; d < len[0]; x = parent[0][x], d++, pos--) out[(size_t)pos * n + t] = nodes[0][(size_t)x * n + t];
                    pos = len[0]; d = 0;
                    for (int x = join[1]; d < len[1]; x = parent[1][x], d++, pos++) out[(size_t)pos * n + t] = nodes[1][(size_t)x * n + t];
                }
                break;
            }
            if (m >= 1) {
                if (t < n) nodes[b][(size_t)cnt[b] * n + t] = cut_joint(rb, t, sh.a[t], sh.b[t], m, S);
                if (t == 0) parent[b][cnt[b]] = vb;
                cnt[b]++;
            }
        }
    }
    if (t == 0) {
        ar.status[w] = status;
        ar.iterations[w] = iterations;
        ar.points[w] = points;
        ar.count[2 * w] = cnt[0];
        ar.count[2 * w + 1] = cnt[1];
    }
}

int nearest_host(const RmRobot& rb, const double* nodes, int cnt, const double* q, double* acc) {
    double bd = INFINITY;
    int bv = TP_NONE;
    for (int v = 0; v < cnt; v++) {
        const double d = wrapped_sq(rb, nodes + (size_t)v * rb.n, q);
        if (key_less(d, v, bd, bv)) { bd = d; bv = v; }
    }
    *acc = bd;
    return bv;
}

// world w of the host twin; the trees go to nodes [2][max_nodes][n] / parent [2][max_nodes] (the caller's rows or scratch)
template <class R>
void plan_world_host(const RmRobot& rb, const TreeArgs& ar, int w, const R& rule, double* nodes0, int32_t* parent0, double* margin) {
    const int n = rb.n, cap = ar.max_nodes;
    const double* start = ar.starts + (size_t)w * n;
    const double* goal = ar.goals + (size_t)w * n;
    const uint64_t seed = ar.seeds[w];
    if (margin) *margin = INFINITY;
    const HostWorld<R> hw{rb, rule, ar.O, ar.edge_step, margin};
    double* nodes[2] = {nodes0, nodes0 + (size_t)cap * n};
    int32_t* parent[2] = {parent0, parent0 + cap};
    int cnt[2] = {0, 0};
    int32_t& status = ar.status[w];
    int32_t& iterations = ar.iterations[w];
    int32_t& points = ar.points[w];
    status = ARMOUR_TREE_NOT_FOUND; iterations = 0; points = 0;
    auto done = [&] { if (ar.count) { ar.count[2 * w] = cnt[0]; ar.count[2 * w + 1] = cnt[1]; } };
    if (!hw.node(start)) { status = ARMOUR_TREE_START_BLOCKED; return done(); }
    if (!hw.node(goal)) { status = ARMOUR_TREE_GOAL_BLOCKED; return done(); }
    int S;
    int m = hw.prefix(start, goal, &S);
    double* out = ar.path ? ar.path + ((size_t)w * ar.max_points) * n : nullptr;
    if (m == S) {
        status = ARMOUR_TREE_FOUND;
        points = 2;
        if (out && points <= ar.max_points) {
            std::memcpy(out, start, n * sizeof(double));
            std::memcpy(out + n, goal, n * sizeof(double));
        }
        return done();
    }
    std::memcpy(nodes[0], start, n * sizeof(double));
    std::memcpy(nodes[1], goal, n * sizeof(double));
    parent[0][0] = parent[1][0] = -1;
    cnt[0] = cnt[1] = 1;
    iterations = ar.max_iterations;
    double qr[ARMOUR_MAX_FACTORS] = {}, qn[ARMOUR_MAX_FACTORS] = {};
    for (int i = 0; i < ar.max_iterations; i++) {
        const int a = i & 1, b = 1 - a;
        if (cnt[a] >= cap || cnt[b] >= cap) { status = ARMOUR_TREE_FULL; iterations = i; break; }
        for (int j = 0; j < n; j++) qr[j] = tree_sample(ar, seed, i, j);
        double acc;
        const int v = nearest_host(rb, nodes[a], cnt[a], qr, &acc);
        if (acc == 0.0) continue;
        const double dist = sqrt(acc);
        const double* near = nodes[a] + (size_t)v * n;
        for (int j = 0; j < n; j++) qn[j] = steer_joint(rb, j, near[j], qr[j], dist, ar.step);
        m = hw.prefix(near, qn, &S);
        if (m == 0) continue;
        if (m < S)
            for (int j = 0; j < n; j++) qn[j] = cut_joint(rb, j, near[j], qn[j], m, S);
        std::memcpy(nodes[a] + (size_t)cnt[a] * n, qn, n * sizeof(double));
        parent[a][cnt[a]] = v;
        const int joined_a = cnt[a]++;
        const int vb = nearest_host(rb, nodes[b], cnt[b], qn, &acc);
        const double* other = nodes[b] + (size_t)vb * n;
        m = hw.prefix(other, qn, &S);
        if (m == S) {
            const int join[2] = {a == 0 ? joined_a : vb, a == 0 ? vb : joined_a};
            int len[2];
            for (int k = 0; k < 2; k++) {
                int d = 0;
                for (int x = join[k]; x >= 0 && x < cnt[k] && d < cnt[k]; x = parent[k][x]) d++;
                len[k] = d;
            }
            status = ARMOUR_TREE_FOUND;
            iterations = i + 1;
            points = len[0] + len[1];
            if (out && points <= ar.max_points) {
                int pos = len[0] - 1, d = 0;
                for (int x = join[0]; d < len[0]; x = parent[0][x], d++, pos--) std::memcpy(out + (size_t)pos * n, nodes[0] + (size_t)x * n, n * sizeof(double));
                pos = len[0]; d = 0;
                for (int x = join[1]; d < len[1]; x = parent[1][x], d++, pos++) std::memcpy(out + (size_t)pos * n, nodes[1] + (size_t)x * n, n * sizeof(double));
            }
            break;
        }
        if (m >= 1) {
            double* x = nodes[b] + (size_t)cnt[b] * n;
            for (int j = 0; j < n; j++) x[j] = cut_joint(rb, j, other[j], qn[j], m, S);
            parent[b][cnt[b]++] = vb;
        }
    }
    done();
}

// the argument rules of both entries, before a device is touched, on ar as the entry filled it; fills rb and ar.lb / ar.ub
int check_args(const char* who, const ArmourRobot* robot, const uint8_t* continuous, RmRobot* rb, TreeCall* ar) {
    const int32_t W = ar->W, O = ar->O;
    if (!robot || !ar->box_lb || !ar->box_ub) { armour_set_error("%s: null argument", who); return ARMOUR_EINVAL; }
    ARMOUR_TRY(armour_check_robot_shape(who, robot));
    ARMOUR_TRY(armour_check_world_counts(who, W, O, ar->obstacles));
    const int n = robot->num_factors;
    if (W > 0 && (!ar->starts || !ar->goals || !ar->seeds || !ar->status || !ar->iterations || !ar->points)) { armour_set_error("%s: null argument", who); return ARMOUR_EINVAL; }
    if (ar->max_nodes < 2 || ar->max_nodes > ARMOUR_TREE_MAX_NODES || ar->max_iterations < 0 || ar->max_iterations > ARMOUR_TREE_MAX_ITERATIONS || ar->max_points < 0) {
        armour_set_error("%s: max_nodes = %d (2..%d), max_iterations = %d (0..%d), max_points = %d", who, ar->max_nodes, ARMOUR_TREE_MAX_NODES, ar->max_iterations,
                         ARMOUR_TREE_MAX_ITERATIONS, ar->max_points);
        return ARMOUR_EINVAL;
    }
    if (!(ar->step > 0.0) || !(ar->edge_step > 0.0) || !std::isfinite(ar->step) || !std::isfinite(ar->edge_step)) {
        armour_set_error("%s: step = %g, edge_step = %g", who, ar->step, ar->edge_step);
        return ARMOUR_EINVAL;
    }
    ARMOUR_TRY(armour_check_box(who, "sampling box", "joint", n, ar->box_lb, ar->box_ub));
    if (!finite_all(ar->obstacles, (size_t)W * O * ARMOUR_OBS_DOUBLES) || !finite_all(ar->starts, (size_t)W * n) || !finite_all(ar->goals, (size_t)W * n)) {
        armour_set_error("%s: a start, a goal or an obstacle is not finite", who);
        return ARMOUR_EINVAL;
    }
    fill_rm_robot(robot, continuous, rb);
    // the extent of a joint: the span of the box, the starts and the goals (any other point: a new node lies between an old one and a sample)
    double extent[ARMOUR_MAX_FACTORS];
    for (int j = 0; j < n; j++) {
        double lo = ar->box_lb[j], hi = ar->box_ub[j];
        for (int32_t w = 0; w < W && !rb->cont[j]; w++) {
            lo = std::fmin(lo, std::fmin(ar->starts[(size_t)w * n + j], ar->goals[(size_t)w * n + j]));
            hi = std::fmax(hi, std::fmax(ar->starts[(size_t)w * n + j], ar->goals[(size_t)w * n + j]));
        }
        extent[j] = hi - lo;
    }
    ARMOUR_TRY(check_joint_spans(who, *rb, extent, ar->edge_step));
    for (int j = 0; j < n; j++) { ar->lb[j] = ar->box_lb[j]; ar->ub[j] = ar->box_ub[j]; }
    return ARMOUR_OK;
}

// the host twin of both rules (mv null: the static one)
int plan_on_host(const char* who, const ArmourRobot* robot, const uint8_t* continuous, TreeCall& ar, const Motion* mv, double* margin) {
    RmRobot rb;
    ARMOUR_TRY(check_args(who, robot, continuous, &rb, &ar));
    std::vector<double> mid, half;
    if (mv) ARMOUR_TRY(check_windows(who, ar.W, ar.O, *mv, &mid, &half));
    const int n = rb.n;
    const int32_t max_nodes = ar.max_nodes;
    double* nodes = ar.nodes;
    int32_t* parent = ar.parent;
    std::vector<double> own_nodes(nodes ? 0 : (size_t)2 * max_nodes * n);
    std::vector<int32_t> own_parent(parent ? 0 : (size_t)2 * max_nodes);
    auto world = [&](int32_t w, const auto& rule, int) {
        plan_world_host(rb, ar, w, rule, nodes ? nodes + (size_t)w * 2 * max_nodes * n : own_nodes.data(), parent ? parent + (size_t)w * 2 * max_nodes : own_parent.data(),
                        margin ? margin + w : nullptr);
    };
    if (mv) for_each_staged<true>(ar.W, ar.O, ar.obstacles, nullptr, world, mv->velocity, mid.data(), half.data());
    else for_each_staged(ar.W, ar.O, ar.obstacles, nullptr, world);
    return armour_check_path_capacity(who, ar.W, ar.points, ar.max_points, ar.path != nullptr);
}

// the device entry of both rules (mv null: the static one)
int plan_on_device(const char* who, const char* host_form, const ArmourRobot* robot, const uint8_t* continuous, TreeCall& ar, const Motion* mv, double* ms) {
    RmRobot rb;
    ARMOUR_TRY(check_args(who, robot, continuous, &rb, &ar));
    std::vector<double> mid, half;
    if (mv) ARMOUR_TRY(check_windows(who, ar.W, ar.O, *mv, &mid, &half));
    const int32_t W = ar.W, O = ar.O, max_nodes = ar.max_nodes, max_points = ar.max_points;
    int32_t *status = ar.status, *iterations = ar.iterations, *points = ar.points, *count = ar.count, *parent = ar.parent;
    double *path = ar.path, *nodes = ar.nodes;
    if (ms) *ms = 0.0;
    if (W == 0) return ARMOUR_OK;
    if (!armour_device_available()) { armour_set_error("%s: no HIP device visible (%s is the host form)", who, host_form); return ARMOUR_EDEVICE; }
    const int n = rb.n;
    const size_t Wn = (size_t)W * n, trees = (size_t)W * 2 * max_nodes, path_len = path ? (size_t)W * max_points * n : 0;
    DevStream st;
    EventPair ev;
    DevBuf<double> d_obs, d_starts, d_goals, d_nodes, d_path, d_vel, d_mid, d_half;
    DevBuf<uint64_t> d_seeds;
    DevBuf<int32_t> d_parent;
    DevColumns<int32_t> out;                              // status | iterations | points [W] each, then count [W][2]
    ARMOUR_TRY(st.create());
    ARMOUR_TRY(d_obs.upload(ar.obstacles, (size_t)W * O * ARMOUR_OBS_DOUBLES, st));
    ARMOUR_TRY(d_starts.upload(ar.starts, Wn, st));
    ARMOUR_TRY(d_goals.upload(ar.goals, Wn, st));
    ARMOUR_TRY(d_seeds.upload(ar.seeds, (size_t)W, st));
    MovingArgs dmv{};
    if (mv) {
        ARMOUR_TRY(d_vel.upload(mv->velocity, (size_t)W * O * 3, st));
        ARMOUR_TRY(d_mid.upload(mid.data(), (size_t)W, st));
        ARMOUR_TRY(d_half.upload(half.data(), (size_t)W, st));
        dmv = MovingArgs{d_vel, d_mid, d_half};
    }
    ARMOUR_TRY(d_nodes.reserve(trees * n));
    ARMOUR_TRY(d_parent.reserve(trees));
    ARMOUR_TRY(out.reserve(5, (size_t)W));
    if (path) ARMOUR_TRY(d_path.reserve(path_len));
    TreeArgs dev = ar;                                    // (the kernel's part)
    dev.obstacles = d_obs; dev.starts = d_starts; dev.goals = d_goals; dev.seeds = d_seeds;
    dev.status = out.column(0); dev.iterations = out.column(1); dev.points = out.column(2); dev.count = out.column(3);
    dev.parent = d_parent; dev.nodes = d_nodes; dev.path = path ? d_path.p : nullptr;
    // at the cap of 256 obstacles 54 KB (static) or 62 KB (moving) of dynamic LDS: above 48 KB, which a block may have once it asks
    const size_t lds = (size_t)O * (mv ? RM_MOV_STRIDE : RM_OBS_STRIDE) * sizeof(double);
    const void* kernel = mv ? reinterpret_cast<const void*>(tree_plan_kernel<true>) : reinterpret_cast<const void*>(tree_plan_kernel<false>);
    ARMOUR_TRY(grant_dynamic_lds(who, kernel, lds));
    ARMOUR_TRY(ev.record_start(st));
    if (mv) hipLaunchKernelGGL(tree_plan_kernel<true>, dim3((unsigned)W), dim3(TP_BLOCK), lds, st, rb, dev, dmv);
    else hipLaunchKernelGGL(tree_plan_kernel<false>, dim3((unsigned)W), dim3(TP_BLOCK), lds, st, rb, dev, dmv);
    HIPCHK(hipGetLastError());
    ARMOUR_TRY(ev.record_stop(st));
    ARMOUR_TRY(out.fetch(st));
    HIPCHK(hipStreamSynchronize(st));
    if (ms) ARMOUR_TRY(ev.elapsed_ms(ms));
    out.copy_out(0, status);
    out.copy_out(1, iterations);
    out.copy_out(2, points);
    out.copy_out(3, count, 2);
    const int32_t* h_count = out.fetched(3);
    // the trees and the paths: only the rows that were written come back (the rest of the caller's arrays is left as it was)
    for (int32_t w = 0; w < W; w++) {
        for (int k = 0; k < 2; k++) {
            const size_t row = (size_t)w * 2 + k, c = (size_t)h_count[2 * w + k];
            if (nodes && c) HIPCHK(hipMemcpyAsync(nodes + row * max_nodes * n, d_nodes + row * max_nodes * n, c * n * sizeof(double), hipMemcpyDeviceToHost, st));
            if (parent && c) HIPCHK(hipMemcpyAsync(parent + row * max_nodes, d_parent + row * max_nodes, c * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        }
        if (path && points[w] > 0 && points[w] <= max_points)
            HIPCHK(hipMemcpyAsync(path + (size_t)w * max_points * n, d_path + (size_t)w * max_points * n, (size_t)points[w] * n * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return armour_check_path_capacity(who, W, points, max_points, path != nullptr);
}

// an entry's arguments into the call record (the moving entries' three go beside it, in a Motion)
TreeCall tree_call(const double* lb, const double* ub, int32_t W, int32_t O, const double* obstacles, const double* starts, const double* goals, const uint64_t* seeds,
                   double step, double edge_step, int32_t max_iterations, int32_t max_nodes, int32_t max_points, int32_t* status, int32_t* iterations, int32_t* points,
                   double* path, int32_t* count, double* nodes, int32_t* parent) {
    TreeCall ar{};
    ar.box_lb = lb; ar.box_ub = ub; ar.W = W; ar.O = O; ar.obstacles = obstacles; ar.starts = starts; ar.goals = goals; ar.seeds = seeds;
    ar.step = step; ar.edge_step = edge_step; ar.max_iterations = max_iterations; ar.max_nodes = max_nodes; ar.max_points = max_points;
    ar.status = status; ar.iterations = iterations; ar.points = points; ar.path = path; ar.count = count; ar.nodes = nodes; ar.parent = parent;
    return ar;
}

}  // namespace

extern "C" int armour_tree_plan_host(const ArmourRobot* robot, const uint8_t* continuous, const double* lb, const double* ub, int32_t W, int32_t O,
                                     const double* obstacles, const double* starts, const double* goals, const uint64_t* seeds, double step, double edge_step,
                                     int32_t max_iterations, int32_t max_nodes, int32_t max_points, int32_t* status, int32_t* iterations, int32_t* points,
                                     double* path, int32_t* count, double* nodes, int32_t* parent, double* margin) {
    TreeCall ar = tree_call(lb, ub, W, O, obstacles, starts, goals, seeds, step, edge_step, max_iterations, max_nodes, max_points, status, iterations, points, path, count,
                            nodes, parent);
    return plan_on_host("armour_tree_plan_host", robot, continuous, ar, nullptr, margin);
}

extern "C" int armour_tree_plan_moving_host(const ArmourRobot* robot, const uint8_t* continuous, const double* lb, const double* ub, int32_t W, int32_t O,
                                            const double* obstacles, const double* velocity, const double* t_from, const double* t_to, const double* starts,
                                            const double* goals, const uint64_t* seeds, double step, double edge_step, int32_t max_iterations, int32_t max_nodes,
                                            int32_t max_points, int32_t* status, int32_t* iterations, int32_t* points, double* path, int32_t* count, double* nodes,
                                            int32_t* parent, double* margin) {
    TreeCall ar = tree_call(lb, ub, W, O, obstacles, starts, goals, seeds, step, edge_step, max_iterations, max_nodes, max_points, status, iterations, points, path, count,
                            nodes, parent);
    const Motion mv{velocity, t_from, t_to};
    return plan_on_host("armour_tree_plan_moving_host", robot, continuous, ar, &mv, margin);
}

extern "C" int armour_tree_plan(const ArmourRobot* robot, const uint8_t* continuous, const double* lb, const double* ub, int32_t W, int32_t O,
                                const double* obstacles, const double* starts, const double* goals, const uint64_t* seeds, double step, double edge_step,
                                int32_t max_iterations, int32_t max_nodes, int32_t max_points, int32_t* status, int32_t* iterations, int32_t* points, double* path,
                                int32_t* count, double* nodes, int32_t* parent, double* ms) {
    TreeCall ar = tree_call(lb, ub, W, O, obstacles, starts, goals, seeds, step, edge_step, max_iterations, max_nodes, max_points, status, iterations, points, path, count,
                            nodes, parent);
    return plan_on_device("armour_tree_plan", "armour_tree_plan_host", robot, continuous, ar, nullptr, ms);
}

extern "C" int armour_tree_plan_moving(const ArmourRobot* robot, const uint8_t* continuous, const double* lb, const double* ub, int32_t W, int32_t O,
                                       const double* obstacles, const double* velocity, const double* t_from, const double* t_to, const double* starts,
                                       const double* goals, const uint64_t* seeds, double step, double edge_step, int32_t max_iterations, int32_t max_nodes,
                                       int32_t max_points, int32_t* status, int32_t* iterations, int32_t* points, double* path, int32_t* count, double* nodes,
                                       int32_t* parent, double* ms) {
    TreeCall ar = tree_call(lb, ub, W, O, obstacles, starts, goals, seeds, step, edge_step, max_iterations, max_nodes, max_points, status, iterations, points, path, count,
                            nodes, parent);
    const Motion mv{velocity, t_from, t_to};
    return plan_on_device("armour_tree_plan_moving", "armour_tree_plan_moving_host", robot, continuous, ar, &mv, ms);
}
