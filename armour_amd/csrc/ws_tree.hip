// Batched workspace RRT* (include/armour_hip.h, armour_ws_tree_plan): the tree of the reference's end-effector planner
// (arm_end_effector_RRT_star_HLP over RRT_star_HLP / RRT_HLP) for W worlds in ONE launch, a block per world, the whole loop inside the block.
// A node is a point of the workspace and a test is an axis-aligned box against an obstacle: rmgeo::pair_separated as it stands, with the
// axes e_0, e_1, e_2.  What is new -- the difference and its squared length, S of an edge, one sub-segment's box, the steer step, the sample
// and the cost of a node -- is written once below as __host__ __device__ code, run by the kernel's lanes and by armour_ws_tree_plan_host's loop.
// The resident trees (armour_ws_trees_*, at the end of this file) are the same run resumed: the kernel's RESUMED form and the host loop with a
// world's state go on from the tree, the iteration index and the rewire count that a handle keeps between calls.
// The moving entries (armour_ws_tree_plan_moving) run the same loop with every box judged over its world's window: kernel and twin reach the
// box test and the stride of a staged obstacle through tree_block.h's Rule<MOVING> and nowhere else.  The resident trees
// stay static.
//
// Nothing but __syncthreads() orders the block: a tree's nodes live in global memory, written and read by this block alone (keeping them
// in LDS was measured and is a few per cent faster only where it fits, up to ~1700 nodes: DESIGN.md 4.12f); every decision
// that steers a loop is taken from values all lanes hold alike, so the barriers are reached by all of them.  The loop is bounded by
// max_iterations, a work list by count * ARMOUR_WS_MAX_SEGMENTS items, a scan and a path walk by the tree's count, the cost re-derivation
// by count passes.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "roadmap_handle.h"
#include "tree_block.h"

using namespace treeblk;   // the block shape, u(seed, i, j), key_less and, through it, rmgeo

namespace {

constexpr int WS_CAP = ARMOUR_WS_MAX_NODES;
constexpr int WS_STATE = 4;                              // words of a resident tree's state: count, iterations done, rewires, (spare)
constexpr int WS_PER_LANE = WS_CAP / TP_BLOCK;           // nodes per lane when the whole tree is dealt to the lanes: node t + k TP_BLOCK is lane t's k-th
static_assert(WS_PER_LANE * TP_BLOCK == WS_CAP && WS_PER_LANE <= 32, "a lane keeps one bit per node of its own");

// What a world's run reads: by value in the kernel's arguments (pointers: the device's; the host twin passes its own)
struct WsArgs {
    double lb[3], ub[3];
    double step, edge_step, rewire_radius, goal_rate, buffer, goal_tol;
    int32_t O, max_iterations, max_nodes, max_points, max_init;
    const double *obstacles, *starts, *goals, *init;
    const int32_t* init_count;
    const uint64_t* seeds;
    int32_t *status, *iterations, *points, *rewires, *chain_kept, *count, *parent;
    double *path_cost, *goal_dist, *path, *nodes, *node_cost, *node_len;
    // the resumed form alone (armour_ws_trees_grow): block / slot l serves world worlds[l]; state [W][WS_STATE] = a world's count, iterations
    // done and rewires between calls
    const int32_t* worlds;
    int32_t* state;
};
// an entry's arguments as it was given them: the kernel's, and what only check_args reads (it copies the box to lb / ub)
struct WsCall : WsArgs {
    const double *box_lb, *box_ub;
    int32_t W;
    bool resident;   // armour_ws_trees_create: no starts and no outputs yet
};

// ---- the scalar steps of the rule, one copy
// D = b - a component by component; returns acc = dot(D, D)
__host__ __device__ inline double ws_diff(const double* a, const double* b, double (&D)[3]) {
#pragma unroll
    for (int i = 0; i < 3; i++) D[i] = b[i] - a[i];
    return dot3(D, D);
}
// S of an edge of length len
__host__ __device__ inline int ws_segments(double len, double edge_step) {
    const double S = ceil(len / edge_step);
    return S < 1.0 ? 1 : S > (double)ARMOUR_WS_MAX_SEGMENTS ? ARMOUR_WS_MAX_SEGMENTS : (int)S;
}
// the box of sub-segment s of S of the edge a -> a + D with buffer buf: centre x, half-sizes h
__host__ __device__ inline void ws_sub_box(const double* a, const double (&D)[3], int s, int S, double buf, double (&x)[3], double (&h)[3]) {
    const double ts = (double)(2 * s + 1) / (double)(2 * S), two_S = (double)(2 * S);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        x[i] = a[i] + ts * D[i];
        h[i] = buf + fabs(D[i]) / two_S;
    }
}
// the box (x, e_0 e_1 e_2, h) against the staged obstacles [o0, o1) of the rule's view: true when every one separates (verdict mode).
// The rule (tree_block.h, Rule<MOVING>::box) is the static test or the window's, and holds the stride of the staging.
template <class R>
__host__ __device__ inline bool ws_box_free(const double (&x)[3], const double (&h)[3], const R& rule, int o0, int o1) {
    for (int o = o0; o < o1; o++)
        if (!rule.box(x, h, o, false, nullptr)) return false;
    return true;
}
// min over the obstacles of the pair clearance of that box (+inf without obstacles): what the host twin's margin is made of
template <class R>
inline double ws_box_clearance(const double (&x)[3], const double (&h)[3], const R& rule, int O) {
    double cl = INFINITY;
    for (int o = 0; o < O; o++) {
        double v;
        rule.box(x, h, o, true, &v);
        cl = std::fmin(cl, v);
    }
    return cl;
}
template <class R>
__host__ __device__ inline bool ws_sub_free(const double* a, const double (&D)[3], int s, int S, double buf, const R& rule, int o0, int o1) {
    double x[3], h[3];
    ws_sub_box(a, D, s, S, buf, x, h);
    return ws_box_free(x, h, rule, o0, o1);
}
// the sample of iteration i
__host__ __device__ inline void ws_sample(const WsArgs& a, uint64_t seed, int i, const double* goal, double (&qr)[3]) {
    const bool to_goal = tree_u(seed, (uint64_t)i, 3) < a.goal_rate;
#pragma unroll
    for (int j = 0; j < 3; j++) qr[j] = to_goal ? goal[j] : a.lb[j] + tree_u(seed, (uint64_t)i, (uint64_t)j) * (a.ub[j] - a.lb[j]);
}
// the steer step from the nearest node xv towards qr (D = qr - xv, dist = sqrt(dot(D, D)))
__host__ __device__ inline void ws_steer(const double* xv, const double (&qr)[3], const double (&D)[3], double dist, double step, double (&qn)[3]) {
    const double f = step / dist;
#pragma unroll
    for (int j = 0; j < 3; j++) qn[j] = dist <= step ? qr[j] : xv[j] + f * D[j];
}

// component t of a point that every lane holds, by selects: no array of a lane's own is indexed at run time (no scratch memory)
__device__ inline double pick3(const double (&a)[3], int t) { return t == 0 ? a[0] : t == 1 ? a[1] : a[2]; }

// ---- the block's cooperative steps: tree_block.h's block_any / block_scan / block_argmin, every call released by the step's own trailing
// barrier.  The obstacle split and the owner search of a round stay inline below: through obstacle_split / item_owner the kernel measured
// 1.7 % slower.
struct WsShared {
    BlockKeys keys;
    BlockWords sums, any;            // the scan's and the any step's words
    int cand[TP_BLOCK];              // a round's candidates (node indices)
    int end[TP_BLOCK];               // one past the last work item of round candidate k
    unsigned char hit[TP_BLOCK];     // 1: some sub-segment of round candidate k did not separate
    unsigned char free_[WS_CAP];     // per node: 1 = a candidate of this iteration whose edge to qn is free
};

// the edge a -> a + D of S sub-segments, dealt to the lanes in chunks of TP_BLOCK: free when every sub-segment separates
template <class R>
__device__ inline bool block_edge_free(WsShared& sh, const double* a, const double (&D)[3], int S, double buf, const R& rule, int O) {
    bool hit = false;
    for (int s = threadIdx.x; s < S; s += TP_BLOCK) hit = hit || !ws_sub_free(a, D, s, S, buf, rule, 0, O);
    return !block_any(sh.any, hit);
}

// grid W, dynamic LDS [O][Rule<MOVING>::STRIDE] doubles.  The tree of world w: nodes [w][max_nodes][3], parent / node_cost / node_len [w][max_nodes].
// RESUMED (armour_ws_trees_grow; grid L): slot l = blockIdx.x serves world w = worlds[l] -- the start and every output are slot l's, the
// obstacles, the goal, the seed and the tree world w's -- and the tree goes on from state[w]: a planted tree (count > 0) skips the start test,
// iteration i of this launch is iteration base + i of the world, and the state is written back at the end.  Not resumed, l = w, base = 0 and
// every `RESUMED` below is a constant: the plan kernel is the code it was.
// MOVING (armour_ws_tree_plan_moving; never RESUMED): the window rule -- dynamic LDS [O][RM_MOV_STRIDE], mv.velocity [W][O][3], mv.mid / mv.half
// [W], this world's two kept in registers.  The static instantiations read nothing of mv.  Every box test below goes through `rule`.
template <bool RESUMED, bool MOVING>
__global__ __launch_bounds__(TP_BLOCK) void ws_tree_kernel(WsArgs ar, MovingArgs mv) {
    static_assert(!(RESUMED && MOVING), "the resident trees stay static");
    extern __shared__ double s_obs[];   // [O][RM_OBS_STRIDE], MOVING: [O][RM_MOV_STRIDE]
    __shared__ WsShared sh;
    const int l = blockIdx.x, w = RESUMED ? ar.worlds[l] : l, t = threadIdx.x, O = ar.O, cap = ar.max_nodes;
    Rule<MOVING> rule{s_obs};
    if constexpr (MOVING) {
        rule.mid = mv.mid[w];
        rule.half = mv.half[w];
        stage_obstacles_moving_lds<TP_BLOCK>(ar.obstacles + (size_t)w * O * ARMOUR_OBS_DOUBLES, mv.velocity + (size_t)w * O * 3, O, s_obs);
    } else {
        stage_obstacles_lds<TP_BLOCK>(ar.obstacles + (size_t)w * O * ARMOUR_OBS_DOUBLES, O, s_obs);
    }
    for (int c = t; c < cap; c += TP_BLOCK) sh.free_[c] = 0;
    const uint64_t seed = ar.seeds[w];
    const double buf = ar.buffer, rr2 = ar.rewire_radius * ar.rewire_radius;
    int cnt = 0, base = 0, rewires = 0;
    if (RESUMED) {
        cnt = ar.state[(size_t)w * WS_STATE];
        base = ar.state[(size_t)w * WS_STATE + 1];
        rewires = ar.state[(size_t)w * WS_STATE + 2];
    }
    const bool planted = RESUMED && cnt > 0;                // (the same in every lane) the start is not read
    double start[3], goal[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        start[j] = planted ? 0.0 : ar.starts[(size_t)l * 3 + j];
        goal[j] = ar.goals[(size_t)w * 3 + j];
    }
    double* nx = ar.nodes + (size_t)w * cap * 3;
    double* ncost = ar.node_cost + (size_t)w * cap;
    double* nlen = ar.node_len + (size_t)w * cap;
    int32_t* par = ar.parent + (size_t)w * cap;
    int status = ARMOUR_WS_START_BLOCKED, iterations = 0, points = 0, kept = 0;
    double path_cost = 0.0, goal_dist;
    {
        double D[3];
        goal_dist = sqrt(ws_diff(start, goal, D));
    }

    // ---- the point rule at start: the obstacles dealt to the lanes
    bool hit = false;
    if (!planted) {
        const double h[3] = {buf, buf, buf};
        for (int o = t; o < O; o += TP_BLOCK) hit = hit || !ws_box_free(start, h, rule, o, o + 1);
    }
    if (planted || !block_any(sh.any, hit)) {
        if (!planted) {
            if (t < 3) nx[t] = pick3(start, t);
            if (t == 0) { par[0] = -1; ncost[0] = 0.0; nlen[0] = 0.0; }
            cnt = 1;
        }
        // ---- the initial chain: edge by edge from the last kept node, up to the first edge that is not free
        const int chain = !RESUMED && ar.init ? ar.init_count[w] : 0;
        double prev[3] = {start[0], start[1], start[2]}, prev_cost = 0.0;
        for (int c = 0; c < chain && cnt < cap; c++) {
            double x[3], D[3];
#pragma unroll
            for (int j = 0; j < 3; j++) x[j] = ar.init[((size_t)w * ar.max_init + c) * 3 + j];
            const double d = sqrt(ws_diff(prev, x, D));
            if (!block_edge_free(sh, prev, D, ws_segments(d, ar.edge_step), buf, rule, O)) break;
            prev_cost = prev_cost + d;
            if (t < 3) nx[(size_t)cnt * 3 + t] = pick3(x, t);
            if (t == 0) { par[cnt] = cnt - 1; nlen[cnt] = d; ncost[cnt] = prev_cost; }
#pragma unroll
            for (int j = 0; j < 3; j++) prev[j] = x[j];
            cnt++;
            kept++;
        }
        iterations = base + ar.max_iterations;
        for (int i = 0; i < ar.max_iterations; i++) {
            if (cnt >= cap) { iterations = base + i; break; }
            __syncthreads();                                // the nodes, parents and costs of iteration i - 1 (or of the launch before) are written
            // ---- sample (every lane: the same arithmetic on the same values), nearest, steer
            double qr[3], qn[3], D[3];
            ws_sample(ar, seed, base + i, goal, qr);
            double acc = INFINITY;
            int v = TP_NONE;
            for (int c = t; c < cnt; c += TP_BLOCK) {
                const double d2 = ws_diff(nx + (size_t)c * 3, qr, D);
                if (key_less(d2, c, acc, v)) { acc = d2; v = c; }
            }
            block_argmin(sh.keys, &acc, &v);
            if (acc == 0.0) continue;
            {
                const double xv[3] = {nx[(size_t)v * 3], nx[(size_t)v * 3 + 1], nx[(size_t)v * 3 + 2]};
                ws_diff(xv, qr, D);
                ws_steer(xv, qr, D, sqrt(acc), ar.step, qn);
            }
            // ---- near set: bit k of `mine` = node t + k TP_BLOCK is a candidate; ranks in lane-major order
            unsigned mine = 0;
#pragma unroll
            for (int k = 0; k < WS_PER_LANE; k++) {
                const int c = t + k * TP_BLOCK;
                if (c < cnt && (c == v || ws_diff(nx + (size_t)c * 3, qn, D) <= rr2)) mine |= 1u << k;
            }
            int C;
            const int rank0 = block_scan(sh.sums, __popc(mine), &C) - __popc(mine);
            // ---- edge tests, TP_BLOCK candidates to a round: a flat list of (candidate, sub-segment) items across the lanes
            for (int r0 = 0; r0 < C; r0 += TP_BLOCK) {
                const int Cr = C - r0 < TP_BLOCK ? C - r0 : TP_BLOCK;
                int rank = rank0;
                for (unsigned m = mine; m; m &= m - 1, rank++)
                    if (rank >= r0 && rank < r0 + TP_BLOCK) sh.cand[rank - r0] = t + (__ffs((int)m) - 1) * TP_BLOCK;
                sh.hit[t] = 0;
                __syncthreads();
                const int c = t < Cr ? sh.cand[t] : 0;
                int S = 0;
                if (t < Cr) S = ws_segments(sqrt(ws_diff(nx + (size_t)c * 3, qn, D)), ar.edge_step);
                int T;
                sh.end[t] = block_scan(sh.sums, S, &T);
                __syncthreads();
                // a short list gives each item G = min(O, TP_BLOCK / T) lanes, lane g of them with the obstacles [g O / G, (g + 1) O / G):
                // tree_block.h's obstacle_split, which says why it is sound, inline
                int G = 1;
                if (2 * T <= TP_BLOCK && O > 1) G = TP_BLOCK / T < O ? TP_BLOCK / T : O;
                const int per = TP_BLOCK / G, g = t % G, o0 = (g * O) / G, o1 = ((g + 1) * O) / G;
                for (int base = 0; base < T; base += per) {
                    const int it = base + t / G;
                    if (t < per * G && it < T) {
                        int lo = 0, hi = Cr - 1;            // the candidate of item `it`: the first k with end[k] > it
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            if (sh.end[mid] > it) hi = mid; else lo = mid + 1;
                        }
                        const int first = lo ? sh.end[lo - 1] : 0;
                        const double* xc = nx + (size_t)sh.cand[lo] * 3;
                        ws_diff(xc, qn, D);
                        if (!ws_sub_free(xc, D, it - first, sh.end[lo] - first, buf, rule, o0, o1)) sh.hit[lo] = 1;   // every lane that stores, stores this 1
                    }
                }
                __syncthreads();
                if (t < Cr) sh.free_[c] = sh.hit[t] ? 0 : 1;
                __syncthreads();                            // sh.cand / sh.end / sh.hit have been read: the next round may write them
            }
            // ---- parent: the free candidate with the smallest (cost_c + d_c, c)
            double pk = INFINITY;
            int p = TP_NONE;
            for (unsigned m = mine; m; m &= m - 1) {
                const int c = t + (__ffs((int)m) - 1) * TP_BLOCK;
                if (!sh.free_[c]) continue;
                const double key = ncost[c] + sqrt(ws_diff(nx + (size_t)c * 3, qn, D));
                if (key_less(key, c, pk, p)) { pk = key; p = c; }
            }
            block_argmin(sh.keys, &pk, &p);
            if (p == TP_NONE) continue;                     // (no candidate is free: no flag is set)
            const double d_p = sqrt(ws_diff(nx + (size_t)p * 3, qn, D)), cost_qn = ncost[p] + d_p;
            // ---- rewire: each free candidate decides for itself, on the costs as they stand; the flags are cleared for the next iteration
            int mine_rewired = 0;
            for (unsigned m = mine; m; m &= m - 1) {
                const int c = t + (__ffs((int)m) - 1) * TP_BLOCK;
                if (!sh.free_[c]) continue;
                sh.free_[c] = 0;
                if (c == p) continue;
                const double d_c = sqrt(ws_diff(nx + (size_t)c * 3, qn, D));
                if (cost_qn + d_c < ncost[c]) { par[c] = cnt; nlen[c] = d_c; mine_rewired++; }
            }
            if (t < 3) nx[(size_t)cnt * 3 + t] = pick3(qn, t);
            if (t == 0) { par[cnt] = p; nlen[cnt] = d_p; ncost[cnt] = cost_qn; }
            cnt++;
            int rewired;
            block_scan(sh.sums, mine_rewired, &rewired);         // (its barriers: the new node, the parents and the lengths are written)
            rewires += rewired;
            // ---- cost re-derivation: cost_k = cost_parent(k) + len_k in passes, each reading the pass before, until a pass changes nothing
            for (int pass = 0; rewired > 0 && pass < cnt; pass++) {
                double nv[WS_PER_LANE];
                bool changed = false;
#pragma unroll
                for (int k = 0; k < WS_PER_LANE; k++) {
                    const int c = t + k * TP_BLOCK;
                    nv[k] = 0.0;
                    if (c < cnt && par[c] >= 0) {
                        nv[k] = ncost[par[c]] + nlen[c];
                        changed = changed || nv[k] != ncost[c];
                    }
                }
                __syncthreads();                            // every lane has read the costs of the pass before
#pragma unroll
                for (int k = 0; k < WS_PER_LANE; k++) {
                    const int c = t + k * TP_BLOCK;
                    if (c < cnt && par[c] >= 0) ncost[c] = nv[k];
                }
                if (!block_any(sh.any, changed)) break;         // (its barriers: the costs of this pass are written)
            }
        }
        __syncthreads();
        // ---- best node: within goal_tol the smallest (cost + distance, index), else the smallest (squared distance, index)
        double bk = INFINITY, ba = INFINITY;
        int bi = TP_NONE, ai = TP_NONE;
        for (int c = t; c < cnt; c += TP_BLOCK) {
            double D[3];
            const double g2 = ws_diff(nx + (size_t)c * 3, goal, D), g = sqrt(g2);
            if (key_less(g2, c, ba, ai)) { ba = g2; ai = c; }
            if (g <= ar.goal_tol) {
                const double key = ncost[c] + g;
                if (key_less(key, c, bk, bi)) { bk = key; bi = c; }
            }
        }
        block_argmin(sh.keys, &bk, &bi);
        block_argmin(sh.keys, &ba, &ai);
        status = bi != TP_NONE ? ARMOUR_WS_REACHED : ARMOUR_WS_PARTIAL;
        const int best = bi != TP_NONE ? bi : ai;
        {
            double D[3];
            goal_dist = sqrt(ws_diff(nx + (size_t)best * 3, goal, D));
        }
        path_cost = ncost[best];
        // the path root -> best: two walks, bounded by the count
        int len = 0;
        for (int x = best; x >= 0 && x < cnt && len < cnt; x = par[x]) len++;
        points = len;
        if (ar.path && points <= ar.max_points && t < 3) {
            double* out = ar.path + ((size_t)l * ar.max_points) * 3;
            int pos = len - 1, d = 0;
            for (int x = best; d < len; x = par[x], d++, pos--) out[(size_t)pos * 3 + t] = nx[(size_t)x * 3 + t];
        }
    }
    if (t == 0) {
        ar.status[l] = status;
        ar.iterations[l] = iterations;
        ar.points[l] = points;
        ar.rewires[l] = rewires;
        ar.chain_kept[l] = kept;
        ar.count[l] = cnt;
        ar.path_cost[l] = path_cost;
        ar.goal_dist[l] = goal_dist;
        if (RESUMED) {                                      // (a blocked start leaves count 0, 0 iterations, 0 rewires)
            ar.state[(size_t)w * WS_STATE] = cnt;
            ar.state[(size_t)w * WS_STATE + 1] = iterations;
            ar.state[(size_t)w * WS_STATE + 2] = rewires;
        }
    }
}

// ---- the host twin: the same functions in a loop.  margin (may be null): min |clearance| over the checks that decide.
template <class R>
struct WsHost {
    R rule;
    int O;
    double buf, edge_step;
    double* margin;

    void note(const double (&x)[3], const double (&h)[3]) const {
        if (margin) *margin = std::fmin(*margin, std::fabs(ws_box_clearance(x, h, rule, O)));
    }
    bool point(const double* p) const {
        const double x[3] = {p[0], p[1], p[2]}, h[3] = {buf, buf, buf};
        note(x, h);
        return ws_box_free(x, h, rule, 0, O);
    }
    // prefix(a, b): sub-segments in ascending order up to the first that does not separate; free when m == S
    bool edge(const double* a, const double* b) const {
        double D[3];
        const int S = ws_segments(sqrt(ws_diff(a, b, D)), edge_step);
        for (int s = 0; s < S; s++) {
            double x[3], h[3];
            ws_sub_box(a, D, s, S, buf, x, h);
            note(x, h);
            if (!ws_box_free(x, h, rule, 0, O)) return false;
        }
        return true;
    }
};

// slot l = world w of the host twin (the plan entry: l = w); the tree goes to nx [max_nodes][3] / par / ncost / nlen [max_nodes] (the caller's
// rows or scratch).  state (null: the plan entry): world w's WS_STATE words of a handle -- the run resumes the tree they describe, as the
// kernel's resumed form does, and writes them back.  rule: the world's staged obstacles with the static rule or its window's; O their number.
template <class R>
void plan_world_host(const WsArgs& ar, int l, int w, const R& rule, double* nx, int32_t* par, double* ncost, double* nlen, double* margin, int32_t* state) {
    const int cap = ar.max_nodes;
    const double* goal = ar.goals + (size_t)w * 3;
    const uint64_t seed = ar.seeds[w];
    const double rr2 = ar.rewire_radius * ar.rewire_radius;
    if (margin) *margin = INFINITY;
    const WsHost<R> hw{rule, ar.O, ar.buffer, ar.edge_step, margin};
    double D[3];
    int cnt = state ? state[0] : 0, rewires = state ? state[2] : 0, kept = 0;
    const int base = state ? state[1] : 0;
    if (cnt == 0) {
        const double* start = ar.starts + (size_t)l * 3;
        ar.status[l] = ARMOUR_WS_START_BLOCKED;
        ar.iterations[l] = ar.points[l] = ar.rewires[l] = ar.chain_kept[l] = 0;
        if (ar.count) ar.count[l] = 0;
        ar.path_cost[l] = 0.0;
        ar.goal_dist[l] = sqrt(ws_diff(start, goal, D));
        if (!hw.point(start)) return;
        std::memcpy(nx, start, 3 * sizeof(double));
        par[0] = -1; ncost[0] = 0.0; nlen[0] = 0.0;
        cnt = 1;
    }
    const int chain = !state && ar.init ? ar.init_count[w] : 0;
    for (int c = 0; c < chain && cnt < cap; c++) {
        const double* x = ar.init + ((size_t)w * ar.max_init + c) * 3;
        const double* prev = nx + (size_t)(cnt - 1) * 3;
        if (!hw.edge(prev, x)) break;
        const double d = sqrt(ws_diff(prev, x, D));
        std::memcpy(nx + (size_t)cnt * 3, x, 3 * sizeof(double));
        par[cnt] = cnt - 1; nlen[cnt] = d; ncost[cnt] = ncost[cnt - 1] + d;
        cnt++;
        kept++;
    }
    int iterations = base + ar.max_iterations;
    std::vector<int> free_c;
    std::vector<double> free_d;
    for (int i = 0; i < ar.max_iterations; i++) {
        if (cnt >= cap) { iterations = base + i; break; }
        double qr[3], qn[3];
        ws_sample(ar, seed, base + i, goal, qr);
        double acc = INFINITY;
        int v = TP_NONE;
        for (int c = 0; c < cnt; c++) {
            const double d2 = ws_diff(nx + (size_t)c * 3, qr, D);
            if (key_less(d2, c, acc, v)) { acc = d2; v = c; }
        }
        if (acc == 0.0) continue;
        ws_diff(nx + (size_t)v * 3, qr, D);
        ws_steer(nx + (size_t)v * 3, qr, D, sqrt(acc), ar.step, qn);
        free_c.clear(); free_d.clear();
        double pk = INFINITY;
        int p = TP_NONE;
        for (int c = 0; c < cnt; c++) {
            const double d2 = ws_diff(nx + (size_t)c * 3, qn, D);
            if (!(c == v || d2 <= rr2) || !hw.edge(nx + (size_t)c * 3, qn)) continue;
            const double d_c = sqrt(d2), key = ncost[c] + d_c;
            free_c.push_back(c); free_d.push_back(d_c);
            if (key_less(key, c, pk, p)) { pk = key; p = c; }
        }
        if (p == TP_NONE) continue;
        const double d_p = sqrt(ws_diff(nx + (size_t)p * 3, qn, D)), cost_qn = ncost[p] + d_p;
        int rewired = 0;
        for (size_t k = 0; k < free_c.size(); k++) {
            const int c = free_c[k];
            if (c != p && cost_qn + free_d[k] < ncost[c]) { par[c] = cnt; nlen[c] = free_d[k]; rewired++; }
        }
        std::memcpy(nx + (size_t)cnt * 3, qn, 3 * sizeof(double));
        par[cnt] = p; nlen[cnt] = d_p; ncost[cnt] = cost_qn;
        cnt++;
        rewires += rewired;
        // the costs, re-derived in place: the same fixed point as the kernel's passes (the definition is recursive from the root)
        for (int pass = 0; rewired > 0 && pass < cnt; pass++) {
            bool changed = false;
            for (int c = 1; c < cnt; c++) {
                const double nv = ncost[par[c]] + nlen[c];
                if (nv != ncost[c]) { ncost[c] = nv; changed = true; }
            }
            if (!changed) break;
        }
    }
    double bk = INFINITY, ba = INFINITY;
    int bi = TP_NONE, ai = TP_NONE;
    for (int c = 0; c < cnt; c++) {
        const double g2 = ws_diff(nx + (size_t)c * 3, goal, D), g = sqrt(g2);
        if (key_less(g2, c, ba, ai)) { ba = g2; ai = c; }
        if (g <= ar.goal_tol) {
            const double key = ncost[c] + g;
            if (key_less(key, c, bk, bi)) { bk = key; bi = c; }
        }
    }
    const int best = bi != TP_NONE ? bi : ai;
    int len = 0;
    for (int x = best; x >= 0 && x < cnt && len < cnt; x = par[x]) len++;
    ar.status[l] = bi != TP_NONE ? ARMOUR_WS_REACHED : ARMOUR_WS_PARTIAL;
    ar.iterations[l] = iterations;
    ar.points[l] = len;
    ar.rewires[l] = rewires;
    ar.chain_kept[l] = kept;
    if (ar.count) ar.count[l] = cnt;
    ar.path_cost[l] = ncost[best];
    ar.goal_dist[l] = sqrt(ws_diff(nx + (size_t)best * 3, goal, D));
    if (state) { state[0] = cnt; state[1] = iterations; state[2] = rewires; }
    if (ar.path && len <= ar.max_points) {
        double* out = ar.path + ((size_t)l * ar.max_points) * 3;
        int pos = len - 1, d = 0;
        for (int x = best; d < len; x = par[x], d++, pos--) std::memcpy(out + (size_t)pos * 3, nx + (size_t)x * 3, 3 * sizeof(double));
    }
}

// the argument rules of the plan entries and of armour_ws_trees_create (`resident`: everything but the starts and the outputs, which come with
// a grow), before a device is touched, on ar as the entry filled it; fills ar.lb / ar.ub and drops a chain's length and counts when there is
// no chain
int check_args(const char* who, WsCall* ar) {
    const int32_t W = ar->W, O = ar->O, max_init = ar->max_init;
    const double step = ar->step, edge_step = ar->edge_step, rewire_radius = ar->rewire_radius;
    if (!ar->box_lb || !ar->box_ub) { armour_set_error("%s: null argument", who); return ARMOUR_EINVAL; }
    ARMOUR_TRY(armour_check_world_counts(who, W, O, ar->obstacles));
    if (W > 0 && (!ar->goals || !ar->seeds || (!ar->resident && (!ar->starts || !ar->status || !ar->iterations || !ar->points || !ar->rewires || !ar->chain_kept || !ar->path_cost || !ar->goal_dist)))) {
        armour_set_error("%s: null argument", who);
        return ARMOUR_EINVAL;
    }
    if (ar->max_nodes < 1 || ar->max_nodes > ARMOUR_WS_MAX_NODES || ar->max_iterations < 0 || ar->max_iterations > ARMOUR_TREE_MAX_ITERATIONS || ar->max_points < 0) {
        armour_set_error("%s: max_nodes = %d (1..%d), max_iterations = %d (0..%d), max_points = %d", who, ar->max_nodes, ARMOUR_WS_MAX_NODES, ar->max_iterations,
                         ARMOUR_TREE_MAX_ITERATIONS, ar->max_points);
        return ARMOUR_EINVAL;
    }
    const double reals[6] = {step, edge_step, rewire_radius, ar->goal_rate, ar->buffer, ar->goal_tol};
    if (!finite_all(reals, 6) || !(step > 0.0) || !(edge_step > 0.0) || rewire_radius < 0.0 || ar->buffer < 0.0 || ar->goal_tol < 0.0 || ar->goal_rate < 0.0 || ar->goal_rate > 1.0) {
        armour_set_error("%s: step = %g, edge_step = %g (> 0), rewire_radius = %g, buffer = %g, goal_tol = %g (>= 0), goal_rate = %g (0..1)", who, step, edge_step,
                         rewire_radius, ar->buffer, ar->goal_tol, ar->goal_rate);
        return ARMOUR_EINVAL;
    }
    ARMOUR_TRY(armour_check_box(who, "sampling box", "axis", 3, ar->box_lb, ar->box_ub));
    if (!finite_all(ar->obstacles, (size_t)W * O * ARMOUR_OBS_DOUBLES) || (!ar->resident && !finite_all(ar->starts, (size_t)W * 3)) || !finite_all(ar->goals, (size_t)W * 3)) {
        armour_set_error("%s: a start, a goal or an obstacle is not finite", who);
        return ARMOUR_EINVAL;
    }
    if (!(std::ceil(std::fmax(step, rewire_radius) / edge_step) <= (double)ARMOUR_WS_MAX_SEGMENTS)) {
        armour_set_error("%s: step = %g, rewire_radius = %g: more than %d sub-segments of edge_step %g", who, step, rewire_radius, ARMOUR_WS_MAX_SEGMENTS, edge_step);
        return ARMOUR_EINVAL;
    }
    if (ar->init) {
        if (max_init < 1 || (W > 0 && !ar->init_count)) { armour_set_error("%s: max_init = %d (>= 1 with init), init_count", who, max_init); return ARMOUR_EINVAL; }
        for (int32_t w = 0; w < W; w++) {
            const int32_t c = ar->init_count[w];
            if (c < 0 || c > max_init) { armour_set_error("%s: init_count[%d] = %d (0..%d)", who, w, c, max_init); return ARMOUR_EINVAL; }
            const double* x = ar->init + (size_t)w * max_init * 3;
            if (!finite_all(x, (size_t)c * 3)) { armour_set_error("%s: world %d's chain is not finite", who, w); return ARMOUR_EINVAL; }
            const double* prev = ar->starts + (size_t)w * 3;
            for (int32_t k = 0; k < c; prev = x + (size_t)k * 3, k++) {
                double D[3];
                const double len = std::sqrt(ws_diff(prev, x + (size_t)k * 3, D));
                if (!(std::ceil(len / edge_step) <= (double)ARMOUR_WS_MAX_SEGMENTS)) {
                    armour_set_error("%s: world %d's chain edge %d of length %g: more than %d sub-segments of edge_step %g", who, w, k, len, ARMOUR_WS_MAX_SEGMENTS, edge_step);
                    return ARMOUR_EINVAL;
                }
            }
        }
    } else {
        ar->max_init = 0;
        ar->init_count = nullptr;
    }
    for (int j = 0; j < 3; j++) { ar->lb[j] = ar->box_lb[j]; ar->ub[j] = ar->box_ub[j]; }
    return ARMOUR_OK;
}

// the host twin of both rules (mv null: the static one)
int plan_on_host(const char* who, WsCall& ar, const Motion* mv, double* margin) {
    ARMOUR_TRY(check_args(who, &ar));
    std::vector<double> mid, half;
    if (mv) ARMOUR_TRY(check_windows(who, ar.W, ar.O, *mv, &mid, &half));
    const size_t cap = (size_t)ar.max_nodes;
    double *nodes = ar.nodes, *node_cost = ar.node_cost;
    int32_t* parent = ar.parent;
    std::vector<double> own_nodes(nodes ? 0 : cap * 3), own_cost(node_cost ? 0 : cap), len(cap);
    std::vector<int32_t> own_parent(parent ? 0 : cap);
    auto world = [&](int32_t w, const auto& rule, int) {
        plan_world_host(ar, w, w, rule, nodes ? nodes + (size_t)w * cap * 3 : own_nodes.data(), parent ? parent + (size_t)w * cap : own_parent.data(),
                        node_cost ? node_cost + (size_t)w * cap : own_cost.data(), len.data(), margin ? margin + w : nullptr, nullptr);
    };
    if (mv) for_each_staged<true>(ar.W, ar.O, ar.obstacles, nullptr, world, mv->velocity, mid.data(), half.data());
    else for_each_staged(ar.W, ar.O, ar.obstacles, nullptr, world);
    return armour_check_path_capacity(who, ar.W, ar.points, ar.max_points, ar.path != nullptr);
}

// the device entry of both rules (mv null: the static one)
int plan_on_device(const char* who, const char* host_form, WsCall& ar, const Motion* mv, double* ms) {
    ARMOUR_TRY(check_args(who, &ar));
    std::vector<double> mid, half;
    if (mv) ARMOUR_TRY(check_windows(who, ar.W, ar.O, *mv, &mid, &half));
    const int32_t W = ar.W, O = ar.O, max_nodes = ar.max_nodes, max_points = ar.max_points, max_init = ar.max_init;
    const double* init = ar.init;
    int32_t *points = ar.points, *parent = ar.parent;
    double *path = ar.path, *nodes = ar.nodes, *node_cost = ar.node_cost;
    if (ms) *ms = 0.0;
    if (W == 0) return ARMOUR_OK;
    if (!armour_device_available()) { armour_set_error("%s: no HIP device visible (%s is the host form)", who, host_form); return ARMOUR_EDEVICE; }
    const size_t cap = (size_t)max_nodes, rows = (size_t)W * cap, path_len = path ? (size_t)W * max_points * 3 : 0;
    DevStream st;
    EventPair ev;
    DevBuf<double> d_obs, d_starts, d_goals, d_init, d_nodes, d_cost, d_len, d_path, d_vel, d_mid, d_half;
    DevBuf<uint64_t> d_seeds;
    DevBuf<int32_t> d_init_count, d_parent;
    DevColumns<int32_t> out;                                // status | iterations | points | rewires | chain_kept | count [W] each
    DevColumns<double> real;                                // path_cost | goal_dist [W] each
    ARMOUR_TRY(st.create());
    ARMOUR_TRY(d_obs.upload(ar.obstacles, (size_t)W * O * ARMOUR_OBS_DOUBLES, st));
    ARMOUR_TRY(d_starts.upload(ar.starts, (size_t)W * 3, st));
    ARMOUR_TRY(d_goals.upload(ar.goals, (size_t)W * 3, st));
    ARMOUR_TRY(d_seeds.upload(ar.seeds, (size_t)W, st));
    if (init) {
        ARMOUR_TRY(d_init.upload(init, (size_t)W * max_init * 3, st));
        ARMOUR_TRY(d_init_count.upload(ar.init_count, (size_t)W, st));
    }
    MovingArgs dmv{};
    if (mv) {
        ARMOUR_TRY(d_vel.upload(mv->velocity, (size_t)W * O * 3, st));
        ARMOUR_TRY(d_mid.upload(mid.data(), (size_t)W, st));
        ARMOUR_TRY(d_half.upload(half.data(), (size_t)W, st));
        dmv = MovingArgs{d_vel, d_mid, d_half};
    }
    ARMOUR_TRY(d_nodes.reserve(rows * 3));
    ARMOUR_TRY(d_cost.reserve(rows));
    ARMOUR_TRY(d_len.reserve(rows));
    ARMOUR_TRY(d_parent.reserve(rows));
    ARMOUR_TRY(out.reserve(6, (size_t)W));
    ARMOUR_TRY(real.reserve(2, (size_t)W));
    if (path) ARMOUR_TRY(d_path.reserve(path_len));
    WsArgs dev = ar;                                        // (the kernel's part)
    dev.obstacles = d_obs; dev.starts = d_starts; dev.goals = d_goals; dev.seeds = d_seeds;
    dev.init = init ? d_init.p : nullptr; dev.init_count = init ? d_init_count.p : nullptr;
    dev.status = out.column(0); dev.iterations = out.column(1); dev.points = out.column(2); dev.rewires = out.column(3);
    dev.chain_kept = out.column(4); dev.count = out.column(5);
    dev.path_cost = real.column(0); dev.goal_dist = real.column(1);
    dev.parent = d_parent; dev.nodes = d_nodes; dev.node_cost = d_cost; dev.node_len = d_len; dev.path = path ? d_path.p : nullptr;
    // at the cap of 256 obstacles 54 KB (static) or 62 KB (moving) of dynamic LDS: above 48 KB, which a block may have once it asks
    const size_t lds = (size_t)O * (mv ? Rule<true>::STRIDE : Rule<false>::STRIDE) * sizeof(double);
    const void* kernel = mv ? reinterpret_cast<const void*>(ws_tree_kernel<false, true>) : reinterpret_cast<const void*>(ws_tree_kernel<false, false>);
    ARMOUR_TRY(grant_dynamic_lds(who, kernel, lds));
    ARMOUR_TRY(ev.record_start(st));
    if (mv) hipLaunchKernelGGL((ws_tree_kernel<false, true>), dim3((unsigned)W), dim3(TP_BLOCK), lds, st, dev, dmv);
    else hipLaunchKernelGGL((ws_tree_kernel<false, false>), dim3((unsigned)W), dim3(TP_BLOCK), lds, st, dev, dmv);
    HIPCHK(hipGetLastError());
    ARMOUR_TRY(ev.record_stop(st));
    ARMOUR_TRY(out.fetch(st));
    ARMOUR_TRY(real.fetch(st));
    HIPCHK(hipStreamSynchronize(st));
    if (ms) ARMOUR_TRY(ev.elapsed_ms(ms));
    int32_t* const ints[6] = {ar.status, ar.iterations, points, ar.rewires, ar.chain_kept, ar.count};
    for (int k = 0; k < 6; k++) out.copy_out(k, ints[k]);
    const int32_t* h_count = out.fetched(5);
    real.copy_out(0, ar.path_cost);
    real.copy_out(1, ar.goal_dist);
    // the trees and the paths: only the rows that were written come back (the rest of the caller's arrays is left as it was)
    for (int32_t w = 0; w < W; w++) {
        const size_t c = (size_t)h_count[w], row = (size_t)w * cap;
        if (nodes && c) HIPCHK(hipMemcpyAsync(nodes + row * 3, d_nodes + row * 3, c * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        if (parent && c) HIPCHK(hipMemcpyAsync(parent + row, d_parent + row, c * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (node_cost && c) HIPCHK(hipMemcpyAsync(node_cost + row, d_cost + row, c * sizeof(double), hipMemcpyDeviceToHost, st));
        if (path && points[w] > 0 && points[w] <= max_points)
            HIPCHK(hipMemcpyAsync(path + (size_t)w * max_points * 3, d_path + (size_t)w * max_points * 3, (size_t)points[w] * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return armour_check_path_capacity(who, W, points, max_points, path != nullptr);
}

// an entry's arguments into the call record (the moving entries' three go beside it, in a Motion)
WsCall ws_call(const double* lb, const double* ub, int32_t W, int32_t O, const double* obstacles, const double* starts, const double* goals, const uint64_t* seeds,
               int32_t max_init, const double* init, const int32_t* init_count, double step, double edge_step, double rewire_radius, double goal_rate, double buffer,
               double goal_tol, int32_t max_iterations, int32_t max_nodes, int32_t max_points, int32_t* status, int32_t* iterations, int32_t* points, int32_t* rewires,
               int32_t* chain_kept, double* path_cost, double* goal_dist, double* path, int32_t* count, double* nodes, int32_t* parent, double* node_cost) {
    WsCall ar{};
    ar.box_lb = lb; ar.box_ub = ub; ar.W = W; ar.O = O; ar.obstacles = obstacles; ar.starts = starts; ar.goals = goals; ar.seeds = seeds; ar.max_init = max_init;
    ar.init = init; ar.init_count = init_count; ar.step = step; ar.edge_step = edge_step; ar.rewire_radius = rewire_radius; ar.goal_rate = goal_rate;
    ar.buffer = buffer; ar.goal_tol = goal_tol; ar.max_iterations = max_iterations; ar.max_nodes = max_nodes; ar.max_points = max_points; ar.status = status;
    ar.iterations = iterations; ar.points = points; ar.rewires = rewires; ar.chain_kept = chain_kept; ar.path_cost = path_cost; ar.goal_dist = goal_dist;
    ar.path = path; ar.count = count; ar.nodes = nodes; ar.parent = parent; ar.node_cost = node_cost;
    return ar;
}

}  // namespace

extern "C" int armour_ws_tree_plan_host(const double* lb, const double* ub, int32_t W, int32_t O, const double* obstacles, const double* starts, const double* goals,
                                        const uint64_t* seeds, int32_t max_init, const double* init, const int32_t* init_count, double step, double edge_step,
                                        double rewire_radius, double goal_rate, double buffer, double goal_tol, int32_t max_iterations, int32_t max_nodes,
                                        int32_t max_points, int32_t* status, int32_t* iterations, int32_t* points, int32_t* rewires, int32_t* chain_kept,
                                        double* path_cost, double* goal_dist, double* path, int32_t* count, double* nodes, int32_t* parent, double* node_cost,
                                        double* margin) {
    WsCall ar = ws_call(lb, ub, W, O, obstacles, starts, goals, seeds, max_init, init, init_count, step, edge_step, rewire_radius, goal_rate, buffer, goal_tol,
                        max_iterations, max_nodes, max_points, status, iterations, points, rewires, chain_kept, path_cost, goal_dist, path, count, nodes, parent, node_cost);
    return plan_on_host("armour_ws_tree_plan_host", ar, nullptr, margin);
}

extern "C" int armour_ws_tree_plan_moving_host(const double* lb, const double* ub, int32_t W, int32_t O, const double* obstacles, const double* velocity,
                                               const double* t_from, const double* t_to, const double* starts, const double* goals, const uint64_t* seeds,
                                               int32_t max_init, const double* init, const int32_t* init_count, double step, double edge_step, double rewire_radius,
                                               double goal_rate, double buffer, double goal_tol, int32_t max_iterations, int32_t max_nodes, int32_t max_points,
                                               int32_t* status, int32_t* iterations, int32_t* points, int32_t* rewires, int32_t* chain_kept, double* path_cost,
                                               double* goal_dist, double* path, int32_t* count, double* nodes, int32_t* parent, double* node_cost, double* margin) {
    WsCall ar = ws_call(lb, ub, W, O, obstacles, starts, goals, seeds, max_init, init, init_count, step, edge_step, rewire_radius, goal_rate, buffer, goal_tol,
                        max_iterations, max_nodes, max_points, status, iterations, points, rewires, chain_kept, path_cost, goal_dist, path, count, nodes, parent, node_cost);
    const Motion mv{velocity, t_from, t_to};
    return plan_on_host("armour_ws_tree_plan_moving_host", ar, &mv, margin);
}

extern "C" int armour_ws_tree_plan(const double* lb, const double* ub, int32_t W, int32_t O, const double* obstacles, const double* starts, const double* goals,
                                   const uint64_t* seeds, int32_t max_init, const double* init, const int32_t* init_count, double step, double edge_step,
                                   double rewire_radius, double goal_rate, double buffer, double goal_tol, int32_t max_iterations, int32_t max_nodes,
                                   int32_t max_points, int32_t* status, int32_t* iterations, int32_t* points, int32_t* rewires, int32_t* chain_kept,
                                   double* path_cost, double* goal_dist, double* path, int32_t* count, double* nodes, int32_t* parent, double* node_cost, double* ms) {
    WsCall ar = ws_call(lb, ub, W, O, obstacles, starts, goals, seeds, max_init, init, init_count, step, edge_step, rewire_radius, goal_rate, buffer, goal_tol,
                        max_iterations, max_nodes, max_points, status, iterations, points, rewires, chain_kept, path_cost, goal_dist, path, count, nodes, parent, node_cost);
    return plan_on_device("armour_ws_tree_plan", "armour_ws_tree_plan_host", ar, nullptr, ms);
}

extern "C" int armour_ws_tree_plan_moving(const double* lb, const double* ub, int32_t W, int32_t O, const double* obstacles, const double* velocity,
                                          const double* t_from, const double* t_to, const double* starts, const double* goals, const uint64_t* seeds,
                                          int32_t max_init, const double* init, const int32_t* init_count, double step, double edge_step, double rewire_radius,
                                          double goal_rate, double buffer, double goal_tol, int32_t max_iterations, int32_t max_nodes, int32_t max_points,
                                          int32_t* status, int32_t* iterations, int32_t* points, int32_t* rewires, int32_t* chain_kept, double* path_cost,
                                          double* goal_dist, double* path, int32_t* count, double* nodes, int32_t* parent, double* node_cost, double* ms) {
    WsCall ar = ws_call(lb, ub, W, O, obstacles, starts, goals, seeds, max_init, init, init_count, step, edge_step, rewire_radius, goal_rate, buffer, goal_tol,
                        max_iterations, max_nodes, max_points, status, iterations, points, rewires, chain_kept, path_cost, goal_dist, path, count, nodes, parent, node_cost);
    const Motion mv{velocity, t_from, t_to};
    return plan_on_device("armour_ws_tree_plan_moving", "armour_ws_tree_plan_moving_host", ar, &mv, ms);
}

// ---- resident trees (include/armour_hip.h, armour_ws_trees_*): the trees of W worlds kept between calls and grown in instalments by the
// kernel's resumed form (the host handle: by plan_world_host with the world's state)
struct ArmourWsTrees {
    int device = 0;                      // < 0: a handle of armour_ws_trees_create_host (no stream, no device buffers)
    int32_t W = 0;
    WsArgs args{};                       // the fixed parameters (box, steps, O, max_nodes); every pointer is set per call
    std::vector<double> obstacles, goals;        // [W][O][12], [W][3]
    std::vector<uint64_t> seeds;                 // [W]
    std::vector<int32_t> state;                  // [W][WS_STATE]: the host handle's state; a device handle's copy of what its kernel wrote back
    // the host handle's trees
    std::vector<double> nodes, node_cost, node_len;
    std::vector<int32_t> parent;
    // the device handle's: uploaded and reserved by the first grow that launches (create touches no device)
    bool on_device = false;
    DevStream stream;
    EventPair ev;
    DevBuf<double> d_obs, d_goals, d_nodes, d_cost, d_len, d_starts, d_path;
    DevBuf<uint64_t> d_seeds;
    DevBuf<int32_t> d_parent, d_state, d_worlds;
    DevColumns<int32_t> out;             // status | iterations | points | rewires | chain_kept | count [L] each
    DevColumns<double> real;             // path_cost | goal_dist [L] each
};

namespace {

int trees_create(const char* who, bool host, const double* lb, const double* ub, int32_t W, int32_t O, const double* obstacles, const double* goals, const uint64_t* seeds,
                 double step, double edge_step, double rewire_radius, double goal_rate, double buffer, double goal_tol, int32_t max_nodes, ArmourWsTrees** out) {
    if (!out) { armour_set_error("%s: null argument", who); return ARMOUR_EINVAL; }
    *out = nullptr;
    WsCall ar{};
    ar.box_lb = lb; ar.box_ub = ub; ar.W = W; ar.O = O; ar.obstacles = obstacles; ar.goals = goals; ar.seeds = seeds; ar.step = step; ar.edge_step = edge_step;
    ar.rewire_radius = rewire_radius; ar.goal_rate = goal_rate; ar.buffer = buffer; ar.goal_tol = goal_tol; ar.max_nodes = max_nodes; ar.resident = true;
    ARMOUR_TRY(check_args(who, &ar));
    ArmourWsTrees* h = new ArmourWsTrees;
    h->device = host ? -1 : 0;
    h->W = W;
    h->args = ar;                                           // (the kernel's part)
    h->args.obstacles = h->args.goals = nullptr;
    h->args.seeds = nullptr;
    if (W > 0 && O > 0) h->obstacles.assign(obstacles, obstacles + (size_t)W * O * ARMOUR_OBS_DOUBLES);
    if (W > 0) {
        h->goals.assign(goals, goals + (size_t)W * 3);
        h->seeds.assign(seeds, seeds + (size_t)W);
    }
    h->state.assign((size_t)W * WS_STATE, 0);
    if (host) {
        const size_t rows = (size_t)W * max_nodes;
        h->nodes.assign(rows * 3, 0.0);
        h->node_cost.assign(rows, 0.0);
        h->node_len.assign(rows, 0.0);
        h->parent.assign(rows, 0);
    }
    *out = h;
    return ARMOUR_OK;
}

// the index list of a grow or a read: every entry in [0, W); `seen` (grow): no world twice, because two blocks would write one tree
int check_worlds(const char* who, const ArmourWsTrees* h, int32_t L, const int32_t* worlds, std::vector<uint8_t>* seen) {
    if (!h || L < 0 || (L > 0 && !worlds)) { armour_set_error("%s: null argument or L = %d", who, L); return ARMOUR_EINVAL; }
    if (seen) seen->assign((size_t)h->W, 0);
    for (int32_t l = 0; l < L; l++) {
        const int32_t w = worlds[l];
        if (w < 0 || w >= h->W) { armour_set_error("%s: worlds[%d] = %d (0..%d)", who, l, w, h->W - 1); return ARMOUR_EINVAL; }
        if (seen && (*seen)[w]) { armour_set_error("%s: world %d is listed twice", who, w); return ARMOUR_EINVAL; }
        if (seen) (*seen)[w] = 1;
    }
    return ARMOUR_OK;
}

// the device handle's fixed inputs and tree storage, once
int trees_to_device(ArmourWsTrees* h) {
    if (h->on_device) return ARMOUR_OK;
    const size_t rows = (size_t)h->W * h->args.max_nodes;
    ARMOUR_TRY(h->stream.create());
    ARMOUR_TRY(h->d_obs.upload(h->obstacles.data(), h->obstacles.size(), h->stream));
    ARMOUR_TRY(h->d_goals.upload(h->goals.data(), h->goals.size(), h->stream));
    ARMOUR_TRY(h->d_seeds.upload(h->seeds.data(), h->seeds.size(), h->stream));
    ARMOUR_TRY(h->d_state.upload(h->state.data(), h->state.size(), h->stream));
    ARMOUR_TRY(h->d_nodes.reserve(rows * 3));
    ARMOUR_TRY(h->d_cost.reserve(rows));
    ARMOUR_TRY(h->d_len.reserve(rows));
    ARMOUR_TRY(h->d_parent.reserve(rows));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->on_device = true;
    return ARMOUR_OK;
}

}  // namespace

extern "C" int armour_ws_trees_create(const double* lb, const double* ub, int32_t W, int32_t O, const double* obstacles, const double* goals, const uint64_t* seeds,
                                      double step, double edge_step, double rewire_radius, double goal_rate, double buffer, double goal_tol, int32_t max_nodes,
                                      ArmourWsTrees** out) {
    return trees_create("armour_ws_trees_create", false, lb, ub, W, O, obstacles, goals, seeds, step, edge_step, rewire_radius, goal_rate, buffer, goal_tol, max_nodes, out);
}

extern "C" int armour_ws_trees_create_host(const double* lb, const double* ub, int32_t W, int32_t O, const double* obstacles, const double* goals, const uint64_t* seeds,
                                           double step, double edge_step, double rewire_radius, double goal_rate, double buffer, double goal_tol, int32_t max_nodes,
                                           ArmourWsTrees** out) {
    return trees_create("armour_ws_trees_create_host", true, lb, ub, W, O, obstacles, goals, seeds, step, edge_step, rewire_radius, goal_rate, buffer, goal_tol, max_nodes, out);
}

extern "C" void armour_ws_trees_destroy(ArmourWsTrees* trees) { delete trees; }

// test hook: what world `world` counts as its iterations done, so that the INT32_MAX rule of a grow can be reached without 2^31 iterations
extern "C" int armour_debug_ws_trees_set_iterations(ArmourWsTrees* h, int32_t world, int32_t done) {
    const char* who = "armour_debug_ws_trees_set_iterations";
    if (!h || world < 0 || world >= h->W || done < 0) { armour_set_error("%s: world = %d, done = %d", who, world, done); return ARMOUR_EINVAL; }
    if (h->on_device) { armour_set_error("%s: the handle's state is on the device", who); return ARMOUR_ESTATE; }
    h->state[(size_t)world * WS_STATE + 1] = done;
    return ARMOUR_OK;
}

extern "C" int armour_ws_trees_grow(ArmourWsTrees* h, int32_t L, const int32_t* worlds, const double* starts, int32_t iterations, int32_t max_points, int32_t* status,
                                    int32_t* iterations_done, int32_t* points, int32_t* rewires, double* path_cost, double* goal_dist, double* path, int32_t* count,
                                    double* ms, double* margin) {
    const char* who = "armour_ws_trees_grow";
    std::vector<uint8_t> seen;
    ARMOUR_TRY(check_worlds(who, h, L, worlds, &seen));
    if (iterations < 0 || iterations > ARMOUR_TREE_MAX_ITERATIONS || max_points < 0) {
        armour_set_error("%s: iterations = %d (0..%d), max_points = %d", who, iterations, ARMOUR_TREE_MAX_ITERATIONS, max_points);
        return ARMOUR_EINVAL;
    }
    if (L > 0 && (!status || !iterations_done || !points || !rewires || !path_cost || !goal_dist)) { armour_set_error("%s: null argument", who); return ARMOUR_EINVAL; }
    if (margin && h->device >= 0) { armour_set_error("%s: margin is the host handle's (armour_ws_trees_create_host)", who); return ARMOUR_EINVAL; }
    for (int32_t l = 0; l < L; l++) {
        const int32_t* st = &h->state[(size_t)worlds[l] * WS_STATE];
        if (st[1] > INT32_MAX - iterations) { armour_set_error("%s: world %d has run %d iterations: %d more pass INT32_MAX", who, worlds[l], st[1], iterations); return ARMOUR_EINVAL; }
        if (st[0] == 0 && (!starts || !finite_all(starts + (size_t)l * 3, 3))) { armour_set_error("%s: world %d's tree is empty and starts[%d] is not finite", who, worlds[l], l); return ARMOUR_EINVAL; }
    }
    if (ms) *ms = 0.0;
    if (L == 0) return ARMOUR_OK;
    const int32_t O = h->args.O;
    const size_t cap = (size_t)h->args.max_nodes;
    WsArgs ar = h->args;
    ar.max_iterations = iterations; ar.max_points = max_points;
    if (h->device < 0) {
        std::vector<int32_t> kept((size_t)L);
        ar.starts = starts; ar.goals = h->goals.data(); ar.seeds = h->seeds.data();
        ar.status = status; ar.iterations = iterations_done; ar.points = points; ar.rewires = rewires; ar.chain_kept = kept.data(); ar.count = count;
        ar.path_cost = path_cost; ar.goal_dist = goal_dist; ar.path = path;
        for_each_staged(L, O, h->obstacles.data(), worlds, [&](int32_t l, const Rule<false>& staged, int) {
            const size_t row = (size_t)worlds[l] * cap;
            plan_world_host(ar, l, worlds[l], staged, &h->nodes[row * 3], &h->parent[row], &h->node_cost[row], &h->node_len[row], margin ? margin + l : nullptr,
                            &h->state[(size_t)worlds[l] * WS_STATE]);
        });
        return armour_check_path_capacity(who, L, points, max_points, path != nullptr);
    }
    if (!armour_device_available()) { armour_set_error("%s: no HIP device visible (armour_ws_trees_create_host makes the host form)", who); return ARMOUR_EDEVICE; }
    ARMOUR_TRY(trees_to_device(h));
    hipStream_t st = h->stream;
    const size_t path_len = path ? (size_t)L * max_points * 3 : 0;
    ARMOUR_TRY(h->d_worlds.upload(worlds, (size_t)L, st));
    ARMOUR_TRY(h->d_starts.upload(starts, (size_t)L * 3, st));       // (starts may be null when every listed tree is planted: reserved, never read)
    ARMOUR_TRY(h->out.reserve(6, (size_t)L));
    ARMOUR_TRY(h->real.reserve(2, (size_t)L));
    if (path) ARMOUR_TRY(h->d_path.reserve(path_len));
    ar.obstacles = h->d_obs; ar.starts = h->d_starts; ar.goals = h->d_goals; ar.seeds = h->d_seeds; ar.worlds = h->d_worlds; ar.state = h->d_state;
    ar.status = h->out.column(0); ar.iterations = h->out.column(1); ar.points = h->out.column(2); ar.rewires = h->out.column(3);
    ar.chain_kept = h->out.column(4); ar.count = h->out.column(5);
    ar.path_cost = h->real.column(0); ar.goal_dist = h->real.column(1);
    ar.parent = h->d_parent; ar.nodes = h->d_nodes; ar.node_cost = h->d_cost; ar.node_len = h->d_len; ar.path = path ? h->d_path.p : nullptr;
    const size_t lds = (size_t)O * Rule<false>::STRIDE * sizeof(double);
    ARMOUR_TRY(grant_dynamic_lds(who, reinterpret_cast<const void*>(ws_tree_kernel<true, false>), lds));
    ARMOUR_TRY(h->ev.record_start(st));
    hipLaunchKernelGGL((ws_tree_kernel<true, false>), dim3((unsigned)L), dim3(TP_BLOCK), lds, st, ar, MovingArgs{});
    HIPCHK(hipGetLastError());
    ARMOUR_TRY(h->ev.record_stop(st));
    ARMOUR_TRY(h->out.fetch(st));
    ARMOUR_TRY(h->real.fetch(st));
    HIPCHK(hipStreamSynchronize(st));
    if (ms) ARMOUR_TRY(h->ev.elapsed_ms(ms));
    int32_t* const ints[6] = {status, iterations_done, points, rewires, nullptr, count};
    for (int k = 0; k < 6; k++) h->out.copy_out(k, ints[k]);
    h->real.copy_out(0, path_cost);
    h->real.copy_out(1, goal_dist);
    const int32_t* h_count = h->out.fetched(5);
    bool any_path = false;
    for (int32_t l = 0; l < L; l++) {
        int32_t* s = &h->state[(size_t)worlds[l] * WS_STATE];
        s[0] = h_count[l]; s[1] = iterations_done[l]; s[2] = rewires[l];
        if (path && points[l] > 0 && points[l] <= max_points) {
            HIPCHK(hipMemcpyAsync(path + (size_t)l * max_points * 3, h->d_path + (size_t)l * max_points * 3, (size_t)points[l] * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
            any_path = true;
        }
    }
    if (any_path) HIPCHK(hipStreamSynchronize(st));
    return armour_check_path_capacity(who, L, points, max_points, path != nullptr);
}

extern "C" int armour_ws_trees_read(ArmourWsTrees* h, int32_t L, const int32_t* worlds, double* nodes, int32_t* parent, double* node_cost, int32_t* count) {
    const char* who = "armour_ws_trees_read";
    ARMOUR_TRY(check_worlds(who, h, L, worlds, nullptr));
    const size_t cap = (size_t)h->args.max_nodes;
    bool copied = false;
    for (int32_t l = 0; l < L; l++) {
        const size_t c = (size_t)h->state[(size_t)worlds[l] * WS_STATE], src = (size_t)worlds[l] * cap, dst = (size_t)l * cap;
        if (count) count[l] = (int32_t)c;
        if (!c) continue;
        if (h->device < 0) {
            if (nodes) std::memcpy(nodes + dst * 3, &h->nodes[src * 3], c * 3 * sizeof(double));
            if (parent) std::memcpy(parent + dst, &h->parent[src], c * sizeof(int32_t));
            if (node_cost) std::memcpy(node_cost + dst, &h->node_cost[src], c * sizeof(double));
            continue;
        }
        hipStream_t st = h->stream;                         // (count > 0: a grow has launched, so the trees are on the device)
        if (nodes) HIPCHK(hipMemcpyAsync(nodes + dst * 3, h->d_nodes + src * 3, c * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        if (parent) HIPCHK(hipMemcpyAsync(parent + dst, h->d_parent + src, c * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (node_cost) HIPCHK(hipMemcpyAsync(node_cost + dst, h->d_cost + src, c * sizeof(double), hipMemcpyDeviceToHost, st));
        copied = true;
    }
    if (copied) HIPCHK(hipStreamSynchronize(h->stream));
    return ARMOUR_OK;
}
