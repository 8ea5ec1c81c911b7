// Path shortening (include/armour_hip.h, armour_path_shortcut): W polylines in W worlds are validated, pruned and refined in ONE launch, a
// block per world (armour_path_shortcut_moving: the same against obstacles in linear motion, by the window rule; tree_block.h Rule<MOVING>).
// The rule reuses the tree planner's definitions as they stand (tree_block.h: the wrapped difference, S of a prefix, one
// sub-segment's enlarged test); what is new -- the midpoint, the bitwise comparison of two points and the order of the passes -- is written
// once below as __host__ __device__ code, run by the kernel's lanes and by armour_path_shortcut_host's loop.
//
// The device's work is edge checks, taken as flat work lists: the candidates of a list (the edges of the path for validate, anchor -> j for
// j = last, last - 1, ... for prune, the two halves of every pair for refine) are laid across the block's 256 lanes, sub-segment by
// sub-segment and several candidates to a chunk, so that lanes are full even when one candidate has few sub-segments.  The verdict of a
// candidate is a pure function of its two end points, so the order in which the lanes evaluate them does not show in the result.
//
// Nothing but __syncthreads() orders the block: the world's path lives in LDS, written and read by this block alone; every decision that
// steers a loop is taken from values all lanes hold alike, so the barriers are reached by all of them.  A work list ends because every
// chunk moves its cursor (candidate, sub-segment) forward, a candidate has at most ARMOUR_TREE_MAX_SEGMENTS sub-segments and a list at most
// 2 ARMOUR_SHORTCUT_MAX_POINTS candidates; prune ends because its anchor moves forward; the passes are counted.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "roadmap_handle.h"
#include "tree_block.h"

using namespace treeblk;

namespace {

constexpr int SC_MAX = ARMOUR_SHORTCUT_MAX_POINTS;
constexpr int SC_PER_LANE = SC_MAX / TP_BLOCK;           // points per lane when a whole list is scanned
static_assert(SC_PER_LANE * TP_BLOCK == SC_MAX, "the position scan deals whole points to lanes");
enum { SC_VALIDATE, SC_PRUNE, SC_REFINE };

// What a world's run reads besides the robot: by value in the kernel's arguments (pointers: the device's; the host twin passes its own)
struct ShortcutArgs {
    double edge_step;
    int32_t O, max_in, max_points, passes;
    const double *obstacles, *paths;
    const int32_t* counts;
    int32_t *status, *points, *first_bad, *passes_done;
    double *out, *length_in, *length_out;
};
// an entry's arguments as it was given them: the kernel's, and what only check_args reads
struct ShortcutCall : ShortcutArgs {
    int32_t W;
};

__host__ __device__ inline bool same_bits(double x, double y) {
    uint64_t a, b;
    memcpy(&a, &x, sizeof(a));
    memcpy(&b, &y, sizeof(b));
    return a == b;
}
// joint j of the midpoint that refine inserts between a and b
__host__ __device__ inline double mid_joint(const RmRobot& rb, int j, double a, double b) { return a + 0.5 * joint_diff(rb, j, a, b); }

// prefix_segments for an edge whose end points a lane holds in arrays of its own: edge_segments' operations in its order, written over all
// ARMOUR_MAX_FACTORS joints with a select (as wrapped_sq is) so that the arrays are never indexed at run time and stay in registers
__device__ inline int lane_segments(const RmRobot& rb, const double (&a)[ARMOUR_MAX_FACTORS], const double (&b)[ARMOUR_MAX_FACTORS], double edge_step) {
    double mx = 0.0;
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) mx = j < rb.n ? fmax(mx, fabs(joint_diff(rb, j, a[j], b[j]))) : mx;
    const double S = ceil(mx / edge_step);
    return S < 1.0 ? 1 : S > (double)ARMOUR_TREE_MAX_SEGMENTS ? ARMOUR_TREE_MAX_SEGMENTS : (int)S;
}

// ---- the block's cooperative steps (on tree_block.h's).  Every result is the same in all lanes.
struct ShortShared {
    int hit[2 * SC_MAX];       // per candidate of the current work list: 1 = some sub-segment's enlarged test did not separate
    int pos[SC_MAX];           // refine: the index of point k in the refined list
    double norm[SC_MAX];       // the wrapped length of segment k, for the sums in index order
    int end[TP_BLOCK];         // a chunk's window: one past the last work item of window candidate t
    BlockWords words;
};

// The work list's candidate k as an edge a -> b, from the list pts [count][n] in LDS.  validate: p_k -> p_{k+1}; prune: p_anchor -> p_{last-k};
// refine: half k & 1 of the pair (p_{k>>1}, p_{(k>>1)+1}) about its midpoint -- false when the pair's points are equal bit for bit (no midpoint
// is inserted there; the candidate counts as not free).
struct EdgeSet { int kind, anchor, last; };
__device__ __forceinline__ bool load_edge(const RmRobot& rb, const EdgeSet& es, const double* pts, int k, double (&a)[ARMOUR_MAX_FACTORS], double (&b)[ARMOUR_MAX_FACTORS]) {
    const int n = rb.n;
    const int ia = es.kind == SC_PRUNE ? es.anchor : es.kind == SC_VALIDATE ? k : k >> 1;
    const int ib = es.kind == SC_PRUNE ? es.last - k : ia + 1;
    bool same = true;
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) {
        a[j] = j < n ? pts[ia * n + j] : 0.0;
        b[j] = j < n ? pts[ib * n + j] : 0.0;
        same = same && same_bits(a[j], b[j]);
    }
    if (es.kind != SC_REFINE) return true;
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) {
        const double mid = j < n ? mid_joint(rb, j, a[j], b[j]) : 0.0;
        if (k & 1) a[j] = mid; else b[j] = mid;
    }
    return !same;
}

// One work list of C candidates (C <= 2 SC_MAX).  A chunk looks at a window of up to TP_BLOCK candidates from its cursor (cbase, and sbase
// sub-segments of candidate cbase already tested), numbers their remaining sub-segments as work items in candidate order and tests the first
// TP_BLOCK of them, a lane each.  When the whole rest of the list is at most TP_BLOCK / 2 items, each item's obstacles are split over
// several lanes (obstacle_split).  A lane whose test does not separate stores 1 to its candidate's word sh.hit -- several lanes may store to one
// word, all of them the same 1.  After the chunk's barrier:
//   validate  returns the first candidate with a hit (candidates are in ascending order, so it is the first edge that is not free);
//   prune     returns the first candidate that is fully tested without a hit -- every candidate above it has a hit;
//   refine    goes through the whole list and leaves the verdicts in sh.hit.
// TP_NONE / C when the list ends without such a candidate.  A candidate with a hit is not tested further.  The caller has put a barrier after
// the last write of pts; on return every lane is past the last read of pts, and (refine) sh.hit is complete.
template <class R>
__device__ inline int run_edges(const RmRobot& rb, ShortShared& sh, const EdgeSet es, int C, const double* pts, double edge_step, const R& rule, int O) {
    const int t = threadIdx.x;
    for (int k = t; k < C; k += TP_BLOCK) sh.hit[k] = 0;
    __syncthreads();
    int cbase = 0, sbase = 0;
    while (cbase < C) {
        const int nw = C - cbase < TP_BLOCK ? C - cbase : TP_BLOCK;
        double a[ARMOUR_MAX_FACTORS], b[ARMOUR_MAX_FACTORS];
        int Sk = 0;
        if (t < nw) {
            const bool edge = load_edge(rb, es, pts, cbase + t, a, b);
            Sk = edge ? lane_segments(rb, a, b, edge_step) : 1;
            if (!edge) sh.hit[cbase + t] = 1;
            if (t == 0) Sk -= sbase;
        }
        int T;
        sh.end[t] = block_scan(sh.words, Sk, &T);
        __syncthreads();
        const ObstacleSplit sp = obstacle_split(T, O, nw == C - cbase, t);
        const int per = sp.per, item = t / sp.G;            // per work items to a chunk
        if (t < per * sp.G && item < T) {
            const int k = item_owner(sh.end, nw, item), start = k ? sh.end[k - 1] : 0, done = k ? 0 : sbase;
            load_edge(rb, es, pts, cbase + k, a, b);
            if (!segment_free(rb, a, b, item - start + done, sh.end[k] - start + done, rule.from(sp.o0), sp.o1 - sp.o0)) sh.hit[cbase + k] = 1;
        }
        __syncthreads();
        const int in_chunk = item_owner(sh.end, nw, per - 1) + 1;   // the candidates with an item in this chunk: 1 + the number of ends < per
        const int kn = in_chunk < nw ? in_chunk : nw;
        const bool full = t < kn && sh.end[t] <= per, h = t < kn && sh.hit[cbase + t] != 0;
        if (es.kind != SC_REFINE) {
            const int stop = block_first(sh.words, es.kind == SC_PRUNE ? (full && !h) : h);
            if (stop != TP_NONE) return cbase + stop;
        }
        const int last = kn - 1;
        if (sh.end[last] > per && !sh.hit[cbase + last]) {  // cut by the chunk's end and still free: go on inside it
            sbase = (last ? 0 : sbase) + per - (last ? sh.end[last - 1] : 0);
            cbase += last;
        } else {
            cbase += kn;
            sbase = 0;
        }
        __syncthreads();                                    // sh.end and sh.hit have been read: the next chunk may write them
    }
    return es.kind == SC_PRUNE ? C : TP_NONE;
}

// prune of the list pts [count][n], in place: the kept points move to the front (slot o <= the anchor's successor, never above a candidate)
template <class R>
__device__ inline int block_prune(const RmRobot& rb, ShortShared& sh, double* pts, int count, double edge_step, const R& rule, int O) {
    const int t = threadIdx.x, n = rb.n, last = count - 1;
    int o = 1, i = 0;
    while (i < last) {                                      // the anchor moves forward every time
        const int C = last - i - 1;                         // candidates last, last - 1, ..., i + 2; i + 1 is an edge of the list: known free
        int j = i + 1;
        if (C > 0) {
            const int k = run_edges(rb, sh, EdgeSet{SC_PRUNE, i, last}, C, pts, edge_step, rule, O);
            if (k < C) j = last - k;
        }
        if (t < n) pts[o * n + t] = pts[j * n + t];
        o++;
        i = j;
        __syncthreads();
    }
    return o;
}

// refine of the list pts [count][n], in place; the caller has checked 2 count - 1 <= the rows of pts.  Returns the new count.
template <class R>
__device__ inline int block_refine(const RmRobot& rb, ShortShared& sh, double* pts, int count, double edge_step, const R& rule, int O) {
    const int t = threadIdx.x, n = rb.n;
    run_edges(rb, sh, EdgeSet{SC_REFINE, 0, 0}, 2 * (count - 1), pts, edge_step, rule, O);
    // point k goes to k + the number of midpoints inserted before it: lane t scans the pairs SC_PER_LANE t ...
    int before[SC_PER_LANE], mine = 0;
#pragma unroll
    for (int u = 0; u < SC_PER_LANE; u++) {
        const int k = SC_PER_LANE * t + u;
        before[u] = mine;
        mine += k < count - 1 && !sh.hit[2 * k] && !sh.hit[2 * k + 1] ? 1 : 0;
    }
    int inserted;
    const int upto = block_scan(sh.words, mine, &inserted) - mine;
#pragma unroll
    for (int u = 0; u < SC_PER_LANE; u++) {
        const int k = SC_PER_LANE * t + u;
        if (k < count) sh.pos[k] = k + upto + before[u];
    }
    __syncthreads();
    // ... and the points move up from the top, TP_BLOCK at a time: a point's new index is not below its old one, so a write lands on rows
    // that were read in this step or in an earlier one.  The one neighbour a lane may need from the step before is read where it went.
    for (int c = (count - 1) / TP_BLOCK; c >= 0; c--) {
        const int k = c * TP_BLOCK + t;
        const bool insert = k < count - 1 && sh.pos[k + 1] - sh.pos[k] == 2;
        double a[ARMOUR_MAX_FACTORS], mid[ARMOUR_MAX_FACTORS];
        if (k < count) {
            const double* nb = pts + (size_t)(t == TP_BLOCK - 1 && insert ? sh.pos[k + 1] : k + 1) * n;
#pragma unroll
            for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) {
                a[j] = j < n ? pts[k * n + j] : 0.0;
                mid[j] = j < n && insert ? mid_joint(rb, j, a[j], nb[j]) : 0.0;
            }
        }
        __syncthreads();
        if (k < count) {
            const int to = sh.pos[k];
#pragma unroll
            for (int j = 0; j < ARMOUR_MAX_FACTORS; j++)
                if (j < n) {
                    pts[to * n + j] = a[j];
                    if (insert) pts[(to + 1) * n + j] = mid[j];
                }
        }
        __syncthreads();
    }
    return count + inserted;
}

// sum of the wrapped lengths of the list's segments in index order (lane 0 adds; the others have computed the terms)
__device__ inline double block_length(const RmRobot& rb, ShortShared& sh, const double* pts, int count) {
    const int t = threadIdx.x, n = rb.n;
    for (int k = t; k < count - 1; k += TP_BLOCK) sh.norm[k] = wrapped_norm(rb, pts + (size_t)k * n, pts + (size_t)(k + 1) * n);
    __syncthreads();
    double acc = 0.0;
    if (t == 0)
        for (int k = 0; k < count - 1; k++) acc += sh.norm[k];
    __syncthreads();                                        // sh.norm has been read
    return acc;                                             // (lane 0's alone is the sum)
}

// grid W, dynamic LDS: the world's obstacles [O][RM_OBS_STRIDE], then its list [max(max_in, max_points)][n]
// MOVING (armour_path_shortcut_moving): the window rule -- the obstacles are [O][RM_MOV_STRIDE], mv.velocity [W][O][3], mv.mid / mv.half [W], this
// world's two kept in registers.  The static instantiation reads nothing of mv and keeps the static rule's calls as they were.
template <bool MOVING>
__global__ __launch_bounds__(TP_BLOCK) void path_shortcut_kernel(RmRobot rb, ShortcutArgs ar, MovingArgs mv) {
    extern __shared__ double s_dyn[];
    __shared__ ShortShared sh;
    const int w = blockIdx.x, t = threadIdx.x, n = rb.n, O = ar.O;
    double* s_obs = s_dyn;
    double* pts = s_dyn + (size_t)O * Rule<MOVING>::STRIDE;
    Rule<MOVING> rule{s_obs};
    if constexpr (MOVING) {
        rule.mid = mv.mid[w];
        rule.half = mv.half[w];
    }
    int count = ar.counts[w];
    const double* in = ar.paths + (size_t)w * ar.max_in * n;
    for (int i = t; i < count * n; i += TP_BLOCK) pts[i] = in[i];
    // (either ends in a barrier: pts is written too)
    if constexpr (MOVING) stage_obstacles_moving_lds<TP_BLOCK>(ar.obstacles + (size_t)w * O * ARMOUR_OBS_DOUBLES, mv.velocity + (size_t)w * O * 3, O, s_obs);
    else stage_obstacles_lds<TP_BLOCK>(ar.obstacles + (size_t)w * O * ARMOUR_OBS_DOUBLES, O, s_obs);
    const double length_in = block_length(rb, sh, pts, count);
    int status = ARMOUR_SHORTCUT_OK, first_bad = -1, passes_done = 0;
    double length_out = 0.0;
    const int bad = run_edges(rb, sh, EdgeSet{SC_VALIDATE, 0, 0}, count - 1, pts, ar.edge_step, rule, O);
    if (bad != TP_NONE) {
        status = ARMOUR_SHORTCUT_INVALID;
        first_bad = bad;
        count = 0;
    } else {
        count = block_prune(rb, sh, pts, count, ar.edge_step, rule, O);
        passes_done = 1;
        for (int p = 1; p < ar.passes && 2 * count - 1 <= ar.max_points; p++) {
            count = block_refine(rb, sh, pts, count, ar.edge_step, rule, O);
            count = block_prune(rb, sh, pts, count, ar.edge_step, rule, O);
            passes_done = p + 1;
        }
        length_out = block_length(rb, sh, pts, count);
        if (ar.out && count <= ar.max_points) {
            double* out = ar.out + (size_t)w * ar.max_points * n;
            for (int i = t; i < count * n; i += TP_BLOCK) out[i] = pts[i];
        }
    }
    if (t == 0) {
        ar.status[w] = status;
        ar.points[w] = count;
        ar.first_bad[w] = first_bad;
        ar.passes_done[w] = passes_done;
        ar.length_in[w] = length_in;
        ar.length_out[w] = length_out;
    }
}

// ---- the host twin: the same functions in a loop
double length_host(const RmRobot& rb, const std::vector<double>& pts, int count) {
    double acc = 0.0;
    for (int k = 0; k + 1 < count; k++) acc += wrapped_norm(rb, pts.data() + (size_t)k * rb.n, pts.data() + (size_t)(k + 1) * rb.n);
    return acc;
}

template <class R>
bool free_host(const HostWorld<R>& hw, const double* a, const double* b) {
    int S;
    return hw.prefix(a, b, &S) == S;
}

// prune: the candidates of an anchor in descending j, each with prefix; i + 1 is taken untested
template <class R>
void prune_host(const HostWorld<R>& hw, std::vector<double>& pts, int* count) {
    const int n = hw.rb.n, last = *count - 1;
    int o = 1, i = 0;
    while (i < last) {
        int j = last;
        while (j > i + 1 && !free_host(hw, pts.data() + (size_t)i * n, pts.data() + (size_t)j * n)) j--;
        std::memmove(pts.data() + (size_t)o * n, pts.data() + (size_t)j * n, n * sizeof(double));
        o++;
        i = j;
    }
    *count = o;
}

// refine: a -> mid is tested first, mid -> b only when it is free
template <class R>
void refine_host(const HostWorld<R>& hw, std::vector<double>& pts, int* count) {
    const int n = hw.rb.n;
    std::vector<double> next;
    next.reserve((size_t)(2 * *count - 1) * n);
    double mid[ARMOUR_MAX_FACTORS];
    for (int k = 0; k < *count; k++) {
        const double* a = pts.data() + (size_t)k * n;
        next.insert(next.end(), a, a + n);
        if (k + 1 == *count) break;
        const double* b = a + n;
        bool same = true;
        for (int j = 0; j < n; j++) {
            same = same && same_bits(a[j], b[j]);
            mid[j] = mid_joint(hw.rb, j, a[j], b[j]);
        }
        if (!same && free_host(hw, a, mid) && free_host(hw, mid, b)) next.insert(next.end(), mid, mid + n);
    }
    *count = (int)(next.size() / n);
    pts.swap(next);
}

template <class R>
void shortcut_world_host(const RmRobot& rb, const ShortcutArgs& ar, int w, const R& rule, double* margin) {
    const int n = rb.n;
    int count = ar.counts[w];
    if (margin) *margin = INFINITY;
    const HostWorld<R> hw{rb, rule, ar.O, ar.edge_step, margin};
    const double* in = ar.paths + (size_t)w * ar.max_in * n;
    std::vector<double> pts(in, in + (size_t)count * n);
    ar.length_in[w] = length_host(rb, pts, count);
    ar.status[w] = ARMOUR_SHORTCUT_OK; ar.first_bad[w] = -1; ar.passes_done[w] = 0; ar.length_out[w] = 0.0; ar.points[w] = 0;
    for (int s = 0; s + 1 < count; s++)
        if (!free_host(hw, pts.data() + (size_t)s * n, pts.data() + (size_t)(s + 1) * n)) {
            ar.status[w] = ARMOUR_SHORTCUT_INVALID;
            ar.first_bad[w] = s;
            return;
        }
    prune_host(hw, pts, &count);
    ar.passes_done[w] = 1;
    for (int p = 1; p < ar.passes && 2 * count - 1 <= ar.max_points; p++) {
        refine_host(hw, pts, &count);
        prune_host(hw, pts, &count);
        ar.passes_done[w] = p + 1;
    }
    ar.points[w] = count;
    ar.length_out[w] = length_host(rb, pts, count);
    if (ar.out && count <= ar.max_points) std::memcpy(ar.out + (size_t)w * ar.max_points * n, pts.data(), (size_t)count * n * sizeof(double));
}

// the argument rules of both entries, before a device is touched, on ar as the entry filled it; fills rb
int check_args(const char* who, const ArmourRobot* robot, const uint8_t* continuous, RmRobot* rb, const ShortcutCall& ar) {
    const int32_t W = ar.W, O = ar.O, max_in = ar.max_in;
    if (!robot) { armour_set_error("%s: null argument", who); return ARMOUR_EINVAL; }
    ARMOUR_TRY(armour_check_robot_shape(who, robot));
    ARMOUR_TRY(armour_check_world_counts(who, W, O, ar.obstacles));
    const int n = robot->num_factors;
    if (W > 0 && (!ar.paths || !ar.counts || !ar.status || !ar.points || !ar.first_bad || !ar.passes_done || !ar.length_in || !ar.length_out)) {
        armour_set_error("%s: null argument", who);
        return ARMOUR_EINVAL;
    }
    if (max_in < 2 || max_in > ARMOUR_SHORTCUT_MAX_POINTS || ar.max_points < 2 || ar.max_points > ARMOUR_SHORTCUT_MAX_POINTS || ar.passes < 1 ||
        ar.passes > ARMOUR_SHORTCUT_MAX_PASSES) {
        armour_set_error("%s: max_in = %d, max_points = %d (2..%d), passes = %d (1..%d)", who, max_in, ar.max_points, ARMOUR_SHORTCUT_MAX_POINTS, ar.passes,
                         ARMOUR_SHORTCUT_MAX_PASSES);
        return ARMOUR_EINVAL;
    }
    if (!(ar.edge_step > 0.0) || !std::isfinite(ar.edge_step)) { armour_set_error("%s: edge_step = %g", who, ar.edge_step); return ARMOUR_EINVAL; }
    for (int32_t w = 0; w < W; w++) {
        if (ar.counts[w] < 2 || ar.counts[w] > max_in) { armour_set_error("%s: world %d's path has %d points (2..max_in = %d)", who, w, ar.counts[w], max_in); return ARMOUR_EINVAL; }
        if (!finite_all(ar.paths + (size_t)w * max_in * n, (size_t)ar.counts[w] * n)) { armour_set_error("%s: a point of world %d's path is not finite", who, w); return ARMOUR_EINVAL; }
    }
    if (!finite_all(ar.obstacles, (size_t)W * O * ARMOUR_OBS_DOUBLES)) { armour_set_error("%s: an obstacle is not finite", who); return ARMOUR_EINVAL; }
    fill_rm_robot(robot, continuous, rb);
    // the extent of a joint: that of the paths' points (any other point: a midpoint lies between two points)
    double extent[ARMOUR_MAX_FACTORS];
    for (int j = 0; j < n; j++) {
        double lo = INFINITY, hi = -INFINITY;
        for (int32_t w = 0; w < W && !rb->cont[j]; w++)
            for (int32_t k = 0; k < ar.counts[w]; k++) {
                const double x = ar.paths[((size_t)w * max_in + k) * n + j];
                lo = std::fmin(lo, x);
                hi = std::fmax(hi, x);
            }
        extent[j] = W > 0 ? hi - lo : 0.0;
    }
    return check_joint_spans(who, *rb, extent, ar.edge_step);
}

// the host twin of both rules (mv null: the static one)
int shortcut_on_host(const char* who, const ArmourRobot* robot, const uint8_t* continuous, const ShortcutCall& ar, const Motion* mv, double* margin) {
    RmRobot rb;
    ARMOUR_TRY(check_args(who, robot, continuous, &rb, ar));
    std::vector<double> mid, half;
    if (mv) ARMOUR_TRY(check_windows(who, ar.W, ar.O, *mv, &mid, &half));
    auto world = [&](int32_t w, const auto& rule, int) { shortcut_world_host(rb, ar, w, rule, margin ? margin + w : nullptr); };
    if (mv) for_each_staged<true>(ar.W, ar.O, ar.obstacles, nullptr, world, mv->velocity, mid.data(), half.data());
    else for_each_staged(ar.W, ar.O, ar.obstacles, nullptr, world);
    return armour_check_path_capacity(who, ar.W, ar.points, ar.max_points, true);
}

// the device entry of both rules (mv null: the static one)
int shortcut_on_device(const char* who, const char* host_form, const ArmourRobot* robot, const uint8_t* continuous, const ShortcutCall& ar, const Motion* mv, double* ms) {
    RmRobot rb;
    ARMOUR_TRY(check_args(who, robot, continuous, &rb, ar));
    std::vector<double> mid, half;
    if (mv) ARMOUR_TRY(check_windows(who, ar.W, ar.O, *mv, &mid, &half));
    const int32_t W = ar.W, O = ar.O, max_in = ar.max_in, max_points = ar.max_points;
    double* out = ar.out;
    if (ms) *ms = 0.0;
    if (W == 0) return ARMOUR_OK;
    if (!armour_device_available()) { armour_set_error("%s: no HIP device visible (%s is the host form)", who, host_form); return ARMOUR_EDEVICE; }
    const int n = rb.n;
    const size_t rows = (size_t)std::max(max_in, max_points), out_len = out ? (size_t)W * max_points * n : 0;
    const size_t lds = ((size_t)O * (mv ? RM_MOV_STRIDE : RM_OBS_STRIDE) + rows * n) * sizeof(double);
    DevStream st;
    EventPair ev;
    DevBuf<double> d_obs, d_paths, d_path_out, d_vel, d_mid, d_half;
    DevBuf<int32_t> d_counts;
    DevColumns<double> len;                               // length_in | length_out [W] each
    DevColumns<int32_t> res;                              // status | points | first_bad | passes_done [W] each
    ARMOUR_TRY(st.create());
    ARMOUR_TRY(d_obs.upload(ar.obstacles, (size_t)W * O * ARMOUR_OBS_DOUBLES, st));
    ARMOUR_TRY(d_paths.upload(ar.paths, (size_t)W * max_in * n, st));
    ARMOUR_TRY(d_counts.upload(ar.counts, (size_t)W, st));
    MovingArgs dmv{};
    if (mv) {
        ARMOUR_TRY(d_vel.upload(mv->velocity, (size_t)W * O * 3, st));
        ARMOUR_TRY(d_mid.upload(mid.data(), (size_t)W, st));
        ARMOUR_TRY(d_half.upload(half.data(), (size_t)W, st));
        dmv = MovingArgs{d_vel, d_mid, d_half};
    }
    ARMOUR_TRY(res.reserve(4, (size_t)W));
    ARMOUR_TRY(len.reserve(2, (size_t)W));
    if (out) ARMOUR_TRY(d_path_out.reserve(out_len));
    ShortcutArgs dev = ar;                                // (the kernel's part)
    dev.obstacles = d_obs; dev.paths = d_paths; dev.counts = d_counts;
    dev.status = res.column(0); dev.points = res.column(1); dev.first_bad = res.column(2); dev.passes_done = res.column(3);
    dev.length_in = len.column(0); dev.length_out = len.column(1);
    dev.out = out ? d_path_out.p : nullptr;
    // beside the kernel's static 21.6 KB: at the caps 54 KB (static) or 62 KB (moving) of obstacles and up to 64 KB of path, which a block may
    // have once it asks, as far as the device grants it
    const void* kernel = mv ? reinterpret_cast<const void*>(path_shortcut_kernel<true>) : reinterpret_cast<const void*>(path_shortcut_kernel<false>);
    ARMOUR_TRY(grant_dynamic_lds(who, kernel, lds));
    ARMOUR_TRY(ev.record_start(st));
    if (mv) hipLaunchKernelGGL(path_shortcut_kernel<true>, dim3((unsigned)W), dim3(TP_BLOCK), lds, st, rb, dev, dmv);
    else hipLaunchKernelGGL(path_shortcut_kernel<false>, dim3((unsigned)W), dim3(TP_BLOCK), lds, st, rb, dev, dmv);
    HIPCHK(hipGetLastError());
    ARMOUR_TRY(ev.record_stop(st));
    ARMOUR_TRY(res.fetch(st));
    ARMOUR_TRY(len.fetch(st));
    HIPCHK(hipStreamSynchronize(st));
    if (ms) ARMOUR_TRY(ev.elapsed_ms(ms));
    int32_t* const ints[4] = {ar.status, ar.points, ar.first_bad, ar.passes_done};
    for (int k = 0; k < 4; k++) res.copy_out(k, ints[k]);
    len.copy_out(0, ar.length_in);
    len.copy_out(1, ar.length_out);
    // only the rows that were written come back (the rest of the caller's array is left as it was)
    for (int32_t w = 0; out && w < W; w++)
        if (ar.points[w] > 0 && ar.points[w] <= max_points)
            HIPCHK(hipMemcpyAsync(out + (size_t)w * max_points * n, d_path_out + (size_t)w * max_points * n, (size_t)ar.points[w] * n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return armour_check_path_capacity(who, W, ar.points, max_points, true);
}

// an entry's arguments into the call record (the moving entries' three go beside it, in a Motion)
ShortcutCall shortcut_call(int32_t W, int32_t O, const double* obstacles, int32_t max_in, const double* paths, const int32_t* counts, double edge_step, int32_t passes,
                           int32_t max_points, int32_t* status, int32_t* points, int32_t* first_bad, int32_t* passes_done, double* out, double* length_in,
                           double* length_out) {
    ShortcutCall ar{};
    ar.W = W; ar.O = O; ar.obstacles = obstacles; ar.max_in = max_in; ar.paths = paths; ar.counts = counts; ar.edge_step = edge_step; ar.passes = passes;
    ar.max_points = max_points; ar.status = status; ar.points = points; ar.first_bad = first_bad; ar.passes_done = passes_done; ar.out = out;
    ar.length_in = length_in; ar.length_out = length_out;
    return ar;
}

}  // namespace

extern "C" int armour_path_shortcut_host(const ArmourRobot* robot, const uint8_t* continuous, int32_t W, int32_t O, const double* obstacles, int32_t max_in,
                                         const double* paths, const int32_t* counts, double edge_step, int32_t passes, int32_t max_points, int32_t* status,
                                         int32_t* points, int32_t* first_bad, int32_t* passes_done, double* out, double* length_in, double* length_out,
                                         double* margin) {
    const ShortcutCall ar = shortcut_call(W, O, obstacles, max_in, paths, counts, edge_step, passes, max_points, status, points, first_bad, passes_done, out, length_in,
                                          length_out);
    return shortcut_on_host("armour_path_shortcut_host", robot, continuous, ar, nullptr, margin);
}

extern "C" int armour_path_shortcut_moving_host(const ArmourRobot* robot, const uint8_t* continuous, int32_t W, int32_t O, const double* obstacles,
                                                const double* velocity, const double* t_from, const double* t_to, int32_t max_in, const double* paths,
                                                const int32_t* counts, double edge_step, int32_t passes, int32_t max_points, int32_t* status, int32_t* points,
                                                int32_t* first_bad, int32_t* passes_done, double* out, double* length_in, double* length_out, double* margin) {
    const ShortcutCall ar = shortcut_call(W, O, obstacles, max_in, paths, counts, edge_step, passes, max_points, status, points, first_bad, passes_done, out, length_in,
                                          length_out);
    const Motion mv{velocity, t_from, t_to};
    return shortcut_on_host("armour_path_shortcut_moving_host", robot, continuous, ar, &mv, margin);
}

extern "C" int armour_path_shortcut(const ArmourRobot* robot, const uint8_t* continuous, int32_t W, int32_t O, const double* obstacles, int32_t max_in,
                                    const double* paths, const int32_t* counts, double edge_step, int32_t passes, int32_t max_points, int32_t* status,
                                    int32_t* points, int32_t* first_bad, int32_t* passes_done, double* out, double* length_in, double* length_out, double* ms) {
    const ShortcutCall ar = shortcut_call(W, O, obstacles, max_in, paths, counts, edge_step, passes, max_points, status, points, first_bad, passes_done, out, length_in,
                                          length_out);
    return shortcut_on_device("armour_path_shortcut", "armour_path_shortcut_host", robot, continuous, ar, nullptr, ms);
}

extern "C" int armour_path_shortcut_moving(const ArmourRobot* robot, const uint8_t* continuous, int32_t W, int32_t O, const double* obstacles, const double* velocity,
                                           const double* t_from, const double* t_to, int32_t max_in, const double* paths, const int32_t* counts, double edge_step,
                                           int32_t passes, int32_t max_points, int32_t* status, int32_t* points, int32_t* first_bad, int32_t* passes_done, double* out,
                                           double* length_in, double* length_out, double* ms) {
    const ShortcutCall ar = shortcut_call(W, O, obstacles, max_in, paths, counts, edge_step, passes, max_points, status, points, first_bad, passes_done, out, length_in,
                                          length_out);
    const Motion mv{velocity, t_from, t_to};
    return shortcut_on_device("armour_path_shortcut_moving", "armour_path_shortcut_moving_host", robot, continuous, ar, &mv, ms);
}
