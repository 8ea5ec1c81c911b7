// Time-sliced roadmap verdicts and the earliest-arrival search over (node, slice) states (include/armour_hip.h, armour_roadmap_check_slices
// / armour_roadmap_arrival).
//
// The sliced check judges every node, edge and extra edge of a roadmap in K <= 64 consecutive windows [t_k, t_k+1] of a world's clock by the
// window rule of armour_roadmap_check_moving, in ONE launch: the forward kinematics of an item do not depend on time, so a lane walks its links
// once and tests each link box against every obstacle at K poses, with the slices still alive in a 64-bit mask.  The pair test is
// roadmap_geometry.h's pair_separated with config_free_moving's expressions for the box centre and the half-sizes, so bit k of a mask is the
// window check's verdict on slice k.
//
// The search is an integer fixed point on those masks (no floating point on the device): reach[v] = the slices at which v can be occupied,
// the least family closed under waiting at a free node and under traversing an edge whose every slice is free.  Every operator is monotone on
// a finite lattice, so the least fixed point is unique and any in-place order reaches it (the argument of 4.12a); one block per world.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "roadmap_handle.h"

using namespace rmgeo;

namespace {

constexpr int SL_BLOCK = 256;                 // four waves; a block serves one world (its obstacles and slice times are staged in LDS)
constexpr int AR_BLOCK = 1024;                // sixteen waves: one block is one world, as roadmap_field_kernel
constexpr int SL_PATH = ARMOUR_ROADMAP_SLICES_MAX;

// the low K ones, K in 1..64 (never a shift by 64)
__host__ __device__ inline uint64_t low_ones(int K) { return K >= 64 ? ~0ull : (1ull << K) - 1ull; }

// The slices of 0..K-1 in which configuration q with per-link enlargement r is free of the O staged moving obstacles: bit k is
// config_free_moving(rb, q, r, obs, O, mid[k], half[k], false, .).  q and r are consumed as config_free_moving consumes them.  A slice leaves
// the mask at its first colliding pair; the walk ends when the mask is empty.  An obstacle at rest (v = 0 exactly; the same branch for every
// lane of the block) is one test for all slices: x - 0 * mid = x and h + (r + 0 * half) = h + r, the operands of every slice's own test.
__host__ __device__ inline uint64_t config_slices(const RmRobot& rb, double (&q)[ARMOUR_MAX_FACTORS], double (&r)[ARMOUR_MAX_JOINTS], const double* obs, int O,
                                                  const double* mid, const double* half, int K) {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
    uint64_t live = low_ones(K);
    for (int l = 0; l < rb.J && live; l++) {
        link_frame(rb, l, q[0], R, p);
        double x[3], u[3][3];
        const double rl = r[0];
#pragma unroll
        for (int j = 0; j + 1 < ARMOUR_MAX_FACTORS; j++) q[j] = q[j + 1];
#pragma unroll
        for (int j = 0; j + 1 < ARMOUR_MAX_JOINTS; j++) r[j] = r[j + 1];
        link_box(rb, l, R, p, x, u);
        for (int o = 0; o < O && live; o++) {
            const double* ob = obs + (size_t)o * RM_MOV_STRIDE;
            const double* v = ob + RM_OBS_STRIDE;
            double xs[3], s[3], val;
            if (v[0] == 0.0 && v[1] == 0.0 && v[2] == 0.0) {
                for (int i = 0; i < 3; i++) s[i] = rb.h[l][i] + rl;
                if (!pair_separated(x, u, s, ob, false, &val)) live = 0;
                continue;
            }
            for (int k = 0; k < K; k++) {
                if (!((live >> k) & 1ull)) continue;
                const double grow = rl + v[3] * half[k];
                for (int i = 0; i < 3; i++) xs[i] = x[i] - v[i] * mid[k];
                for (int i = 0; i < 3; i++) s[i] = rb.h[l][i] + grow;
                if (!pair_separated(xs, u, s, ob, false, &val)) live &= ~(1ull << k);
            }
        }
    }
    return live;
}

__global__ __launch_bounds__(SL_BLOCK) void slices_fill_kernel(uint64_t* __restrict__ rows, size_t count, uint64_t value) {
    const size_t i = (size_t)blockIdx.x * SL_BLOCK + threadIdx.x;
    if (i < count) rows[i] = value;
}

// One launch: grid (ceil((N + M + most extra sub-segments of a world) / SL_BLOCK), W).  Item i < N is node i; item N + k, k < M, is edge
// sub-segment k as roadmap_check_kernel cuts them; the items after those are the sub-segments of world w's extra edges,
// x_item [x_off[w] .. x_off[w + 1])[3] = (extra edge, sub-segment, S), the edge's ends at x_q [extra][2][n].  edge_slices and extra_slices
// must hold the low K ones on entry; a sub-segment that lost slices ANDs its mask in (a 64-bit vector atomic; AND commutes).
__global__ __launch_bounds__(SL_BLOCK) void roadmap_slices_kernel(RmRobot rb, int32_t N, int64_t M, const double* __restrict__ nodes,
                                                                   const int32_t* __restrict__ edges, const int64_t* __restrict__ edge_off,
                                                                   const int32_t* __restrict__ sample_edge, const double* __restrict__ obstacles,
                                                                   const double* __restrict__ velocity, const double* __restrict__ mid,
                                                                   const double* __restrict__ half, int32_t O, int32_t E, int32_t K,
                                                                   const int32_t* __restrict__ x_off, const int32_t* __restrict__ x_item,
                                                                   const double* __restrict__ x_q, uint64_t* __restrict__ node_slices,
                                                                   uint64_t* edge_slices, uint64_t* extra_slices) {
    extern __shared__ double s_obs[];   // [O][RM_MOV_STRIDE], then mid [K], half [K]
    const int w = blockIdx.y;
    double* s_mid = s_obs + (size_t)O * RM_MOV_STRIDE;
    double* s_half = s_mid + K;
    for (int k = threadIdx.x; k < K; k += SL_BLOCK) {
        s_mid[k] = mid[(size_t)w * K + k];
        s_half[k] = half[(size_t)w * K + k];
    }
    stage_obstacles_moving_lds<SL_BLOCK>(obstacles + (size_t)w * O * ARMOUR_OBS_DOUBLES, velocity + (size_t)w * O * 3, O, s_obs);   // (ends at the barrier)
    const int64_t item = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x;
    const int32_t x0 = x_off[w], nx = x_off[w + 1] - x0;
    if (item >= (int64_t)N + M + nx) return;
    double q[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS];
    uint64_t* row = nullptr;            // the edge or extra row this sub-segment belongs to (null: a node)
    if (item < N) {
#pragma unroll
        for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q[j] = j < rb.n ? nodes[(size_t)item * rb.n + j] : 0.0;
#pragma unroll
        for (int l = 0; l < ARMOUR_MAX_JOINTS; l++) r[l] = 0.0;
    } else if (item < (int64_t)N + M) {
        const int64_t k = item - N;
        const int e = sample_edge[k];
        const int64_t s = k - edge_off[e], S = edge_off[e + 1] - edge_off[e];
        edge_sample(rb, nodes + (size_t)edges[2 * e] * rb.n, nodes + (size_t)edges[2 * e + 1] * rb.n, s, S, q, r);
        row = edge_slices + (size_t)w * E + e;
    } else {
        const int32_t* it = x_item + 3 * ((size_t)x0 + (size_t)(item - N - M));
        const double* a = x_q + (size_t)it[0] * 2 * rb.n;
        edge_sample(rb, a, a + rb.n, it[1], it[2], q, r);
        row = extra_slices + it[0];
    }
    const uint64_t live = config_slices(rb, q, r, s_obs, O, s_mid, s_half, K);
    if (!row) node_slices[(size_t)w * N + item] = live;
    else if (live != low_ones(K)) atomicAnd(reinterpret_cast<unsigned long long*>(row), (unsigned long long)live);
}

// ---- the operators of the search on 64-bit masks (include/armour_hip.h); none shifts by 64
__host__ __device__ inline uint64_t shl_sat(uint64_t x, int c) { return c >= 64 ? 0ull : x << c; }
// AND over i < c of (m >> i), 1 <= c <= 64: the slices from which c consecutive slices are free
__host__ __device__ inline uint64_t avail(uint64_t m, int c) {
    uint64_t a = m;
    for (int done = 1; done < c;) {
        const int s = done < c - done ? done : c - done;   // <= 32
        a &= a >> s;
        done += s;
    }
    return a;
}
// the least y that holds x & m and, with a slice of y, the next slice when m has it: waiting at a node while it stays free (a parallel
// prefix over the runs of m)
__host__ __device__ inline uint64_t fill(uint64_t x, uint64_t m) {
    uint64_t g = x & m, p = m;
    g |= p & (g << 1);  p &= p << 1;
    g |= p & (g << 2);  p &= p << 2;
    g |= p & (g << 4);  p &= p << 4;
    g |= p & (g << 8);  p &= p << 8;
    g |= p & (g << 16); p &= p << 16;
    g |= p & (g << 32);
    return g;
}

// world w's graph as the search reads it; reach is written in place
struct ArWorld {
    int32_t N, K, X;
    const int32_t *row_off, *col, *eid, *steps;     // the roadmap's rows, steps [E]
    const uint64_t *nm, *em;                        // node_slices[w], edge_slices[w]
    const int32_t *xu, *xv, *xs;                    // the world's extra edges: ends in [0, N + 2), steps
    const uint64_t* xm;
    uint64_t start, goal;                           // the masks of node N and node N + 1
    uint64_t* reach;                                // [N + 2]
};
__host__ __device__ inline uint64_t ar_mask(const ArWorld& g, int v) { return v < g.N ? g.nm[v] : v == g.N ? g.start : g.goal; }
// what reaches the far end (mask `to`) over an edge of mask m and c <= K steps from the slices `from` of the near end
__host__ __device__ inline uint64_t ar_move(uint64_t from, uint64_t m, int c, uint64_t to) { return shl_sat(from & avail(m, c), c) & to; }
// row v after the roadmap's edges at v are pulled in and the waits are closed
__host__ __device__ inline uint64_t ar_pull(const ArWorld& g, int v, uint64_t cur) {
    const uint64_t mv = ar_mask(g, v);
    if (v < g.N && mv)
        for (int k = g.row_off[v], k1 = g.row_off[v + 1]; k < k1; k++) {
            const int e = g.eid[k], c = g.steps[e];
            if (c > g.K) continue;
            cur |= ar_move(g.reach[g.col[k]], g.em[e], c, mv);
        }
    return fill(cur, mv);
}
// extra edge i in direction dir (0: xu -> xv): the far end and what reaches it
__host__ __device__ inline uint64_t ar_push(const ArWorld& g, int i, int dir, int* to) {
    const int u = dir ? g.xv[i] : g.xu[i], v = dir ? g.xu[i] : g.xv[i], c = g.xs[i];
    *to = v;
    return c > g.K ? 0ull : ar_move(g.reach[u], g.xm[i], c, ar_mask(g, v));
}
// The backward walk from (N + 1, goal_slice): at (v, k) the first usable incident edge (the roadmap's in row order, then the extras in list
// order) with c <= k and bit k - c set in reach[u] and in avail(m, c), else the wait (v, k - 1).  A node is listed with its arrival slice when
// the walk leaves it, the start with the slice at which the path leaves it.  pn / ps [SL_PATH] are filled from the back; returns the number
// of entries, -1 when the rows are not a fixed point of the rules (the caller's ARMOUR_ESTATE).
__host__ __device__ inline int ar_walk(const ArWorld& g, int goal_slice, int32_t* pn, int32_t* ps) {
    int v = g.N + 1, k = goal_slice, len = 0;
    for (int guard = 0; v != g.N; guard++) {
        if (guard > 2 * SL_PATH || len >= SL_PATH - 1) return -1;
        int u = -1, cu = 0;
        if (v < g.N)
            for (int j = g.row_off[v], j1 = g.row_off[v + 1]; j < j1 && u < 0; j++) {
                const int e = g.eid[j], c = g.steps[e];
                if (c > g.K || c > k) continue;
                if (((g.reach[g.col[j]] >> (k - c)) & 1ull) && ((avail(g.em[e], c) >> (k - c)) & 1ull)) { u = g.col[j]; cu = c; }
            }
        for (int i = 0; i < g.X && u < 0; i++) {
            if (g.xu[i] != v && g.xv[i] != v) continue;
            const int far = g.xu[i] == v ? g.xv[i] : g.xu[i], c = g.xs[i];
            if (c > g.K || c > k) continue;
            if (((g.reach[far] >> (k - c)) & 1ull) && ((avail(g.xm[i], c) >> (k - c)) & 1ull)) { u = far; cu = c; }
        }
        if (u >= 0) {
            pn[SL_PATH - 1 - len] = v;
            ps[SL_PATH - 1 - len] = k;
            len++;
            v = u;
            k -= cu;
        } else {
            if (k == 0 || !((g.reach[v] >> (k - 1)) & 1ull)) return -1;
            k--;
        }
    }
    pn[SL_PATH - 1 - len] = v;
    ps[SL_PATH - 1 - len] = k;
    return len + 1;
}
// the entries to the front of the rows (dest below source: a forward copy), -1 behind them
__host__ __device__ inline void ar_front(int len, int32_t* pn, int32_t* ps) {
    if (len < 0) len = 0;
    for (int i = 0; len < SL_PATH && i < len; i++) {
        pn[i] = pn[SL_PATH - len + i];
        ps[i] = ps[SL_PATH - len + i];
    }
    for (int i = len; i < SL_PATH; i++) pn[i] = ps[i] = -1;
}

// grid W, one block per world.  Thread t owns the rows v = t (mod AR_BLOCK) of reach[w][0 .. N + 2): it alone stores them in the pull phase;
// the extra edges push into rows of other owners with a 64-bit vector atomic OR in a phase of their own.  A lane that reads a row from
// before or after a store of the same sweep reads a state of the iteration either way (the rows only grow).  ends [W][2]: the masks of
// node N and N + 1.  out [W][3] = goal_slice, path_len, sweeps; path [W][2][SL_PATH] = nodes, slices.
__global__ __launch_bounds__(AR_BLOCK) void roadmap_arrival_kernel(int32_t N, int32_t E, int32_t K, const int32_t* __restrict__ row_off, const int32_t* __restrict__ col,
                                                                    const int32_t* __restrict__ eid, const int32_t* __restrict__ steps,
                                                                    const uint64_t* __restrict__ node_slices, const uint64_t* __restrict__ edge_slices,
                                                                    const int32_t* __restrict__ x_off, const int32_t* __restrict__ x_u,
                                                                    const int32_t* __restrict__ x_v, const int32_t* __restrict__ x_steps,
                                                                    const uint64_t* __restrict__ x_mask, const uint64_t* __restrict__ ends, uint64_t* reach,
                                                                    int32_t* __restrict__ out, int32_t* __restrict__ path, int32_t* __restrict__ status) {
    const int w = blockIdx.x, t = threadIdx.x;
    const int32_t x0 = x_off[w];
    ArWorld g;
    g.N = N; g.K = K; g.X = x_off[w + 1] - x0;
    g.row_off = row_off; g.col = col; g.eid = eid; g.steps = steps;
    g.nm = node_slices + (size_t)w * N;
    g.em = edge_slices + (size_t)w * E;
    g.xu = x_u + x0; g.xv = x_v + x0; g.xs = x_steps + x0; g.xm = x_mask + x0;
    g.start = ends[2 * w]; g.goal = ends[2 * w + 1];
    g.reach = reach + (size_t)w * (N + 2);
    for (int v = t; v < N + 2; v += AR_BLOCK) g.reach[v] = v == N ? fill(1ull, g.start) : 0ull;
    __syncthreads();
    int n_sweeps = 0;
    bool capped = false;
    for (;;) {
        int changed = 0;
        for (int j = t; j < 2 * g.X; j += AR_BLOCK) {
            int to;
            const uint64_t val = ar_push(g, j >> 1, j & 1, &to);
            if (val & ~g.reach[to]) {
                atomicOr(reinterpret_cast<unsigned long long*>(g.reach + to), (unsigned long long)val);
                changed = 1;
            }
        }
        __syncthreads();
        for (int v = t; v < N + 2; v += AR_BLOCK) {
            const uint64_t old = g.reach[v], now = ar_pull(g, v, old);
            if (now != old) {
                g.reach[v] = now;
                changed = 1;
            }
        }
        n_sweeps++;
        if (!__syncthreads_or(changed)) break;
        if (n_sweeps > K + 1) { capped = true; break; }
    }
    if (t == 0) {
        const uint64_t at_goal = g.reach[N + 1];
        const int goal_slice = at_goal ? __builtin_ctzll(at_goal) : -1;
        int32_t *pn = path + (size_t)w * 2 * SL_PATH, *ps = pn + SL_PATH;
        int len = 0;
        if (goal_slice >= 0 && !capped) len = ar_walk(g, goal_slice, pn, ps);
        ar_front(len, pn, ps);
        out[3 * w] = goal_slice;
        out[3 * w + 1] = len < 0 ? 0 : len;
        out[3 * w + 2] = n_sweeps;
        if (capped) *status = 1;          // (no atomics: every writer writes the same value)
        else if (len < 0) *status = 2;
    }
}

// the argument rules of both sliced checks, before a device is touched
int slices_args(const char* who, const ArmourRoadmap* rm, int32_t W, int32_t O, const double* obstacles, const double* velocity, const double* t0, double dt,
                int32_t K, int32_t Q, const int32_t* extra_world, const double* extra_a, const double* extra_b) {
    if (!rm) { armour_set_error("%s: null handle", who); return ARMOUR_EINVAL; }
    ARMOUR_TRY(armour_check_world_counts(who, W, O, obstacles));
    const size_t nobs = (size_t)W * O * ARMOUR_OBS_DOUBLES;
    if (const size_t i = first_nonfinite(obstacles, nobs); i < nobs) { armour_set_error("%s: obstacle %zu is not finite", who, i / ARMOUR_OBS_DOUBLES); return ARMOUR_EINVAL; }
    if ((W > 0 && O > 0 && !velocity) || (W > 0 && !t0)) { armour_set_error("%s: null velocity or t0", who); return ARMOUR_EINVAL; }
    if (!finite_all(velocity, (size_t)W * O * 3) || !finite_all(t0, (size_t)W)) { armour_set_error("%s: a velocity or a t0 is not finite", who); return ARMOUR_EINVAL; }
    if (K < 1 || K > ARMOUR_ROADMAP_SLICES_MAX) { armour_set_error("%s: K = %d (1..%d)", who, K, ARMOUR_ROADMAP_SLICES_MAX); return ARMOUR_EINVAL; }
    if (!std::isfinite(dt) || !(dt > 0.0)) { armour_set_error("%s: dt = %g", who, dt); return ARMOUR_EINVAL; }
    for (int32_t w = 0; w < W; w++)
        if (!std::isfinite(t0[w] + (double)K * dt)) { armour_set_error("%s: world %d: the last slice ends at %g", who, w, t0[w] + (double)K * dt); return ARMOUR_EINVAL; }
    if (Q < 0 || (Q > 0 && (!extra_world || !extra_a || !extra_b))) { armour_set_error("%s: Q = %d, or a null extra array", who, Q); return ARMOUR_EINVAL; }
    const int n = rm->rb.n;
    for (int32_t i = 0; i < Q; i++) {
        if (extra_world[i] < 0 || extra_world[i] >= W) { armour_set_error("%s: extra edge %d names world %d of %d", who, i, extra_world[i], W); return ARMOUR_EINVAL; }
        if (!finite_all(extra_a + (size_t)i * n, (size_t)n) || !finite_all(extra_b + (size_t)i * n, (size_t)n)) { armour_set_error("%s: extra edge %d is not finite", who, i); return ARMOUR_EINVAL; }
    }
    return ARMOUR_OK;
}

// the slice boundaries and, from those doubles, every slice's midpoint and half width: what the kernel, the host twin and a caller of
// armour_roadmap_check_moving on [times[k], times[k + 1]] all judge by
void slice_tables(int32_t W, int32_t K, const double* t0, double dt, std::vector<double>* times, std::vector<double>* mid, std::vector<double>* half) {
    times->resize((size_t)W * (K + 1));
    mid->resize((size_t)W * K);
    half->resize((size_t)W * K);
    for (int32_t w = 0; w < W; w++) {
        double* t = times->data() + (size_t)w * (K + 1);
        for (int k = 0; k <= K; k++) t[k] = t0[w] + (double)k * dt;
        for (int k = 0; k < K; k++) {
            (*mid)[(size_t)w * K + k] = 0.5 * (t[k] + t[k + 1]);
            (*half)[(size_t)w * K + k] = 0.5 * (t[k + 1] - t[k]);
        }
    }
}

void keep_slices(ArmourRoadmap* rm, int32_t W, int32_t O, int32_t K, double dt, const double* t0) {
    rm->sl_W = W;
    rm->sl_O = O;
    rm->sl_K = K;
    rm->sl_dt = dt;
    rm->sl_t0.assign(t0, t0 + W);
}

// the roadmap's edge lengths and rows, once per handle: armour_roadmap_field's (neighbour ascending, then edge id), on the host
int slices_csr(ArmourRoadmap* rm) {
    if (rm->sl_csr_ready) return ARMOUR_OK;
    const int n = rm->rb.n, N = rm->N, E = rm->E;
    if (2 * (int64_t)E > INT32_MAX) { armour_set_error("armour_roadmap_arrival: %d edges, room for 2^30 - 1", E); return ARMOUR_ECAPACITY; }
    rm->sl_len.resize((size_t)E);
    rm->sl_row_off.assign((size_t)N + 1, 0);
    rm->sl_col.resize((size_t)2 * E);
    rm->sl_eid.resize((size_t)2 * E);
    for (int e = 0; e < E; e++) {
        const int a = rm->edges[2 * e], b = rm->edges[2 * e + 1];
        rm->sl_len[e] = rmhost::wrapped_distance(rm->rb, &rm->nodes[(size_t)a * n], &rm->nodes[(size_t)b * n]);
        rm->sl_row_off[a + 1]++;
        rm->sl_row_off[b + 1]++;
    }
    for (int v = 0; v < N; v++) rm->sl_row_off[v + 1] += rm->sl_row_off[v];
    std::vector<std::pair<int32_t, int32_t>> ent((size_t)2 * E);
    std::vector<int32_t> at(rm->sl_row_off.begin(), rm->sl_row_off.end() - 1);
    for (int e = 0; e < E; e++) {
        const int a = rm->edges[2 * e], b = rm->edges[2 * e + 1];
        ent[at[a]++] = {b, e};
        ent[at[b]++] = {a, e};
    }
    for (int v = 0; v < N; v++) std::sort(ent.begin() + rm->sl_row_off[v], ent.begin() + rm->sl_row_off[v + 1]);
    for (size_t k = 0; k < ent.size(); k++) {
        rm->sl_col[k] = ent[k].first;
        rm->sl_eid[k] = ent[k].second;
    }
    rm->sl_csr_ready = true;
    return ARMOUR_OK;
}

// steps(len) = max(1, ceil(len / step_len)); anything above K is K + 1 (unusable), so the device sees a small int32
int32_t steps_of(double len, double step_len, int32_t K) {
    const double c = std::ceil(len / step_len);
    return !(c <= (double)K) ? K + 1 : c < 1.0 ? 1 : (int32_t)c;
}

// what both arrival entries check and prepare on the host
struct ArrivalInput {
    std::vector<int32_t> steps, x_off, x_steps;
    std::vector<uint64_t> x_mask, ends;
};
int arrival_args(const char* who, ArmourRoadmap* rm, double step_len, int32_t X, const int32_t* x_world, const int32_t* x_u, const int32_t* x_v, const double* x_len,
                 const uint64_t* x_mask, const uint64_t* start_mask, const uint64_t* goal_mask, ArrivalInput* in) {
    if (!rm) { armour_set_error("%s: null handle", who); return ARMOUR_EINVAL; }
    if (rm->sl_W < 0) { armour_set_error("%s: no armour_roadmap_check_slices yet", who); return ARMOUR_ESTATE; }
    if (rm->self_on) { armour_set_error("%s: the self masks are on (armour_roadmap_use_self); the space-time search does not read them", who); return ARMOUR_ESTATE; }
    const int32_t W = rm->sl_W, K = rm->sl_K, N = rm->N, E = rm->E;
    if (!std::isfinite(step_len) || !(step_len > 0.0)) { armour_set_error("%s: step_len = %g", who, step_len); return ARMOUR_EINVAL; }
    if (X < 0 || (X > 0 && (!x_world || !x_u || !x_v || !x_len || !x_mask)) || (W > 0 && (!start_mask || !goal_mask))) {
        armour_set_error("%s: X = %d, or a null array", who, X);
        return ARMOUR_EINVAL;
    }
    const uint64_t ones = low_ones(K);
    in->x_off.assign((size_t)W + 1, 0);
    in->x_steps.resize((size_t)X);
    in->x_mask.resize((size_t)X);
    for (int32_t i = 0; i < X; i++) {
        if (x_world[i] < 0 || x_world[i] >= W || (i > 0 && x_world[i] < x_world[i - 1])) { armour_set_error("%s: extra edge %d: world %d of %d, or not sorted by world", who, i, x_world[i], W); return ARMOUR_EINVAL; }
        if (x_u[i] < 0 || x_u[i] > N + 1 || x_v[i] < 0 || x_v[i] > N + 1) { armour_set_error("%s: extra edge %d joins %d and %d of %d", who, i, x_u[i], x_v[i], N + 2); return ARMOUR_EINVAL; }
        if (!std::isfinite(x_len[i]) || x_len[i] < 0.0) { armour_set_error("%s: extra edge %d: length %g", who, i, x_len[i]); return ARMOUR_EINVAL; }
        in->x_off[(size_t)x_world[i] + 1]++;
        in->x_steps[i] = steps_of(x_len[i], step_len, K);
        in->x_mask[i] = x_mask[i] & ones;
    }
    for (int32_t w = 0; w < W; w++) in->x_off[w + 1] += in->x_off[w];
    in->ends.resize((size_t)2 * W);
    for (int32_t w = 0; w < W; w++) {
        in->ends[2 * w] = (start_mask[w] | 1ull) & ones;
        in->ends[2 * w + 1] = goal_mask[w] & ones;
    }
    ARMOUR_TRY(slices_csr(rm));
    in->steps.resize((size_t)E);
    for (int e = 0; e < E; e++) in->steps[e] = steps_of(rm->sl_len[e], step_len, K);
    return ARMOUR_OK;
}

// one world's extra edges and the sub-segments they are cut into, for the sliced check
struct ExtraItems {
    std::vector<int32_t> off, item;   // [W + 1]; [..][3] = extra edge, sub-segment, S, world by world
    std::vector<double> q;            // [Q][2][n]
    int32_t most = 0;                 // the most sub-segments a world has
};
int extra_items(const char* who, const ArmourRoadmap* rm, int32_t W, int32_t Q, const int32_t* extra_world, const double* extra_a, const double* extra_b, ExtraItems* x) {
    const int n = rm->rb.n;
    std::vector<int64_t> S((size_t)Q), count((size_t)W + 1, 0);
    x->q.resize((size_t)Q * 2 * n);
    for (int32_t i = 0; i < Q; i++) {
        S[i] = edge_segments(rm->rb, extra_a + (size_t)i * n, extra_b + (size_t)i * n, rm->edge_step);
        count[(size_t)extra_world[i] + 1] += S[i];
        std::memcpy(&x->q[(size_t)i * 2 * n], extra_a + (size_t)i * n, n * sizeof(double));
        std::memcpy(&x->q[(size_t)i * 2 * n + n], extra_b + (size_t)i * n, n * sizeof(double));
    }
    for (int32_t w = 0; w < W; w++) {
        x->most = (int32_t)std::min<int64_t>(std::max<int64_t>(x->most, count[w + 1]), INT32_MAX);
        count[w + 1] += count[w];
    }
    if (count[W] > INT32_MAX / 4 || (int64_t)rm->N + rm->M + x->most > INT32_MAX) {
        armour_set_error("%s: %lld sub-segments of extra edges (edge_step %g too small)", who, (long long)count[W], rm->edge_step);
        return ARMOUR_ECAPACITY;
    }
    x->off.resize((size_t)W + 1);
    for (int32_t w = 0; w <= W; w++) x->off[w] = (int32_t)count[w];
    x->item.resize((size_t)count[W] * 3);
    std::vector<int64_t> at(count.begin(), count.end() - 1);
    for (int32_t i = 0; i < Q; i++)
        for (int64_t s = 0; s < S[i]; s++) {
            int32_t* it = &x->item[(size_t)at[extra_world[i]]++ * 3];
            it[0] = i; it[1] = (int32_t)s; it[2] = (int32_t)S[i];
        }
    return ARMOUR_OK;
}

}  // namespace

extern "C" int armour_roadmap_check_slices(ArmourRoadmap* rm, int32_t W, int32_t O, const double* obstacles, const double* velocity, const double* t0, double dt,
                                           int32_t K, int32_t Q, const int32_t* extra_world, const double* extra_a, const double* extra_b,
                                           uint64_t* node_slices, uint64_t* edge_slices, uint64_t* extra_slices, double* slice_times, double* ms) {
    const char* who = "armour_roadmap_check_slices";
    ARMOUR_TRY(slices_args(who, rm, W, O, obstacles, velocity, t0, dt, K, Q, extra_world, extra_a, extra_b));
    if (rm->device < 0) { armour_set_error("%s: the handle was made by armour_roadmap_create_host and holds nothing on a device", who); return ARMOUR_EDEVICE; }
    ExtraItems x;
    ARMOUR_TRY(extra_items(who, rm, W, Q, extra_world, extra_a, extra_b, &x));
    std::vector<double> times, mid, half;
    slice_tables(W, K, t0, dt, &times, &mid, &half);
    HIPCHK(hipSetDevice(rm->device));
    rm->sl_W = -1;             // the tables are rewritten from here on: a call that fails below leaves none
    const size_t WN = (size_t)W * rm->N, WE = (size_t)W * rm->E;
    ARMOUR_TRY(rm->d_sl_node.reserve(WN));
    ARMOUR_TRY(rm->d_sl_edge.reserve(WE));
    ARMOUR_TRY(rm->d_sl_extra.reserve((size_t)Q));
    ARMOUR_TRY(rm->d_sl_obs.upload(obstacles, (size_t)W * O * ARMOUR_OBS_DOUBLES, rm->stream));
    ARMOUR_TRY(rm->d_sl_vel.upload(velocity, (size_t)W * O * 3, rm->stream));
    ARMOUR_TRY(rm->d_sl_mid.upload(mid.data(), mid.size(), rm->stream));
    ARMOUR_TRY(rm->d_sl_half.upload(half.data(), half.size(), rm->stream));
    ARMOUR_TRY(rm->d_sl_xoff.upload(x.off.data(), x.off.size(), rm->stream));
    ARMOUR_TRY(rm->d_sl_xitem.upload(x.item.data(), x.item.size(), rm->stream));
    ARMOUR_TRY(rm->d_sl_xq.upload(x.q.data(), x.q.size(), rm->stream));
    const uint64_t ones = low_ones(K);
    ARMOUR_TRY(rm->ev.record_start(rm->stream));
    if (WE) hipLaunchKernelGGL(slices_fill_kernel, dim3((unsigned)((WE + SL_BLOCK - 1) / SL_BLOCK)), dim3(SL_BLOCK), 0, rm->stream, rm->d_sl_edge.p, WE, ones);
    if (Q) hipLaunchKernelGGL(slices_fill_kernel, dim3((unsigned)(((size_t)Q + SL_BLOCK - 1) / SL_BLOCK)), dim3(SL_BLOCK), 0, rm->stream, rm->d_sl_extra.p, (size_t)Q, ones);
    const int64_t items = (int64_t)rm->N + rm->M + x.most;
    if (W > 0 && items > 0) {
        const dim3 grid((unsigned)((items + SL_BLOCK - 1) / SL_BLOCK), (unsigned)W);
        const size_t lds = ((size_t)O * RM_MOV_STRIDE + 2 * (size_t)K) * sizeof(double);
        hipLaunchKernelGGL(roadmap_slices_kernel, grid, dim3(SL_BLOCK), lds, rm->stream, rm->rb, rm->N, rm->M, rm->d_nodes, rm->d_edges, rm->d_edge_off,
                           rm->d_sample_edge, rm->d_sl_obs, rm->d_sl_vel, rm->d_sl_mid, rm->d_sl_half, O, rm->E, K, rm->d_sl_xoff, rm->d_sl_xitem, rm->d_sl_xq,
                           rm->d_sl_node, rm->d_sl_edge, rm->d_sl_extra);
    }
    HIPCHK(hipGetLastError());
    ARMOUR_TRY(rm->ev.record_stop(rm->stream));
    rm->sl_on_host = node_slices && edge_slices;
    if (rm->sl_on_host) {
        rm->sl_node.resize(WN);
        rm->sl_edge.resize(WE);
    }
    if (node_slices && WN) HIPCHK(hipMemcpyAsync(rm->sl_on_host ? rm->sl_node.data() : node_slices, rm->d_sl_node, WN * sizeof(uint64_t), hipMemcpyDeviceToHost, rm->stream));
    if (edge_slices && WE) HIPCHK(hipMemcpyAsync(rm->sl_on_host ? rm->sl_edge.data() : edge_slices, rm->d_sl_edge, WE * sizeof(uint64_t), hipMemcpyDeviceToHost, rm->stream));
    if (extra_slices && Q) HIPCHK(hipMemcpyAsync(extra_slices, rm->d_sl_extra, (size_t)Q * sizeof(uint64_t), hipMemcpyDeviceToHost, rm->stream));
    HIPCHK(hipStreamSynchronize(rm->stream));
    if (ms) ARMOUR_TRY(rm->ev.elapsed_ms(ms));
    if (rm->sl_on_host && WN) std::memcpy(node_slices, rm->sl_node.data(), WN * sizeof(uint64_t));
    if (rm->sl_on_host && WE) std::memcpy(edge_slices, rm->sl_edge.data(), WE * sizeof(uint64_t));
    if (slice_times && W) std::memcpy(slice_times, times.data(), times.size() * sizeof(double));
    keep_slices(rm, W, O, K, dt, t0);
    return ARMOUR_OK;
}

// the same verdicts by the kernel's function in a host loop, on a handle of armour_roadmap_create_host
extern "C" int armour_roadmap_check_slices_host(ArmourRoadmap* rm, int32_t W, int32_t O, const double* obstacles, const double* velocity, const double* t0, double dt,
                                                int32_t K, int32_t Q, const int32_t* extra_world, const double* extra_a, const double* extra_b,
                                                uint64_t* node_slices, uint64_t* edge_slices, uint64_t* extra_slices, double* slice_times) {
    const char* who = "armour_roadmap_check_slices_host";
    ARMOUR_TRY(slices_args(who, rm, W, O, obstacles, velocity, t0, dt, K, Q, extra_world, extra_a, extra_b));
    if (rm->device >= 0) { armour_set_error("%s: the handle holds a device; make one with armour_roadmap_create_host", who); return ARMOUR_EINVAL; }
    std::vector<double> times, mid, half, staged((size_t)W * O * RM_MOV_STRIDE);
    slice_tables(W, K, t0, dt, &times, &mid, &half);
    stage_obstacles_moving(obstacles, velocity, (size_t)W * O, staged.data());
    rm->sl_W = -1;
    const int n = rm->rb.n, N = rm->N, E = rm->E;
    const uint64_t ones = low_ones(K);
    rm->sl_on_host = true;
    rm->sl_node.assign((size_t)W * N, 0);
    rm->sl_edge.assign((size_t)W * E, ones);
    double q[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS];
    // an edge's slices: the AND over its sub-segments; a row that is empty already needs no further sub-segment
    auto edge_rule = [&](int32_t w, const double* a, const double* b) {
        const double* obs = staged.data() + (size_t)w * O * RM_MOV_STRIDE;
        const int64_t S = edge_segments(rm->rb, a, b, rm->edge_step);
        uint64_t row = ones;
        for (int64_t s = 0; s < S && row; s++) {
            edge_sample(rm->rb, a, b, s, S, q, r);
            row &= config_slices(rm->rb, q, r, obs, O, &mid[(size_t)w * K], &half[(size_t)w * K], K);
        }
        return row;
    };
    for (int32_t w = 0; w < W; w++) {
        const double* obs = staged.data() + (size_t)w * O * RM_MOV_STRIDE;
        for (int i = 0; i < N; i++) {
            for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q[j] = j < n ? rm->nodes[(size_t)i * n + j] : 0.0;
            for (int l = 0; l < ARMOUR_MAX_JOINTS; l++) r[l] = 0.0;
            rm->sl_node[(size_t)w * N + i] = config_slices(rm->rb, q, r, obs, O, &mid[(size_t)w * K], &half[(size_t)w * K], K);
        }
        for (int e = 0; e < E; e++)
            rm->sl_edge[(size_t)w * E + e] = edge_rule(w, &rm->nodes[(size_t)rm->edges[2 * e] * n], &rm->nodes[(size_t)rm->edges[2 * e + 1] * n]);
    }
    for (int32_t i = 0; i < Q; i++) {
        const uint64_t row = edge_rule(extra_world[i], extra_a + (size_t)i * n, extra_b + (size_t)i * n);
        if (extra_slices) extra_slices[i] = row;
    }
    if (node_slices && W && N) std::memcpy(node_slices, rm->sl_node.data(), (size_t)W * N * sizeof(uint64_t));
    if (edge_slices && W && E) std::memcpy(edge_slices, rm->sl_edge.data(), (size_t)W * E * sizeof(uint64_t));
    if (slice_times && W) std::memcpy(slice_times, times.data(), times.size() * sizeof(double));
    keep_slices(rm, W, O, K, dt, t0);
    return ARMOUR_OK;
}

extern "C" int armour_roadmap_arrival(ArmourRoadmap* rm, double step_len, int32_t X, const int32_t* x_world, const int32_t* x_u, const int32_t* x_v, const double* x_len,
                                      const uint64_t* x_mask, const uint64_t* start_mask, const uint64_t* goal_mask, uint64_t* reach, int32_t* goal_slice,
                                      int32_t* path_len, int32_t* path_node, int32_t* path_slice, int32_t* sweeps, double* ms) {
    const char* who = "armour_roadmap_arrival";
    ArrivalInput in;
    ARMOUR_TRY(arrival_args(who, rm, step_len, X, x_world, x_u, x_v, x_len, x_mask, start_mask, goal_mask, &in));
    if (rm->device < 0) { armour_set_error("%s: the handle was made by armour_roadmap_create_host and holds nothing on a device", who); return ARMOUR_EDEVICE; }
    const int32_t W = rm->sl_W, K = rm->sl_K, N = rm->N, E = rm->E;
    if (ms) *ms = 0.0;
    HIPCHK(hipSetDevice(rm->device));
    if (!rm->sl_csr_on_device) {
        ARMOUR_TRY(rm->d_sl_row_off.upload(rm->sl_row_off.data(), rm->sl_row_off.size(), rm->stream));
        ARMOUR_TRY(rm->d_sl_col.upload(rm->sl_col.data(), rm->sl_col.size(), rm->stream));
        ARMOUR_TRY(rm->d_sl_eid.upload(rm->sl_eid.data(), rm->sl_eid.size(), rm->stream));
        rm->sl_csr_on_device = true;
    }
    const size_t rows = (size_t)W * ((size_t)N + 2);
    ARMOUR_TRY(rm->d_sl_steps.upload(in.steps.data(), in.steps.size(), rm->stream));
    ARMOUR_TRY(rm->d_sl_xoff.upload(in.x_off.data(), in.x_off.size(), rm->stream));
    ARMOUR_TRY(rm->d_sl_xu.upload(x_u, (size_t)X, rm->stream));
    ARMOUR_TRY(rm->d_sl_xv.upload(x_v, (size_t)X, rm->stream));
    ARMOUR_TRY(rm->d_sl_xsteps.upload(in.x_steps.data(), (size_t)X, rm->stream));
    ARMOUR_TRY(rm->d_sl_xmask.upload(in.x_mask.data(), (size_t)X, rm->stream));
    ARMOUR_TRY(rm->d_sl_ends.upload(in.ends.data(), in.ends.size(), rm->stream));
    ARMOUR_TRY(rm->d_sl_reach.reserve(rows));
    ARMOUR_TRY(rm->d_sl_out.reserve((size_t)3 * W));
    ARMOUR_TRY(rm->d_sl_path.reserve((size_t)2 * SL_PATH * W));
    ARMOUR_TRY(rm->d_sl_status.reserve(1));
    HIPCHK(hipMemsetAsync(rm->d_sl_status, 0, sizeof(int32_t), rm->stream));
    ARMOUR_TRY(rm->ev.record_start(rm->stream));
    if (W > 0) {
        hipLaunchKernelGGL(roadmap_arrival_kernel, dim3((unsigned)W), dim3(AR_BLOCK), 0, rm->stream, N, E, K, rm->d_sl_row_off, rm->d_sl_col, rm->d_sl_eid, rm->d_sl_steps,
                           rm->d_sl_node, rm->d_sl_edge, rm->d_sl_xoff, rm->d_sl_xu, rm->d_sl_xv, rm->d_sl_xsteps, rm->d_sl_xmask, rm->d_sl_ends, rm->d_sl_reach, rm->d_sl_out,
                           rm->d_sl_path, rm->d_sl_status);
        HIPCHK(hipGetLastError());
    }
    ARMOUR_TRY(rm->ev.record_stop(rm->stream));
    std::vector<int32_t> out((size_t)3 * W), path((size_t)2 * SL_PATH * W);
    int32_t status = 0;
    if (reach && rows) HIPCHK(hipMemcpyAsync(reach, rm->d_sl_reach, rows * sizeof(uint64_t), hipMemcpyDeviceToHost, rm->stream));
    if (W) HIPCHK(hipMemcpyAsync(out.data(), rm->d_sl_out, out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, rm->stream));
    if (W) HIPCHK(hipMemcpyAsync(path.data(), rm->d_sl_path, path.size() * sizeof(int32_t), hipMemcpyDeviceToHost, rm->stream));
    HIPCHK(hipMemcpyAsync(&status, rm->d_sl_status, sizeof(int32_t), hipMemcpyDeviceToHost, rm->stream));
    HIPCHK(hipStreamSynchronize(rm->stream));
    if (ms) ARMOUR_TRY(rm->ev.elapsed_ms(ms));
    if (status == 1) { armour_set_error("%s: a world's sweeps did not settle within K + 1 = %d", who, K + 1); return ARMOUR_ESTATE; }
    if (status != 0) { armour_set_error("%s: a world's backward walk left its reach rows", who); return ARMOUR_ESTATE; }
    for (int32_t w = 0; w < W; w++) {
        if (goal_slice) goal_slice[w] = out[3 * w];
        if (path_len) path_len[w] = out[3 * w + 1];
        if (sweeps) sweeps[w] = out[3 * w + 2];
        if (path_node) std::memcpy(path_node + (size_t)w * SL_PATH, &path[(size_t)w * 2 * SL_PATH], SL_PATH * sizeof(int32_t));
        if (path_slice) std::memcpy(path_slice + (size_t)w * SL_PATH, &path[(size_t)w * 2 * SL_PATH + SL_PATH], SL_PATH * sizeof(int32_t));
    }
    return ARMOUR_OK;
}

// the same fixed point and the same walk by the kernel's functions, world after world on the host (sweeps may differ: the order does)
extern "C" int armour_roadmap_arrival_host(ArmourRoadmap* rm, double step_len, int32_t X, const int32_t* x_world, const int32_t* x_u, const int32_t* x_v,
                                           const double* x_len, const uint64_t* x_mask, const uint64_t* start_mask, const uint64_t* goal_mask, uint64_t* reach,
                                           int32_t* goal_slice, int32_t* path_len, int32_t* path_node, int32_t* path_slice, int32_t* sweeps) {
    const char* who = "armour_roadmap_arrival_host";
    ArrivalInput in;
    ARMOUR_TRY(arrival_args(who, rm, step_len, X, x_world, x_u, x_v, x_len, x_mask, start_mask, goal_mask, &in));
    if (rm->device >= 0) { armour_set_error("%s: the handle holds a device; make one with armour_roadmap_create_host", who); return ARMOUR_EINVAL; }
    const int32_t W = rm->sl_W, K = rm->sl_K, N = rm->N, E = rm->E;
    std::vector<uint64_t> rows((size_t)N + 2);
    for (int32_t w = 0; w < W; w++) {
        const int32_t x0 = in.x_off[w];
        ArWorld g;
        g.N = N; g.K = K; g.X = in.x_off[w + 1] - x0;
        g.row_off = rm->sl_row_off.data(); g.col = rm->sl_col.data(); g.eid = rm->sl_eid.data(); g.steps = in.steps.data();
        g.nm = rm->sl_node.data() + (size_t)w * N;
        g.em = rm->sl_edge.data() + (size_t)w * E;
        g.xu = x_u + x0; g.xv = x_v + x0; g.xs = in.x_steps.data() + x0; g.xm = in.x_mask.data() + x0;
        g.start = in.ends[2 * w]; g.goal = in.ends[2 * w + 1];
        g.reach = rows.data();
        std::fill(rows.begin(), rows.end(), 0ull);
        rows[N] = fill(1ull, g.start);
        int n_sweeps = 0;
        for (bool changed = true; changed;) {
            changed = false;
            for (int j = 0; j < 2 * g.X; j++) {
                int to;
                const uint64_t val = ar_push(g, j >> 1, j & 1, &to);
                if (val & ~rows[to]) { rows[to] |= val; changed = true; }
            }
            for (int v = 0; v < N + 2; v++) {
                const uint64_t now = ar_pull(g, v, rows[v]);
                if (now != rows[v]) { rows[v] = now; changed = true; }
            }
            n_sweeps++;
            if (changed && n_sweeps > K + 1) { armour_set_error("%s: world %d's sweeps did not settle within K + 1 = %d", who, w, K + 1); return ARMOUR_ESTATE; }
        }
        const int gs = rows[N + 1] ? __builtin_ctzll(rows[N + 1]) : -1;
        int32_t pn[SL_PATH], ps[SL_PATH];
        std::fill(pn, pn + SL_PATH, -1);
        std::fill(ps, ps + SL_PATH, -1);
        int len = 0;
        if (gs >= 0) {
            len = ar_walk(g, gs, pn, ps);
            if (len < 0) { armour_set_error("%s: world %d's backward walk left its reach rows", who, w); return ARMOUR_ESTATE; }
            ar_front(len, pn, ps);
        }
        if (reach) std::memcpy(reach + (size_t)w * (N + 2), rows.data(), rows.size() * sizeof(uint64_t));
        if (goal_slice) goal_slice[w] = gs;
        if (path_len) path_len[w] = len;
        if (sweeps) sweeps[w] = n_sweeps;
        if (path_node) std::memcpy(path_node + (size_t)w * SL_PATH, pn, sizeof(pn));
        if (path_slice) std::memcpy(path_slice + (size_t)w * SL_PATH, ps, sizeof(ps));
    }
    return ARMOUR_OK;
}
