// Nearest-neighbour search over a roadmap's nodes and the batched joins built on it (include/armour_hip.h, armour_roadmap_knn,
// armour_roadmap_connect_batch, armour_roadmap_descend_batch).  Brute force: the distance is the roadmap's wrapped distance (wrapped_sq /
// wrapped_norm in roadmap_handle.h, the one copy the host searches use too), and a result is the first k candidates in the total order
// (distance, index).  A total order makes every result unique, so the kernels below may deal the nodes to lanes, slices and tiles in any
// way and merge in any order: the test is bit equality with the host loop.
//
// Four kernels; no block waits on another (the merge is a launch of its own on the handle's stream):
//   knn_scan_kernel   many queries: a lane per query, the nodes of its slice staged in LDS tile by tile and read by all lanes at one address
//                     (a broadcast), the lane's sorted list in LDS (column t of [k][64]), its k-th key in registers as the admission test;
//   knn_tile_kernel   few queries: a block per (query, 256 nodes), a lane per node; a candidate's place in the tile's list is its rank,
//                     the number of smaller keys among the 256 in LDS;
//   knn_merge_kernel  a block per query: every entry of the query's P sorted partial lists finds its rank in the union by a binary
//                     search in each other list, and the first k ranks are the result.
//   connect_edges_kernel  a block per query of armour_roadmap_connect_batch: the edge rule of roadmap.hip's check kernel (edge_sample +
//                     config_free, and self_edge_sample + self_row_free with the self masks on) over (candidate, sub-segment) items.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "roadmap_handle.h"
#include "self_geometry.h"

using namespace rmgeo;

namespace {

constexpr int KS_BLOCK = 64;                  // scan: one wave, a query per lane; 12 k B of LDS per lane for its list
constexpr int KS_TILE = 64;                   // nodes staged per step
constexpr int KS_MAX_SLICES = 16;
constexpr int KS_FILL_LANES = 131072;         // lanes that fill the device twice over: fewer queries than this cut the nodes into slices
constexpr int KT_BLOCK = 256;                 // tile and merge: four waves
constexpr int CE_BLOCK = 256;                 // connect edges: four waves, a block per query
constexpr int KNN_NONE = INT_MAX;             // the index of "no candidate": (inf, KNN_NONE) follows every key of a node

// acc <= sq_bound(x) whenever sqrt(acc) <= x in fp64: sqrt is correctly rounded, so sqrt(acc) <= x gives acc <= x^2 (1 + 2^-53)^2, and
// fl(x * x) >= x^2 (1 - 2^-53); 1e-15 is nine times 2^-53.  Below 1e-290 (x * x may have lost bits or underflowed: x < 1e-145) the bound
// is held at 1e-290, above every such x^2.  It only spares square roots: what passes is decided by the distance itself.
__device__ inline double sq_bound(double x) { return fmax((x * x) * (1.0 + 1e-15), 1e-290); }

__device__ inline bool node_is_free(const uint8_t* __restrict__ node_free, const uint8_t* __restrict__ self_free, int32_t N, int w, int v) {
    return w < 0 || (node_free[(size_t)w * N + v] != 0 && (self_free == nullptr || self_free[v] != 0));
}

// grid (ceil(Q / KS_BLOCK), S): lane t of block x is query i = x KS_BLOCK + t, slice y holds the nodes [y per, (y + 1) per).  Dynamic LDS:
// s_ld [k][KS_BLOCK] doubles, s_tile [KS_TILE][n] doubles, s_lv [k][KS_BLOCK] ints.  Out: the lane's sorted list pd / pv [Q][S][k] and its
// length pcount [Q][S].
__global__ __launch_bounds__(KS_BLOCK) void knn_scan_kernel(RmRobot rb, int32_t N, int32_t Q, int32_t per, const double* __restrict__ nodes,
                                                             const double* __restrict__ queries, const int32_t* __restrict__ mask_row,
                                                             const int32_t* __restrict__ exclude, const uint8_t* __restrict__ node_free,
                                                             const uint8_t* __restrict__ self_free, int32_t k, double radius, double* __restrict__ pd,
                                                             int32_t* __restrict__ pv, int32_t* __restrict__ pcount) {
    extern __shared__ double s_raw[];
    const int n = rb.n, t = threadIdx.x;
    double* s_ld = s_raw;
    double* s_tile = s_raw + (size_t)k * KS_BLOCK;
    int32_t* s_lv = reinterpret_cast<int32_t*>(s_tile + (size_t)KS_TILE * n);
    const int i = blockIdx.x * KS_BLOCK + t, S = gridDim.y, y = blockIdx.y;
    const bool active = i < Q;
    double q[ARMOUR_MAX_FACTORS];
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q[j] = (active && j < n) ? queries[(size_t)i * n + j] : 0.0;
    const int w = (active && mask_row) ? mask_row[i] : -1;
    const int ex = (active && exclude) ? exclude[i] : -1;
    const int64_t v0 = (int64_t)y * per, v1 = v0 + per < N ? v0 + per : N;
    const double r_bound = sq_bound(radius);
    double bound = r_bound, kd = INFINITY;
    int kv = KNN_NONE, cnt = 0;
    for (int64_t base = v0; base < v1; base += KS_TILE) {
        const int m = (int)(v1 - base < KS_TILE ? v1 - base : KS_TILE);
        __syncthreads();                                                  // the last tile has been read
        for (int c = t; c < m * n; c += KS_BLOCK) s_tile[c] = nodes[(size_t)base * n + c];
        __syncthreads();
        for (int u = 0; u < m; u++) {
            const int v = (int)base + u;
            const double acc = wrapped_sq(rb, q, s_tile + u * n);
            if (!active || v == ex || !(acc <= bound) || !node_is_free(node_free, self_free, N, w, v)) continue;
            const double d = sqrt(acc);
            if (!(d <= radius) || (cnt == k && !key_less(d, v, kd, kv))) continue;
            int p = cnt < k ? cnt : k - 1;                                // the slot that opens; the larger keys move up one
            while (p > 0 && key_less(d, v, s_ld[(p - 1) * KS_BLOCK + t], s_lv[(p - 1) * KS_BLOCK + t])) {
                s_ld[p * KS_BLOCK + t] = s_ld[(p - 1) * KS_BLOCK + t];
                s_lv[p * KS_BLOCK + t] = s_lv[(p - 1) * KS_BLOCK + t];
                p--;
            }
            s_ld[p * KS_BLOCK + t] = d;
            s_lv[p * KS_BLOCK + t] = v;
            if (cnt < k) cnt++;
            if (cnt == k) {
                kd = s_ld[(k - 1) * KS_BLOCK + t];
                kv = s_lv[(k - 1) * KS_BLOCK + t];
                bound = fmin(r_bound, sq_bound(kd));
            }
        }
    }
    if (!active) return;
    const size_t list = (size_t)i * S + y;
    for (int r = 0; r < cnt; r++) {
        pd[list * k + r] = s_ld[r * KS_BLOCK + t];
        pv[list * k + r] = s_lv[r * KS_BLOCK + t];
    }
    pcount[list] = cnt;
}

// grid (P, Q), P = ceil(N / KT_BLOCK): lane t of block (x, i) is node v = x KT_BLOCK + t for query i.  Out: the tile's sorted list
// pd / pv [Q][P][k] and its length pcount [Q][P].
__global__ __launch_bounds__(KT_BLOCK) void knn_tile_kernel(RmRobot rb, int32_t N, const double* __restrict__ nodes, const double* __restrict__ queries,
                                                             const int32_t* __restrict__ mask_row, const int32_t* __restrict__ exclude,
                                                             const uint8_t* __restrict__ node_free, const uint8_t* __restrict__ self_free, int32_t k,
                                                             double radius, double* __restrict__ pd, int32_t* __restrict__ pv, int32_t* __restrict__ pcount) {
    __shared__ double s_d[KT_BLOCK];
    __shared__ int32_t s_v[KT_BLOCK];
    const int n = rb.n, t = threadIdx.x, i = blockIdx.y, P = gridDim.x;
    const int64_t v64 = (int64_t)blockIdx.x * KT_BLOCK + t;
    const int w = mask_row ? mask_row[i] : -1;
    const int ex = exclude ? exclude[i] : -1;
    bool valid = v64 < N && (int)v64 != ex && node_is_free(node_free, self_free, N, w, (int)v64);
    double d = INFINITY;
    if (valid) {
        double q[ARMOUR_MAX_FACTORS];
#pragma unroll
        for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q[j] = j < n ? queries[(size_t)i * n + j] : 0.0;
        d = wrapped_norm(rb, q, nodes + (size_t)v64 * n);
        valid = d <= radius;
    }
    const double kd = valid ? d : INFINITY;
    const int kv = valid ? (int)v64 : KNN_NONE;
    s_d[t] = kd;
    s_v[t] = kv;
    const int total = __syncthreads_count(valid);
    int rank = 0;
    for (int u = 0; u < KT_BLOCK; u++) rank += key_less(s_d[u], s_v[u], kd, kv) ? 1 : 0;
    const size_t list = (size_t)i * P + blockIdx.x;
    if (valid && rank < k) {
        pd[list * k + rank] = kd;
        pv[list * k + rank] = kv;
    }
    if (t == 0) pcount[list] = total < k ? total : k;
}

// grid Q: the P sorted lists of query i -> index / dist [Q][k] (padded) and count [Q]
__global__ __launch_bounds__(KT_BLOCK) void knn_merge_kernel(int32_t P, int32_t k, const double* __restrict__ pd, const int32_t* __restrict__ pv,
                                                              const int32_t* __restrict__ pcount, int32_t* __restrict__ index, double* __restrict__ dist,
                                                              int32_t* __restrict__ count) {
    __shared__ int s_total;
    const int t = threadIdx.x, i = blockIdx.x;
    const size_t first = (size_t)i * P;
    if (t == 0) s_total = 0;
    __syncthreads();
    int mine = 0;
    for (int l = t; l < P; l += KT_BLOCK) mine += pcount[first + l];
    if (mine) atomicAdd(&s_total, mine);
    const int64_t items = (int64_t)P * k;
    for (int64_t item = t; item < items; item += KT_BLOCK) {
        const int l = (int)(item / k), r = (int)(item % k);
        if (r >= pcount[first + l]) continue;
        const double d = pd[(first + l) * k + r];
        const int v = pv[(first + l) * k + r];
        int rank = r;                                                    // the smaller keys of its own list
        for (int o = 0; o < P && rank < k; o++) {
            if (o == l) continue;
            const double* od = pd + (first + o) * k;
            const int32_t* ov = pv + (first + o) * k;
            int lo = 0, hi = pcount[first + o];                          // the number of keys of list o below (d, v)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (key_less(od[mid], ov[mid], d, v)) lo = mid + 1; else hi = mid;
            }
            rank += lo;
        }
        if (rank < k) {
            dist[(size_t)i * k + rank] = d;
            index[(size_t)i * k + rank] = v;
        }
    }
    __syncthreads();
    const int found = s_total < k ? s_total : k;
    for (int r = found + t; r < k; r += KT_BLOCK) {
        dist[(size_t)i * k + r] = INFINITY;
        index[(size_t)i * k + r] = -1;
    }
    if (t == 0) count[i] = found;
}

// grid Q, dynamic LDS [O][RM_OBS_STRIDE] doubles: query i's candidates c < count[i] are the edges q[i] -> nodes[index[i][c]], candidate
// c = k (with target) the edge q[i] -> target[i].  An item is (candidate, sub-segment); a candidate found colliding is skipped by the items
// that have not started (s_ok: every writer writes 0).  on / shrink: the self table, null with the self masks off.
// MOVING (after armour_roadmap_check_moving): the window rule of roadmap.hip's moving check -- dynamic LDS [O][RM_MOV_STRIDE], velocity
// [W][O][3], mid / half [W] of the last check.  The static instantiation reads none of the three.
template <bool MOVING>
__global__ __launch_bounds__(CE_BLOCK) void connect_edges_kernel(RmRobot rb, double edge_step, int32_t k, const double* __restrict__ nodes,
                                                                  const double* __restrict__ q, const double* __restrict__ target,
                                                                  const int32_t* __restrict__ world, const double* __restrict__ obstacles,
                                                                  const double* __restrict__ velocity, const double* __restrict__ mid,
                                                                  const double* __restrict__ half, int32_t O,
                                                                  const int32_t* __restrict__ index, const int32_t* __restrict__ count,
                                                                  const uint8_t* __restrict__ on, const double* __restrict__ shrink, int32_t rows,
                                                                  uint8_t* __restrict__ ok /* [Q][k + 1] */) {
    extern __shared__ double s_obs[];   // [O][RM_OBS_STRIDE], MOVING: [O][RM_MOV_STRIDE]
    __shared__ int s_off[ARMOUR_ROADMAP_KNN_MAX + 2];
    __shared__ int s_ok[ARMOUR_ROADMAP_KNN_MAX + 1];
    const int n = rb.n, t = threadIdx.x, i = blockIdx.x;
    const double* a = q + (size_t)i * n;
    if constexpr (MOVING) stage_obstacles_moving_lds<CE_BLOCK>(obstacles + (size_t)world[i] * O * ARMOUR_OBS_DOUBLES, velocity + (size_t)world[i] * O * 3, O, s_obs);
    else stage_obstacles_lds<CE_BLOCK>(obstacles + (size_t)world[i] * O * ARMOUR_OBS_DOUBLES, O, s_obs);
    const int cands = count[i], C = k + 1;
    auto end_of = [&](int c) -> const double* {
        if (c < cands) return nodes + (size_t)index[(size_t)i * k + c] * n;
        return (c == k && target) ? target + (size_t)i * n : nullptr;
    };
    if (t == 0) {
        int off = 0;
        for (int c = 0; c < C; c++) {
            s_off[c] = off;
            const double* b = end_of(c);
            s_ok[c] = b ? 1 : 0;
            if (b) {
                const int64_t S = edge_segments(rb, a, b, edge_step);
                off = (int64_t)off + S > INT_MAX / 2 ? INT_MAX / 2 : off + (int)S;   // (an edge of 2^30 sub-segments: its tail is not tested, and the
                if (off == INT_MAX / 2) s_ok[c] = 0;                                  //  edge is refused)
            }
        }
        s_off[C] = off;
    }
    __syncthreads();
    const int items = s_off[C];
    for (int item = t; item < items; item += CE_BLOCK) {
        int c = 0;
        while (item >= s_off[c + 1]) c++;
        if (!s_ok[c]) continue;
        const double* b = end_of(c);
        const int64_t s = item - s_off[c], S = s_off[c + 1] - s_off[c];
        double x[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS];
        edge_sample(rb, a, b, s, S, x, r);
        bool free_;
        if constexpr (MOVING) free_ = config_free_moving(rb, x, r, s_obs, O, mid[world[i]], half[world[i]], false, nullptr);
        else free_ = config_free(rb, x, r, s_obs, O, false, nullptr);
        for (int row = 0; free_ && on && row < rows; row++) {
            double delta[ARMOUR_MAX_FACTORS], cl;
            int which;
            self_edge_sample(rb, a, b, s, S, x, delta);
            free_ = self_row_free(rb, row, x, delta, on + row * rb.J, shrink + row * rb.J, false, &cl, &which);
        }
        if (!free_) s_ok[c] = 0;
    }
    __syncthreads();
    for (int c = t; c < C; c += CE_BLOCK) ok[(size_t)i * C + c] = (uint8_t)s_ok[c];
}

// ---- what the entries share
struct KnnArgs {
    int32_t Q;
    const double* queries;
    const int32_t *mask_row, *exclude;
    int32_t k;
    double radius;
};

// the argument and state rules of armour_roadmap_knn / _knn_host; *masked = some query names a world
int check_knn(const char* who, const ArmourRoadmap* rm, const KnnArgs& a, const int32_t* index, const double* dist, const int32_t* count, bool* masked) {
    *masked = false;
    if (!rm) { armour_set_error("%s: null handle", who); return ARMOUR_EINVAL; }
    if (a.k < 1 || a.k > ARMOUR_ROADMAP_KNN_MAX) { armour_set_error("%s: k = %d (1..%d)", who, a.k, ARMOUR_ROADMAP_KNN_MAX); return ARMOUR_EINVAL; }
    if (a.Q < 0 || !(a.radius >= 0.0)) { armour_set_error("%s: Q = %d, radius = %g", who, a.Q, a.radius); return ARMOUR_EINVAL; }
    if (a.Q == 0 || rm->N == 0) return ARMOUR_OK;
    if (!a.queries || !index || !dist || !count) { armour_set_error("%s: null argument", who); return ARMOUR_EINVAL; }
    const size_t nq = (size_t)a.Q * rm->rb.n;
    if (const size_t i = first_nonfinite(a.queries, nq); i < nq) { armour_set_error("%s: query %zu is not finite", who, i / rm->rb.n); return ARMOUR_EINVAL; }
    for (int32_t i = 0; a.mask_row && i < a.Q; i++) {
        const int32_t w = a.mask_row[i];
        if (w < 0) continue;
        if (rm->W < 0) { armour_set_error("%s: query %d names world %d and there is no armour_roadmap_check yet", who, i, w); return ARMOUR_ESTATE; }
        if (rm->self_on && !rm->self_checked) { armour_set_error("%s: self masks are on and no armour_roadmap_check_self yet", who); return ARMOUR_ESTATE; }
        if (w >= rm->W) { armour_set_error("%s: query %d names world %d of %d", who, i, w, rm->W); return ARMOUR_EINVAL; }
        *masked = true;
    }
    return ARMOUR_OK;
}

// the search on the device: the queries are uploaded, the results stay in rm->d_kidx / d_kdist / d_kcount ([Q][k], [Q]) on the stream
int knn_launch(ArmourRoadmap* rm, const KnnArgs& a, bool masked) {
    const int n = rm->rb.n, N = rm->N, Q = a.Q, k = a.k;
    ARMOUR_TRY(rm->d_kq.upload(a.queries, (size_t)Q * n, rm->stream));
    if (masked) ARMOUR_TRY(rm->d_kmask.upload(a.mask_row, (size_t)Q, rm->stream));
    if (a.exclude) ARMOUR_TRY(rm->d_kexcl.upload(a.exclude, (size_t)Q, rm->stream));
    const bool self = masked && rm->self_on;
    if (self) ARMOUR_TRY(rm->d_self_node_free.upload(rm->self_node_free.data(), (size_t)N, rm->stream));
    const int32_t* d_mask = masked ? rm->d_kmask.p : nullptr;
    const int32_t* d_excl = a.exclude ? rm->d_kexcl.p : nullptr;
    const uint8_t* d_free = masked ? rm->d_node_free.p : nullptr;
    const uint8_t* d_self = self ? rm->d_self_node_free.p : nullptr;
    // the shape: a lane per query once the queries are many, else a block per (query, tile of nodes)
    const bool many = Q >= ARMOUR_ROADMAP_KNN_MANY;
    int P, per = 0;
    if (many) {
        const int want = (KS_FILL_LANES + Q - 1) / Q, room = (N + KS_TILE - 1) / KS_TILE;
        const int S = std::max(1, std::min({want, room, KS_MAX_SLICES}));
        per = (N + S - 1) / S;
        P = (N + per - 1) / per;
    } else {
        P = (N + KT_BLOCK - 1) / KT_BLOCK;
    }
    const size_t lists = (size_t)Q * P;
    ARMOUR_TRY(rm->d_pdist.reserve(lists * k));
    ARMOUR_TRY(rm->d_pidx.reserve(lists * k));
    ARMOUR_TRY(rm->d_pcount.reserve(lists));
    ARMOUR_TRY(rm->d_kdist.reserve((size_t)Q * k));
    ARMOUR_TRY(rm->d_kidx.reserve((size_t)Q * k));
    ARMOUR_TRY(rm->d_kcount.reserve((size_t)Q));
    if (many) {
        const size_t lds = ((size_t)k * KS_BLOCK + (size_t)KS_TILE * n) * sizeof(double) + (size_t)k * KS_BLOCK * sizeof(int32_t);
        hipLaunchKernelGGL(knn_scan_kernel, dim3((unsigned)((Q + KS_BLOCK - 1) / KS_BLOCK), (unsigned)P), dim3(KS_BLOCK), lds, rm->stream, rm->rb, N, Q, per,
                           rm->d_nodes, rm->d_kq, d_mask, d_excl, d_free, d_self, k, a.radius, rm->d_pdist, rm->d_pidx, rm->d_pcount);
    } else {
        hipLaunchKernelGGL(knn_tile_kernel, dim3((unsigned)P, (unsigned)Q), dim3(KT_BLOCK), 0, rm->stream, rm->rb, N, rm->d_nodes, rm->d_kq, d_mask, d_excl, d_free,
                           d_self, k, a.radius, rm->d_pdist, rm->d_pidx, rm->d_pcount);
    }
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)Q), dim3(KT_BLOCK), 0, rm->stream, P, k, rm->d_pdist, rm->d_pidx, rm->d_pcount, rm->d_kidx, rm->d_kdist,
                       rm->d_kcount);
    HIPCHK(hipGetLastError());
    return ARMOUR_OK;
}

int need_device(const char* who, const ArmourRoadmap* rm) {
    if (rm->device >= 0) return ARMOUR_OK;
    armour_set_error("%s: the handle was made by armour_roadmap_create_host and holds nothing on a device", who);
    return ARMOUR_EDEVICE;
}

// armour_roadmap_connect_batch after its argument checks; direct may be null
int connect_batch(ArmourRoadmap* rm, int32_t Q, const int32_t* world, const double* q, const double* target, int32_t k, int32_t* node, double* dist,
                  uint8_t* edge_ok, int32_t* count, uint8_t* direct, double* ms) {
    const int n = rm->rb.n, N = rm->N;
    if (ms) *ms = 0.0;
    // no node to join: nothing but the direct edges is left, and without a target nothing at all
    const int kk = (k > 0 && N > 0) ? k : 0;
    for (int32_t i = 0; i < Q; i++) count[i] = 0;
    for (size_t c = 0; c < (size_t)Q * k; c++) { node[c] = -1; dist[c] = INFINITY; edge_ok[c] = 0; }
    if (kk == 0 && !target) return ARMOUR_OK;
    ARMOUR_TRY(need_device("armour_roadmap_connect_batch", rm));
    HIPCHK(hipSetDevice(rm->device));
    ARMOUR_TRY(rm->ev.record_start(rm->stream));
    if (kk > 0) {
        ARMOUR_TRY(knn_launch(rm, KnnArgs{Q, q, world, nullptr, kk, INFINITY}, true));
    } else {
        ARMOUR_TRY(rm->d_kq.upload(q, (size_t)Q * n, rm->stream));
        ARMOUR_TRY(rm->d_kmask.upload(world, (size_t)Q, rm->stream));
        ARMOUR_TRY(rm->d_kcount.reserve((size_t)Q));
        ARMOUR_TRY(rm->d_kidx.reserve(1));
        HIPCHK(hipMemsetAsync(rm->d_kcount, 0, (size_t)Q * sizeof(int32_t), rm->stream));
    }
    if (target) ARMOUR_TRY(rm->d_ktarget.upload(target, (size_t)Q * n, rm->stream));
    if (rm->self_on) {
        ARMOUR_TRY(rm->d_self_on.upload(rm->self_table.on, sizeof(rm->self_table.on), rm->stream));
        ARMOUR_TRY(rm->d_self_shrink.upload(rm->self_table.shrink, sizeof(rm->self_table.shrink) / sizeof(double), rm->stream));
    }
    const int C = kk + 1;
    ARMOUR_TRY(rm->d_kok.reserve((size_t)Q * C));
    // the one place where the batched joins choose between the static and the window rule: the last check's
    const size_t lds = (size_t)rm->O * (rm->moving ? RM_MOV_STRIDE : RM_OBS_STRIDE) * sizeof(double);
    const double* none = nullptr;
    hipLaunchKernelGGL(rm->moving ? connect_edges_kernel<true> : connect_edges_kernel<false>, dim3((unsigned)Q), dim3(CE_BLOCK), lds, rm->stream, rm->rb,
                       rm->edge_step, kk, rm->d_nodes, rm->d_kq, target ? rm->d_ktarget.p : nullptr, rm->d_kmask, rm->d_obs, rm->moving ? rm->d_vel.p : none,
                       rm->moving ? rm->d_mid.p : none, rm->moving ? rm->d_half.p : none, rm->O, rm->d_kidx, rm->d_kcount,
                       rm->self_on ? rm->d_self_on.p : nullptr, rm->self_on ? rm->d_self_shrink.p : nullptr, rm->self_on ? rm->self_table.rows : 0, rm->d_kok);
    HIPCHK(hipGetLastError());
    ARMOUR_TRY(rm->ev.record_stop(rm->stream));
    std::vector<int32_t> h_idx((size_t)Q * kk);
    std::vector<double> h_dist((size_t)Q * kk);
    std::vector<uint8_t> h_ok((size_t)Q * C);
    if (kk > 0) {
        HIPCHK(hipMemcpyAsync(h_idx.data(), rm->d_kidx, h_idx.size() * sizeof(int32_t), hipMemcpyDeviceToHost, rm->stream));
        HIPCHK(hipMemcpyAsync(h_dist.data(), rm->d_kdist, h_dist.size() * sizeof(double), hipMemcpyDeviceToHost, rm->stream));
        HIPCHK(hipMemcpyAsync(count, rm->d_kcount, (size_t)Q * sizeof(int32_t), hipMemcpyDeviceToHost, rm->stream));
    }
    HIPCHK(hipMemcpyAsync(h_ok.data(), rm->d_kok, h_ok.size(), hipMemcpyDeviceToHost, rm->stream));
    HIPCHK(hipStreamSynchronize(rm->stream));
    if (ms) ARMOUR_TRY(rm->ev.elapsed_ms(ms));
    for (int32_t i = 0; i < Q; i++) {
        for (int c = 0; c < kk; c++) {
            node[(size_t)i * k + c] = h_idx[(size_t)i * kk + c];
            dist[(size_t)i * k + c] = h_dist[(size_t)i * kk + c];
            edge_ok[(size_t)i * k + c] = h_ok[(size_t)i * C + c];
        }
        if (direct) direct[i] = target ? h_ok[(size_t)i * C + kk] : 0;
    }
    return ARMOUR_OK;
}

// the state and argument rules the two batch entries share (armour_roadmap_plan's)
int check_batch(const char* who, const ArmourRoadmap* rm, int32_t Q, const int32_t* world, const double* q, int32_t connect_k) {
    if (connect_k < 0 || connect_k > ARMOUR_ROADMAP_KNN_MAX || Q < 0 || (Q > 0 && (!world || !q))) {
        armour_set_error("%s: Q = %d, connect_k = %d (0..%d), or a null argument", who, Q, connect_k, ARMOUR_ROADMAP_KNN_MAX);
        return ARMOUR_EINVAL;
    }
    if (rm->W < 0) { armour_set_error("%s: no armour_roadmap_check yet", who); return ARMOUR_ESTATE; }
    if (rm->self_on && !rm->self_checked) { armour_set_error("%s: self masks are on and no armour_roadmap_check_self yet", who); return ARMOUR_ESTATE; }
    for (int32_t i = 0; i < Q; i++)
        if (world[i] < 0 || world[i] >= rm->W) { armour_set_error("%s: query %d names world %d of %d", who, i, world[i], rm->W); return ARMOUR_EINVAL; }
    if (!finite_all(q, (size_t)Q * rm->rb.n)) { armour_set_error("%s: a query is not finite", who); return ARMOUR_EINVAL; }
    return ARMOUR_OK;
}

}  // namespace

extern "C" int armour_roadmap_knn_host(ArmourRoadmap* rm, int32_t Q, const double* queries, const int32_t* mask_row, const int32_t* exclude, int32_t k,
                                       double radius, int32_t* index, double* dist, int32_t* count, double* ms) {
    bool masked;
    ARMOUR_TRY(check_knn("armour_roadmap_knn_host", rm, KnnArgs{Q, queries, mask_row, exclude, k, radius}, index, dist, count, &masked));
    if (ms) *ms = 0.0;
    if (Q == 0 || rm->N == 0) return ARMOUR_OK;
    const int n = rm->rb.n, N = rm->N;
    std::vector<std::pair<double, int>> cand;
    rmhost::WorldView view;
    int viewed = -1;
    for (int32_t i = 0; i < Q; i++) {
        const int w = mask_row ? mask_row[i] : -1;
        if (w >= 0 && w != viewed) {
            rmhost::world_view(rm, w, &view);
            viewed = w;
        }
        const int ex = exclude ? exclude[i] : -1;
        cand.clear();
        for (int v = 0; v < N; v++) {
            if (v == ex || (w >= 0 && !view.nf[v])) continue;
            const double d = rmhost::wrapped_distance(rm->rb, queries + (size_t)i * n, &rm->nodes[(size_t)v * n]);
            if (d <= radius) cand.push_back({d, v});
        }
        const size_t found = std::min<size_t>((size_t)k, cand.size());
        std::partial_sort(cand.begin(), cand.begin() + found, cand.end());
        for (size_t c = 0; c < (size_t)k; c++) {
            index[(size_t)i * k + c] = c < found ? cand[c].second : -1;
            dist[(size_t)i * k + c] = c < found ? cand[c].first : INFINITY;
        }
        count[i] = (int32_t)found;
    }
    return ARMOUR_OK;
}

extern "C" int armour_roadmap_knn(ArmourRoadmap* rm, int32_t Q, const double* queries, const int32_t* mask_row, const int32_t* exclude, int32_t k, double radius,
                                  int32_t* index, double* dist, int32_t* count, double* ms) {
    bool masked;
    const KnnArgs a{Q, queries, mask_row, exclude, k, radius};
    ARMOUR_TRY(check_knn("armour_roadmap_knn", rm, a, index, dist, count, &masked));
    if (ms) *ms = 0.0;
    if (Q == 0 || rm->N == 0) return ARMOUR_OK;
    ARMOUR_TRY(need_device("armour_roadmap_knn", rm));
    HIPCHK(hipSetDevice(rm->device));
    ARMOUR_TRY(rm->ev.record_start(rm->stream));
    ARMOUR_TRY(knn_launch(rm, a, masked));
    ARMOUR_TRY(rm->ev.record_stop(rm->stream));
    HIPCHK(hipMemcpyAsync(index, rm->d_kidx, (size_t)Q * k * sizeof(int32_t), hipMemcpyDeviceToHost, rm->stream));
    HIPCHK(hipMemcpyAsync(dist, rm->d_kdist, (size_t)Q * k * sizeof(double), hipMemcpyDeviceToHost, rm->stream));
    HIPCHK(hipMemcpyAsync(count, rm->d_kcount, (size_t)Q * sizeof(int32_t), hipMemcpyDeviceToHost, rm->stream));
    HIPCHK(hipStreamSynchronize(rm->stream));
    if (ms) ARMOUR_TRY(rm->ev.elapsed_ms(ms));
    return ARMOUR_OK;
}

extern "C" int armour_roadmap_connect_batch(ArmourRoadmap* rm, int32_t Q, const int32_t* world, const double* q, const double* target, int32_t connect_k,
                                            int32_t* node, double* dist, uint8_t* edge_ok, int32_t* count, uint8_t* direct, double* ms) {
    const char* who = "armour_roadmap_connect_batch";
    if (!rm) { armour_set_error("%s: null handle", who); return ARMOUR_EINVAL; }
    ARMOUR_TRY(check_batch(who, rm, Q, world, q, connect_k));
    if (Q > 0 && (!count || (connect_k > 0 && (!node || !dist || !edge_ok)) || (target && !direct))) { armour_set_error("%s: null output", who); return ARMOUR_EINVAL; }
    if (target && !finite_all(target, (size_t)Q * rm->rb.n)) { armour_set_error("%s: a target is not finite", who); return ARMOUR_EINVAL; }
    if (ms) *ms = 0.0;
    if (Q == 0) return ARMOUR_OK;
    return connect_batch(rm, Q, world, q, target, connect_k, node, dist, edge_ok, count, direct, ms);
}

extern "C" int armour_roadmap_descend_batch(ArmourRoadmap* rm, int32_t Q, const int32_t* world, const double* q_start, int32_t connect_k, int32_t seq_capacity,
                                            int32_t* seq_off, int32_t* seq, uint8_t* status, double* length) {
    const char* who = "armour_roadmap_descend_batch";
    if (!rm || !seq_off || seq_capacity < 0 || (seq_capacity > 0 && !seq) || (Q > 0 && !status)) { armour_set_error("%s: bad argument", who); return ARMOUR_EINVAL; }
    if (!rm->field_valid) { armour_set_error("%s: no armour_roadmap_field since the last check / self check / armour_roadmap_use_self", who); return ARMOUR_ESTATE; }
    ARMOUR_TRY(check_batch(who, rm, Q, world, q_start, connect_k));
    seq_off[0] = 0;
    if (Q == 0) return ARMOUR_OK;
    const int n = rm->rb.n, N = rm->N, k = connect_k;
    std::vector<double> target((size_t)Q * n), dist((size_t)Q * k);
    for (int32_t i = 0; i < Q; i++) std::memcpy(&target[(size_t)i * n], &rm->field_goals[(size_t)world[i] * n], n * sizeof(double));
    std::vector<int32_t> node((size_t)Q * k), count((size_t)Q);
    std::vector<uint8_t> edge_ok((size_t)Q * k), direct((size_t)Q);
    ARMOUR_TRY(connect_batch(rm, Q, world, q_start, target.data(), k, node.data(), dist.data(), edge_ok.data(), count.data(), direct.data(), nullptr));
    std::vector<int> all, seq_i;
    std::vector<std::pair<double, int>> joined;
    for (int32_t i = 0; i < Q; i++) {
        const int w = world[i];
        double total = INFINITY;
        status[i] = 0;
        if (direct[i]) {
            status[i] = 1;
            total = rmhost::wrapped_distance(rm->rb, q_start + (size_t)i * n, &target[(size_t)i * n]);
        } else {
            joined.clear();
            for (int c = 0; c < count[i]; c++)
                if (edge_ok[(size_t)i * k + c]) joined.push_back({dist[(size_t)i * k + c], node[(size_t)i * k + c]});
            ARMOUR_TRY(rmhost::descend_walk(who, N, w, rm->field_cost.data() + (size_t)w * N, rm->field_next.data() + (size_t)w * N, joined, &seq_i, &total));
            if (!seq_i.empty()) status[i] = 2;
            all.insert(all.end(), seq_i.begin(), seq_i.end());
        }
        if (all.size() > (size_t)INT32_MAX) { armour_set_error("%s: more than 2^31 - 1 path nodes", who); return ARMOUR_ECAPACITY; }
        seq_off[i + 1] = (int32_t)all.size();
        if (length) length[i] = total;
    }
    if (seq_off[Q] > seq_capacity) {
        armour_set_error("%s: %d path nodes, room for %d", who, seq_off[Q], seq_capacity);
        return ARMOUR_ECAPACITY;
    }
    for (size_t c = 0; c < all.size(); c++) seq[c] = all[c];
    return ARMOUR_OK;
}
