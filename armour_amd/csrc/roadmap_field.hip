// Cost-to-go fields of a checked roadmap (include/armour_hip.h, armour_roadmap_field / armour_roadmap_descend): for every world of the last
// armour_roadmap_check, the shortest free-graph distance from every node to that world's goal and a successor pointer, in ONE launch; then
// a waypoint query on the host is a nearest-node scan, a few edge checks and a pointer walk, with no search.
//
// The field is the greatest solution of cost[v] = min(seed[v], min over free edges (u, v) of fl(cost[u] + len[e])).  x -> fl(x + len) is
// monotone and never decreases x, so that solution is unique and ANY relaxation order reaches the same doubles: the
// kernel sweeps in place without atomics, a block per world, and a reader that sees a neighbour's cost from before or after a store of the
// same sweep sees a valid state of the iteration either way.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "roadmap_handle.h"

using namespace rmgeo;

namespace {

constexpr int RF_BLOCK = 1024;                // sixteen waves: one block is one world, and one world runs on one CU

// grid W, one block per world.  Thread t owns the nodes v = t (mod RF_BLOCK): only it writes cost[w][v].  Row v of the CSR lists the
// edges at v as (neighbour col, edge id eid), neighbours ascending.  cost is set up here (+inf, then the world's seeds
// seed_node / seed_val [seed_off[w] .. seed_off[w + 1])), so it never rises above a seed.  self_free [E] may be null.
__global__ __launch_bounds__(RF_BLOCK) void roadmap_field_kernel(int32_t N, int32_t E, const int32_t* __restrict__ row_off, const int32_t* __restrict__ col,
                                                                  const int32_t* __restrict__ eid, const double* __restrict__ len,
                                                                  const uint8_t* __restrict__ edge_free, const uint8_t* __restrict__ self_free,
                                                                  const int32_t* __restrict__ seed_off, const int32_t* __restrict__ seed_node,
                                                                  const double* __restrict__ seed_val, double* cost, int32_t* next,
                                                                  int32_t* __restrict__ reached, int32_t* __restrict__ sweeps, int32_t* __restrict__ status) {
    __shared__ int s_count[RF_BLOCK / 64];
    const int w = blockIdx.x, t = threadIdx.x;
    const uint8_t* ef = edge_free + (size_t)w * E;
    double* c = cost + (size_t)w * N;
    int32_t* nx = next + (size_t)w * N;
    const int s0 = seed_off[w], s1 = seed_off[w + 1];
    for (int v = t; v < N; v += RF_BLOCK) c[v] = INFINITY;
    __syncthreads();
    for (int s = s0 + t; s < s1; s += RF_BLOCK) c[seed_node[s]] = seed_val[s];
    __syncthreads();
    // in-place sweeps until one changes nothing; N + 1 is more than in-place Bellman-Ford can need, so reaching it is a bug, not a hang
    int n_sweeps = 0;
    bool capped = false;
    for (;;) {
        int changed = 0;
        for (int v = t; v < N; v += RF_BLOCK) {
            const double old = c[v];
            double best = old;
            for (int k = row_off[v], k1 = row_off[v + 1]; k < k1; k++) {
                const int e = eid[k];
                if (!ef[e] || (self_free && !self_free[e])) continue;
                const double d = c[col[k]] + len[e];
                best = d < best ? d : best;
            }
            if (best < old) {
                c[v] = best;
                changed = 1;
            }
        }
        n_sweeps++;
        if (!__syncthreads_or(changed)) break;
        if (n_sweeps > N) { capped = true; break; }
    }
    // successors: -1 unreachable; else the smallest neighbour of a lower cost that attains the cost (lower: an edge of length 0, or one
    // below half an ulp of the cost, joins equal costs, and the walk must never turn back); a seed that attains it overrides below
    int count = 0;
    for (int v = t; v < N; v += RF_BLOCK) {
        const double cv = c[v];
        int succ = -1;
        if (cv < INFINITY) {
            count++;
            for (int k = row_off[v], k1 = row_off[v + 1]; k < k1; k++) {
                const int e = eid[k];
                if (!ef[e] || (self_free && !self_free[e])) continue;
                const double cu = c[col[k]];
                if (cu < cv && cu + len[e] == cv) { succ = col[k]; break; }
            }
        }
        nx[v] = succ;
    }
    __syncthreads();
    for (int s = s0 + t; s < s1; s += RF_BLOCK)
        if (seed_val[s] == c[seed_node[s]]) nx[seed_node[s]] = ARMOUR_ROADMAP_NEXT_GOAL;
    for (int o = 32; o > 0; o >>= 1) count += __shfl_down(count, o);
    if ((t & 63) == 0) s_count[t >> 6] = count;
    __syncthreads();
    if (t == 0) {
        int total = 0;
        for (int i = 0; i < RF_BLOCK / 64; i++) total += s_count[i];
        reached[w] = total;
        sweeps[w] = n_sweeps;
        if (capped) *status = 1;   // (no atomics: every writer writes 1)
    }
}

// the edge lengths and the CSR rows of the roadmap, once per handle
int build_csr(ArmourRoadmap* rm) {
    if (rm->csr_ready) return ARMOUR_OK;
    const int n = rm->rb.n, N = rm->N, E = rm->E;
    if (2 * (int64_t)E > INT32_MAX) { armour_set_error("armour_roadmap_field: %d edges, room for 2^30 - 1", E); return ARMOUR_ECAPACITY; }
    std::vector<double> len((size_t)E);
    std::vector<int32_t> row_off((size_t)N + 1, 0), col((size_t)2 * E), id((size_t)2 * E);
    for (int e = 0; e < E; e++) {
        const int a = rm->edges[2 * e], b = rm->edges[2 * e + 1];
        len[e] = rmhost::wrapped_distance(rm->rb, &rm->nodes[(size_t)a * n], &rm->nodes[(size_t)b * n]);
        row_off[a + 1]++;
        row_off[b + 1]++;
    }
    for (int v = 0; v < N; v++) row_off[v + 1] += row_off[v];
    std::vector<std::pair<int32_t, int32_t>> ent((size_t)2 * E);   // (neighbour, edge id), row by row
    std::vector<int32_t> fill(row_off.begin(), row_off.end() - 1);
    for (int e = 0; e < E; e++) {
        const int a = rm->edges[2 * e], b = rm->edges[2 * e + 1];
        ent[fill[a]++] = {b, e};
        ent[fill[b]++] = {a, e};
    }
    for (int v = 0; v < N; v++) std::sort(ent.begin() + row_off[v], ent.begin() + row_off[v + 1]);
    for (size_t k = 0; k < ent.size(); k++) {
        col[k] = ent[k].first;
        id[k] = ent[k].second;
    }
    ARMOUR_TRY(rm->d_edge_len.upload(len.data(), len.size(), rm->stream));
    ARMOUR_TRY(rm->d_row_off.upload(row_off.data(), row_off.size(), rm->stream));
    ARMOUR_TRY(rm->d_col.upload(col.data(), col.size(), rm->stream));
    ARMOUR_TRY(rm->d_eid.upload(id.data(), id.size(), rm->stream));
    HIPCHK(hipStreamSynchronize(rm->stream));   // (the vectors are read by the copies)
    rm->csr_ready = true;
    return ARMOUR_OK;
}

}  // namespace

extern "C" int armour_roadmap_field(ArmourRoadmap* rm, const double* goals, int32_t connect_k, double* cost, int32_t* next, int32_t* reached,
                                    int32_t* sweeps, double* ms) {
    if (!rm || connect_k < 0) { armour_set_error("armour_roadmap_field: bad argument"); return ARMOUR_EINVAL; }
    if (rm->W < 0) { armour_set_error("armour_roadmap_field: no armour_roadmap_check yet"); return ARMOUR_ESTATE; }
    if (rm->self_on && !rm->self_checked) { armour_set_error("armour_roadmap_field: self masks are on and no armour_roadmap_check_self yet"); return ARMOUR_ESTATE; }
    const int n = rm->rb.n, N = rm->N, E = rm->E, W = rm->W;
    if (W > 0 && !goals) { armour_set_error("armour_roadmap_field: null goals"); return ARMOUR_EINVAL; }
    if (const size_t i = first_nonfinite(goals, (size_t)W * n); i < (size_t)W * n) { armour_set_error("armour_roadmap_field: goal %zu is not finite", i / n); return ARMOUR_EINVAL; }
    rm->field_valid = false;
    if (ms) *ms = 0.0;
    // ---- seeds: every goal joined to the roadmap as armour_roadmap_plan joins it
    std::vector<int32_t> seed_off((size_t)W + 1, 0), seed_node;
    std::vector<double> seed_val;
    std::vector<std::pair<double, int>> joined;
    for (int w = 0; w < W; w++) {
        rmhost::WorldView view;
        rmhost::world_view(rm, w, &view);
        rmhost::connect(rm, view, goals + (size_t)w * n, connect_k, &joined);
        for (const auto& c : joined) {
            seed_val.push_back(c.first);
            seed_node.push_back(c.second);
        }
        seed_off[w + 1] = (int32_t)seed_node.size();
    }
    // ---- the device
    const size_t WN = (size_t)W * N;
    HIPCHK(hipSetDevice(rm->device));
    ARMOUR_TRY(build_csr(rm));
    ARMOUR_TRY(rm->d_seed_off.upload(seed_off.data(), seed_off.size(), rm->stream));
    ARMOUR_TRY(rm->d_seed_node.upload(seed_node.data(), seed_node.size(), rm->stream));
    ARMOUR_TRY(rm->d_seed_val.upload(seed_val.data(), seed_val.size(), rm->stream));
    if (rm->self_on) ARMOUR_TRY(rm->d_self_edge_free.upload(rm->self_edge_free.data(), (size_t)E, rm->stream));
    ARMOUR_TRY(rm->d_cost.reserve(WN));
    ARMOUR_TRY(rm->d_next.reserve(WN));
    ARMOUR_TRY(rm->d_reached.reserve((size_t)W));
    ARMOUR_TRY(rm->d_sweeps.reserve((size_t)W));
    ARMOUR_TRY(rm->d_field_status.reserve(1));
    HIPCHK(hipMemsetAsync(rm->d_field_status, 0, sizeof(int32_t), rm->stream));
    ARMOUR_TRY(rm->ev.record_start(rm->stream));
    if (W > 0) {
        hipLaunchKernelGGL(roadmap_field_kernel, dim3((unsigned)W), dim3(RF_BLOCK), 0, rm->stream, N, E, rm->d_row_off, rm->d_col, rm->d_eid, rm->d_edge_len,
                           rm->d_edge_free, rm->self_on ? rm->d_self_edge_free.p : nullptr, rm->d_seed_off, rm->d_seed_node, rm->d_seed_val, rm->d_cost,
                           rm->d_next, rm->d_reached, rm->d_sweeps, rm->d_field_status);
        HIPCHK(hipGetLastError());
    }
    ARMOUR_TRY(rm->ev.record_stop(rm->stream));
    rm->field_cost.resize(WN);
    rm->field_next.resize(WN);
    std::vector<int32_t> h_reached((size_t)W), h_sweeps((size_t)W);
    int32_t status = 0;
    if (WN) HIPCHK(hipMemcpyAsync(rm->field_cost.data(), rm->d_cost, WN * sizeof(double), hipMemcpyDeviceToHost, rm->stream));
    if (WN) HIPCHK(hipMemcpyAsync(rm->field_next.data(), rm->d_next, WN * sizeof(int32_t), hipMemcpyDeviceToHost, rm->stream));
    if (W) HIPCHK(hipMemcpyAsync(h_reached.data(), rm->d_reached, (size_t)W * sizeof(int32_t), hipMemcpyDeviceToHost, rm->stream));
    if (W) HIPCHK(hipMemcpyAsync(h_sweeps.data(), rm->d_sweeps, (size_t)W * sizeof(int32_t), hipMemcpyDeviceToHost, rm->stream));
    HIPCHK(hipMemcpyAsync(&status, rm->d_field_status, sizeof(int32_t), hipMemcpyDeviceToHost, rm->stream));
    HIPCHK(hipStreamSynchronize(rm->stream));
    if (ms) ARMOUR_TRY(rm->ev.elapsed_ms(ms));
    if (status != 0) { armour_set_error("armour_roadmap_field: a world's sweeps did not settle within N + 1 = %d", N + 1); return ARMOUR_ESTATE; }
    if (cost && WN) std::memcpy(cost, rm->field_cost.data(), WN * sizeof(double));
    if (next && WN) std::memcpy(next, rm->field_next.data(), WN * sizeof(int32_t));
    if (reached && W) std::memcpy(reached, h_reached.data(), (size_t)W * sizeof(int32_t));
    if (sweeps && W) std::memcpy(sweeps, h_sweeps.data(), (size_t)W * sizeof(int32_t));
    rm->field_goals.assign(goals, goals + (size_t)W * n);
    rm->field_valid = true;
    return ARMOUR_OK;
}

int rmhost::descend_walk(const char* who, int32_t N, int32_t w, const double* cost, const int32_t* next, const std::vector<std::pair<double, int>>& joined,
                         std::vector<int>* seq, double* total) {
    seq->clear();
    *total = INFINITY;
    int first = -1;
    for (const auto& c : joined) {
        const double sum = c.first + cost[c.second];
        if (sum < *total) { *total = sum; first = c.second; }
    }
    if (first < 0) return ARMOUR_OK;
    seq->push_back(first);
    for (int v = first; next[v] != ARMOUR_ROADMAP_NEXT_GOAL;) {
        v = next[v];
        if (v < 0 || v >= N || (int64_t)seq->size() > (int64_t)N + 1) { armour_set_error("%s: the successors of world %d do not lead to the goal", who, w); return ARMOUR_ESTATE; }
        seq->push_back(v);
    }
    return ARMOUR_OK;
}

extern "C" int armour_roadmap_descend(ArmourRoadmap* rm, int32_t w, const double* q_start, int32_t connect_k, int32_t max_points, double* path,
                                      int32_t* points, double* length) {
    if (!rm || !q_start || !points || max_points < 0 || (max_points > 0 && !path) || connect_k < 0) {
        armour_set_error("armour_roadmap_descend: bad argument");
        return ARMOUR_EINVAL;
    }
    *points = 0;
    if (length) *length = INFINITY;
    if (!rm->field_valid) { armour_set_error("armour_roadmap_descend: no armour_roadmap_field since the last check / self check / armour_roadmap_use_self"); return ARMOUR_ESTATE; }
    if (w < 0 || w >= rm->W) { armour_set_error("armour_roadmap_descend: world %d of %d", w, rm->W); return ARMOUR_EINVAL; }
    const int n = rm->rb.n, N = rm->N;
    if (!finite_all(q_start, (size_t)n)) { armour_set_error("armour_roadmap_descend: start not finite"); return ARMOUR_EINVAL; }
    const double* goal = &rm->field_goals[(size_t)w * n];
    const double* cost = rm->field_cost.data() + (size_t)w * N;
    const int32_t* next = rm->field_next.data() + (size_t)w * N;
    rmhost::WorldView view;
    rmhost::world_view(rm, w, &view);
    std::vector<int> seq;   // the roadmap nodes between start and goal
    double total;
    if (rmhost::edge_free(rm, view, q_start, goal)) {
        total = rmhost::wrapped_distance(rm->rb, q_start, goal);
    } else {
        std::vector<std::pair<double, int>> joined;
        rmhost::connect(rm, view, q_start, connect_k, &joined);
        ARMOUR_TRY(rmhost::descend_walk("armour_roadmap_descend", N, w, cost, next, joined, &seq, &total));
        if (seq.empty()) return ARMOUR_OK;   // *points = 0: no path
    }
    *points = (int32_t)seq.size() + 2;
    if (length) *length = total;
    if (*points > max_points) {
        armour_set_error("armour_roadmap_descend: path of %d points, room for %d", *points, max_points);
        return ARMOUR_ECAPACITY;
    }
    std::memcpy(path, q_start, n * sizeof(double));
    for (size_t i = 0; i < seq.size(); i++) std::memcpy(path + (i + 1) * n, &rm->nodes[(size_t)seq[i] * n], n * sizeof(double));
    std::memcpy(path + (seq.size() + 1) * n, goal, n * sizeof(double));
    return ARMOUR_OK;
}
