// Roadmap high-level planner (include/armour_hip.h, armour_roadmap_*): node and edge verdicts of a joint-space roadmap against W worlds
// in one launch, and the host-side search over one world's free graph.  The rule itself is written once as __host__ __device__ code
// (forward kinematics and the 15-plane separation test of a link box and an obstacle in roadmap_geometry.h, shared with path_audit.hip;
// the enlarged midpoint boxes of an edge below): the kernel runs it per work item, armour_roadmap_plan runs it on the host for the few
// edges that join start and goal to the roadmap.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <queue>
#include <vector>

#include "common.h"
#include "roadmap_handle.h"
#include "self_geometry.h"

using namespace rmgeo;

namespace {

constexpr int RM_BLOCK = 256;                 // four waves; a block serves one world (its obstacles are staged in LDS)

// One launch: grid (ceil((N + M) / RM_BLOCK), W); item i < N is node i, item N + k is edge sub-segment k (edge sample_edge[k],
// sub-segment k - edge_off[e]).  edge_free must hold 1 on entry; a colliding sub-segment stores 0 (no atomics: every writer writes 0).
// MOVING (armour_roadmap_check_moving): the window rule -- velocity [W][O][3], mid / half [W] as the host computed them, the obstacles staged
// with RM_MOV_STRIDE.  The static instantiation reads none of the three and keeps the static rule's calls as they were.
template <bool MOVING>
__global__ __launch_bounds__(RM_BLOCK) void roadmap_check_kernel(RmRobot rb, int32_t N, int64_t M, const double* __restrict__ nodes,
                                                                  const int32_t* __restrict__ edges, const int64_t* __restrict__ edge_off,
                                                                  const int32_t* __restrict__ sample_edge, const double* __restrict__ obstacles,
                                                                  const double* __restrict__ velocity, const double* __restrict__ mid,
                                                                  const double* __restrict__ half, int32_t O, int32_t E,
                                                                  uint8_t* __restrict__ node_free, uint8_t* __restrict__ edge_free,
                                                                  double* __restrict__ clearance) {
    extern __shared__ double s_obs[];   // [O][RM_OBS_STRIDE], MOVING: [O][RM_MOV_STRIDE]
    const int w = blockIdx.y;
    if constexpr (MOVING) stage_obstacles_moving_lds<RM_BLOCK>(obstacles + (size_t)w * O * ARMOUR_OBS_DOUBLES, velocity + (size_t)w * O * 3, O, s_obs);
    else stage_obstacles_lds<RM_BLOCK>(obstacles + (size_t)w * O * ARMOUR_OBS_DOUBLES, O, s_obs);
    const int64_t item = (int64_t)blockIdx.x * RM_BLOCK + threadIdx.x;
    if (item >= (int64_t)N + M) return;
    double q[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS];
    const bool is_node = item < N;
    int e = 0;
    if (is_node) {
#pragma unroll
        for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q[j] = j < rb.n ? nodes[(size_t)item * rb.n + j] : 0.0;
#pragma unroll
        for (int l = 0; l < ARMOUR_MAX_JOINTS; l++) r[l] = 0.0;
    } else {
        const int64_t k = item - N;
        e = sample_edge[k];
        const int64_t s = k - edge_off[e], S = edge_off[e + 1] - edge_off[e];
        const int a = edges[2 * e], b = edges[2 * e + 1];
        edge_sample(rb, nodes + (size_t)a * rb.n, nodes + (size_t)b * rb.n, s, S, q, r);
    }
    const bool full = is_node && clearance != nullptr;   // node clearance: no early exit
    double cl;
    bool ok;
    if constexpr (MOVING) ok = config_free_moving(rb, q, r, s_obs, O, mid[w], half[w], full, &cl);
    else ok = config_free(rb, q, r, s_obs, O, full, &cl);
    if (is_node) {
        node_free[(size_t)w * N + item] = ok ? 1 : 0;
        if (full) clearance[(size_t)w * N + item] = cl;
    } else if (!ok) {
        edge_free[(size_t)w * E + e] = 0;
    }
}

}  // namespace

namespace rmhost {

double wrapped_distance(const RmRobot& rb, const double* a, const double* b) { return wrapped_norm(rb, a, b); }

bool edge_free(const ArmourRoadmap* rm, const WorldView& v, const double* a, const double* b) {
    const int64_t S = edge_segments(rm->rb, a, b, rm->edge_step);
    double q[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS];
    for (int64_t s = 0; s < S; s++) {
        edge_sample(rm->rb, a, b, s, S, q, r);
        const bool ok = v.moving ? config_free_moving(rm->rb, q, r, v.obs, rm->O, v.mid, v.half, false, nullptr)
                                 : config_free(rm->rb, q, r, v.obs, rm->O, false, nullptr);
        if (!ok) return false;
    }
    // with the self masks switched on (armour_roadmap_use_self) the same edge passes the self edge rule as well
    return !rm->self_on || self_edge_free(rm->rb, rm->self_table, rm->edge_step, a, b);
}

void world_view(const ArmourRoadmap* rm, int32_t w, WorldView* v) {
    const int N = rm->N, E = rm->E;
    v->moving = rm->moving;
    v->obs = rm->obs.data() + (size_t)w * rm->O * (rm->moving ? RM_MOV_STRIDE : RM_OBS_STRIDE);
    v->mid = rm->moving ? rm->mid[w] : 0.0;
    v->half = rm->moving ? rm->half[w] : 0.0;
    v->nf = rm->node_free.data() + (size_t)w * N;
    v->ef = rm->edge_free.data() + (size_t)w * E;
    // free in both masks when the self masks are on
    if (rm->self_on) {
        v->both_n.assign(v->nf, v->nf + N);
        v->both_e.assign(v->ef, v->ef + E);
        for (int i = 0; i < N; i++) v->both_n[i] = v->both_n[i] && rm->self_node_free[i];
        for (int e = 0; e < E; e++) v->both_e[e] = v->both_e[e] && rm->self_edge_free[e];
        v->nf = v->both_n.data();
        v->ef = v->both_e.data();
    }
}

void connect(const ArmourRoadmap* rm, const WorldView& v, const double* q, int32_t connect_k, std::vector<std::pair<double, int>>* out) {
    const int n = rm->rb.n, N = rm->N;
    std::vector<std::pair<double, int>> cand;
    for (int i = 0; i < N; i++)
        if (v.nf[i]) cand.push_back({wrapped_distance(rm->rb, q, &rm->nodes[(size_t)i * n]), i});
    const size_t k = std::min<size_t>((size_t)connect_k, cand.size());
    std::partial_sort(cand.begin(), cand.begin() + k, cand.end());
    out->clear();
    for (size_t c = 0; c < k; c++)
        if (edge_free(rm, v, q, &rm->nodes[(size_t)cand[c].second * n])) out->push_back(cand[c]);
}

}  // namespace rmhost

using rmhost::wrapped_distance;

// armour_roadmap_create and armour_roadmap_create_host (on_device = false: the host half alone, device -1)
static int create_roadmap(const ArmourRobot* robot, int32_t N, const double* nodes, int32_t E, const int32_t* edges, const uint8_t* continuous, double edge_step,
                          bool on_device, int32_t device, ArmourRoadmap** out) {
    if (!robot || !out || (N > 0 && !nodes) || (E > 0 && !edges)) { armour_set_error("armour_roadmap_create: null argument"); return ARMOUR_EINVAL; }
    *out = nullptr;
    ARMOUR_TRY(armour_check_robot_shape("armour_roadmap_create", robot));
    if (N < 0 || E < 0 || !(edge_step > 0.0) || !std::isfinite(edge_step)) {
        armour_set_error("armour_roadmap_create: N = %d, E = %d, edge_step = %g", N, E, edge_step);
        return ARMOUR_EINVAL;
    }
    const int n = robot->num_factors;
    if (const size_t i = first_nonfinite(nodes, (size_t)N * n); i < (size_t)N * n) { armour_set_error("armour_roadmap_create: node %lld is not finite", (long long)(i / n)); return ARMOUR_EINVAL; }
    for (int64_t i = 0; i < 2 * (int64_t)E; i++)
        if (edges[i] < 0 || edges[i] >= N) { armour_set_error("armour_roadmap_create: edge %lld names node %d of %d", (long long)(i / 2), edges[i], N); return ARMOUR_EINVAL; }
    ArmourRoadmap* rm = new (std::nothrow) ArmourRoadmap();
    if (!rm) { armour_set_error("armour_roadmap_create: out of host memory"); return ARMOUR_EDEVICE; }
    std::unique_ptr<ArmourRoadmap> guard(rm);
    fill_rm_robot(robot, continuous, &rm->rb);
    rm->device = device;
    rm->N = N;
    rm->E = E;
    rm->edge_step = edge_step;
    rm->nodes.assign(nodes, nodes + (size_t)N * n);
    rm->edges.assign(edges, edges + (size_t)2 * E);
    std::vector<int64_t> off((size_t)E + 1, 0);
    for (int e = 0; e < E; e++) {
        off[e + 1] = off[e] + edge_segments(rm->rb, &rm->nodes[(size_t)edges[2 * e] * n], &rm->nodes[(size_t)edges[2 * e + 1] * n], edge_step);
        if (off[e + 1] + N > INT32_MAX) {
            armour_set_error("armour_roadmap_create: more than 2^31 - 1 nodes + edge sub-segments (edge_step %g too small)", edge_step);
            return ARMOUR_ECAPACITY;
        }
    }
    rm->M = off[E];
    std::vector<int32_t> sample_edge((size_t)rm->M);
    for (int e = 0; e < E; e++)
        for (int64_t k = off[e]; k < off[e + 1]; k++) sample_edge[(size_t)k] = e;
    if (!on_device) {
        *out = guard.release();
        return ARMOUR_OK;
    }
    HIPCHK(hipSetDevice(device));
    ARMOUR_TRY(rm->stream.create());
    ARMOUR_TRY(rm->d_nodes.upload(rm->nodes.data(), rm->nodes.size(), rm->stream));
    ARMOUR_TRY(rm->d_edges.upload(rm->edges.data(), rm->edges.size(), rm->stream));
    ARMOUR_TRY(rm->d_edge_off.upload(off.data(), off.size(), rm->stream));
    ARMOUR_TRY(rm->d_sample_edge.upload(sample_edge.data(), sample_edge.size(), rm->stream));
    HIPCHK(hipStreamSynchronize(rm->stream));   // (`off` and `sample_edge` are read by the copies)
    *out = guard.release();
    return ARMOUR_OK;
}

extern "C" int armour_roadmap_create(const ArmourRobot* robot, int32_t N, const double* nodes, int32_t E, const int32_t* edges,
                                     const uint8_t* continuous, double edge_step, int32_t device, ArmourRoadmap** out) {
    return create_roadmap(robot, N, nodes, E, edges, continuous, edge_step, true, device, out);
}

extern "C" int armour_roadmap_create_host(const ArmourRobot* robot, int32_t N, const double* nodes, int32_t E, const int32_t* edges,
                                          const uint8_t* continuous, double edge_step, ArmourRoadmap** out) {
    return create_roadmap(robot, N, nodes, E, edges, continuous, edge_step, false, -1, out);
}

extern "C" void armour_roadmap_destroy(ArmourRoadmap* rm) {
    if (!rm) return;
    if (rm->device >= 0) (void)hipSetDevice(rm->device);
    delete rm;
}

extern "C" int armour_roadmap_get_sizes(const ArmourRoadmap* rm, int32_t* N, int32_t* E, int64_t* edge_samples) {
    if (!rm) { armour_set_error("armour_roadmap_get_sizes: null handle"); return ARMOUR_EINVAL; }
    if (N) *N = rm->N;
    if (E) *E = rm->E;
    if (edge_samples) *edge_samples = rm->M;
    return ARMOUR_OK;
}

// the motion of a moving check as the caller passed it (null: a static check)
struct Motion {
    const double *velocity, *t_from, *t_to;
};

// the argument rules of the three check entries, before a device is touched
static int check_check_args(const char* who, const ArmourRoadmap* rm, int32_t W, int32_t O, const double* obstacles, const Motion* mv) {
    if (!rm) { armour_set_error("%s: null handle", who); return ARMOUR_EINVAL; }
    ARMOUR_TRY(armour_check_world_counts(who, W, O, obstacles));
    const size_t nobs = (size_t)W * O * ARMOUR_OBS_DOUBLES;
    if (const size_t i = first_nonfinite(obstacles, nobs); i < nobs) { armour_set_error("%s: obstacle %zu is not finite", who, i / ARMOUR_OBS_DOUBLES); return ARMOUR_EINVAL; }
    if (!mv) return ARMOUR_OK;
    if ((W > 0 && O > 0 && !mv->velocity) || (W > 0 && (!mv->t_from || !mv->t_to))) { armour_set_error("%s: null velocity or window", who); return ARMOUR_EINVAL; }
    if (!finite_all(mv->velocity, (size_t)W * O * 3) || !finite_all(mv->t_from, (size_t)W) || !finite_all(mv->t_to, (size_t)W)) {
        armour_set_error("%s: a velocity or a window is not finite", who);
        return ARMOUR_EINVAL;
    }
    for (int32_t w = 0; w < W; w++)
        if (mv->t_from[w] > mv->t_to[w]) { armour_set_error("%s: world %d: t_from = %g > t_to = %g", who, w, mv->t_from[w], mv->t_to[w]); return ARMOUR_EINVAL; }
    return ARMOUR_OK;
}

// What a check leaves on the host for the searches: the obstacles as the kernel staged them and, after a moving check, every world's window
// as the two numbers the rule reads.  Called before the launch, so that the kernel is given these mid and half.
static void keep_worlds(ArmourRoadmap* rm, int32_t W, int32_t O, const double* obstacles, const Motion* mv) {
    rm->moving = mv != nullptr;
    rm->obs.resize((size_t)W * O * (mv ? RM_MOV_STRIDE : RM_OBS_STRIDE));
    if (mv) stage_obstacles_moving(obstacles, mv->velocity, (size_t)W * O, rm->obs.data());
    else stage_obstacles(obstacles, (size_t)W * O, rm->obs.data());
    rm->mid.resize(mv ? (size_t)W : 0);
    rm->half.resize(mv ? (size_t)W : 0);
    for (int32_t w = 0; mv && w < W; w++) {
        rm->mid[w] = 0.5 * (mv->t_from[w] + mv->t_to[w]);
        rm->half[w] = 0.5 * (mv->t_to[w] - mv->t_from[w]);
    }
}

// the device entry of both checks (mv null: the static one)
static int check_on_device(const char* who, ArmourRoadmap* rm, int32_t W, int32_t O, const double* obstacles, const Motion* mv, uint8_t* node_free,
                           uint8_t* edge_free, double* node_clearance, double* ms) {
    ARMOUR_TRY(check_check_args(who, rm, W, O, obstacles, mv));
    if (rm->device < 0) { armour_set_error("%s: the handle was made by armour_roadmap_create_host and holds nothing on a device", who); return ARMOUR_EDEVICE; }
    const size_t nobs = (size_t)W * O * ARMOUR_OBS_DOUBLES;
    HIPCHK(hipSetDevice(rm->device));
    rm->field_valid = false;   // the fields of armour_roadmap_field belong to the check they were computed from
    rm->W = -1;                // from here on d_edge_free is rewritten: a check that fails below leaves no worlds, not the last check's host masks
    keep_worlds(rm, W, O, obstacles, mv);
    const size_t WN = (size_t)W * rm->N, WE = (size_t)W * rm->E;
    ARMOUR_TRY(rm->d_node_free.reserve(WN));
    ARMOUR_TRY(rm->d_edge_free.reserve(WE));
    if (node_clearance) ARMOUR_TRY(rm->d_clear.reserve(WN));
    ARMOUR_TRY(rm->d_obs.upload(obstacles, nobs, rm->stream));
    if (mv) {
        ARMOUR_TRY(rm->d_vel.upload(mv->velocity, (size_t)W * O * 3, rm->stream));
        ARMOUR_TRY(rm->d_mid.upload(rm->mid.data(), (size_t)W, rm->stream));
        ARMOUR_TRY(rm->d_half.upload(rm->half.data(), (size_t)W, rm->stream));
    }
    if (WE) HIPCHK(hipMemsetAsync(rm->d_edge_free, 1, WE, rm->stream));
    const int64_t items = (int64_t)rm->N + rm->M;
    ARMOUR_TRY(rm->ev.record_start(rm->stream));
    if (W > 0 && items > 0) {
        const dim3 grid((unsigned)((items + RM_BLOCK - 1) / RM_BLOCK), (unsigned)W);
        if (mv) {
            const size_t lds = (size_t)O * RM_MOV_STRIDE * sizeof(double);
            hipLaunchKernelGGL(roadmap_check_kernel<true>, grid, dim3(RM_BLOCK), lds, rm->stream, rm->rb, rm->N, rm->M, rm->d_nodes, rm->d_edges,
                               rm->d_edge_off, rm->d_sample_edge, rm->d_obs, rm->d_vel, rm->d_mid, rm->d_half, O, rm->E, rm->d_node_free, rm->d_edge_free,
                               node_clearance ? rm->d_clear : nullptr);
        } else {
            const size_t lds = (size_t)O * RM_OBS_STRIDE * sizeof(double);
            hipLaunchKernelGGL(roadmap_check_kernel<false>, grid, dim3(RM_BLOCK), lds, rm->stream, rm->rb, rm->N, rm->M, rm->d_nodes, rm->d_edges,
                               rm->d_edge_off, rm->d_sample_edge, rm->d_obs, nullptr, nullptr, nullptr, O, rm->E, rm->d_node_free, rm->d_edge_free,
                               node_clearance ? rm->d_clear : nullptr);
        }
        HIPCHK(hipGetLastError());
    }
    ARMOUR_TRY(rm->ev.record_stop(rm->stream));
    rm->node_free.resize(WN);
    rm->edge_free.resize(WE);
    if (WN) HIPCHK(hipMemcpyAsync(rm->node_free.data(), rm->d_node_free, WN, hipMemcpyDeviceToHost, rm->stream));
    if (WE) HIPCHK(hipMemcpyAsync(rm->edge_free.data(), rm->d_edge_free, WE, hipMemcpyDeviceToHost, rm->stream));
    if (node_clearance && WN) HIPCHK(hipMemcpyAsync(node_clearance, rm->d_clear, WN * sizeof(double), hipMemcpyDeviceToHost, rm->stream));
    HIPCHK(hipStreamSynchronize(rm->stream));
    if (ms) ARMOUR_TRY(rm->ev.elapsed_ms(ms));
    if (node_free && WN) std::memcpy(node_free, rm->node_free.data(), WN);
    if (edge_free && WE) std::memcpy(edge_free, rm->edge_free.data(), WE);
    rm->W = W;
    rm->O = O;
    return ARMOUR_OK;
}

extern "C" int armour_roadmap_check(ArmourRoadmap* rm, int32_t W, int32_t O, const double* obstacles, uint8_t* node_free, uint8_t* edge_free,
                                    double* node_clearance, double* ms) {
    return check_on_device("armour_roadmap_check", rm, W, O, obstacles, nullptr, node_free, edge_free, node_clearance, ms);
}

extern "C" int armour_roadmap_check_moving(ArmourRoadmap* rm, int32_t W, int32_t O, const double* obstacles, const double* velocity, const double* t_from,
                                           const double* t_to, uint8_t* node_free, uint8_t* edge_free, double* node_clearance, double* ms) {
    const Motion mv{velocity, t_from, t_to};
    return check_on_device("armour_roadmap_check_moving", rm, W, O, obstacles, &mv, node_free, edge_free, node_clearance, ms);
}

// the window rule by the kernel's functions in a host loop, on a handle of armour_roadmap_create_host; it leaves the host state of a device check
extern "C" int armour_roadmap_check_moving_host(ArmourRoadmap* rm, int32_t W, int32_t O, const double* obstacles, const double* velocity,
                                                const double* t_from, const double* t_to, uint8_t* node_free, uint8_t* edge_free,
                                                double* node_clearance) {
    const char* who = "armour_roadmap_check_moving_host";
    const Motion mv{velocity, t_from, t_to};
    ARMOUR_TRY(check_check_args(who, rm, W, O, obstacles, &mv));
    if (rm->device >= 0) { armour_set_error("%s: the handle holds a device; make one with armour_roadmap_create_host", who); return ARMOUR_EINVAL; }
    rm->field_valid = false;
    rm->W = -1;
    keep_worlds(rm, W, O, obstacles, &mv);
    const int n = rm->rb.n, N = rm->N, E = rm->E;
    rm->node_free.assign((size_t)W * N, 0);
    rm->edge_free.assign((size_t)W * E, 1);
    double q[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS];
    for (int32_t w = 0; w < W; w++) {
        const double* obs = rm->obs.data() + (size_t)w * O * RM_MOV_STRIDE;
        for (int i = 0; i < N; i++) {
            for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q[j] = j < n ? rm->nodes[(size_t)i * n + j] : 0.0;
            for (int l = 0; l < ARMOUR_MAX_JOINTS; l++) r[l] = 0.0;
            double cl;
            const bool full = node_clearance != nullptr;
            rm->node_free[(size_t)w * N + i] = config_free_moving(rm->rb, q, r, obs, O, rm->mid[w], rm->half[w], full, &cl) ? 1 : 0;
            if (full) node_clearance[(size_t)w * N + i] = cl;
        }
        for (int e = 0; e < E; e++) {
            const double *a = &rm->nodes[(size_t)rm->edges[2 * e] * n], *b = &rm->nodes[(size_t)rm->edges[2 * e + 1] * n];
            const int64_t S = edge_segments(rm->rb, a, b, rm->edge_step);
            for (int64_t s = 0; s < S; s++) {
                edge_sample(rm->rb, a, b, s, S, q, r);
                if (!config_free_moving(rm->rb, q, r, obs, O, rm->mid[w], rm->half[w], false, nullptr)) {
                    rm->edge_free[(size_t)w * E + e] = 0;
                    break;
                }
            }
        }
    }
    if (node_free && W && N) std::memcpy(node_free, rm->node_free.data(), (size_t)W * N);
    if (edge_free && W && E) std::memcpy(edge_free, rm->edge_free.data(), (size_t)W * E);
    rm->W = W;
    rm->O = O;
    return ARMOUR_OK;
}

extern "C" int armour_roadmap_plan(ArmourRoadmap* rm, int32_t w, const double* q_start, const double* q_goal, int32_t connect_k,
                                   int32_t max_points, double* path, int32_t* points) {
    if (!rm || !q_start || !q_goal || !points || max_points < 0 || (max_points > 0 && !path) || connect_k < 0) {
        armour_set_error("armour_roadmap_plan: bad argument");
        return ARMOUR_EINVAL;
    }
    *points = 0;
    if (rm->W < 0) { armour_set_error("armour_roadmap_plan: no armour_roadmap_check yet"); return ARMOUR_ESTATE; }
    if (rm->self_on && !rm->self_checked) { armour_set_error("armour_roadmap_plan: self masks are on and no armour_roadmap_check_self yet"); return ARMOUR_ESTATE; }
    if (w < 0 || w >= rm->W) { armour_set_error("armour_roadmap_plan: world %d of %d", w, rm->W); return ARMOUR_EINVAL; }
    const int n = rm->rb.n, N = rm->N;
    for (int j = 0; j < n; j++)
        if (!std::isfinite(q_start[j]) || !std::isfinite(q_goal[j])) { armour_set_error("armour_roadmap_plan: start / goal not finite"); return ARMOUR_EINVAL; }
    rmhost::WorldView view;
    rmhost::world_view(rm, w, &view);
    const uint8_t* ef = view.ef;
    auto node = [&](int i) -> const double* { return i == N ? q_start : i == N + 1 ? q_goal : &rm->nodes[(size_t)i * n]; };
    auto emit = [&](const std::vector<int>& seq) -> int {
        *points = (int32_t)seq.size();
        if ((int)seq.size() > max_points) {
            armour_set_error("armour_roadmap_plan: path of %d points, room for %d", (int)seq.size(), max_points);
            return ARMOUR_ECAPACITY;
        }
        for (size_t i = 0; i < seq.size(); i++) std::memcpy(path + i * n, node(seq[i]), n * sizeof(double));
        return ARMOUR_OK;
    };
    if (rmhost::edge_free(rm, view, q_start, q_goal)) return emit({N, N + 1});
    // graph: roadmap nodes 0..N-1, start N, goal N+1
    std::vector<std::vector<std::pair<int, double>>> adj((size_t)N + 2);
    for (int e = 0; e < rm->E; e++) {
        if (!ef[e]) continue;
        const int a = rm->edges[2 * e], b = rm->edges[2 * e + 1];
        const double len = wrapped_distance(rm->rb, node(a), node(b));
        adj[a].push_back({b, len});
        adj[b].push_back({a, len});
    }
    std::vector<std::pair<double, int>> joined;
    for (int end = N; end <= N + 1; end++) {
        rmhost::connect(rm, view, node(end), connect_k, &joined);
        for (const auto& c : joined) {
            adj[end].push_back({c.second, c.first});
            adj[c.second].push_back({end, c.first});
        }
    }
    // A* from start to goal; the heuristic (wrapped distance to the goal) is a metric lower bound of every path's length
    const int s = N, g = N + 1;
    std::vector<double> dist((size_t)N + 2, INFINITY);
    std::vector<int> prev((size_t)N + 2, -1);
    std::vector<char> done((size_t)N + 2, 0);
    using Ent = std::pair<double, int>;
    std::priority_queue<Ent, std::vector<Ent>, std::greater<Ent>> open;
    dist[s] = 0.0;
    open.push({wrapped_distance(rm->rb, node(s), node(g)), s});
    while (!open.empty()) {
        const int v = open.top().second;
        open.pop();
        if (done[v]) continue;
        done[v] = 1;
        if (v == g) break;
        for (const auto& nb : adj[v]) {
            const double d = dist[v] + nb.second;
            if (d < dist[nb.first]) {
                dist[nb.first] = d;
                prev[nb.first] = v;
                open.push({d + wrapped_distance(rm->rb, node(nb.first), node(g)), nb.first});
            }
        }
    }
    if (!done[g]) return ARMOUR_OK;   // *points = 0: no path
    std::vector<int> seq;
    for (int v = g; v != -1; v = prev[v]) seq.push_back(v);
    std::reverse(seq.begin(), seq.end());
    return emit(seq);
}
