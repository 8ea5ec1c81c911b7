// The roadmap handle and the edge rule's sub-segments (include/armour_hip.h, armour_roadmap_*), shared by roadmap.hip (the world check and
// the search), self_check.hip (the self-collision masks of the same roadmap) and roadmap_field.hip (the cost-to-go fields).
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "common.h"
#include "roadmap_geometry.h"
#include "self_geometry.h"

namespace rmgeo {

// Sub-segment s of S of the edge a -> b: midpoint configuration and per-link enlargement.
__host__ __device__ inline void edge_sample(const RmRobot& rb, const double* a, const double* b, int64_t s, int64_t S, double (&q)[ARMOUR_MAX_FACTORS],
                                            double (&r)[ARMOUR_MAX_JOINTS]) {
    double D[ARMOUR_MAX_FACTORS];
    const double t = (double)(2 * s + 1) / (double)(2 * S);
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) {
        D[j] = j < rb.n ? (rb.cont[j] ? wrap_diff(a[j], b[j]) : b[j] - a[j]) : 0.0;
        q[j] = j < rb.n ? a[j] + t * D[j] : 0.0;
    }
#pragma unroll
    for (int l = 0; l < ARMOUR_MAX_JOINTS; l++) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < ARMOUR_MAX_FACTORS && j <= l; j++) acc = j < rb.n ? acc + rb.rho[j][l] * fabs(D[j]) : acc;
        r[l] = acc / (double)(2 * S);
    }
}

// The roadmap's wrapped distance a -> b, its one copy: D_j joint by joint in index order (wrapped on continuous joints), acc += D_j * D_j
// from 0 (wrapped_sq), then one square root.  Written over all ARMOUR_MAX_FACTORS joints with a select so that a lane whose a is an array
// of its own keeps it in registers; the operations and their order are those of the loop over rb.n joints.
__host__ __device__ inline double wrapped_sq(const RmRobot& rb, const double* a, const double* b) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) {
        const double aj = j < rb.n ? a[j] : 0.0, bj = j < rb.n ? b[j] : 0.0;
        const double d = rb.cont[j] ? wrap_diff(aj, bj) : bj - aj;
        acc = j < rb.n ? acc + d * d : acc;
    }
    return acc;
}
__host__ __device__ inline double wrapped_norm(const RmRobot& rb, const double* a, const double* b) { return sqrt(wrapped_sq(rb, a, b)); }
// the total order (distance, index) of the nearest-neighbour search and of the tree planner's nearest node: the smaller index on a tie
__host__ __device__ inline bool key_less(double da, int va, double db, int vb) { return da < db || (da == db && va < vb); }

}  // namespace rmgeo

struct ArmourRoadmap {
    int device = 0;                      // < 0: a handle of armour_roadmap_create_host (no stream, no device buffers)
    rmgeo::RmRobot rb;
    int32_t N = 0, E = 0;
    int64_t M = 0;
    double edge_step = 0.0;
    std::vector<double> nodes;           // [N][n]
    std::vector<int32_t> edges;          // [E][2]
    DevBuf<double> d_nodes, d_obs, d_clear;
    DevBuf<double> d_vel, d_mid, d_half;  // the last moving check: velocity [W][O][3], the windows' midpoints and half widths [W]
    DevBuf<int32_t> d_edges, d_sample_edge;
    DevBuf<int64_t> d_edge_off;
    DevBuf<uint8_t> d_node_free, d_edge_free;
    DevStream stream;
    EventPair ev;
    // the last check, on the host
    int32_t W = -1, O = 0;
    std::vector<double> obs;             // [W][O][RM_OBS_STRIDE], staged as the kernel stages them ([W][O][RM_MOV_STRIDE] when `moving`)
    // the last check was armour_roadmap_check_moving: every later test of geometry for its worlds uses the window rule
    bool moving = false;
    std::vector<double> mid, half;       // [W]: 0.5 (t_from + t_to), 0.5 (t_to - t_from), the numbers the kernels are given
    std::vector<uint8_t> node_free, edge_free;
    // the self-collision masks (armour_roadmap_check_self, self_check.hip): world-independent, kept until the next self check
    bool self_on = false, self_checked = false;
    rmgeo::SelfTable self_table;
    std::vector<uint8_t> self_node_free, self_edge_free;   // [N], [E]
    // the cost-to-go fields (armour_roadmap_field, roadmap_field.hip).  The edge lengths and the CSR rows (neighbour ascending, then edge id)
    // depend on the roadmap alone: built and uploaded on first use.
    bool csr_ready = false;
    DevBuf<double> d_edge_len, d_seed_val, d_cost;
    DevBuf<int32_t> d_row_off, d_col, d_eid, d_seed_off, d_seed_node, d_next, d_reached, d_sweeps, d_field_status;
    DevBuf<uint8_t> d_self_edge_free;
    // the last field, on the host, for armour_roadmap_descend; a check, a self check or armour_roadmap_use_self ends it
    bool field_valid = false;
    std::vector<double> field_goals, field_cost;   // [W][n], [W][N]
    std::vector<int32_t> field_next;                // [W][N]
    // the nearest-neighbour search and the batched joins (roadmap_knn.hip): queries in, partial lists, results out
    DevBuf<double> d_kq, d_kdist, d_pdist, d_ktarget, d_self_shrink;
    DevBuf<int32_t> d_kmask, d_kexcl, d_kidx, d_kcount, d_pidx, d_pcount;
    DevBuf<uint8_t> d_self_node_free, d_self_on, d_kok;
    // the time slices (armour_roadmap_check_slices / armour_roadmap_arrival, roadmap_slices.hip): state of their own, beside the last check's.
    // sl_W < 0: no sliced check yet.  The device keeps the tables of a device handle; the host keeps them on a host handle, and on a device
    // handle when the caller asked for them (sl_on_host).
    int32_t sl_W = -1, sl_O = 0, sl_K = 0;
    double sl_dt = 0.0;
    bool sl_on_host = false;
    std::vector<double> sl_t0;                      // [W]
    std::vector<uint64_t> sl_node, sl_edge;         // [W][N], [W][E]
    DevBuf<uint64_t> d_sl_node, d_sl_edge, d_sl_extra, d_sl_reach, d_sl_xmask, d_sl_ends;
    DevBuf<double> d_sl_obs, d_sl_vel, d_sl_mid, d_sl_half, d_sl_xq;
    DevBuf<int32_t> d_sl_xitem, d_sl_xoff, d_sl_row_off, d_sl_col, d_sl_eid, d_sl_steps, d_sl_xu, d_sl_xv, d_sl_xsteps, d_sl_out, d_sl_path, d_sl_status;
    // the roadmap's edge lengths and CSR rows in the field's order (neighbour ascending, then edge id), built on first use; on the device
    // as well (d_sl_row_off / d_sl_col / d_sl_eid) once sl_csr_on_device
    bool sl_csr_ready = false, sl_csr_on_device = false;
    std::vector<double> sl_len;                     // [E]
    std::vector<int32_t> sl_row_off, sl_col, sl_eid;
};

// ---- what armour_roadmap_plan (roadmap.hip) and the field entries (roadmap_field.hip) share; defined in roadmap.hip
namespace rmhost {

double wrapped_distance(const rmgeo::RmRobot& rb, const double* a, const double* b);
// World w of the last check as a search reads it: its staged obstacles and its node / edge masks, ANDed with the self masks when those are on.
// After a moving check: moving = true, the obstacles staged with RM_MOV_STRIDE, and the world's window as mid and half.
struct WorldView {
    const double* obs = nullptr;
    bool moving = false;
    double mid = 0.0, half = 0.0;
    const uint8_t *nf = nullptr, *ef = nullptr;
    std::vector<uint8_t> both_n, both_e;
};
void world_view(const ArmourRoadmap* rm, int32_t w, WorldView* v);

// the edge rule on the host in the world of `v` (the window rule after a moving check), for an edge that is not in the roadmap (with the self
// masks on: the self edge rule as well).  The one place where the host searches choose between the static and the moving rule.
bool edge_free(const ArmourRoadmap* rm, const WorldView& v, const double* a, const double* b);

// q's connect_k nearest free nodes by wrapped_distance(q, node) (ties: the smaller index), in that order, those whose connecting edge is free:
// (distance, node)
void connect(const ArmourRoadmap* rm, const WorldView& v, const double* q, int32_t connect_k, std::vector<std::pair<double, int>>* out);

// armour_roadmap_descend's choice and walk (roadmap_field.hip), shared with armour_roadmap_descend_batch: among `joined` ((distance, node) in
// nearest order, edges free) the node of the smallest fl(distance + cost), first on a tie, then next[] to the goal.  cost / next: world w's
// rows of the field.  seq is cleared and filled with the nodes (empty: no path, *total = +inf).  ARMOUR_ESTATE when the successors do not
// lead to the goal within N + 1 steps.
int descend_walk(const char* who, int32_t N, int32_t w, const double* cost, const int32_t* next, const std::vector<std::pair<double, int>>& joined,
                 std::vector<int>* seq, double* total);

}  // namespace rmhost

