// Self-collision checks (include/armour_hip.h, armour_self_*, armour_roadmap_check_self, armour_path_audit_self): the arm's link boxes
// against each other, for configurations, roadmap edges and executed plan pieces.  The pair rule is written once as __host__ __device__
// code (self_geometry.h); the kernels run it per work item, the _host entries run the same functions in a loop without a device.
//
// Kernel shape: one lane per (item, first link a), a = blockIdx.y.  The lane runs the chain once, keeps box a when it passes it and tests
// every listed b as the chain reaches it, so it holds two boxes (30 doubles) and never all J (135 doubles, which would spill); the chain is
// repeated once per first link, which is cheap next to the 15-axis tests.  a is uniform in a block, so "is this link a / past a" is a scalar
// branch and nothing is indexed by a lane's own value.  The alternative -- a block's boxes through LDS, (item, pair) dealt to lanes -- needs
// a barrier and 120 B of LDS per link and item for the same tests.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "audit_host.h"
#include "common.h"
#include "path_pieces.h"
#include "roadmap_handle.h"
#include "self_geometry.h"

using namespace rmgeo;

namespace {

constexpr int SC_BLOCK = 256;                 // four waves

// grid (ceil((N + M) / SC_BLOCK), rows): item i < N is configuration i, item N + k is edge sub-segment k (edge sample_edge[k], sub-segment
// k - edge_off[e]), both against the pairs of first link a = blockIdx.y.  node_free / edge_free must hold 1 on entry; a colliding row
// stores 0 (no atomics: every writer writes 0).  row_clear / row_which [N][rows] (each may be null): the row's result of a configuration;
// with row_clear the configurations are tested without an early exit.
__global__ __launch_bounds__(SC_BLOCK) void self_check_kernel(RmRobot rb, int32_t rows, int32_t N, int64_t M, const double* __restrict__ nodes,
                                                               const int32_t* __restrict__ edges, const int64_t* __restrict__ edge_off,
                                                               const int32_t* __restrict__ sample_edge, const uint8_t* __restrict__ on,
                                                               const double* __restrict__ shrink, uint8_t* __restrict__ node_free,
                                                               uint8_t* __restrict__ edge_free, double* __restrict__ row_clear,
                                                               int32_t* __restrict__ row_which) {
    const int a = blockIdx.y;
    const int64_t item = (int64_t)blockIdx.x * SC_BLOCK + threadIdx.x;
    if (item >= (int64_t)N + M) return;
    double q[ARMOUR_MAX_FACTORS], delta[ARMOUR_MAX_FACTORS];
    const bool is_node = item < N;
    int e = 0;
    if (is_node) {
#pragma unroll
        for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) {
            q[j] = j < rb.n ? nodes[(size_t)item * rb.n + j] : 0.0;
            delta[j] = 0.0;
        }
    } else {
        const int64_t k = item - N;
        e = sample_edge[k];
        const int64_t s = k - edge_off[e], S = edge_off[e + 1] - edge_off[e];
        self_edge_sample(rb, nodes + (size_t)edges[2 * e] * rb.n, nodes + (size_t)edges[2 * e + 1] * rb.n, s, S, q, delta);
    }
    const bool full = is_node && row_clear != nullptr;
    double cl;
    int b;
    const bool ok = self_row_free(rb, a, q, delta, on + a * rb.J, shrink + a * rb.J, full, &cl, &b);
    if (is_node) {
        if (!ok && node_free) node_free[item] = 0;
        if (full) row_clear[(size_t)item * rows + a] = cl;
        if (row_which) row_which[(size_t)item * rows + a] = b;
    } else if (!ok) {
        edge_free[e] = 0;
    }
}

// One (piece, sub-interval) against the pairs of first link a: its audit_state.  full: *clearance = the sample test's clearance of the row,
// computed without an early exit.
__host__ __device__ inline int self_item_state(const RmRobot& rb, const PaPieces& pc, int a, int64_t p, int64_t s, int64_t S, const uint8_t* on,
                                               const double* shrink, bool full, double* clearance) {
    double q[ARMOUR_MAX_FACTORS], q1[ARMOUR_MAX_FACTORS], dev[ARMOUR_MAX_FACTORS], still[ARMOUR_MAX_FACTORS];
    piece_point(rb, pc, p, s, S, q, dev);
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) {
        q1[j] = q[j];
        still[j] = 0.0;
    }
    int b;
    return audit_state(
        full, [&] { return self_row_free(rb, a, q, dev, on, shrink, false, clearance, &b); },   // box b enlarged
        [&](bool no_exit) { return self_row_free(rb, a, q1, still, on, shrink, no_exit, clearance, &b); });
}

// grid (ceil(items / SC_BLOCK), rows): item i is sub-interval i - piece_off[p] of piece p = item_piece[i], against first link a = blockIdx.y;
// first_hit / undecided as audit_record expects them.  With item_clear [items][rows] no item is skipped and every item writes its row's clearance.
__global__ __launch_bounds__(SC_BLOCK) void self_audit_kernel(RmRobot rb, PaPieces pc, int32_t rows, int64_t items, const int32_t* __restrict__ item_piece,
                                                               const int64_t* __restrict__ piece_off, const uint8_t* __restrict__ on,
                                                               const double* __restrict__ shrink, int32_t* __restrict__ first_hit,
                                                               uint8_t* __restrict__ undecided, double* __restrict__ item_clear) {
    const int a = blockIdx.y;
    const int64_t item = (int64_t)blockIdx.x * SC_BLOCK + threadIdx.x;
    if (item >= items) return;
    const bool full = item_clear != nullptr;
    int p;
    int64_t s, S;
    if (!audit_item(item, item_piece, piece_off, first_hit, full, &p, &s, &S)) return;
    double cl;
    const int state = self_item_state(rb, pc, a, p, s, S, on + a * rb.J, shrink + a * rb.J, full, &cl);
    if (full) item_clear[(size_t)item * rows + a] = cl;
    audit_record(state, s, &first_hit[p], &undecided[p]);
}

// ---- what the entries share: argument checks and the pair table
int table_for_handle(const char* who, const RmRobot& rb, const uint8_t* pairs, const double* shrink, SelfTable* tb) {
    for (int a = 0; shrink && a < rb.J; a++)
        for (int b = a + 1; b < rb.J; b++)
            if (!std::isfinite(shrink[a * rb.J + b]) || shrink[a * rb.J + b] < 0.0) {
                armour_set_error("%s: shrink of pair (%d, %d) is %g (must be finite and >= 0)", who, a, b, shrink[a * rb.J + b]);
                return ARMOUR_EINVAL;
            }
    fill_self_table(rb, pairs, shrink, tb);
    return ARMOUR_OK;
}

int make_table(const char* who, const ArmourRobot* robot, const uint8_t* continuous, const uint8_t* pairs, const double* shrink, RmRobot* rb, SelfTable* tb) {
    if (!robot) { armour_set_error("%s: null robot", who); return ARMOUR_EINVAL; }
    ARMOUR_TRY(armour_check_robot_shape(who, robot));
    fill_rm_robot(robot, continuous, rb);
    return table_for_handle(who, *rb, pairs, shrink, tb);
}

// a configuration's results from its rows' (device order = host order: rows ascending, the first minimum / the first colliding pair wins)
void merge_rows(const SelfTable& tb, bool full, const double* row_clear, const int32_t* row_which, uint8_t* free_, double* clearance, int32_t* worst) {
    double cl = INFINITY;
    int wp = -1;
    bool ok = true;
    for (int a = 0; a < tb.rows; a++) {
        const int b = row_which[a];
        if (!full) {
            if (b >= 0) { ok = false; wp = a * tb.J + b; break; }
        } else if (b >= 0) {
            if (row_clear[a] < cl) { cl = row_clear[a]; wp = a * tb.J + b; }
            ok = ok && row_clear[a] > 0.0;
        }
    }
    if (free_) *free_ = ok ? 1 : 0;
    if (clearance) *clearance = cl;
    if (worst) *worst = wp;
}

int check_configs(const char* who, const RmRobot& rb, int32_t N, const double* q) {
    if (N < 0 || (N > 0 && !q)) { armour_set_error("%s: N = %d, q = %p", who, N, (const void*)q); return ARMOUR_EINVAL; }
    const size_t nn = (size_t)N * rb.n;
    if (const size_t i = first_nonfinite(q, nn); i < nn) { armour_set_error("%s: configuration %zu is not finite", who, i / rb.n); return ARMOUR_EINVAL; }
    return ARMOUR_OK;
}

// the pieces of a self audit: the checks of armour_path_audit without a world, and the sub-interval offsets in the caller's order
struct SelfAudit {
    RmRobot rb;
    SelfTable tb;
    PaPieces pc;                          // host pointers
    std::vector<int64_t> piece_off;       // [P + 1]
};

int make_audit(const char* who, const ArmourRobot* robot, const uint8_t* pairs, const double* shrink, const PieceArgs& a, const int32_t* verdict, SelfAudit* au) {
    if (!robot) { armour_set_error("%s: null argument", who); return ARMOUR_EINVAL; }
    ARMOUR_TRY(make_table(who, robot, nullptr, pairs, shrink, &au->rb, &au->tb));
    ARMOUR_TRY(check_pieces(who, au->rb.n, a, verdict, &au->pc));
    return piece_offsets(who, au->rb, au->pc, a.P, &au->piece_off);
}

// the launch of self_check_kernel and the merge of its rows; the buffers are the caller's
int run_self_check(const RmRobot& rb, const SelfTable& tb, int32_t N, int64_t M, int32_t E, const double* d_nodes, const int32_t* d_edges, const int64_t* d_edge_off,
                   const int32_t* d_sample_edge, hipStream_t st, EventPair* ev, uint8_t* node_free, uint8_t* edge_free, double* clearance, int32_t* worst,
                   double* ms) {
    const int rows = tb.rows;
    const bool full = clearance != nullptr, want_rows = full || worst != nullptr;
    DevBuf<uint8_t> d_on, d_node_free, d_edge_free;
    DevBuf<double> d_shrink, d_clear;
    DevBuf<int32_t> d_which;
    const size_t NR = (size_t)N * rows;
    ARMOUR_TRY(d_on.upload(tb.on, sizeof(tb.on), st));
    ARMOUR_TRY(d_shrink.upload(tb.shrink, sizeof(tb.shrink) / sizeof(double), st));
    ARMOUR_TRY(d_node_free.reserve((size_t)N));
    ARMOUR_TRY(d_edge_free.reserve((size_t)E));
    if (N) HIPCHK(hipMemsetAsync(d_node_free, 1, (size_t)N, st));
    if (E) HIPCHK(hipMemsetAsync(d_edge_free, 1, (size_t)E, st));
    if (full) ARMOUR_TRY(d_clear.reserve(NR));
    if (want_rows) ARMOUR_TRY(d_which.reserve(NR));
    const int64_t items = (int64_t)N + M;
    ARMOUR_TRY(ev->record_start(st));
    if (rows > 0 && items > 0) {
        const dim3 grid((unsigned)((items + SC_BLOCK - 1) / SC_BLOCK), (unsigned)rows);
        hipLaunchKernelGGL(self_check_kernel, grid, dim3(SC_BLOCK), 0, st, rb, rows, N, M, d_nodes, d_edges, d_edge_off, d_sample_edge, d_on, d_shrink,
                           d_node_free, d_edge_free, full ? d_clear : nullptr, want_rows ? d_which : nullptr);
        HIPCHK(hipGetLastError());
    }
    ARMOUR_TRY(ev->record_stop(st));
    std::vector<uint8_t> nf((size_t)N);
    std::vector<double> row_clear(full ? NR : 0);
    std::vector<int32_t> row_which(want_rows ? NR : 0);
    if (N) HIPCHK(hipMemcpyAsync(nf.data(), d_node_free, (size_t)N, hipMemcpyDeviceToHost, st));
    if (E && edge_free) HIPCHK(hipMemcpyAsync(edge_free, d_edge_free, (size_t)E, hipMemcpyDeviceToHost, st));
    if (full && NR) HIPCHK(hipMemcpyAsync(row_clear.data(), d_clear, NR * sizeof(double), hipMemcpyDeviceToHost, st));
    if (want_rows && NR) HIPCHK(hipMemcpyAsync(row_which.data(), d_which, NR * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ms) ARMOUR_TRY(ev->elapsed_ms(ms));
    for (int32_t i = 0; i < N; i++) {
        if (want_rows) {
            uint8_t f;
            merge_rows(tb, full, full ? row_clear.data() + (size_t)i * rows : nullptr, row_which.data() + (size_t)i * rows, &f,
                       clearance ? clearance + i : nullptr, worst ? worst + i : nullptr);
            if (node_free) node_free[i] = f;
        } else if (node_free) {
            node_free[i] = nf[i];
        }
    }
    return ARMOUR_OK;
}

}  // namespace

extern "C" int armour_self_pairs_default(const ArmourRobot* robot, uint8_t* pairs) {
    if (!robot || !pairs) { armour_set_error("armour_self_pairs_default: null argument"); return ARMOUR_EINVAL; }
    ARMOUR_TRY(armour_check_robot_shape("armour_self_pairs_default", robot));
    const int J = robot->num_joints;
    for (int a = 0; a < J; a++)
        for (int b = 0; b < J; b++) pairs[a * J + b] = b - a >= 2 ? 1 : 0;
    return ARMOUR_OK;
}

extern "C" int armour_self_check_host(const ArmourRobot* robot, const uint8_t* pairs, const double* shrink, int32_t N, const double* q, uint8_t* free_,
                                      double* clearance, int32_t* worst_pair) {
    RmRobot rb;
    SelfTable tb;
    ARMOUR_TRY(make_table("armour_self_check_host", robot, nullptr, pairs, shrink, &rb, &tb));
    ARMOUR_TRY(check_configs("armour_self_check_host", rb, N, q));
    const double still[ARMOUR_MAX_FACTORS] = {};
    for (int32_t i = 0; i < N; i++) {
        int wp;
        const bool ok = self_config_free(rb, tb, q + (size_t)i * rb.n, still, clearance != nullptr, clearance ? clearance + i : nullptr, &wp);
        if (free_) free_[i] = ok ? 1 : 0;
        if (worst_pair) worst_pair[i] = wp;
    }
    return ARMOUR_OK;
}

extern "C" int armour_self_check(const ArmourRobot* robot, const uint8_t* pairs, const double* shrink, int32_t N, const double* q, uint8_t* free_,
                                 double* clearance, int32_t* worst_pair, double* ms) {
    RmRobot rb;
    SelfTable tb;
    ARMOUR_TRY(make_table("armour_self_check", robot, nullptr, pairs, shrink, &rb, &tb));
    ARMOUR_TRY(check_configs("armour_self_check", rb, N, q));
    if (ms) *ms = 0.0;
    if (N == 0) return ARMOUR_OK;
    if (!armour_device_available()) { armour_set_error("armour_self_check: no HIP device visible (armour_self_check_host runs without one)"); return ARMOUR_EDEVICE; }
    DevStream st;
    EventPair ev;
    ARMOUR_TRY(st.create());
    DevBuf<double> d_q;
    ARMOUR_TRY(d_q.upload(q, (size_t)N * rb.n, st));
    return run_self_check(rb, tb, N, 0, 0, d_q, nullptr, nullptr, nullptr, st, &ev, free_, nullptr, clearance, worst_pair, ms);
}

extern "C" int armour_self_edges_host(const ArmourRobot* robot, const uint8_t* continuous, double edge_step, const uint8_t* pairs, const double* shrink, int32_t E,
                                      const double* qa, const double* qb, uint8_t* edge_free) {
    RmRobot rb;
    SelfTable tb;
    ARMOUR_TRY(make_table("armour_self_edges_host", robot, continuous, pairs, shrink, &rb, &tb));
    if (!(edge_step > 0.0) || !std::isfinite(edge_step) || E < 0 || (E > 0 && (!qa || !qb || !edge_free))) {
        armour_set_error("armour_self_edges_host: E = %d, edge_step = %g", E, edge_step);
        return ARMOUR_EINVAL;
    }
    if (!finite_all(qa, (size_t)E * rb.n) || !finite_all(qb, (size_t)E * rb.n)) { armour_set_error("armour_self_edges_host: non-finite input"); return ARMOUR_EINVAL; }
    for (int32_t e = 0; e < E; e++) edge_free[e] = self_edge_free(rb, tb, edge_step, qa + (size_t)e * rb.n, qb + (size_t)e * rb.n) ? 1 : 0;
    return ARMOUR_OK;
}

extern "C" int armour_roadmap_check_self(ArmourRoadmap* rm, const uint8_t* pairs, const double* shrink, uint8_t* node_free, uint8_t* edge_free,
                                         double* node_clearance, double* ms) {
    if (!rm) { armour_set_error("armour_roadmap_check_self: null handle"); return ARMOUR_EINVAL; }
    SelfTable tb;
    ARMOUR_TRY(table_for_handle("armour_roadmap_check_self", rm->rb, pairs, shrink, &tb));
    HIPCHK(hipSetDevice(rm->device));
    rm->field_valid = false;   // (armour_roadmap_field: a field belongs to the masks it was computed from)
    std::vector<uint8_t> nf((size_t)rm->N), ef((size_t)rm->E);
    ARMOUR_TRY(run_self_check(rm->rb, tb, rm->N, rm->M, rm->E, rm->d_nodes, rm->d_edges, rm->d_edge_off, rm->d_sample_edge, rm->stream, &rm->ev, nf.data(),
                              ef.data(), node_clearance, nullptr, ms));
    if (node_free && rm->N) std::memcpy(node_free, nf.data(), nf.size());
    if (edge_free && rm->E) std::memcpy(edge_free, ef.data(), ef.size());
    rm->self_table = tb;
    rm->self_node_free.swap(nf);
    rm->self_edge_free.swap(ef);
    rm->self_checked = true;
    return ARMOUR_OK;
}

extern "C" int armour_roadmap_use_self(ArmourRoadmap* rm, int32_t on) {
    if (!rm) { armour_set_error("armour_roadmap_use_self: null handle"); return ARMOUR_EINVAL; }
    rm->self_on = on != 0;
    rm->field_valid = false;
    return ARMOUR_OK;
}

extern "C" int armour_path_audit_self_host(const ArmourRobot* robot, const uint8_t* pairs, const double* shrink, int32_t P, const double* q0, const double* qd0,
                                           const double* qdd0, const double* k, const double* k_range, double duration, const double* ta, const double* tb,
                                           const double* tube, double step, int32_t* verdict, double* t_hit, double* clearance) {
    SelfAudit au;
    ARMOUR_TRY(make_audit("armour_path_audit_self_host", robot, pairs, shrink, {P, q0, qd0, qdd0, k, k_range, duration, ta, tb, tube, step}, verdict, &au));
    const int rows = au.tb.rows, J = au.tb.J;
    AuditMerge mg(P, clearance ? (size_t)au.piece_off[P] * rows : 0);
    for (int p = 0; p < P; p++) {
        const int64_t S = au.piece_off[p + 1] - au.piece_off[p];
        for (int64_t s = 0; s < S && (clearance || mg.first_hit[p] == PA_NO_HIT); s++)
            for (int a = 0; a < rows; a++) {
                double cl;
                const int state = self_item_state(au.rb, au.pc, a, p, s, S, au.tb.on + a * J, au.tb.shrink + a * J, clearance != nullptr, &cl);
                if (clearance) mg.item_clear[(size_t)(au.piece_off[p] + s) * rows + a] = cl;
                audit_record(state, s, &mg.first_hit[p], &mg.undecided[p]);
            }
    }
    finish_pieces(au.pc, au.piece_off, nullptr, rows, P, mg, verdict, t_hit, clearance);
    return ARMOUR_OK;
}

extern "C" int armour_path_audit_self(const ArmourRobot* robot, const uint8_t* pairs, const double* shrink, int32_t P, const double* q0, const double* qd0,
                                      const double* qdd0, const double* k, const double* k_range, double duration, const double* ta, const double* tb,
                                      const double* tube, double step, int32_t* verdict, double* t_hit, double* clearance, double* ms) {
    // ---- arguments and the work list, before the device is touched
    SelfAudit au;
    ARMOUR_TRY(make_audit("armour_path_audit_self", robot, pairs, shrink, {P, q0, qd0, qdd0, k, k_range, duration, ta, tb, tube, step}, verdict, &au));
    if (ms) *ms = 0.0;
    const int rows = au.tb.rows;
    const int64_t items = au.piece_off[P];
    AuditMerge mg(P, clearance ? (size_t)items * rows : 0);
    if (P > 0 && rows > 0) {
        // ---- the device
        if (!armour_device_available()) { armour_set_error("armour_path_audit_self: no HIP device visible (armour_path_audit_self_host runs without one)"); return ARMOUR_EDEVICE; }
        AuditDevice dev;
        PaPieces dpc;
        ARMOUR_TRY(dev.upload(au.pc, P, au.rb.n, au.piece_off, mg, &dpc));
        DevBuf<double> d_shrink;
        DevBuf<uint8_t> d_on;
        ARMOUR_TRY(d_on.upload(au.tb.on, sizeof(au.tb.on), dev.st));
        ARMOUR_TRY(d_shrink.upload(au.tb.shrink, sizeof(au.tb.shrink) / sizeof(double), dev.st));
        ARMOUR_TRY(dev.ev.record_start(dev.st));
        if (items > 0) {
            const dim3 grid((unsigned)((items + SC_BLOCK - 1) / SC_BLOCK), (unsigned)rows);
            hipLaunchKernelGGL(self_audit_kernel, grid, dim3(SC_BLOCK), 0, dev.st, au.rb, dpc, rows, items, dev.item_piece, dev.piece_off, d_on, d_shrink,
                               dev.first_hit, dev.undecided, clearance ? dev.clear.p : nullptr);
            HIPCHK(hipGetLastError());
        }
        ARMOUR_TRY(dev.download(&mg, ms));
    }
    finish_pieces(au.pc, au.piece_off, nullptr, rows, P, mg, verdict, t_hit, clearance);
    return ARMOUR_OK;
}
