// Path audit (include/armour_hip.h, armour_path_audit): a sound collision audit of executed Bezier plan pieces against worlds' obstacles,
// all pieces in one launch.  A piece is the plan (q0, qd0, qdd0, k) on a time window [ta, tb]; it is cut into sub-intervals, and each
// (piece, sub-interval) is one work item that evaluates the curve at the sub-interval's midpoint and runs the roadmap's node rule
// (roadmap_geometry.h) there: with the link boxes enlarged by what the arm can move inside the sub-interval (the tube test) and, if that
// does not separate, with the boxes as they are (the sample test).  The rule is written once as __host__ __device__ code: the kernel runs it
// per item, armour_path_audit_host runs the same functions in a loop without a device.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "bezier.h"
#include "common.h"
#include "path_pieces.h"
#include "roadmap_geometry.h"

using namespace rmgeo;

namespace {

constexpr int PA_BLOCK = 256;                 // four waves; a block serves one world (its obstacles are staged in LDS)
constexpr int32_t PA_NO_HIT = INT32_MAX;      // first_hit[p] before any sample test collided

// One item against its world's staged obstacles: 0 the tube test separates, 1 the sample test collides, 2 neither.  full: *clearance = the
// sample test's clearance, computed without an early exit (a flag and an always-valid pointer, as config_free takes them: a pointer that
// may be null would force the caller's value into scratch memory).
__host__ __device__ inline int item_state(const RmRobot& rb, const PaPieces& pc, int64_t p, int64_t s, int64_t S, const double* obs, int O, bool full,
                                          double* clearance) {
    double q[ARMOUR_MAX_FACTORS], q1[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS], r0[ARMOUR_MAX_JOINTS];
    piece_sample(rb, pc, p, s, S, q, r);
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q1[j] = q[j];
#pragma unroll
    for (int l = 0; l < ARMOUR_MAX_JOINTS; l++) r0[l] = 0.0;
    if (full) {
        const bool sample_free = config_free(rb, q1, r0, obs, O, true, clearance);
        if (!sample_free) return 1;
        return config_free(rb, q, r, obs, O, false, nullptr) ? 0 : 2;
    }
    if (config_free(rb, q, r, obs, O, false, nullptr)) return 0;   // enlarged boxes separated: the boxes themselves are
    return config_free(rb, q1, r0, obs, O, false, nullptr) ? 2 : 1;
}

// One launch, 1-D grid: block b serves items [blk_item0[b], blk_item0[b] + blk_count[b]) of world blk_world[b] (items are sorted by world, a
// block never spans two).  Item i is sub-interval i - piece_off[p] of piece p = item_piece[i].  first_hit must hold PA_NO_HIT and undecided 0
// on entry: a colliding item lowers first_hit[p] to its sub-interval (an integer minimum), an undecided one stores 1 (every writer writes 1).
// Without item_clear (verdict mode) an item behind a recorded hit of its piece returns at once: it can change neither the minimum nor the verdict.
__global__ __launch_bounds__(PA_BLOCK) void path_audit_kernel(RmRobot rb, PaPieces pc, const int32_t* __restrict__ blk_world,
                                                               const int64_t* __restrict__ blk_item0, const int32_t* __restrict__ blk_count,
                                                               const int32_t* __restrict__ item_piece, const int64_t* __restrict__ piece_off,
                                                               const double* __restrict__ obstacles, int32_t O, int32_t* __restrict__ first_hit,
                                                               uint8_t* __restrict__ undecided, double* __restrict__ item_clear) {
    extern __shared__ double s_obs[];   // [O][RM_OBS_STRIDE]
    const int w = blk_world[blockIdx.x];
    const double* Zw = obstacles + (size_t)w * O * ARMOUR_OBS_DOUBLES;
    for (int i = threadIdx.x; i < O * ARMOUR_OBS_DOUBLES; i += PA_BLOCK)
        s_obs[(i / ARMOUR_OBS_DOUBLES) * RM_OBS_STRIDE + i % ARMOUR_OBS_DOUBLES] = Zw[i];
    for (int o = threadIdx.x; o < O; o += PA_BLOCK) obstacle_normals(Zw + (size_t)o * ARMOUR_OBS_DOUBLES, s_obs + (size_t)o * RM_OBS_STRIDE + 12);
    __syncthreads();
    if ((int)threadIdx.x >= blk_count[blockIdx.x]) return;
    const int64_t item = blk_item0[blockIdx.x] + threadIdx.x;
    const int p = item_piece[item];
    const int64_t s = item - piece_off[p], S = piece_off[p + 1] - piece_off[p];
    if (!item_clear && (int64_t)__atomic_load_n(&first_hit[p], __ATOMIC_RELAXED) < s) return;
    double cl;
    const bool full = item_clear != nullptr;
    const int state = item_state(rb, pc, p, s, S, s_obs, O, full, &cl);
    if (full) item_clear[item] = cl;
    if (state == 1) atomicMin(&first_hit[p], (int32_t)s);
    else if (state == 2) undecided[p] = 1;
}

// What both entries share: the argument checks and the work list (pieces in world order, their sub-interval offsets).
struct AuditPlan {
    RmRobot rb;
    PaPieces pc;                          // host pointers
    std::vector<int32_t> order;           // the caller's pieces sorted by world (stable)
    std::vector<int64_t> piece_off;       // [P + 1]: sorted piece i owns items [piece_off[i], piece_off[i + 1])
    int64_t items = 0;
};

int make_plan(const char* who, const ArmourRobot* robot, int32_t W, int32_t O, const double* obstacles, int32_t P, const int32_t* world_of_piece,
              const double* q0, const double* qd0, const double* qdd0, const double* k, const double* k_range, double duration, const double* ta,
              const double* tb, const double* tube, double step, const int32_t* verdict, AuditPlan* pl) {
    if (!robot || !k_range || P < 0 || (P > 0 && (!world_of_piece || !q0 || !qd0 || !qdd0 || !k || !ta || !tb || !verdict))) {
        armour_set_error("%s: null argument", who);
        return ARMOUR_EINVAL;
    }
    ARMOUR_TRY(armour_check_robot_shape(who, robot));
    ARMOUR_TRY(armour_check_world_counts(who, W, O, obstacles));
    if (!(step > 0.0) || !std::isfinite(step) || !(duration > 0.0) || !std::isfinite(duration)) {
        armour_set_error("%s: step = %g, duration = %g (both must be positive)", who, step, duration);
        return ARMOUR_EINVAL;
    }
    const int n = robot->num_factors;
    const size_t pn = (size_t)P * n;
    if (!finite_all(obstacles, (size_t)W * O * ARMOUR_OBS_DOUBLES) || !finite_all(k_range, n) || !finite_all(q0, pn) || !finite_all(qd0, pn) ||
        !finite_all(qdd0, pn) || !finite_all(k, pn) || (tube && !finite_all(tube, pn))) {
        armour_set_error("%s: non-finite input", who);
        return ARMOUR_EINVAL;
    }
    for (int p = 0; p < P; p++) {
        if (world_of_piece[p] < 0 || world_of_piece[p] >= W) { armour_set_error("%s: piece %d names world %d of %d", who, p, world_of_piece[p], W); return ARMOUR_EINVAL; }
        if (!(ta[p] >= 0.0) || !(tb[p] >= ta[p]) || !(tb[p] <= duration)) {
            armour_set_error("%s: piece %d has the window [%g, %g], need 0 <= ta <= tb <= duration = %g", who, p, ta[p], tb[p], duration);
            return ARMOUR_EINVAL;
        }
        for (int j = 0; tube && j < n; j++)
            if (!(tube[(size_t)p * n + j] >= 0.0)) { armour_set_error("%s: piece %d has a negative tube radius", who, p); return ARMOUR_EINVAL; }
    }
    fill_rm_robot(robot, nullptr, &pl->rb);
    PaPieces& pc = pl->pc;
    std::memset(&pc, 0, sizeof(pc));
    pc.q0 = q0; pc.qd0 = qd0; pc.qdd0 = qdd0; pc.k = k; pc.ta = ta; pc.tb = tb; pc.tube = tube;
    for (int j = 0; j < n; j++) pc.k_range[j] = k_range[j];
    pc.duration = duration;
    pc.step = step;
    pl->order.resize(P);
    for (int p = 0; p < P; p++) pl->order[p] = p;
    std::stable_sort(pl->order.begin(), pl->order.end(), [&](int32_t a, int32_t b) { return world_of_piece[a] < world_of_piece[b]; });
    pl->piece_off.assign((size_t)P + 1, 0);
    pl->items = 0;
    return ARMOUR_OK;
}

// Pieces renumbered into world order (stable), so that piece_off is a plain prefix sum and a world's items are contiguous: from here on the
// device and the host loop both see piece i = the caller's piece order[i].
struct Sorted {
    std::vector<double> q0, qd0, qdd0, k, ta, tb, tube;
    std::vector<int32_t> world;
};

int sort_pieces(const char* who, AuditPlan* pl, const int32_t* world_of_piece, int32_t P, Sorted* sd) {
    const int n = pl->rb.n;
    const PaPieces src = pl->pc;
    auto gather = [&](const double* from, std::vector<double>* to, int width) {
        to->resize((size_t)P * width);
        for (int i = 0; i < P; i++) std::memcpy(to->data() + (size_t)i * width, from + (size_t)pl->order[i] * width, width * sizeof(double));
    };
    gather(src.q0, &sd->q0, n); gather(src.qd0, &sd->qd0, n); gather(src.qdd0, &sd->qdd0, n); gather(src.k, &sd->k, n);
    gather(src.ta, &sd->ta, 1); gather(src.tb, &sd->tb, 1);
    if (src.tube) gather(src.tube, &sd->tube, n);
    sd->world.resize(P);
    for (int i = 0; i < P; i++) sd->world[i] = world_of_piece[pl->order[i]];
    PaPieces& pc = pl->pc;
    pc.q0 = sd->q0.data(); pc.qd0 = sd->qd0.data(); pc.qdd0 = sd->qdd0.data(); pc.k = sd->k.data(); pc.ta = sd->ta.data(); pc.tb = sd->tb.data();
    pc.tube = src.tube ? sd->tube.data() : nullptr;
    for (int i = 0; i < P; i++) {
        const double S = piece_intervals(pl->rb, pc, i);
        if (!(S + (double)pl->piece_off[i] <= (double)(INT32_MAX - 1))) {
            armour_set_error("%s: more than 2^31 - 2 (piece, sub-interval) items (step %g too small)", who, pc.step);
            return ARMOUR_ECAPACITY;
        }
        pl->piece_off[i + 1] = pl->piece_off[i] + (int64_t)S;
    }
    pl->items = pl->piece_off[P];
    return ARMOUR_OK;
}

// the per-piece results from what the items left: first_hit / undecided / item_clear are in world order
void finish(const AuditPlan& pl, int32_t P, const int32_t* first_hit, const uint8_t* undecided, const double* item_clear, int32_t* verdict, double* t_hit,
            double* clearance) {
    for (int i = 0; i < P; i++) {
        const int p = pl.order[i];
        const int64_t S = pl.piece_off[i + 1] - pl.piece_off[i];
        const bool hit = first_hit[i] != PA_NO_HIT;
        verdict[p] = hit ? 1 : undecided[i] ? 2 : 0;
        if (t_hit) {
            const double ta = pl.pc.ta[i], w = pl.pc.tb[i] - ta;
            t_hit[p] = hit ? ta + ((double)(2 * (int64_t)first_hit[i] + 1) * w) / (double)(2 * S) : NAN;
        }
        if (clearance) {
            double cl = INFINITY;
            for (int64_t x = pl.piece_off[i]; x < pl.piece_off[i + 1]; x++) cl = fmin(cl, item_clear[x]);
            clearance[p] = cl;
        }
    }
}
}  // namespace

extern "C" int armour_path_audit_host(const ArmourRobot* robot, int32_t W, int32_t O, const double* obstacles, int32_t P, const int32_t* world_of_piece,
                                      const double* q0, const double* qd0, const double* qdd0, const double* k, const double* k_range, double duration,
                                      const double* ta, const double* tb, const double* tube, double step, int32_t* verdict, double* t_hit,
                                      double* clearance) {
    AuditPlan pl;
    Sorted sd;
    int rc = make_plan("armour_path_audit_host", robot, W, O, obstacles, P, world_of_piece, q0, qd0, qdd0, k, k_range, duration, ta, tb, tube, step, verdict, &pl);
    if (rc != ARMOUR_OK) return rc;
    if ((rc = sort_pieces("armour_path_audit_host", &pl, world_of_piece, P, &sd)) != ARMOUR_OK) return rc;
    std::vector<double> obs((size_t)W * O * RM_OBS_STRIDE);   // staged as the kernel stages them
    stage_obstacles(obstacles, (size_t)W * O, obs.data());
    std::vector<int32_t> first_hit(P, PA_NO_HIT);
    std::vector<uint8_t> undecided(P, 0);
    std::vector<double> item_clear(clearance ? (size_t)pl.items : 0);
    for (int i = 0; i < P; i++) {
        const double* ob = obs.data() + (size_t)sd.world[i] * O * RM_OBS_STRIDE;
        const int64_t S = pl.piece_off[i + 1] - pl.piece_off[i];
        for (int64_t s = 0; s < S; s++) {
            double cl;
            const int state = item_state(pl.rb, pl.pc, i, s, S, ob, O, clearance != nullptr, &cl);
            if (clearance) item_clear[(size_t)(pl.piece_off[i] + s)] = cl;
            if (state == 1) { first_hit[i] = std::min(first_hit[i], (int32_t)s); if (!clearance) break; }
            else if (state == 2) undecided[i] = 1;
        }
    }
    finish(pl, P, first_hit.data(), undecided.data(), item_clear.data(), verdict, t_hit, clearance);
    return ARMOUR_OK;
}

extern "C" int armour_path_audit(const ArmourRobot* robot, int32_t W, int32_t O, const double* obstacles, int32_t P, const int32_t* world_of_piece,
                                 const double* q0, const double* qd0, const double* qdd0, const double* k, const double* k_range, double duration,
                                 const double* ta, const double* tb, const double* tube, double step, int32_t* verdict, double* t_hit, double* clearance,
                                 double* ms) {
    // ---- arguments and the work list, before the device is touched
    AuditPlan pl;
    Sorted sd;
    int rc = make_plan("armour_path_audit", robot, W, O, obstacles, P, world_of_piece, q0, qd0, qdd0, k, k_range, duration, ta, tb, tube, step, verdict, &pl);
    if (rc != ARMOUR_OK) return rc;
    if ((rc = sort_pieces("armour_path_audit", &pl, world_of_piece, P, &sd)) != ARMOUR_OK) return rc;
    if (ms) *ms = 0.0;
    const int n = pl.rb.n;
    const int64_t items = pl.items;
    std::vector<int32_t> item_piece((size_t)items), blk_world, blk_count;
    std::vector<int64_t> blk_item0;
    for (int i = 0; i < P; i++)
        for (int64_t x = pl.piece_off[i]; x < pl.piece_off[i + 1]; x++) item_piece[(size_t)x] = i;
    for (int i = 0; i < P;) {   // one run of pieces per world, cut into blocks of PA_BLOCK items
        int e = i;
        while (e < P && sd.world[e] == sd.world[i]) e++;
        for (int64_t x = pl.piece_off[i]; x < pl.piece_off[e]; x += PA_BLOCK) {
            blk_world.push_back(sd.world[i]);
            blk_item0.push_back(x);
            blk_count.push_back((int32_t)std::min<int64_t>(PA_BLOCK, pl.piece_off[e] - x));
        }
        i = e;
    }
    std::vector<int32_t> first_hit(P, PA_NO_HIT);
    std::vector<uint8_t> undecided(P, 0);
    std::vector<double> item_clear(clearance ? (size_t)items : 0);
    if (P > 0) {
        // ---- the device
        if (!armour_device_available()) { armour_set_error("armour_path_audit: no HIP device visible (there is no CPU path)"); return ARMOUR_EDEVICE; }
        DevStream st;
        EventPair ev;
        ARMOUR_TRY(st.create());
        DevBuf<double> d_q0, d_qd0, d_qdd0, d_k, d_ta, d_tb, d_tube, d_obs, d_clear;
        DevBuf<int32_t> d_blk_world, d_blk_count, d_item_piece, d_first_hit;
        DevBuf<int64_t> d_blk_item0, d_piece_off;
        DevBuf<uint8_t> d_undecided;
        const size_t pn = (size_t)P * n;
        ARMOUR_TRY(d_q0.upload(pl.pc.q0, pn, st));
        ARMOUR_TRY(d_qd0.upload(pl.pc.qd0, pn, st));
        ARMOUR_TRY(d_qdd0.upload(pl.pc.qdd0, pn, st));
        ARMOUR_TRY(d_k.upload(pl.pc.k, pn, st));
        ARMOUR_TRY(d_ta.upload(pl.pc.ta, P, st));
        ARMOUR_TRY(d_tb.upload(pl.pc.tb, P, st));
        if (tube) ARMOUR_TRY(d_tube.upload(pl.pc.tube, pn, st));
        ARMOUR_TRY(d_obs.upload(obstacles, (size_t)W * O * ARMOUR_OBS_DOUBLES, st));
        ARMOUR_TRY(d_blk_world.upload(blk_world.data(), blk_world.size(), st));
        ARMOUR_TRY(d_blk_count.upload(blk_count.data(), blk_count.size(), st));
        ARMOUR_TRY(d_blk_item0.upload(blk_item0.data(), blk_item0.size(), st));
        ARMOUR_TRY(d_item_piece.upload(item_piece.data(), item_piece.size(), st));
        ARMOUR_TRY(d_piece_off.upload(pl.piece_off.data(), pl.piece_off.size(), st));
        ARMOUR_TRY(d_first_hit.upload(first_hit.data(), P, st));
        ARMOUR_TRY(d_undecided.upload(undecided.data(), P, st));
        if (clearance) ARMOUR_TRY(d_clear.upload(nullptr, (size_t)items, st));
        PaPieces dpc = pl.pc;
        dpc.q0 = d_q0; dpc.qd0 = d_qd0; dpc.qdd0 = d_qdd0; dpc.k = d_k; dpc.ta = d_ta; dpc.tb = d_tb;
        dpc.tube = tube ? d_tube : nullptr;
        ARMOUR_TRY(ev.record_start(st));
        if (!blk_world.empty()) {
            const size_t lds = (size_t)O * RM_OBS_STRIDE * sizeof(double);
            hipLaunchKernelGGL(path_audit_kernel, dim3((unsigned)blk_world.size()), dim3(PA_BLOCK), lds, st, pl.rb, dpc, d_blk_world, d_blk_item0,
                               d_blk_count, d_item_piece, d_piece_off, d_obs, O, d_first_hit, d_undecided, clearance ? d_clear : nullptr);
            HIPCHK(hipGetLastError());
        }
        ARMOUR_TRY(ev.record_stop(st));
        HIPCHK(hipMemcpyAsync(first_hit.data(), d_first_hit, (size_t)P * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(undecided.data(), d_undecided, (size_t)P, hipMemcpyDeviceToHost, st));
        if (clearance && items) HIPCHK(hipMemcpyAsync(item_clear.data(), d_clear, (size_t)items * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (ms) ARMOUR_TRY(ev.elapsed_ms(ms));
    }
    finish(pl, P, first_hit.data(), undecided.data(), item_clear.data(), verdict, t_hit, clearance);
    return ARMOUR_OK;
}

extern "C" int armour_path_audit_items(const ArmourRobot* robot, int32_t P, const double* q0, const double* qd0, const double* qdd0, const double* k,
                                       const double* k_range, double duration, const double* ta, const double* tb, double step, int64_t* items) {
    if (!robot || !k_range || !items || P < 0 || (P > 0 && (!q0 || !qd0 || !qdd0 || !k || !ta || !tb)) || !(step > 0.0) || !(duration > 0.0) ||
        !armour_robot_shape_ok(robot)) {
        armour_set_error("armour_path_audit_items: bad argument");
        return ARMOUR_EINVAL;
    }
    RmRobot rb;
    fill_rm_robot(robot, nullptr, &rb);
    PaPieces pc;
    std::memset(&pc, 0, sizeof(pc));
    pc.q0 = q0; pc.qd0 = qd0; pc.qdd0 = qdd0; pc.k = k; pc.ta = ta; pc.tb = tb;
    for (int j = 0; j < rb.n; j++) pc.k_range[j] = k_range[j];
    pc.duration = duration;
    pc.step = step;
    for (int p = 0; p < P; p++) items[p] = (int64_t)std::fmin(piece_intervals(rb, pc, p), 9e18);
    return ARMOUR_OK;
}
