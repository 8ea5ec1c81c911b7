// Path audit (include/armour_hip.h, armour_path_audit): a sound collision audit of executed Bezier plan pieces against worlds' obstacles,
// all pieces in one launch.  A piece is the plan (q0, qd0, qdd0, k) on a time window [ta, tb]; it is cut into sub-intervals, and each
// (piece, sub-interval) is one work item that evaluates the curve at the sub-interval's midpoint and runs the roadmap's node rule
// (roadmap_geometry.h) there: with the link boxes enlarged by what the arm can move inside the sub-interval (the tube test) and, if that
// does not separate, with the boxes as they are (the sample test).  The rule is written once as __host__ __device__ code: the kernel runs it
// per item, armour_path_audit_host runs the same functions in a loop without a device.  armour_path_audit_moving is the same audit against
// obstacles in linear motion: its items run config_free_moving at the world time of their midpoint, in a kernel of their own (the static
// kernel and the functions it compiles are not touched by it).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "audit_host.h"
#include "bezier.h"
#include "common.h"
#include "path_pieces.h"
#include "roadmap_geometry.h"

using namespace rmgeo;

namespace {

constexpr int PA_BLOCK = 256;                 // four waves; a block serves one world (its obstacles are staged in LDS)

// One item against its world's staged obstacles: its audit_state.  full: *clearance = the sample test's clearance, computed without an
// early exit (a flag and an always-valid pointer, as config_free takes them: a pointer that may be null would force the caller's value
// into scratch memory).
__host__ __device__ inline int item_state(const RmRobot& rb, const PaPieces& pc, int64_t p, int64_t s, int64_t S, const double* obs, int O, bool full,
                                          double* clearance) {
    double q[ARMOUR_MAX_FACTORS], q1[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS], r0[ARMOUR_MAX_JOINTS];
    piece_sample(rb, pc, p, s, S, q, r);
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q1[j] = q[j];
#pragma unroll
    for (int l = 0; l < ARMOUR_MAX_JOINTS; l++) r0[l] = 0.0;
    return audit_state(
        full, [&] { return config_free(rb, q, r, obs, O, false, clearance); },
        [&](bool no_exit) { return config_free(rb, q1, r0, obs, O, no_exit, clearance); });
}

// One launch, 1-D grid: block b serves items [blk_item0[b], blk_item0[b] + blk_count[b]) of world blk_world[b] (items are sorted by world, a
// block never spans two).  Item i is sub-interval i - piece_off[p] of piece p = item_piece[i]; first_hit / undecided as audit_record expects
// them.  With item_clear (clearance mode) no item is skipped and every item writes its sample clearance.
__global__ __launch_bounds__(PA_BLOCK) void path_audit_kernel(RmRobot rb, PaPieces pc, const int32_t* __restrict__ blk_world,
                                                               const int64_t* __restrict__ blk_item0, const int32_t* __restrict__ blk_count,
                                                               const int32_t* __restrict__ item_piece, const int64_t* __restrict__ piece_off,
                                                               const double* __restrict__ obstacles, int32_t O, int32_t* __restrict__ first_hit,
                                                               uint8_t* __restrict__ undecided, double* __restrict__ item_clear) {
    extern __shared__ double s_obs[];   // [O][RM_OBS_STRIDE]
    stage_obstacles_lds<PA_BLOCK>(obstacles + (size_t)blk_world[blockIdx.x] * O * ARMOUR_OBS_DOUBLES, O, s_obs);
    if ((int)threadIdx.x >= blk_count[blockIdx.x]) return;
    const int64_t item = blk_item0[blockIdx.x] + threadIdx.x;
    const bool full = item_clear != nullptr;
    int p;
    int64_t s, S;
    if (!audit_item(item, item_piece, piece_off, first_hit, full, &p, &s, &S)) return;
    double cl;
    const int state = item_state(rb, pc, p, s, S, s_obs, O, full, &cl);
    if (full) item_clear[item] = cl;
    audit_record(state, s, &first_hit[p], &undecided[p]);
}

// item_state against moving obstacles (staged with stride RM_MOV_STRIDE): both tests at the obstacles' poses of world time
// tau = t_world[p] + t_s; the tube test grows every half-size by |v_o| half besides (config_free_moving).
__host__ __device__ inline int item_state_moving(const RmRobot& rb, const PaPieces& pc, const double* t_world, int64_t p, int64_t s, int64_t S, const double* obs,
                                                 int O, bool full, double* clearance) {
    double q[ARMOUR_MAX_FACTORS], q1[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS], r0[ARMOUR_MAX_JOINTS];
    const double tau = t_world[p] + piece_sample(rb, pc, p, s, S, q, r);
    const double half = (pc.tb[p] - pc.ta[p]) / (double)(2 * S);
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q1[j] = q[j];
#pragma unroll
    for (int l = 0; l < ARMOUR_MAX_JOINTS; l++) r0[l] = 0.0;
    return audit_state(
        full, [&] { return config_free_moving(rb, q, r, obs, O, tau, half, false, clearance); },
        [&](bool no_exit) { return config_free_moving(rb, q1, r0, obs, O, tau, 0.0, no_exit, clearance); });
}

// path_audit_kernel for moving obstacles: the same grid, blocks and merge words; velocity [W][O][3], t_world [P] in the pieces' (sorted) order
__global__ __launch_bounds__(PA_BLOCK) void path_audit_moving_kernel(RmRobot rb, PaPieces pc, const int32_t* __restrict__ blk_world,
                                                                      const int64_t* __restrict__ blk_item0, const int32_t* __restrict__ blk_count,
                                                                      const int32_t* __restrict__ item_piece, const int64_t* __restrict__ piece_off,
                                                                      const double* __restrict__ obstacles, const double* __restrict__ velocity,
                                                                      const double* __restrict__ t_world, int32_t O, int32_t* __restrict__ first_hit,
                                                                      uint8_t* __restrict__ undecided, double* __restrict__ item_clear) {
    extern __shared__ double s_obs[];   // [O][RM_MOV_STRIDE]
    const size_t w = (size_t)blk_world[blockIdx.x];
    stage_obstacles_moving_lds<PA_BLOCK>(obstacles + w * O * ARMOUR_OBS_DOUBLES, velocity + w * O * 3, O, s_obs);
    if ((int)threadIdx.x >= blk_count[blockIdx.x]) return;
    const int64_t item = blk_item0[blockIdx.x] + threadIdx.x;
    const bool full = item_clear != nullptr;
    int p;
    int64_t s, S;
    if (!audit_item(item, item_piece, piece_off, first_hit, full, &p, &s, &S)) return;
    double cl;
    const int state = item_state_moving(rb, pc, t_world, p, s, S, s_obs, O, full, &cl);
    if (full) item_clear[item] = cl;
    audit_record(state, s, &first_hit[p], &undecided[p]);
}

// What both entries share: the argument checks and the work list (pieces in world order, their sub-interval offsets).  Pieces are
// renumbered into world order (stable), so that piece_off is a plain prefix sum and a world's items are contiguous: from the sort on the
// device and the host loop both see piece i = the caller's piece order[i].
struct AuditPlan {
    RmRobot rb;
    PaPieces pc;                          // host pointers: the caller's until the sort, then the sorted copies below
    std::vector<int32_t> order;           // the caller's pieces sorted by world (stable)
    std::vector<int64_t> piece_off;       // [P + 1]: sorted piece i owns items [piece_off[i], piece_off[i + 1])
    std::vector<double> q0, qd0, qdd0, k, ta, tb, tube;
    std::vector<int32_t> world;           // [P]: sorted piece i's world
    std::vector<double> t_world;          // [P]: sorted piece i's world time of its plan time 0 (the moving audit alone)
};

// the motion of a moving audit as the caller passed it (velocity null: a static audit)
struct Motion {
    const double *velocity, *t_world;
};

int make_plan(const char* who, const ArmourRobot* robot, int32_t W, int32_t O, const double* obstacles, const int32_t* world_of_piece, const PieceArgs& a,
              const int32_t* verdict, AuditPlan* pl, const Motion* mv = nullptr) {
    const int32_t P = a.P;
    if (!robot || (P > 0 && !world_of_piece)) {
        armour_set_error("%s: null argument", who);
        return ARMOUR_EINVAL;
    }
    ARMOUR_TRY(armour_check_robot_shape(who, robot));
    ARMOUR_TRY(armour_check_world_counts(who, W, O, obstacles));
    if (mv && ((W > 0 && O > 0 && !mv->velocity) || (P > 0 && !mv->t_world))) {
        armour_set_error("%s: null argument", who);
        return ARMOUR_EINVAL;
    }
    const int n = robot->num_factors;
    ARMOUR_TRY(check_pieces(who, n, a, verdict, &pl->pc));
    if (!finite_all(obstacles, (size_t)W * O * ARMOUR_OBS_DOUBLES) || (mv && (!finite_all(mv->velocity, (size_t)W * O * 3) || !finite_all(mv->t_world, P)))) {
        armour_set_error("%s: non-finite input", who);
        return ARMOUR_EINVAL;
    }
    for (int p = 0; p < P; p++)
        if (world_of_piece[p] < 0 || world_of_piece[p] >= W) { armour_set_error("%s: piece %d names world %d of %d", who, p, world_of_piece[p], W); return ARMOUR_EINVAL; }
    fill_rm_robot(robot, nullptr, &pl->rb);
    pl->order.resize(P);
    for (int p = 0; p < P; p++) pl->order[p] = p;
    std::stable_sort(pl->order.begin(), pl->order.end(), [&](int32_t x, int32_t y) { return world_of_piece[x] < world_of_piece[y]; });
    const PaPieces src = pl->pc;
    auto gather = [&](const double* from, std::vector<double>* to, int width) {
        to->resize((size_t)P * width);
        for (int i = 0; i < P; i++) std::memcpy(to->data() + (size_t)i * width, from + (size_t)pl->order[i] * width, width * sizeof(double));
    };
    gather(src.q0, &pl->q0, n); gather(src.qd0, &pl->qd0, n); gather(src.qdd0, &pl->qdd0, n); gather(src.k, &pl->k, n);
    gather(src.ta, &pl->ta, 1); gather(src.tb, &pl->tb, 1);
    if (src.tube) gather(src.tube, &pl->tube, n);
    if (mv) gather(mv->t_world, &pl->t_world, 1);
    pl->world.resize(P);
    for (int i = 0; i < P; i++) pl->world[i] = world_of_piece[pl->order[i]];
    PaPieces& pc = pl->pc;
    pc.q0 = pl->q0.data(); pc.qd0 = pl->qd0.data(); pc.qdd0 = pl->qdd0.data(); pc.k = pl->k.data(); pc.ta = pl->ta.data(); pc.tb = pl->tb.data();
    pc.tube = src.tube ? pl->tube.data() : nullptr;
    return piece_offsets(who, pl->rb, pc, P, &pl->piece_off);
}
}  // namespace

// the host twin of both audits (mv null: the static one)
static int audit_on_host(const char* who, const ArmourRobot* robot, int32_t W, int32_t O, const double* obstacles, const Motion* mv, const int32_t* world_of_piece,
                         const PieceArgs& a, int32_t* verdict, double* t_hit, double* clearance) {
    const int32_t P = a.P;
    AuditPlan pl;
    ARMOUR_TRY(make_plan(who, robot, W, O, obstacles, world_of_piece, a, verdict, &pl, mv));
    const int stride = mv ? RM_MOV_STRIDE : RM_OBS_STRIDE;
    std::vector<double> obs((size_t)W * O * stride);   // staged as the kernels stage them
    if (mv) stage_obstacles_moving(obstacles, mv->velocity, (size_t)W * O, obs.data());
    else stage_obstacles(obstacles, (size_t)W * O, obs.data());
    AuditMerge mg(P, clearance ? (size_t)pl.piece_off[P] : 0);
    for (int i = 0; i < P; i++) {
        const double* ob = obs.data() + (size_t)pl.world[i] * O * stride;
        const int64_t S = pl.piece_off[i + 1] - pl.piece_off[i];
        for (int64_t s = 0; s < S; s++) {
            double cl;
            const int state = mv ? item_state_moving(pl.rb, pl.pc, pl.t_world.data(), i, s, S, ob, O, clearance != nullptr, &cl)
                                 : item_state(pl.rb, pl.pc, i, s, S, ob, O, clearance != nullptr, &cl);
            if (clearance) mg.item_clear[(size_t)(pl.piece_off[i] + s)] = cl;
            audit_record(state, s, &mg.first_hit[i], &mg.undecided[i]);
            if (state == 1 && !clearance) break;
        }
    }
    finish_pieces(pl.pc, pl.piece_off, pl.order.data(), 1, P, mg, verdict, t_hit, clearance);
    return ARMOUR_OK;
}

extern "C" int armour_path_audit_host(const ArmourRobot* robot, int32_t W, int32_t O, const double* obstacles, int32_t P, const int32_t* world_of_piece,
                                      const double* q0, const double* qd0, const double* qdd0, const double* k, const double* k_range, double duration,
                                      const double* ta, const double* tb, const double* tube, double step, int32_t* verdict, double* t_hit,
                                      double* clearance) {
    return audit_on_host("armour_path_audit_host", robot, W, O, obstacles, nullptr, world_of_piece, {P, q0, qd0, qdd0, k, k_range, duration, ta, tb, tube, step},
                         verdict, t_hit, clearance);
}

extern "C" int armour_path_audit_moving_host(const ArmourRobot* robot, int32_t W, int32_t O, const double* obstacles, const double* velocity, int32_t P,
                                             const int32_t* world_of_piece, const double* t_world, const double* q0, const double* qd0, const double* qdd0,
                                             const double* k, const double* k_range, double duration, const double* ta, const double* tb, const double* tube,
                                             double step, int32_t* verdict, double* t_hit, double* clearance) {
    const Motion mv{velocity, t_world};
    return audit_on_host("armour_path_audit_moving_host", robot, W, O, obstacles, &mv, world_of_piece, {P, q0, qd0, qdd0, k, k_range, duration, ta, tb, tube, step},
                         verdict, t_hit, clearance);
}

// the device entry of both audits (mv null: the static one)
static int audit_on_device(const char* who, const ArmourRobot* robot, int32_t W, int32_t O, const double* obstacles, const Motion* mv, const int32_t* world_of_piece,
                           const PieceArgs& a, int32_t* verdict, double* t_hit, double* clearance, double* ms) {
    const int32_t P = a.P;
    // ---- arguments and the work list, before the device is touched
    AuditPlan pl;
    ARMOUR_TRY(make_plan(who, robot, W, O, obstacles, world_of_piece, a, verdict, &pl, mv));
    if (ms) *ms = 0.0;
    std::vector<int32_t> blk_world, blk_count;
    std::vector<int64_t> blk_item0;
    for (int i = 0; i < P;) {   // one run of pieces per world, cut into blocks of PA_BLOCK items
        int e = i;
        while (e < P && pl.world[e] == pl.world[i]) e++;
        for (int64_t x = pl.piece_off[i]; x < pl.piece_off[e]; x += PA_BLOCK) {
            blk_world.push_back(pl.world[i]);
            blk_item0.push_back(x);
            blk_count.push_back((int32_t)std::min<int64_t>(PA_BLOCK, pl.piece_off[e] - x));
        }
        i = e;
    }
    AuditMerge mg(P, clearance ? (size_t)pl.piece_off[P] : 0);
    if (P > 0) {
        // ---- the device
        if (!armour_device_available()) { armour_set_error("%s: no HIP device visible (there is no CPU path)", who); return ARMOUR_EDEVICE; }
        AuditDevice dev;
        PaPieces dpc;
        ARMOUR_TRY(dev.upload(pl.pc, P, pl.rb.n, pl.piece_off, mg, &dpc));
        DevBuf<double> d_obs, d_vel, d_tw;
        DevBuf<int32_t> d_blk_world, d_blk_count;
        DevBuf<int64_t> d_blk_item0;
        ARMOUR_TRY(d_obs.upload(obstacles, (size_t)W * O * ARMOUR_OBS_DOUBLES, dev.st));
        if (mv) {
            ARMOUR_TRY(d_vel.upload(mv->velocity, (size_t)W * O * 3, dev.st));
            ARMOUR_TRY(d_tw.upload(pl.t_world.data(), (size_t)P, dev.st));
        }
        ARMOUR_TRY(d_blk_world.upload(blk_world.data(), blk_world.size(), dev.st));
        ARMOUR_TRY(d_blk_count.upload(blk_count.data(), blk_count.size(), dev.st));
        ARMOUR_TRY(d_blk_item0.upload(blk_item0.data(), blk_item0.size(), dev.st));
        ARMOUR_TRY(dev.ev.record_start(dev.st));
        if (!blk_world.empty() && mv) {
            const size_t lds = (size_t)O * RM_MOV_STRIDE * sizeof(double);
            hipLaunchKernelGGL(path_audit_moving_kernel, dim3((unsigned)blk_world.size()), dim3(PA_BLOCK), lds, dev.st, pl.rb, dpc, d_blk_world, d_blk_item0,
                               d_blk_count, dev.item_piece, dev.piece_off, d_obs, d_vel, d_tw, O, dev.first_hit, dev.undecided, clearance ? dev.clear.p : nullptr);
            HIPCHK(hipGetLastError());
        } else if (!blk_world.empty()) {
            const size_t lds = (size_t)O * RM_OBS_STRIDE * sizeof(double);
            hipLaunchKernelGGL(path_audit_kernel, dim3((unsigned)blk_world.size()), dim3(PA_BLOCK), lds, dev.st, pl.rb, dpc, d_blk_world, d_blk_item0,
                               d_blk_count, dev.item_piece, dev.piece_off, d_obs, O, dev.first_hit, dev.undecided, clearance ? dev.clear.p : nullptr);
            HIPCHK(hipGetLastError());
        }
        ARMOUR_TRY(dev.download(&mg, ms));
    }
    finish_pieces(pl.pc, pl.piece_off, pl.order.data(), 1, P, mg, verdict, t_hit, clearance);
    return ARMOUR_OK;
}

extern "C" int armour_path_audit(const ArmourRobot* robot, int32_t W, int32_t O, const double* obstacles, int32_t P, const int32_t* world_of_piece,
                                 const double* q0, const double* qd0, const double* qdd0, const double* k, const double* k_range, double duration,
                                 const double* ta, const double* tb, const double* tube, double step, int32_t* verdict, double* t_hit, double* clearance,
                                 double* ms) {
    return audit_on_device("armour_path_audit", robot, W, O, obstacles, nullptr, world_of_piece, {P, q0, qd0, qdd0, k, k_range, duration, ta, tb, tube, step}, verdict,
                           t_hit, clearance, ms);
}

extern "C" int armour_path_audit_moving(const ArmourRobot* robot, int32_t W, int32_t O, const double* obstacles, const double* velocity, int32_t P,
                                        const int32_t* world_of_piece, const double* t_world, const double* q0, const double* qd0, const double* qdd0,
                                        const double* k, const double* k_range, double duration, const double* ta, const double* tb, const double* tube,
                                        double step, int32_t* verdict, double* t_hit, double* clearance, double* ms) {
    const Motion mv{velocity, t_world};
    return audit_on_device("armour_path_audit_moving", robot, W, O, obstacles, &mv, world_of_piece, {P, q0, qd0, qdd0, k, k_range, duration, ta, tb, tube, step},
                           verdict, t_hit, clearance, ms);
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
    fill_pieces(rb.n, {P, q0, qd0, qdd0, k, k_range, duration, ta, tb, nullptr, step}, &pc);
    for (int p = 0; p < P; p++) items[p] = (int64_t)std::fmin(piece_intervals(rb, pc, p), 9e18);
    return ARMOUR_OK;
}
