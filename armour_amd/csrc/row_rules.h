// What a constraint row means, once: its bounds (RT/NLPclass.cu:87-165), the test "outside the finalize_solution slack" (RT/NLPclass.cu:422-538;
// ARMTD mode CMP/NLPclass.cu:391-402) and the violation record of armour_eval_violations with its reduction tree.  Host and device read the same
// functions (-ffp-contract=off: the same bits), so the contracts culled record = full record, sweep record = armour_eval_violations and
// host solver = device solver = culled solver hold by construction.  Needs nothing of the library but the public structs.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/armour_hip.h"

namespace slv {
// Row order of g: row0 torque rows (t * n + j; none in ARMTD mode or with input constraints off), Q collision rows, 4 n limit rows (min
// position, max position, min velocity, max velocity).  Filled from the handle by armour_row_rule (common.h).
struct RowRule {
    int n, T, m, row0, Q;
    int n_checked;   // collision rows the verdict re-checks: all Q, ARMTD mode the first (n - 1) links' (armour_checked_collision_rows)
    double torque_slack, collision_slack;
};
// what the bounds are made of besides the torque radii (armour_row_limits, common.h)
struct RowLimits {
    double torque_limits[ARMOUR_MAX_FACTORS], lb[ARMOUR_MAX_FACTORS], ub[ARMOUR_MAX_FACTORS], speed[ARMOUR_MAX_FACTORS];
    double qe, qde;   // the ultimate bound on the position / velocity error
};
// g_l, g_u of row r.  torque_radius: the problem's radii [n][T] (read for a torque row only).
__host__ __device__ inline void row_bounds(const RowRule& R, const RowLimits& L, int r, const double* torque_radius, double* l, double* u) {
    if (r < R.row0) {   // RT/NLPclass.cu:117
        const int t = r / R.n, j = r - t * R.n;
        const double tr = torque_radius[j * R.T + t];
        *l = -L.torque_limits[j] + tr; *u = L.torque_limits[j] - tr;
    } else if (r < R.row0 + R.Q) { *l = -1e19; *u = 0; }
    else {
        const int e = r - R.row0 - R.Q, rep = e / R.n, i = e - rep * R.n;
        if (rep < 2) { *l = L.lb[i] + L.qe; *u = L.ub[i] - L.qe; }
        else { *l = -L.speed[i] + L.qde; *u = L.speed[i] - L.qde; }
    }
}
// finalize_solution rejects row r at value v: beyond its bounds by more than the slack of its class (torque, checked collision, limit = 0).
// A collision row at or behind n_checked is never rejected.
__host__ __device__ inline bool outside_slack(const RowRule& R, int r, double v, double l, double u) {
    const int ic = r - R.row0 - R.n_checked;   // >= 0: behind the re-checked collision rows
    const double slack = r < R.row0 ? R.torque_slack : ic < 0 ? R.collision_slack : 0.0;
    return (ic < 0 || ic >= R.Q - R.n_checked) && (v < l - slack || v > u + slack);
}
// LDS of the record's tree: the 256 threads' partial records of C evaluation points side by side
template <int C> struct ViolShared {
    double l1[C][256], worst[C][256];
    int wrow[C][256], nv[C][256], no[C][256];
};
// One thread's part of an ArmourViolation.  Thread t of 256 takes the rows r = t (mod 256) in ascending order; tree_reduce combines the 256
// parts in a fixed tree: the record depends on (problem, k) alone, l1 included.
struct ViolPartial {
    double l1 = 0.0, worst = 0.0;
    int wrow = -1, nv = 0, no = 0;
    __host__ __device__ inline void take(const RowRule& R, int r, double v, double l, double u) {
        const double viol = fmax(0.0, fmax(l - v, v - u));
        l1 += viol;
        if (viol > 0.0) nv++;
        if (viol > worst) { worst = viol; wrow = r; }
        if (outside_slack(R, r, v, l, u)) no++;
    }
    template <int C>
    __host__ __device__ inline void store(ViolShared<C>& sh, int c, int tid) const {
        sh.l1[c][tid] = l1; sh.worst[c][tid] = worst; sh.wrow[c][tid] = wrow; sh.nv[c][tid] = nv; sh.no[c][tid] = no;
    }
    // one step of the tree: entry tid + s joins entry tid.  The larger violation wins; among equals the lower row.
    template <int C>
    __host__ __device__ static inline void tree_step(ViolShared<C>& sh, int c, int tid, int s) {
        sh.l1[c][tid] += sh.l1[c][tid + s]; sh.nv[c][tid] += sh.nv[c][tid + s]; sh.no[c][tid] += sh.no[c][tid + s];
        const double ow = sh.worst[c][tid + s];
        const int orow = sh.wrow[c][tid + s];
        if (ow > sh.worst[c][tid] || (ow == sh.worst[c][tid] && orow >= 0 && (sh.wrow[c][tid] < 0 || orow < sh.wrow[c][tid]))) { sh.worst[c][tid] = ow; sh.wrow[c][tid] = orow; }
    }
#ifdef __HIPCC__
    // the block's 256 threads, each with its C partial records: afterwards entry 0 of every record holds the whole
    template <int C>
    __device__ static inline void tree_reduce(ViolShared<C>& sh, const ViolPartial (&p)[C], int tid) {
#pragma unroll
        for (int c = 0; c < C; c++) p[c].store(sh, c, tid);
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) {
#pragma unroll
                for (int c = 0; c < C; c++) tree_step(sh, c, tid, s);
            }
            __syncthreads();
        }
    }
#endif
    // the record of evaluation point c after the tree
    template <int C>
    __host__ __device__ static inline ArmourViolation finish(const ViolShared<C>& sh, int c) {
        ArmourViolation o;
        o.l1_violation = sh.l1[c][0]; o.worst = sh.worst[c][0]; o.worst_row = sh.wrow[c][0]; o.n_violated = sh.nv[c][0];
        o.n_outside_slack = sh.no[c][0]; o.feasible = sh.no[c][0] == 0 ? 1 : 0;
        return o;
    }
};
}  // namespace slv
