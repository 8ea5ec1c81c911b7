// armour_sweep: S candidate trajectory parameters k of the SAME problems judged in one go -- the row test of armour_eval_violations and the cost of
// armour_eval_f per candidate, and the best safe candidate per problem picked on the device.
//
// Why: armour_solve is a local method (the reference's too: RT/NLPclass.cu:193-198 marks its start at 0 as a weakness).  When a solve comes back
// infeasible a caller wants to know whether ANY safe plan exists in this reach set, and where to start the solver again.  S calls of the culled
// row test answer that with three launches each and read every table S times; this unit answers it with two launches whatever S.
//
// Layout.  A block serves one problem and a compile-time tile of C candidates (C k-power tables in LDS).  It walks the rows the culled row test
// walks -- the torque rows, the LISTED collision rows (relevance.hip: ~2 % of them), the limit rows -- and for each row reads the row's table
// entries ONCE (keys and coefficients of a torque row; link-PZ monomials and packed planes of a listed collision row; the closed form of a
// limit row) and evaluates them for its C candidates.  The arithmetic is that of p2_sparse.h's sparse_torque_row / sparse_collision_row and of
// p2_tiles.h's limit_block, statement for statement with the candidate index added, so every g is the fused evaluation's bit for bit.
// The record is row_rules.h's, C of them side by side: thread t of the 256 owns the rows r = t (mod 256) in ascending order, so l1_violation
// is the row test's sum bit for bit as well.  The C partial records of a thread live in registers (every loop over the candidates has a
// compile-time trip count; nothing is indexed by a run-time candidate number), and no g is ever stored: there is no scratch buffer that
// grows with S.
#include <cmath>
#include <vector>

#include "p2_sparse.h"
#include "solver_common.h"

using namespace p2;

namespace {

// Candidates per block (-DARMOUR_SWEEP_TILE=c builds another).  Compiler's resource report, gfx950: C = 2: 116 VGPRs, 4 waves per SIMD; C = 4: 150
// VGPRs, 3 waves per SIMD; C = 8: 256 VGPRs + 2 AGPRs, 1 wave per SIMD -- no scratch in any of them.  Measured: a lone problem is
// fastest with 2 (more, shorter blocks), a batch of 128 with 8 (tables read half as often); 4 is within 1.5x of the best at both ends.
#ifndef ARMOUR_SWEEP_TILE
#define ARMOUR_SWEEP_TILE 4
#endif
constexpr int kTile = ARMOUR_SWEEP_TILE;
constexpr int kPlaneBatch = 6;   // planes of a listed row requested together, as sparse_collision_row does

struct SweepArgs {
    P2Tables tb;
    slv::RowRule rule;
    SparseList sl;                                // the relevance lists: rows [B][Q] ascending, their packed plane entries
    const int* rows_res; const int* count_res;    // the same rows by (row index mod 256): [B][256][ceil(Q / 256)] | [B][256]
    const double* lo; const double* hi;           // bounds [B][m]
    const double* k;                              // candidates [S][n], or [B][S][n] with k_pstride = S * n
    long long k_pstride;
    int S, strideT;
    const double* coef;                           // [B][4][n]: the plan point's c0, c1, c2 (armour_plan_coeffs) and q_des
    int continuous_mask;
    double t_plan, cost_scale;
    ArmourSweepRecord* out;                       // [B][S]
};

// g of the limit row of joint i in block blk (0 .. 3: the n rows of min position, max position, min velocity, max velocity) of problem b at the joint's parameter kj:
// bez::select_extrema on the four values p2_tiles.h's limit_block takes (there one lane per value and one wave per path family, here one
// thread for all four: the same bezier.h calls on the same arguments); ARMTD mode: cacc::joint_extrema
__device__ inline double limit_row_g(const P2Tables& tb, int b, int i, int blk, double kj) {
    const int n = tb.n;
    const double* bz = tb.bez + (size_t)b * 3 * n;
    if (tb.mode == ARMOUR_MODE_ARMTD) {
        const cacc::Extrema e = cacc::joint_extrema(bz[i], bz[n + i], bz[2 * n + i] * kj);
        return blk == 0 ? e.q_min.v : blk == 1 ? e.q_max.v : blk == 2 ? e.qd_min.v : e.qd_max.v;
    }
    const bool vel = blk >= 2;
    const double q0 = bz[i], a = bz[n + i], bb = bz[2 * n + i], ka = tb.k_range[i] * kj;
    double e2, e3;
    if (!vel) bez::q_stationary(a, bb, ka, &e2, &e3); else bez::qd_stationary(a, bb, ka, &e2, &e3);
    const double v1 = vel ? bez::qd_des(q0, a, bb, ka, 0.0) : bez::q_des(q0, a, bb, ka, 0.0);
    const double v2 = vel ? bez::qd_des(q0, a, bb, ka, e2) : bez::q_des(q0, a, bb, ka, e2);
    const double v3 = vel ? bez::qd_des(q0, a, bb, ka, e3) : bez::q_des(q0, a, bb, ka, e3);
    const double v4 = vel ? bez::qd_des(q0, a, bb, ka, 1.0) : bez::q_des(q0, a, bb, ka, 1.0);
    double mn, mx;
    int mnId, mxId;
    bez::select_extrema(v1, v2, v3, v4, e2, e3, &mn, &mx, &mnId, &mxId);
    const double v = (blk & 1) ? mx : mn;
    return vel ? v / tb.duration : v;
}

template <int C>
__global__ __launch_bounds__(256) void armour_sweep_kernel(SweepArgs a) {
    __shared__ KPow kp[C];
    __shared__ slv::ViolShared<C> sh;
    __shared__ double s_sq[C][slv::NV];
    const P2Tables& tb = a.tb;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int s0 = blockIdx.x * C;
    const int n = tb.n, m = tb.m, row0 = tb.row0, Q = tb.Q;
    // the tile's points; a tile past the end repeats the last candidate (evaluated, not written)
    const double* kb = a.k + (size_t)b * a.k_pstride;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const int s = min(s0 + c, a.S - 1);
        fill_kpow(kp[c], tid < n ? kb[(size_t)s * n + tid] : 0.0, n);
    }
    __syncthreads();
    const double* lo = a.lo + (size_t)b * m;
    const double* hi = a.hi + (size_t)b * m;
    slv::ViolPartial p[C];   // one partial record per candidate
    // row r with the values v[c] of the C candidates
    auto take = [&](int r, const double* v) {
        const double l = lo[r], u = hi[r];
#pragma unroll
        for (int c = 0; c < C; c++) p[c].take(a.rule, r, v[c], l, u);
    };
    // ---- torque rows r = t * n + j: sparse_torque_row's sums (value only), the row's keys and coefficients read once
    for (int r = tid; r < row0; r += 256) {
        const int t = r / n, j = r - t * n;
        const size_t idx = ((size_t)b * n + j) * tb.T + t;
        const int cnt = min(tb.tq_count[idx], a.strideT);
        double cen[C];
        const double cen0 = tb.tq_center[idx];
#pragma unroll
        for (int c = 0; c < C; c++) cen[c] = cen0;
        const uint32_t* keys = tb.tq_keys + idx * tb.capT;
        const double* co = tb.tq_coeff + idx * tb.capT;
        const int cmax = cnt > 0 ? cnt - 1 : 0;
#pragma unroll 1
        for (int m0 = 0; m0 < cnt; m0 += 4) {
            uint32_t key[4]; double cf[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { const int mo = min(m0 + u, cmax); key[u] = keys[mo]; cf[u] = co[mo]; }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (m0 + u < cnt) {
#pragma unroll
                    for (int c = 0; c < C; c++) {
                        double f[ARMOUR_MAX_FACTORS];
                        mono_factors(kp[c], key[u], n, f);
                        cen[c] += mono_product(cf[u], f);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);   // one monomial's C x n table reads in flight at a time: hoisted together they cost 200 VGPRs
            }
        }
        const double ind = tb.tq_indep[idx];
        double v[C];
#pragma unroll
        for (int c = 0; c < C; c++) v[c] = interval_center(cen[c], ind);
        take(r, v);
    }
    // ---- the listed collision rows of this thread's residue class, ascending: sparse_collision_row<false>'s arithmetic
    {
        const int per = (Q + 255) / 256;
        const int* mine = a.rows_res + ((size_t)b * 256 + tid) * per;
        const int cntc = a.count_res[(size_t)b * 256 + tid];
        const int* rows = a.sl.rows + (size_t)b * Q;
        const int nlist = a.sl.count[b];
        const int O = tb.O, JT = tb.J * tb.T;
        const double* src0 = a.sl.packed + a.sl.pack_off[2 * b];
        const size_t stride = (size_t)a.sl.pack_off[2 * b + 1];
        const unsigned long long live = ~tb.plane_skip[b] & ((1ull << ARMOUR_NPLANES) - 1ull);
        const int nlive = __popcll(live);
        for (int ii = 0; ii < cntc; ii++) {
            const int q = mine[ii];
            // the row's position in the ascending list (its packed plane entries are stored by that position)
            int i = 0;
            { int hi_ = nlist - 1; while (i < hi_) { const int mid = (i + hi_) >> 1; if (rows[mid] < q) i = mid + 1; else hi_ = mid; } }
            const int lt = q / O;
            const size_t idx = (size_t)b * JT + lt;
            const int cnt = min(tb.link_count[idx], tb.capL);
            double acc[C][3];
            {
                const double c0 = tb.link_center[idx * 3 + 0], c1 = tb.link_center[idx * 3 + 1], c2 = tb.link_center[idx * 3 + 2];
#pragma unroll
                for (int c = 0; c < C; c++) { acc[c][0] = c0; acc[c][1] = c1; acc[c][2] = c2; }
            }
            const uint32_t* kk_ = tb.link_keys + idx * tb.capL;
            const double* cc = tb.link_coeff + idx * tb.capL * 3;
            const int cmax = cnt > 0 ? cnt - 1 : 0;
#pragma unroll 1
            for (int m0 = 0; m0 < cnt; m0 += 2) {
                uint32_t key[2]; double c3[2][3];
#pragma unroll
                for (int u = 0; u < 2; u++) { const int mo = min(m0 + u, cmax); key[u] = kk_[mo]; c3[u][0] = cc[mo * 3]; c3[u][1] = cc[mo * 3 + 1]; c3[u][2] = cc[mo * 3 + 2]; }
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    if (m0 + u < cnt) {
#pragma unroll
                        for (int c = 0; c < C; c++) {   // (p2_tiles.h mono_factors / mono_product: mono_all<false>'s product, the key decoded once for the three axes)
                            double f[ARMOUR_MAX_FACTORS];
                            mono_factors(kp[c], key[u], n, f);
#pragma unroll
                            for (int e = 0; e < 3; e++) acc[c][e] += mono_product(c3[u][e], f);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);   // (as in the torque rows)
                }
            }
            double x[C][3], max_elt[C];
            {
                const double i0 = tb.link_indep[idx * 3 + 0], i1 = tb.link_indep[idx * 3 + 1], i2 = tb.link_indep[idx * 3 + 2];
#pragma unroll
                for (int c = 0; c < C; c++) {
                    x[c][0] = interval_center(acc[c][0], i0); x[c][1] = interval_center(acc[c][1], i1); x[c][2] = interval_center(acc[c][2], i2);
                    max_elt[c] = -100000000.0;
                }
            }
            const double* src = src0 + i;
#pragma unroll 1
            for (int j0 = 0; j0 < nlive; j0 += kPlaneBatch) {
                PlaneVals pv[kPlaneBatch];
#pragma unroll
                for (int u = 0; u < kPlaneBatch; u++) {
                    const int j = min(j0 + u, nlive - 1);
                    pv[u].a0 = src[(size_t)(j * 5 + 0) * stride]; pv[u].a1 = src[(size_t)(j * 5 + 1) * stride]; pv[u].a2 = src[(size_t)(j * 5 + 2) * stride];
                    pv[u].dd = src[(size_t)(j * 5 + 3) * stride]; pv[u].dl = src[(size_t)(j * 5 + 4) * stride];
                }
#pragma unroll
                for (int u = 0; u < kPlaneBatch; u++) {
                    const bool nz = j0 + u < nlive && ((pv[u].a0 != 0.0) | (pv[u].a1 != 0.0) | (pv[u].a2 != 0.0));
#pragma unroll
                    for (int c = 0; c < C; c++) {
                        const double dot = pv[u].a0 * x[c][0] + pv[u].a1 * x[c][1] + pv[u].a2 * x[c][2];
                        const double pos_res = nz ? dot - (pv[u].dd + pv[u].dl) : -100000000.0;
                        const double neg_res = nz ? -dot - (-pv[u].dd + pv[u].dl) : -100000000.0;
                        const bool c1 = pos_res > max_elt[c];
                        max_elt[c] = c1 ? pos_res : max_elt[c];
                        const bool c2 = neg_res > max_elt[c];
                        max_elt[c] = c2 ? neg_res : max_elt[c];
                    }
                }
            }
            double v[C];
#pragma unroll
            for (int c = 0; c < C; c++) v[c] = -max_elt[c];
            take(row0 + q, v);
        }
    }
    // ---- limit rows
    {
        const int lim0 = row0 + Q;
        for (int r = lim0 + ((tid - lim0) & 255); r < m; r += 256) {
            const int rl = r - lim0, blk = rl / n, i = rl - blk * n;
            double v[C];
#pragma unroll
            for (int c = 0; c < C; c++) v[c] = limit_row_g(tb, b, i, blk, kp[c].pw[i][1]);
            take(r, v);
        }
    }
    slv::ViolPartial::tree_reduce(sh, p, tid);
    // ---- one thread per candidate: the record and the cost (armour_eval_f's)
    if (tid < C && s0 + tid < a.S) {
        const int c = tid;
        ArmourSweepRecord o;
        o.v = slv::ViolPartial::finish(sh, c);
        const double* cf = a.coef + (size_t)b * 4 * n;
        double* sq = s_sq[c];   // (LDS: indexed by a run-time joint number)
        for (int i = 0; i < n; i++) {
            const double qp = slv::plan_point(tb.mode, cf[i], cf[n + i], cf[2 * n + i], tb.k_range[i], kp[c].pw[i][1], a.t_plan);
            const double e = ((a.continuous_mask >> i) & 1) ? slv::wrap_to_pi(cf[3 * n + i] - qp) : (cf[3 * n + i] - qp);
            sq[i] = e * e;
        }
        o.cost = slv::cost_from_sq(n, a.continuous_mask, sq, a.cost_scale);
        a.out[(size_t)b * a.S + s0 + c] = o;
    }
}

// best[b]: the feasible candidate of the smallest cost, the lowest index among equals; -1 if none.  One block per problem; thread t scans the
// candidates t, t + 256, ... in ascending order, a tree combines.
__global__ __launch_bounds__(256) void armour_sweep_best_kernel(const ArmourSweepRecord* __restrict__ rec, int S, int* __restrict__ best) {
    __shared__ double s_c[256];
    __shared__ int s_i[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    double bc = 0.0;
    int bi = -1;
    for (int s = tid; s < S; s += 256) {
        const ArmourSweepRecord& r = rec[(size_t)b * S + s];
        if (r.v.feasible == 1 && (bi < 0 || r.cost < bc)) { bc = r.cost; bi = s; }
    }
    s_c[tid] = bc; s_i[tid] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const double oc = s_c[tid + s];
            const int oi = s_i[tid + s];
            if (oi >= 0 && (s_i[tid] < 0 || oc < s_c[tid] || (oc == s_c[tid] && oi < s_i[tid]))) { s_c[tid] = oc; s_i[tid] = oi; }
        }
        __syncthreads();
    }
    if (tid == 0) best[b] = s_i[0];
}

}  // namespace

extern "C" int armour_sweep_tile(void) { return kTile; }

extern "C" int armour_sweep(ArmourPlanner* h, int32_t S, const double* k_cand, int32_t per_problem, ArmourSweepRecord* records, int32_t* best, double* ms) {
    if (!k_cand) { armour_set_error("null argument"); return ARMOUR_EINVAL; }
    NEED_READY(h);
    if (S < 1 || S > ARMOUR_SWEEP_MAX_CANDIDATES) { armour_set_error("armour_sweep: S = %d is outside [1, %d]", S, ARMOUR_SWEEP_MAX_CANDIDATES); return ARMOUR_EINVAL; }
    if (per_problem != 0 && per_problem != 1) { armour_set_error("armour_sweep: per_problem is 0 or 1"); return ARMOUR_EINVAL; }
    const size_t B = (size_t)h->B, n = (size_t)h->n;
    const size_t nk = (per_problem ? B : 1) * (size_t)S * n;
    // the row lists say "never violated for a k of [-1, 1]^n": a point outside the box cannot be judged on them
    for (size_t i = 0; i < nk; i++)
        if (!(std::fabs(k_cand[i]) <= 1.0)) { armour_set_error("armour_sweep: k_cand[%zu] = %g is outside [-1, 1]", i, k_cand[i]); return ARMOUR_EINVAL; }
    const int strideT = h->max_torque > 0 ? h->max_torque : 1;
    if (strideT > 32 * P2_TQ_ROUNDS) { armour_set_error("torque PZ with %d monomials exceeds the P2 kernel's %d", strideT, 32 * P2_TQ_ROUNDS); return ARMOUR_ECAPACITY; }
    HIPCHK(hipSetDevice(h->device));
    int rc = armour_upload_bounds(h);
    if (rc != ARMOUR_OK) return rc;
    if ((rc = armour_relevance_build(h, false)) != ARMOUR_OK) return rc;
    // one device block: the candidates | the cost's coefficients | the records | best
    const size_t off_coef = nk * sizeof(double);
    const size_t off_rec = off_coef + B * 4 * n * sizeof(double);
    const size_t off_best = off_rec + B * (size_t)S * sizeof(ArmourSweepRecord);
    const size_t bytes = off_best + B * sizeof(int);
    ARMOUR_TRY(h->d_sweep.reserve(bytes));
    unsigned char* const blk = h->d_sweep;
    std::vector<double> coef(B * 4 * n);
    for (size_t b = 0; b < B; b++)
        for (size_t i = 0; i < n; i++) {
            double c[3];
            armour_plan_coeffs(h, b * n + i, c);
            coef[(b * 4 + 0) * n + i] = c[0]; coef[(b * 4 + 1) * n + i] = c[1]; coef[(b * 4 + 2) * n + i] = c[2];
            coef[(b * 4 + 3) * n + i] = h->h_qdes[b * n + i];
        }
    HIPCHK(hipMemcpyAsync(blk, k_cand, nk * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(blk + off_coef, coef.data(), coef.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    SweepArgs a;
    a.tb = armour_make_tables(h);
    a.rule = armour_row_rule(h);
    a.sl = SparseList{h->rel.rows, h->rel.count, h->rel.packed, h->rel.pack_off};
    a.rows_res = h->rel.extra; a.count_res = h->rel.count + B;
    a.lo = h->d_bounds; a.hi = h->d_bounds + B * h->m;
    a.k = reinterpret_cast<const double*>(blk); a.k_pstride = per_problem ? (long long)S * (long long)n : 0;
    a.S = S; a.strideT = strideT;
    a.coef = reinterpret_cast<const double*>(blk + off_coef);
    a.continuous_mask = h->continuous_mask();
    a.t_plan = h->params.t_plan; a.cost_scale = h->params.cost_scale;
    a.out = reinterpret_cast<ArmourSweepRecord*>(blk + off_rec);
    int* d_best = reinterpret_cast<int*>(blk + off_best);
    EventPair ev;
    ARMOUR_TRY(ev.record_start(h->stream));
    hipLaunchKernelGGL(armour_sweep_kernel<kTile>, dim3((S + kTile - 1) / kTile, h->B), dim3(256), 0, h->stream, a);
    hipLaunchKernelGGL(armour_sweep_best_kernel, dim3(h->B), dim3(256), 0, h->stream, a.out, S, d_best);
    HIPCHK(hipGetLastError());
    ARMOUR_TRY(ev.record_stop(h->stream));
    if (records) HIPCHK(hipMemcpyAsync(records, blk + off_rec, B * (size_t)S * sizeof(ArmourSweepRecord), hipMemcpyDeviceToHost, h->stream));
    if (best) HIPCHK(hipMemcpyAsync(best, d_best, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ms ? ev.elapsed_ms(ms) : ARMOUR_OK;
}
