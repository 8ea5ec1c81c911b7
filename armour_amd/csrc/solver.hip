// armour_solve: the NLP solve of one planning iteration on top of the device callbacks.
//
// Replaces, for this library, what the reference delegates to IPOPT (RT/armour_main.cu:237-304: OptimizeTNLP with
// tol 1e-4, a wall-time limit, L-BFGS Hessian, start x = 0) and armtd_NLP::finalize_solution
// (RT/NLPclass.cu:422-538).  IPOPT / HSL are not available here, so this is a from-scratch solver sized for the
// problem ARMOUR actually poses: n = 7 variables in [-1,1], an exactly quadratic cost (q(t_plan) is affine in k, so
// the Hessian is the constant diagonal 2*scale*(dq/dk)^2) and m ~ 1e4 inequality rows whose values and dense Jacobian
// come from ONE fused device launch per iterate for all B problems of the handle:
//
//   SQP:  d = argmin grad_f.d + 1/2 d'Hd   s.t.  g_l <= g + J d <= g_u,  -1 <= x + d <= 1      (dense QP, n = 7)
//         L1-merit backtracking line search (trial points need eval_g only), start x = 0
//   QP:   Goldfarb-Idnani dual active-set method; with n <= 7 the operators H = G^-1(I - N N*) and
//         N* = (N'G^-1N)^-1 N'G^-1 are re-formed from the <= n active normals at every step instead of being
//         updated by Givens rotations.
//
// g and jac stay on the device: after each evaluation armour_solve_scan_kernel (below) hands the host the L1 violation,
// the rows the QP can see and, at the end, finalize_solution's verdict.  The 7-variable QPs run on the host.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "bezier.h"
#include "common.h"
#include "solver_common.h"
#include "solver_device.h"

using slv::NV;
using slv::SolveRow;

namespace {

constexpr double kInf = 1e300;
using Clock = std::chrono::steady_clock;

// ---- tiny dense helpers (q <= NV) ----
// solve M y = rhs for symmetric positive definite M (q x q, row-major NV stride) by Cholesky; false if not SPD
// Divisions are taken once per pivot: every other use multiplies by the stored reciprocal (the device form runs this chain on one
// wave, where a dependent fp64 division costs ~40x a multiplication; both forms use the same expressions, so they agree bit for bit).
bool spd_solve(const double* M, int q, const double* rhs, double* y) {
    double L[NV][NV], inv[NV];
    for (int i = 0; i < q; i++)
        for (int j = 0; j <= i; j++) {
            double s = M[i * NV + j];
            for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
            if (i == j) {
                if (s <= 1e-14 * std::fabs(M[i * NV + i]) || s <= 0) return false;
                L[i][i] = std::sqrt(s);
                inv[i] = 1.0 / L[i][i];
            } else {
                L[i][j] = s * inv[j];
            }
        }
    double t[NV];
    for (int i = 0; i < q; i++) {
        double s = rhs[i];
        for (int k = 0; k < i; k++) s -= L[i][k] * t[k];
        t[i] = s * inv[i];
    }
    for (int i = q - 1; i >= 0; i--) {
        double s = t[i];
        for (int k = i + 1; k < q; k++) s -= L[k][i] * y[k];
        y[i] = s * inv[i];
    }
    return true;
}

// One inequality a'x >= b of the QP.  Rows come from three sources: upper sides (-J_i d >= g_i - hi_i), lower sides
// (J_i d >= lo_i - g_i) and the variable bounds.
struct QpRow {
    double a[NV];
    double b;
};

struct QpResult {
    double x[NV];
    double max_mult;  // largest multiplier (for the merit penalty)
    int iterations;
    bool feasible;
    // what the active-set method did on the way (armour_debug_qp_elastic reports them; nothing in the solver reads them): rows dropped from the
    // active set, those of them that were not its last row (the factor's rows behind them move up), rows excluded, and the active rows at the end
    int dropped, dropped_mid, excluded, active;
};

// Goldfarb-Idnani for  min 1/2 x'Gx + g0'x  s.t.  a_i'x >= b_i,  G = diag(Gd) > 0.
// box_rows = 2 n: the LAST 2 n rows are the variables' box, lower then upper bound of variable 0, 1, ... (what gather_rows appends); 0: no such promise.
QpResult solve_qp(int n, const double* Gd, const double* g0, const std::vector<QpRow>& rows, int max_iter = slv::kQpMaxSteps, int box_rows = 0) {
    QpResult res;
    res.iterations = 0; res.feasible = true; res.max_mult = 0;
    res.dropped = res.dropped_mid = res.excluded = res.active = 0;
    double x[NV], invG[NV];
    for (int j = 0; j < n; j++) { invG[j] = 1.0 / Gd[j]; x[j] = -g0[j] * invG[j]; }
    if (box_rows == 2 * n && (int)rows.size() >= box_rows) {   // the box-clipped minimiser first (solver_common.h)
        const int m0 = (int)rows.size() - box_rows;
        double lo[NV], hi[NV], d[NV];
        for (int j = 0; j < n; j++) { lo[j] = rows[m0 + 2 * j].b; hi[j] = -rows[m0 + 2 * j + 1].b; }
        const double mm = slv::box_clipped_step(n, Gd, invG, g0, lo, hi, d);
        bool ok = true;
        for (int i = 0; i < (int)rows.size() && ok; i++) {
            double s = -rows[i].b;
            for (int j = 0; j < n; j++) s += rows[i].a[j] * d[j];
            if (s < -1e-7) ok = false;
        }
        if (ok) {
            for (int j = 0; j < n; j++) res.x[j] = d[j];
            res.max_mult = mm;
            return res;
        }
    }
    int A[NV];       // active row ids
    double u[NV + 1];  // multipliers of the active rows (+ the entering one)
    int q = 0;
    const int m = (int)rows.size();
    std::vector<char> is_active(m, 0), excluded(m, 0);
    for (;;) {
        // most violated inactive row
        int p = -1;
        double worst = -1e-10;
        for (int i = 0; i < m; i++) {
            if (is_active[i] || excluded[i]) continue;
            double s = -rows[i].b;
            for (int j = 0; j < n; j++) s += rows[i].a[j] * x[j];
            // scale-free test: violation relative to the row norm
            if (s < worst) { worst = s; p = i; }
        }
        if (p < 0) break;
        if (++res.iterations > max_iter) { res.feasible = false; break; }
        const double* np = rows[p].a;
        double up = 0.0;
        bool added = false;
        for (int guard = 0; guard < 4 * NV + 8 && !added; guard++) {
            // r = N* np,  z = G^-1 (np - N r)
            double r[NV] = {0}, z[NV];
            if (q > 0) {
                double M[NV * NV], rhs[NV];
                for (int i = 0; i < q; i++) {
                    for (int k = 0; k <= i; k++) {
                        double s = 0;
                        for (int j = 0; j < n; j++) s += rows[A[i]].a[j] * rows[A[k]].a[j] * invG[j];
                        M[i * NV + k] = s; M[k * NV + i] = s;
                    }
                    double s = 0;
                    for (int j = 0; j < n; j++) s += rows[A[i]].a[j] * np[j] * invG[j];
                    rhs[i] = s;
                }
                if (!spd_solve(M, q, rhs, r)) { excluded[p] = 1; res.excluded++; break; }  // dependent active set: skip this row
            }
            double zz = 0, znp = 0;
            for (int j = 0; j < n; j++) {
                double s = np[j];
                for (int i = 0; i < q; i++) s -= rows[A[i]].a[j] * r[i];
                z[j] = s * invG[j];
                zz += z[j] * z[j];
                znp += z[j] * np[j];
            }
            // step lengths
            double t1 = kInf;
            int l = -1;
            for (int i = 0; i < q; i++)
                if (r[i] > 1e-14 && u[i] / r[i] < t1) { t1 = u[i] / r[i]; l = i; }
            double sp = -rows[p].b;
            for (int j = 0; j < n; j++) sp += np[j] * x[j];
            double t2 = kInf;
            if (zz > 1e-24 && znp > 1e-16) t2 = -sp / znp;
            if (t2 < 0) t2 = 0;
            const double t = t1 < t2 ? t1 : t2;
            if (t >= kInf) { res.feasible = false; break; }
            if (t2 >= kInf) {  // dual step only, drop the blocking row
                for (int i = 0; i < q; i++) u[i] -= t * r[i];
                up += t;
                is_active[A[l]] = 0;
                res.dropped++; if (l < q - 1) res.dropped_mid++;
                for (int i = l; i < q - 1; i++) { A[i] = A[i + 1]; u[i] = u[i + 1]; }
                q--;
                continue;
            }
            for (int j = 0; j < n; j++) x[j] += t * z[j];
            for (int i = 0; i < q; i++) u[i] -= t * r[i];
            up += t;
            if (t == t2) {  // full step: the row becomes active
                if (q >= n) { res.feasible = false; break; }
                A[q] = p; u[q] = up; q++;
                is_active[p] = 1;
                added = true;
            } else {        // partial step: drop the blocking row and try again
                is_active[A[l]] = 0;
                res.dropped++; if (l < q - 1) res.dropped_mid++;
                for (int i = l; i < q - 1; i++) { A[i] = A[i + 1]; u[i] = u[i + 1]; }
                q--;
            }
        }
        if (!res.feasible) break;
        if (!added && !excluded[p]) { excluded[p] = 1; res.excluded++; }  // could not make progress on this row
    }
    res.active = q;
    for (int j = 0; j < n; j++) res.x[j] = x[j];
    for (int i = 0; i < q; i++) if (u[i] > res.max_mult) res.max_mult = u[i];
    // The result is VERIFIED against every row, active ones included.  Excluded rows that remain violated mean the linearisation is inconsistent;
    // and an ACTIVE row can have drifted: with an ill-conditioned M = N'G^-1 N (cost Hessian entries four orders of magnitude apart, near-parallel
    // collision normals) z is not exactly in the null space of the active normals, the rows that are "satisfied with equality" are no longer, and
    // nothing above looks at them again.  Round 5 met a step that broke a variable's bound by 1.6 that way and was taken as feasible (a trajectory
    // parameter of -2.56 in a box of +-1: tools/dev/solve_stress.py, profiles/r05_solve_batches.txt).  A result that fails the check is infeasible:
    // the next elastic attempt, or the end of the solve -- so every accepted step keeps x + d inside the box to 1e-7.
    for (int i = 0; i < m && res.feasible; i++) {
        double s = -rows[i].b;
        for (int j = 0; j < n; j++) s += rows[i].a[j] * x[j];
        if (s < -1e-7) res.feasible = false;
    }
    return res;
}

// ---- the elastic attempts of one QP ----
// sigma = the fraction of its violation a violated row may keep: 0, 0.5, 0.9, 0.99 one after the other, the first feasible attempt wins.
// `rows_at(sigma)` fills `rows` for an attempt (the candidate rows with their elastic right-hand sides, then the variables' box as 2 n trailing
// rows).  Returns the attempt taken -- the last one, infeasible, when none was feasible -- with its number and sigma; `tried`, if given,
// receives every attempt run ([0, *attempt]).  One copy for qp_step and for the test hook armour_debug_qp_elastic.
constexpr int kElasticAttempts = 4;
inline double elastic_sigma(int attempt) { return attempt == 0 ? 0.0 : attempt == 1 ? 0.5 : attempt == 2 ? 0.9 : 0.99; }
inline double elastic_rhs(double v, double sigma) { return v - (v > 0 ? sigma * v : 0.0); }
template <class RowsAt>
QpResult solve_qp_elastic(int n, const double* Hd, const double* gradf, std::vector<QpRow>& rows, RowsAt&& rows_at, double* sigma_out, int* attempt_out, QpResult* tried = nullptr) {
    QpResult qp;
    int attempt = 0;
    for (;; attempt++) {
        rows_at(elastic_sigma(attempt));
        qp = solve_qp(n, Hd, gradf, rows, slv::kQpMaxSteps, 2 * n);
        if (tried) tried[attempt] = qp;
        if (qp.feasible || attempt == kElasticAttempts - 1) break;
    }
    *sigma_out = elastic_sigma(attempt);
    *attempt_out = attempt;
    return qp;
}
// the variables' box x_l <= x + d <= x_u as 2 n rows on the step d: lower then upper bound of variable 0, 1, ...
inline void append_box_rows(int n, const double* xl, const double* xu, const double* x, std::vector<QpRow>& rows) {
    for (int j = 0; j < n; j++) {
        QpRow r; memset(&r, 0, sizeof(r)); r.a[j] = 1.0; r.b = xl[j] - x[j]; rows.push_back(r);
        QpRow r2; memset(&r2, 0, sizeof(r2)); r2.a[j] = -1.0; r2.b = -(xu[j] - x[j]); rows.push_back(r2);
    }
}

// ---- device-side scan of one evaluation: what the host QP needs instead of the whole g / jac ----
// One block per problem walks the rows in order and leaves (a) the L1 violation of g_l <= g <= g_u and, with ROWS,
// (b) the rows the QP has to see -- those that can become active for some |d|_inf <= 2, the filter of the host loop
// below -- compacted IN ROW ORDER (upper side before lower side of a row), each as {row, side, v = violation-signed
// distance to the bound, a = -+J_i}.  A problem with 20 obstacles moves a few hundred such rows instead of 0.94 MB.
constexpr int kScanRowsPerBlock = 2048;

// MODE 0: violation only (line-search trials); 1: violation + candidate rows (new linearisation); 2: violation + number of
// rows outside the slacks of armtd_NLP::finalize_solution (RT/NLPclass.cu:422-538: torque rows 1e-2, collision rows 1e-4,
// limit rows 0; row_rules.h) -- the verdict armour_check_feasible gives on the host.
template <int MODE>
__global__ __launch_bounds__(256) void armour_solve_scan_kernel(slv::RowRule rule, const double* __restrict__ g_all, const double* __restrict__ jac_all,
                                                                const double* __restrict__ lo_all, const double* __restrict__ hi_all, int cap,
                                                                long long* __restrict__ viol_out, int* __restrict__ count_out, SolveRow* __restrict__ rows_out) {
    // grid (segments, B): a block owns kScanRowsPerBlock consecutive rows and its own slice of the outputs; the host
    // concatenates the slices in segment order
    const int b = blockIdx.y, seg = blockIdx.x, nseg = gridDim.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int m = rule.m, n = rule.n;
    const double* g = g_all + (size_t)b * m;
    constexpr bool ROWS = MODE == 1;
    const double* jac = ROWS ? jac_all + (size_t)b * m * n : nullptr;
    const double* lo = lo_all + (size_t)b * m;
    const double* hi = hi_all + (size_t)b * m;
    SolveRow* rows = ROWS ? rows_out + ((size_t)b * nseg + seg) * cap : nullptr;
    const int row_end = min(m, (seg + 1) * kScanRowsPerBlock);
    __shared__ int wave_tot[4];
    __shared__ long long red[256];
    int base = 0, bad = 0;
    long long vsum = 0;   // L1 violation in 2^-32 fixed point: the sum does not depend on the reduction order (solver_common.h)
    for (int i0 = seg * kScanRowsPerBlock; i0 < row_end; i0 += 256) {
        const int i = i0 + tid;
        const bool in = i < row_end;
        const double gi = in ? g[i] : 0.0, li = in ? lo[i] : -1e300, ui = in ? hi[i] : 1e300;
        vsum += slv::row_violation(gi, li, ui);
        if (MODE == 2 && in && slv::outside_slack(rule, i, gi, li, ui)) bad++;
        if (ROWS) {
            double J[NV], l1 = 0.0;
#pragma unroll
            for (int j = 0; j < NV; j++) { J[j] = (in && j < n) ? jac[(size_t)i * n + j] : 0.0; l1 += fabs(J[j]); }
            const bool fh = in && slv::row_upper_candidate(gi, ui, l1);
            const bool fl = in && slv::row_lower_candidate(gi, li, l1);
            const unsigned long long bh = __ballot(fh), bl = __ballot(fl);
            const unsigned long long below = (1ull << lane) - 1ull;
            if (lane == 0) wave_tot[wv] = __popcll(bh) + __popcll(bl);
            __syncthreads();
            int pos = base + __popcll(bh & below) + __popcll(bl & below);
            for (int w2 = 0; w2 < wv; w2++) pos += wave_tot[w2];
            if (fh) {
                if (pos < cap) {
                    SolveRow r; r.idx = i; r.side = 0; r.v = gi - ui;
#pragma unroll
                    for (int j = 0; j < NV; j++) r.a[j] = -J[j];
                    rows[pos] = r;
                }
                pos++;
            }
            if (fl && pos < cap) {
                SolveRow r; r.idx = i; r.side = 1; r.v = li - gi;
#pragma unroll
                for (int j = 0; j < NV; j++) r.a[j] = J[j];
                rows[pos] = r;
            }
            base += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
            __syncthreads();
        }
    }
    red[tid] = vsum;
    __syncthreads();
    for (int s2 = 128; s2 > 0; s2 >>= 1) {
        if (tid < s2) red[tid] += red[tid + s2];
        __syncthreads();
    }
    if (MODE == 2) {
        __shared__ int bad_tot;
        if (tid == 0) bad_tot = 0;
        __syncthreads();
        if (bad) atomicAdd(&bad_tot, bad);
        __syncthreads();
        base = bad_tot;
    }
    if (tid == 0) { viol_out[(size_t)b * nseg + seg] = red[0]; if (MODE != 0) count_out[(size_t)b * nseg + seg] = base; }
}

}  // namespace

extern "C" void armour_solve_options_default(ArmourSolveOptions* o) {
    memset(o, 0, sizeof(*o));
    o->max_iterations = 60;
    o->max_line_search = 12;
    o->tolerance = 1e-4;       // IPOPT_OPTIMIZATION_TOLERANCE, RT/Parameters.h:50
    o->max_wall_time_s = 0.0;  // 0 = no limit (the reference passes 0.5 s - t(P1) - 0.05 s, RT/armour_main.cu:227-229)
}

// test hook: the QP solver alone.  rows: lo <= A x <= hi (|bound| >= 1e18 = absent).  Returns 0 / ARMOUR_EINVAL; feasible flag in *feasible.
extern "C" int armour_debug_qp(int32_t n, const double* Gd, const double* g0, int32_t m, const double* Amat, const double* lo,
                               const double* hi, double* x, int32_t* feasible) {
    if (n < 1 || n > NV || m < 0) { armour_set_error("armour_debug_qp: bad size"); return ARMOUR_EINVAL; }
    std::vector<QpRow> rows;
    for (int i = 0; i < m; i++) {
        if (hi[i] < 1e18) { QpRow r; for (int j = 0; j < n; j++) r.a[j] = -Amat[i * n + j]; r.b = -hi[i]; rows.push_back(r); }
        if (lo[i] > -1e18) { QpRow r; for (int j = 0; j < n; j++) r.a[j] = Amat[i * n + j]; r.b = lo[i]; rows.push_back(r); }
    }
    const QpResult q = solve_qp(n, Gd, g0, rows);
    for (int j = 0; j < n; j++) x[j] = q.x[j];
    *feasible = q.feasible ? 1 : 0;
    return ARMOUR_OK;
}

// test hook: the QP as armour_solve poses it -- the rows above, then the variables' box x_lo <= x <= x_hi as 2 n trailing rows -- with (first_try = 1)
// or without (0) the box-clipped first try of solver_common.h.  steps = active-set steps taken (0: the clipped point passed every row).
extern "C" int armour_debug_qp_box(int32_t n, const double* Gd, const double* g0, int32_t m, const double* Amat, const double* lo, const double* hi,
                                   const double* x_lo, const double* x_hi, int32_t first_try, double* x, int32_t* feasible, int32_t* steps, double* max_mult) {
    if (n < 1 || n > NV || m < 0 || !x_lo || !x_hi) { armour_set_error("armour_debug_qp_box: bad argument"); return ARMOUR_EINVAL; }
    std::vector<QpRow> rows;
    for (int i = 0; i < m; i++) {
        if (hi[i] < 1e18) { QpRow r; for (int j = 0; j < n; j++) r.a[j] = -Amat[i * n + j]; r.b = -hi[i]; rows.push_back(r); }
        if (lo[i] > -1e18) { QpRow r; for (int j = 0; j < n; j++) r.a[j] = Amat[i * n + j]; r.b = lo[i]; rows.push_back(r); }
    }
    for (int j = 0; j < n; j++) {
        QpRow r; memset(&r, 0, sizeof(r)); r.a[j] = 1.0; r.b = x_lo[j]; rows.push_back(r);
        QpRow r2; memset(&r2, 0, sizeof(r2)); r2.a[j] = -1.0; r2.b = -x_hi[j]; rows.push_back(r2);
    }
    const QpResult q = solve_qp(n, Gd, g0, rows, slv::kQpMaxSteps, first_try ? 2 * n : 0);
    for (int j = 0; j < n; j++) x[j] = q.x[j];
    *feasible = q.feasible ? 1 : 0;
    if (steps) *steps = q.iterations;
    if (max_mult) *max_mult = q.max_mult;
    return ARMOUR_OK;
}

// the arguments the two hooks below share: the QP as armour_solve poses it at the iterate x
static int check_posed_qp(const char* who, int32_t n, const double* Hd, const double* gradf, const double* x, int32_t ncand, const double* a, const double* v) {
    if (n < 1 || n > NV || ncand < 0 || ncand > 16384 || !Hd || !gradf || !x || (ncand > 0 && (!a || !v))) { armour_set_error("%s: bad argument (n = %d, ncand = %d)", who, n, ncand); return ARMOUR_EINVAL; }
    bool ok = finite_all(Hd, n) && finite_all(gradf, n) && finite_all(x, n) && finite_all(a, (size_t)ncand * n) && finite_all(v, ncand);
    for (int j = 0; j < n && ok; j++) ok = Hd[j] > 0;
    if (!ok) { armour_set_error("%s: non-finite input or Hd <= 0", who); return ARMOUR_EINVAL; }
    return ARMOUR_OK;
}

// test hook: the QP of one SQP step with its elastic attempts, the host form's code (solve_qp_elastic, solve_qp).  The QP as armour_solve poses it:
// n variables, the cost's diagonal Hd and gradient gradf, the iterate x (the box rows -1 - x <= d <= 1 - x are appended as the solver appends them)
// and ncand candidate rows  a_i'd >= v_i - sigma max(v_i, 0)  (a: [ncand][n] row-major).  Host-only.
extern "C" int armour_debug_qp_elastic(int32_t n, const double* Hd, const double* gradf, const double* x, int32_t ncand, const double* a, const double* v,
                                       double* d, int32_t* feasible, int32_t* attempt, double* max_mult, int32_t* steps, int32_t* dropped,
                                       int32_t* dropped_mid, int32_t* excluded, int32_t* active) {
    ARMOUR_TRY(check_posed_qp("armour_debug_qp_elastic", n, Hd, gradf, x, ncand, a, v));
    if (!d || !feasible || !attempt) { armour_set_error("armour_debug_qp_elastic: null output"); return ARMOUR_EINVAL; }
    double xl[NV], xu[NV];
    for (int j = 0; j < NV; j++) { xl[j] = -1.0; xu[j] = 1.0; }
    std::vector<QpRow> rows;
    const auto rows_at = [&](double sigma) {
        rows.clear();
        for (int i = 0; i < ncand; i++) {
            QpRow r; for (int j = 0; j < n; j++) r.a[j] = a[(size_t)i * n + j];
            r.b = elastic_rhs(v[i], sigma); rows.push_back(r);
        }
        append_box_rows(n, xl, xu, x, rows);
    };
    QpResult tried[kElasticAttempts];
    double sigma = 0.0;
    int k = 0;
    const QpResult qp = solve_qp_elastic(n, Hd, gradf, rows, rows_at, &sigma, &k, tried);
    for (int j = 0; j < n; j++) d[j] = qp.x[j];
    *feasible = qp.feasible ? 1 : 0;
    *attempt = k;
    if (max_mult) *max_mult = qp.max_mult;
    for (int e = 0; e < kElasticAttempts; e++) {
        const bool ran = e <= k;
        if (steps) steps[e] = ran ? tried[e].iterations : -1;
        if (dropped) dropped[e] = ran ? tried[e].dropped : -1;
        if (dropped_mid) dropped_mid[e] = ran ? tried[e].dropped_mid : -1;
        if (excluded) excluded[e] = ran ? tried[e].excluded : -1;
        if (active) active[e] = ran ? tried[e].active : -1;
    }
    return ARMOUR_OK;
}

// test hook: the same QP through the device form's solve_qp_wave (solver_device.hip: armour_qp_probe_kernel, one plain launch of one block).  wps: the
// build (1 or 2 waves per SIMD); lds_rows: candidate rows the LDS staging holds (0: what armour_solve gives that build; less: the tests' small regimes).
extern "C" int armour_debug_qp_device(int32_t n, const double* Hd, const double* gradf, const double* x, int32_t ncand, const double* a, const double* v,
                                      int32_t wps, int32_t lds_rows, double* d, int32_t* feasible, int32_t* attempt, double* max_mult, int32_t* qp_iter) {
    ARMOUR_TRY(check_posed_qp("armour_debug_qp_device", n, Hd, gradf, x, ncand, a, v));
    if (!d || !feasible || !attempt || (wps != 1 && wps != 2) || lds_rows < 0 || lds_rows > armour_qp_probe_lds_rows(wps)) {
        armour_set_error("armour_debug_qp_device: wps = %d (1, 2), lds_rows = %d (0..%d), or a null output", wps, lds_rows, armour_qp_probe_lds_rows(wps == 2 ? 2 : 1));
        return ARMOUR_EINVAL;
    }
    if (!armour_device_available()) { armour_set_error("armour_debug_qp_device: no HIP device visible (armour_debug_qp_elastic runs without one)"); return ARMOUR_EDEVICE; }
    QpProbe io;
    memset(&io, 0, sizeof(io));
    for (int j = 0; j < NV; j++) { io.x[j] = j < n ? x[j] : 0.0; io.gradf[j] = j < n ? gradf[j] : 0.0; io.Hd[j] = j < n ? Hd[j] : 1e-12; }   // (past n: what the solve kernel puts there)
    io.ncand = ncand;
    std::vector<SolveRow> rows((size_t)ncand);
    for (int i = 0; i < ncand; i++) {
        SolveRow& r = rows[i];
        r.idx = i; r.side = 0; r.v = v[i];
        for (int j = 0; j < NV; j++) r.a[j] = j < n ? a[(size_t)i * n + j] : 0.0;
    }
    ARMOUR_TRY(armour_qp_probe(n, rows.data(), wps, lds_rows, &io));
    for (int j = 0; j < n; j++) d[j] = io.d[j];
    *feasible = io.feasible;
    *attempt = io.attempt;
    if (max_mult) *max_mult = io.max_mult;
    if (qp_iter) for (int e = 0; e < 4; e++) qp_iter[e] = e <= io.attempt ? io.qp_iter[e] : -1;   // (attempts above the one taken may have been cut short: not reported)
    return ARMOUR_OK;
}

// ---- the device-resident form (solver_device.hip): one persistent launch runs every problem's SQP to the end ----
// It hands the batch back to the host-driven form when the device has no co-resident grid for it, or when a problem's candidate rows outgrew
// the device buffers or its group lost a block.
enum class DeviceOutcome { Solved, HandBack };

// how a batch is launched: the row walk, the cut into sub-batches, the blocks per problem, the candidate rows they keep
struct DevicePlan {
    SolvePlan plan;                  // (plan.capacity < 1: no co-resident grid)
    bool culled = false;
    p2::SparseList sl = {nullptr, nullptr, nullptr, nullptr};
    const int* tq_tiles = nullptr; const int* tq_count = nullptr;
    int tq_cap = 0, n_tiles_culled = 0;
    int Bs = 0, n_launch = 0, nb = 0, tiles_per_block = 0, cap_blk = 0, cap_rows = 0;
};

static int plan_device_solve(ArmourPlanner* h, const P2Tables& tb, DevicePlan& p) {
    const int B = h->B, m = h->m;
    SolvePlan& plan = p.plan;
    int rc;
    // The culled form (ARMOUR_OPT_SOLVE_CULL; relevance.hip, solver_device.h): the kernel walks only the rows that can pass the candidate filter
    // for some k.  Same iterates; the lists cost one pass over the half-space table per problem set (about one evaluation) and 0.2 ms of host
    // round trips, so automatic = from kSolveCullMinRows collision rows in the batch on.
    const int cull_opt = h->tune(ARMOUR_OPT_SOLVE_CULL);
    constexpr long long kSolveCullMinRows = 150000;   // (first solve after armour_set_problems, lists included, O = 20: B = 8 1.43 against 1.44 ms, B = 16 1.61 against 1.98, B = 64 2.2 against 4.5)
    p.culled = h->Q > 0 && (cull_opt > 0 || (cull_opt < 0 && (long long)B * h->Q >= kSolveCullMinRows));
    if (p.culled) {
        if ((rc = armour_solver_lists(h, &p.sl, &p.tq_tiles, &p.tq_count, &p.tq_cap)) != ARMOUR_OK) return rc;
        for (int b = 0; b < B; b++) p.n_tiles_culled = std::max(p.n_tiles_culled, (h->rel2.h_tq_count[b] + P2_BLOCK - 1) / P2_BLOCK + (h->rel2.h_count[b] + P2_BLOCK - 1) / P2_BLOCK + 1);
    }
    if ((rc = armour_solve_device_capacity(tb, h->max_link, h->max_torque, h->h_plane_skip.data(), h->device, B, h->tune(ARMOUR_OPT_SOLVE_WAVES_PER_SIMD), &plan, p.n_tiles_culled)) != ARMOUR_OK) return rc;
    if (plan.capacity < 1) return ARMOUR_OK;
    // A block walks its tiles one after the other (~4 us each), so what a phase costs is the tiles PER BLOCK, and the co-resident
    // grid has to be shared by the problems of a launch.  Round 2 ran the whole batch in one launch and fell back to the host form
    // where that left a block more than 100 tiles (B = 128 at O = 50: 4 blocks per problem, 159 tiles each, 50 ms against the host
    // form's 30).  Now such a batch is cut into SUB-BATCHES launched back to back on the handle's stream -- each a persistent
    // cooperative launch of its own over problems [b0, b0 + Bs) of the same tables, with enough blocks per problem for about
    // `sub_tiles` tiles per block; iterates and results do not depend on the cut (a problem's blocks see only that problem).
    const int sub_tiles = std::max(1, h->tune(ARMOUR_OPT_SOLVE_SUB_TILES));   // default 48: tiles per block aimed at (swept on B = 64 ... 256, O = 20 ... 50: profiles/r03_solve_subtiles.txt)
    // When to cut (profiles/r03_solve_subtiles.txt, swept with candidate buffers large enough never to overflow): one launch is best or within
    // 3 % up to ~154 tiles per block (B = 128 at O = 20 / 30 / 40: 10.2 / 15.0 / 13.3 ms; B = 256 at O = 20: 19.7 against 24.9 cut); at 159
    // (B = 128, O = 50) the cut wins, 14.3 against 18.7 ms.  The threshold sits between those two measurements.
    const int cut_tiles = std::max(1, h->tune(ARMOUR_OPT_SOLVE_CUT_TILES));   // default 156
    int Bs = B;
    if (plan.capacity < B || (plan.n_tiles + std::max(1, plan.capacity / B) - 1) / std::max(1, plan.capacity / B) > cut_tiles) {
        const int nb_want = std::min(plan.n_tiles, (plan.n_tiles + sub_tiles - 1) / sub_tiles);
        Bs = std::max(1, std::min(B, plan.capacity / std::max(1, nb_want)));
        if ((rc = armour_solve_device_capacity(tb, h->max_link, h->max_torque, h->h_plane_skip.data(), h->device, Bs, h->tune(ARMOUR_OPT_SOLVE_WAVES_PER_SIMD), &plan, p.n_tiles_culled)) != ARMOUR_OK) return rc;
        Bs = std::max(1, std::min(Bs, plan.capacity));
    }
    int nb = std::min(std::min(plan.n_tiles, plan.capacity / Bs), 1024);
    if (h->tune(ARMOUR_OPT_SOLVE_BLOCKS) > 0) nb = std::max(1, std::min(nb, h->tune(ARMOUR_OPT_SOLVE_BLOCKS)));          // tuning / tests
    if (h->tune(ARMOUR_OPT_SOLVE_SUB_BATCH) > 0) Bs = std::max(1, std::min(Bs, h->tune(ARMOUR_OPT_SOLVE_SUB_BATCH)));    // tuning / tests: force the cut
    p.Bs = Bs; p.nb = nb;
    p.n_launch = (B + Bs - 1) / Bs;
    // rows a block owns: at most ceil(n_tiles / nb) tiles of <= 64 rows, two candidates per row
    p.tiles_per_block = (plan.n_tiles + nb - 1) / nb;
    // (an overflow of either sends the whole batch to the host-driven form, i.e. costs a second solve: B = 128 at O = 20 with 77 tiles per
    //  block overflowed 1024 rows per block on two of four world seeds -- 25 ms instead of 10; the buffers are 72 B per row)
    p.cap_blk = std::min(2 * p.tiles_per_block * (p.culled ? P2_BLOCK : 64), 4096);
    p.cap_rows = std::min(2 * m, 16384);
    if (h->tune(ARMOUR_OPT_SOLVE_ROW_CAP) > 0) p.cap_blk = std::max(1, std::min(p.cap_blk, h->tune(ARMOUR_OPT_SOLVE_ROW_CAP)));  // tests: force the overflow fallback
    return ARMOUR_OK;
}

// what the launches read: the device buffers, and ONE control block filled by ONE copy from its page-locked mirror
struct DeviceStage {
    SolveArgs a;
    ArmourSolveResult* hres = nullptr;   // page-locked: the kernel writes the results straight into it
    unsigned char* hblock = nullptr;     // page-locked mirror of the control block
    long long* hstamps = nullptr;        // ARMOUR_SOLVE_TIMING: the kernel's phase stamps [B][64]
    size_t off_args = 0, args_stride = 0, block_bytes = 0;
    double hard_s = 0;                   // no wait of the kernel outlasts this
};

static int stage_device_solve(ArmourPlanner* h, const ArmourSolveOptions& opt, const double* k_start, const P2Tables& tb, const DevicePlan& p, Clock::time_point t_begin, DeviceStage& s) {
    const int B = h->B, n = h->n, m = h->m;
    const SolvePlan& plan = p.plan;
    int rc;
    if ((rc = armour_upload_bounds(h)) != ARMOUR_OK) return rc;
    SolveDeviceWork& w = h->solve_dev;
    // everything the host hands the kernel sits in ONE device block, filled by ONE copy from its page-locked mirror: the per-problem
    // control words, the goals, the argument block (three copies and a fill ahead of the launch cost ~10 us of a 150 us solve)
    const size_t off_qdes = ((size_t)B * sizeof(SolveCtl) + 255) & ~(size_t)255;
    s.off_args = (off_qdes + (size_t)B * n * sizeof(double) + 255) & ~(size_t)255;
    s.args_stride = (sizeof(SolveArgs) + 255) & ~(size_t)255;
    s.block_bytes = s.off_args + (size_t)p.n_launch * s.args_stride;
    ARMOUR_TRY(w.ctl.reserve(s.block_bytes));
    // the blocks' flag words: zero before a launch.  Every block clears its own word when it leaves the kernel, so a fill is only
    // needed when the array is new (or grew)
    // (sized for ONE sub-batch: the launches of a cut batch run one after the other on the stream and index these buffers by
    //  b - b0, so a batch of 1024 problems holds the candidate rows of the <= Bs it solves at a time -- ADVICE round 3)
    bool fresh = false;
    ARMOUR_TRY(w.blk_word.reserve((size_t)p.Bs * p.nb * sizeof(BlockWord), &fresh));
    if (fresh || !w.words_clean) HIPCHK(hipMemsetAsync(w.blk_word, 0, w.blk_word.cap, h->stream));
    w.words_clean = 0;   // until this launch has been seen to end
    ARMOUR_TRY(w.blk_rows.reserve((size_t)p.Bs * p.nb * p.cap_blk * sizeof(SolveRow)));
    ARMOUR_TRY(w.qp_rows.reserve((size_t)p.Bs * p.cap_rows * sizeof(SolveRow)));
    ARMOUR_TRY(w.flags.reserve((size_t)p.Bs * 8 * (p.cap_rows + 2 * NV)));   // (active / excluded) x the four QP attempts
    ARMOUR_TRY(w.h_res.reserve((size_t)B));
    ARMOUR_TRY(w.h_ctl.reserve(s.block_bytes));
    s.hres = w.h_res;
    s.hblock = w.h_ctl;
    SolveCtl* hctl = w.h_ctl.as<SolveCtl>();
    memset(s.hres, 0, (size_t)B * sizeof(ArmourSolveResult));
    memset(hctl, 0, (size_t)B * sizeof(SolveCtl));
    for (int b = 0; b < B; b++) {   // phase 0: CMD_EVAL_GJ at the start point (zeros, or armour_solve_from's)
        hctl[b].go = 1; s.hres[b].status = -2;
        if (k_start) for (int j = 0; j < n; j++) hctl[b].x[j] = k_start[(size_t)b * n + j];
    }
    memcpy(s.hblock + off_qdes, h->h_qdes.data(), (size_t)B * n * sizeof(double));
    SolveArgs& a = s.a;
    memset(&a, 0, sizeof(a));
    a.tb = tb; a.lp = plan.lp; a.nb = p.nb; a.n_tiles = plan.n_tiles; a.cap_blk = p.cap_blk; a.cap_rows = p.cap_rows;
    a.lds_rows = (int)(plan.smem / ((NV + 1) * sizeof(double)));
    a.culled = p.culled ? 1 : 0; a.sl = p.sl; a.tq_tiles = p.tq_tiles; a.tq_count = p.tq_count; a.tq_cap = p.tq_cap;
    a.lo = h->d_bounds; a.hi = h->d_bounds + (size_t)B * m; a.g = h->d_g; a.jac = h->d_jac;
    a.ctl = w.ctl.as<SolveCtl>(); a.blk_word = w.blk_word.as<BlockWord>();
    a.blk_rows = w.blk_rows.as<SolveRow>(); a.qp_rows = w.qp_rows.as<SolveRow>(); a.flags = w.flags;
    a.q_des = reinterpret_cast<const double*>(w.ctl + off_qdes); a.out = s.hres;   // the kernel writes the results straight into page-locked host memory
    a.continuous_mask = h->continuous_mask();
    a.max_iter = opt.max_iterations; a.max_ls = opt.max_line_search; a.tol = opt.tolerance;
    const slv::RowRule rule = armour_row_rule(h);
    a.n_checked_collision = rule.n_checked; a.torque_slack = rule.torque_slack; a.collision_slack = rule.collision_slack;
    a.t_plan = h->params.t_plan; a.cost_scale = h->params.cost_scale;
    a.budget_ticks = -1;
    if (opt.max_wall_time_s > 0) {   // (sub-batches run one after the other: each gets an equal share of what is left)
        const double left_ms = (opt.max_wall_time_s - std::chrono::duration<double>(Clock::now() - t_begin).count()) * 1e3 / p.n_launch;
        a.budget_ticks = left_ms > 0 ? (long long)(left_ms * plan.ticks_per_ms) : 0;
    }
    // no wait of the persistent kernel outlasts the budget by more than a second (without a budget: from the iteration limit and the tiles per block, below); the host's own poll gives up a little later.  ARMOUR_OPT_SOLVE_HARD_CAP_S: tuning / tests.
    const double hard_cap_s = h->tune_f(ARMOUR_OPT_SOLVE_HARD_CAP_S);
    // without a budget: 50 x what max_iterations iterations of (1 + max_line_search) evaluations cost at ~4 us per row tile of a block, at least 5 s
    const double no_budget_s = std::max(5.0, 1.0 + 50.0 * (double)std::max(1, opt.max_iterations) * (1.0 + std::max(0, opt.max_line_search)) * p.tiles_per_block * 4e-6);
    s.hard_s = hard_cap_s > 0 ? hard_cap_s : (a.budget_ticks >= 0 ? a.budget_ticks / plan.ticks_per_ms * 1e-3 + 1.0 : no_budget_s);
    a.hard_ticks = std::max<long long>(1, (long long)(s.hard_s * 1e3 * plan.ticks_per_ms));
    if (armour_trace_solve()) {
        ARMOUR_TRY(w.h_stamps.reserve((size_t)B * 64));
        s.hstamps = w.h_stamps;
        memset(s.hstamps, 0, (size_t)B * 64 * sizeof(long long));
    }
    a.stamps = s.hstamps;
    return ARMOUR_OK;
}

// ARMOUR_SOLVE_TIMING: where the device form's time went
static void report_device_timing(const ArmourPlanner* h, const DevicePlan& p, const DeviceStage& s, double ms, Clock::time_point t_begin, Clock::time_point t_launch) {
    const SolvePlan& plan = p.plan;
    const ArmourSolveResult* hres = s.hres;
    const long long* hstamps = s.hstamps;
    const int B = h->B, n_launch = p.n_launch, Bs = p.Bs, nb = p.nb, n_tiles_culled = p.n_tiles_culled;
    if (p.culled) fprintf(stderr, "[armour_solve, device form] culled: at most %d listed tiles per problem (problem 0: %d of %d collision rows, %d of %d torque rows), lists %.3f + %.3f ms\n",
                          n_tiles_culled, h->rel2.h_count[0], h->Q, h->rel2.h_tq_count[0], h->row0, h->rel.ms, h->rel2.ms);
    fprintf(stderr, "[armour_solve, device form] B=%d in %d launch(es) of <= %d problems: %d blocks per problem (%d tiles), %.3f ms wall (%.3f ms before the launch), kernel %.3f ms (problem 0); phases of problem 0 in us (barrier passed / leader done):", B, n_launch, Bs, nb, plan.n_tiles, ms,
            std::chrono::duration<double, std::milli>(t_launch - t_begin).count(), hres[0].time_ms / plan.ticks_per_ms);
    int bs = 0;   // the problem whose group left last: what the launch waited for
    for (int b = 1; b < B; b++) if (hres[b].time_ms > hres[bs].time_ms) bs = b;
    for (int which = 0; which < 2; which++) {
        const int b = which == 0 ? 0 : bs;
        const long long* st = hstamps + (size_t)b * 64;
        if (which == 1) fprintf(stderr, "\n   slowest problem %d: kernel %.3f ms, %d iterations, %d evaluations, status %d, %lld QP solves with %lld steps in all; phases in us:", b, hres[b].time_ms / plan.ticks_per_ms,
                                hres[b].iterations, hres[b].evaluations, hres[b].status, st[43], st[42]);
        for (int i = 0; i < 32 && (i < 2 || st[i]); i++) fprintf(stderr, " %.1f", st[i] / plan.ticks_per_ms * 1e3);
        fprintf(stderr, " | first leader step: bookkeeping %.1f, candidates gathered %.1f, QP done %.1f us (%lld QP steps, %lld candidate rows)", st[32] / plan.ticks_per_ms * 1e3,
                st[33] / plan.ticks_per_ms * 1e3, st[34] / plan.ticks_per_ms * 1e3, st[40], st[41]);
        fprintf(stderr, " | QP steps by attempt (sigma 0, 0.5, 0.9, 0.99), all solves: %lld %lld %lld %lld", st[44], st[45], st[46], st[47]);
        fprintf(stderr, " | attempt 0, all steps, us: row search %.1f, entering row %.1f, M + rhs %.1f, factor + solves %.1f, z + step lengths %.1f, update %.1f",
                st[50] / plan.ticks_per_ms * 1e3, st[51] / plan.ticks_per_ms * 1e3, st[52] / plan.ticks_per_ms * 1e3, st[53] / plan.ticks_per_ms * 1e3, st[54] / plan.ticks_per_ms * 1e3, st[55] / plan.ticks_per_ms * 1e3);
    }
    long long longest_ok = 0, long_bad = 0, steps_all = 0;
    for (int b = 0; b < B; b++) { const long long* st = hstamps + (size_t)b * 64; longest_ok = std::max(longest_ok, st[48]); long_bad += st[49]; steps_all += st[44] + st[45] + st[46] + st[47]; }
    fprintf(stderr, "\n   all problems: %lld QP steps; longest attempt that ended feasible %lld steps; attempts of more than 60 steps that ended infeasible: %lld\n", steps_all, longest_ok, long_bad);
}

static int solve_on_device(ArmourPlanner* h, const ArmourSolveOptions& opt, const double* k_start, ArmourSolveResult* results, Clock::time_point t_begin, DeviceOutcome* out) {
    *out = DeviceOutcome::HandBack;
    const P2Tables tb = armour_make_tables(h);
    DevicePlan p;
    DeviceStage s;
    int rc;
    if ((rc = plan_device_solve(h, tb, p)) != ARMOUR_OK || p.plan.capacity < 1) return rc;
    if ((rc = stage_device_solve(h, opt, k_start, tb, p, t_begin, s)) != ARMOUR_OK) return rc;
    SolveDeviceWork& w = h->solve_dev;
    const int B = h->B, n_launch = p.n_launch;
    const auto t_launch = Clock::now();
    for (int li = 0; li < n_launch; li++) { s.a.b0 = li * p.Bs; memcpy(s.hblock + s.off_args + (size_t)li * s.args_stride, &s.a, sizeof(SolveArgs)); }
    HIPCHK(hipMemcpyAsync(w.ctl, s.hblock, s.block_bytes, hipMemcpyHostToDevice, h->stream));   // (asynchronous from page-locked memory, ordered before the launches)
    for (int li = 0; li < n_launch; li++)
        if ((rc = armour_solve_device_launch(reinterpret_cast<const SolveArgs*>(w.ctl + s.off_args + (size_t)li * s.args_stride), p.nb, p.plan,
                                             std::min(p.Bs, B - li * p.Bs), h->stream)) != ARMOUR_OK) return rc;
    for (unsigned long long polls = 0;; polls++) {  // poll the stream: the whole solve is tens of microseconds, a sleeping wait would dominate it
        const hipError_t q = hipStreamQuery(h->stream);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) { armour_set_error("armour_solve (device form): %s", hipGetErrorString(q)); return ARMOUR_EDEVICE; }
        // the kernel bounds its own waits by hard_s; a stream that is still busy well after that is a device the caller must give up on
        // (recover in a fresh process; never by re-exec of this one)
        if ((polls & 0xfffull) == 0xfffull && std::chrono::duration<double>(Clock::now() - t_launch).count() > n_launch * (2.0 * s.hard_s + 5.0)) {
            armour_set_error("armour_solve (device form): the persistent kernel did not finish within %.1f s", n_launch * (2.0 * s.hard_s + 5.0));
            return ARMOUR_EDEVICE;
        }
    }
    w.words_clean = 1;
    for (int b = 0; b < B; b++)
        if (s.hres[b].status < 0) { w.words_clean = 0; return ARMOUR_OK; }   // candidate buffers too small for some problem, or a group lost a block
    const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t_begin).count();
    if (s.hstamps) report_device_timing(h, p, s, ms, t_begin, t_launch);
    for (int b = 0; b < B; b++) { results[b] = s.hres[b]; results[b].time_ms = ms; }
    *out = DeviceOutcome::Solved;
    return ARMOUR_OK;
}

// ---- the host-driven form: evaluations and scans on the device, the QPs on host threads ----
enum class Scan { Violation = 0, Rows = 1, Verdict = 2 };   // armour_solve_scan_kernel's MODE

struct ProblemState {
    double x[NV] = {}, f, gradf[NV], viol, mu = 1.0;   // get_starting_point: x = 0 (armour_solve_from: setup_host_solve overwrites it)
    int iters = 0, evals = 0, status = 0;  // 0 running, 1 converged, 2 max iterations, 3 QP infeasible, 4 line search failed, 5 time limit
    bool done = false;
    bool searching = false;                // in this iteration's line search: step d, length alpha, merit phi0 at x and its slope dphi
    double d[NV], alpha, phi0, dphi;
};

// what the stages of the host-driven form share
struct HostSolve {
    ArmourPlanner* h;
    ArmourSolveOptions opt;
    int B, n, m, nseg, cap_rows;
    // page-locked mirrors owned by the handle: the point evaluated [B][n]; the scan's per-segment violations, row counts and candidate rows;
    // the whole g / jac, which only the row-buffer overflow fallback allocates (full_on_host: they hold the current linearisation)
    double* hk; long long* hviol_seg; int* hcount; SolveRow* hrows;
    double *hg = nullptr, *hj = nullptr;
    bool full_on_host = false;
    std::vector<double> xl, xu, Hd;      // the variables' box; [B][NV] the cost's constant diagonal Hessian
    std::vector<double> viol, f, gradf;  // at hk: [B] L1 violation (from the scan), [B] f, [B][n] grad f
    std::vector<ProblemState> st;
    double t_eval = 0, t_qp = 0;         // ARMOUR_SOLVE_TIMING
};

static int setup_host_solve(ArmourPlanner* h, const ArmourSolveOptions& opt, const double* k_start, HostSolve& s) {
    const int B = h->B, n = h->n, m = h->m;
    int rc;
    s.h = h; s.opt = opt; s.B = B; s.n = n; s.m = m;
    // (the page-locked mirrors are kept across solves; armour_eval_g_jac_device reads k from hk in place)
    SolveHostWork& w = h->solve_host;
    ARMOUR_TRY(w.k.reserve((size_t)B * n));
    s.hk = w.k;
    s.xl.resize(n); s.xu.resize(n);
    if ((rc = armour_upload_bounds(h)) != ARMOUR_OK) return rc;   // (d_bounds: once per problem set, on the device)
    if (!h->bounds_on_host) {  // this form's own host copy, once per problem set
        h->h_gl.resize((size_t)B * m); h->h_gu.resize((size_t)B * m);
        if ((rc = armour_get_bounds(h, s.xl.data(), s.xu.data(), h->h_gl.data(), h->h_gu.data())) != ARMOUR_OK) return rc;
        h->bounds_on_host = true;
    } else if ((rc = armour_get_bounds(h, s.xl.data(), s.xu.data(), nullptr, nullptr)) != ARMOUR_OK) return rc;
    s.nseg = (m + kScanRowsPerBlock - 1) / kScanRowsPerBlock;
    // rows a segment may hand back (its slice of the page-locked buffer): everything if the batch is small
    s.cap_rows = (int)std::max<size_t>(64, std::min<size_t>(2 * kScanRowsPerBlock, ((size_t)128 << 20) / ((size_t)B * s.nseg * sizeof(SolveRow))));
    if (h->tune(ARMOUR_OPT_SOLVE_ROW_CAP) > 0) s.cap_rows = std::max(1, h->tune(ARMOUR_OPT_SOLVE_ROW_CAP));  // tests: force the overflow fallback
    ARMOUR_TRY(w.viol_seg.reserve((size_t)B * s.nseg));
    ARMOUR_TRY(w.count.reserve((size_t)B * s.nseg));
    ARMOUR_TRY(w.rows.reserve((size_t)B * s.nseg * s.cap_rows * sizeof(SolveRow)));
    s.hviol_seg = w.viol_seg; s.hcount = w.count; s.hrows = w.rows.as<SolveRow>();
    s.viol.resize(B); s.f.resize(B); s.gradf.resize((size_t)B * n);
    // constant diagonal Hessian of the cost (solver_common.h)
    s.Hd.assign((size_t)B * NV, 1e-12);
    for (int b = 0; b < B; b++)
        for (int j = 0; j < n; j++) {
            const size_t ix = (size_t)b * n + j;
            const double dk = slv::plan_dk(h->mode, h->mode == ARMOUR_MODE_ARMTD ? h->h_krange[ix] : 0.0, h->params.k_range[j], h->params.t_plan);
            s.Hd[(size_t)b * NV + j] = slv::hess_diag(h->params.cost_scale, dk);
        }
    s.st.assign(B, ProblemState());
    std::fill(s.hk, s.hk + (size_t)B * n, 0.0);
    if (k_start)
        for (int b = 0; b < B; b++) for (int j = 0; j < n; j++) s.hk[(size_t)b * n + j] = s.st[b].x[j] = k_start[(size_t)b * n + j];
    return ARMOUR_OK;
}

// One fused evaluation of all problems at hk into the handle's device buffers, then the scan; the host waits once.  Scan::Rows evaluates the
// Jacobian too, and brings the whole linearisation over when some segment found more candidate rows than its slice of the buffer holds.
static int evaluate(HostSolve& s, Scan mode) {
    const auto e0 = Clock::now();
    struct Acc { double& t; decltype(e0) s; ~Acc() { t += std::chrono::duration<double, std::milli>(Clock::now() - s).count(); } } acc{s.t_eval, e0};
    ArmourPlanner* h = s.h;
    const int B = s.B, n = s.n, m = s.m, nseg = s.nseg;
    const size_t bm = (size_t)B * m;
    const bool rows = mode == Scan::Rows;
    int r = armour_eval_g_jac_device(h, s.hk, h->d_g, rows ? h->d_jac : nullptr, h->stream);
    if (r != ARMOUR_OK) return r;
    const auto scan = mode == Scan::Violation ? armour_solve_scan_kernel<0> : rows ? armour_solve_scan_kernel<1> : armour_solve_scan_kernel<2>;
    hipLaunchKernelGGL(scan, dim3(nseg, B), dim3(256), 0, h->stream, armour_row_rule(h), h->d_g, rows ? h->d_jac : nullptr,
                       h->d_bounds, h->d_bounds + bm, s.cap_rows, s.hviol_seg, mode == Scan::Violation ? nullptr : s.hcount, rows ? s.hrows : nullptr);
    HIPCHK(hipGetLastError());
    if ((r = armour_spin_on_stream(h->stream)) != ARMOUR_OK) return r;
    for (int b = 0; b < B; b++) {
        long long v = 0;
        for (int sg = 0; sg < nseg; sg++) v += s.hviol_seg[(size_t)b * nseg + sg];
        s.viol[b] = slv::viol_from_fixed(v);
    }
    s.full_on_host = false;
    if (!rows) return ARMOUR_OK;
    bool overflow = false;
    for (size_t i = 0; i < (size_t)B * nseg; i++) overflow = overflow || s.hcount[i] > s.cap_rows;
    if (overflow) {  // more candidate rows than the buffer holds: bring the whole linearisation over, as before
        ARMOUR_TRY(h->solve_host.g.reserve(bm));
        ARMOUR_TRY(h->solve_host.jac.reserve(bm * n));
        s.hg = h->solve_host.g; s.hj = h->solve_host.jac;
        HIPCHK(hipMemcpyAsync(s.hg, h->d_g, bm * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(s.hj, h->d_jac, bm * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if ((r = armour_spin_on_stream(h->stream)) != ARMOUR_OK) return r;
        s.full_on_host = true;
    }
    return ARMOUR_OK;
}

// The rows of problem b's QP at sigma, the fraction of its violation a violated row may keep (elastic retry): the scan's candidate rows in row
// order -- or, after an overflow, the same filter over the whole linearisation -- then the variables' box as 2 n trailing rows.
static void gather_rows(const HostSolve& s, int b, double sigma, std::vector<QpRow>& rows) {
    const int n = s.n, m = s.m, nseg = s.nseg;
    const auto elastic = [sigma](double v) { return elastic_rhs(v, sigma); };
    rows.clear();
    if (!s.full_on_host) {
        for (int sg = 0; sg < nseg; sg++) {
            const SolveRow* cr = s.hrows + ((size_t)b * nseg + sg) * s.cap_rows;
            for (int r0 = 0; r0 < s.hcount[(size_t)b * nseg + sg]; r0++) {
                QpRow r; for (int j = 0; j < n; j++) r.a[j] = cr[r0].a[j];
                r.b = elastic(cr[r0].v); rows.push_back(r);
            }
        }
    } else {
        const double* g = s.hg + (size_t)b * m;
        const double* J = s.hj + (size_t)b * m * n;
        const double* lo = s.h->h_gl.data() + (size_t)b * m;
        const double* hi = s.h->h_gu.data() + (size_t)b * m;
        for (int i = 0; i < m; i++) {
            const double* Ji = J + (size_t)i * n;
            double l1 = 0;
            for (int j = 0; j < n; j++) l1 += std::fabs(Ji[j]);
            if (slv::row_upper_candidate(g[i], hi[i], l1)) { QpRow r; for (int j = 0; j < n; j++) r.a[j] = -Ji[j]; r.b = elastic(g[i] - hi[i]); rows.push_back(r); }
            if (slv::row_lower_candidate(g[i], lo[i], l1)) { QpRow r; for (int j = 0; j < n; j++) r.a[j] = Ji[j]; r.b = elastic(lo[i] - g[i]); rows.push_back(r); }
        }
    }
    append_box_rows(n, s.xl.data(), s.xu.data(), s.st[b].x, rows);
}

// The QP step of SQP iteration `it` for problems [b0, b1) (one host thread's share): up to four elastic attempts, the convergence test, and
// the L1 merit function's penalty and slope for the line search.
static void qp_step(HostSolve& s, int it, int b0, int b1) {
    const int n = s.n;
    const ArmourSolveOptions& opt = s.opt;
    std::vector<QpRow> rows;
    for (int b = b0; b < b1; b++) {
        ProblemState& p = s.st[b];
        if (p.done) continue;
        double sigma = 0.0;
        int attempt = 0;
        const QpResult qp = solve_qp_elastic(n, &s.Hd[(size_t)b * NV], p.gradf, rows, [&](double sg) { gather_rows(s, b, sg, rows); }, &sigma, &attempt);
        if (armour_trace_solve() && s.B == 1) {
            fprintf(stderr, "[armour_solve, host form] iteration %d: QP %s at sigma %.2f after %d steps, %zu rows; x =", it, qp.feasible ? "feasible" : "INFEASIBLE", sigma, qp.iterations, rows.size());
            for (int j = 0; j < n; j++) fprintf(stderr, " %.6g", p.x[j]);
            fprintf(stderr, "; d =");
            for (int j = 0; j < n; j++) fprintf(stderr, " %.6g", qp.x[j]);
            fprintf(stderr, "; viol %.6g\n", p.viol);
        }
        if (!qp.feasible) { p.done = true; p.status = 3; continue; }
        double dn = 0, gd = 0;
        for (int j = 0; j < n; j++) { p.d[j] = qp.x[j]; dn = std::fmax(dn, std::fabs(qp.x[j])); gd += p.gradf[j] * qp.x[j]; }
        if (dn <= opt.tolerance * 1e-2 || (dn <= opt.tolerance && p.viol <= opt.tolerance)) { p.done = true; p.status = 1; continue; }
        p.mu = std::fmax(p.mu, 1.5 * qp.max_mult + 1e-3);
        p.phi0 = p.f + p.mu * p.viol;
        p.dphi = gd - p.mu * (1.0 - sigma) * p.viol;
        if (p.dphi > -1e-14) p.dphi = -1e-14;
        p.alpha = 1.0;
        p.searching = true;
    }
}

// L1-merit backtracking line search, all problems in lock step (one evaluation launch per trial).  *linearised: the new linearisation of
// every problem that was searching is at hand (each took its full step, where the first trial also evaluated the Jacobian and the rows).
static int line_search(HostSolve& s, bool* linearised) {
    const int B = s.B, n = s.n, max_ls = s.opt.max_line_search;
    int rc;
    *linearised = false;
    for (int ls = 0; ls <= max_ls; ls++) {
        bool need = false;
        for (int b = 0; b < B; b++) {
            const ProblemState& p = s.st[b];
            for (int j = 0; j < n; j++) s.hk[b * n + j] = p.x[j] + (p.searching ? p.alpha * p.d[j] : 0.0);
            need = need || p.searching;
        }
        if (!need) break;
        // The full step is accepted nine times in ten, and the new linearisation is then wanted at exactly this point: the first trial is
        // evaluated WITH the Jacobian and the candidate rows (the same fused launch, 2 us more), and if every problem that was searching
        // takes it the round trip of the re-linearisation is saved (an evaluation request less in flight, not in `evaluations`: that
        // counts what the algorithm asked for, in both forms of the solver).
        const bool speculative = ls == 0;
        if ((rc = evaluate(s, speculative ? Scan::Rows : Scan::Violation)) != ARMOUR_OK) return rc;
        if (speculative) *linearised = true;
        if ((rc = armour_eval_f(s.h, s.hk, s.f.data())) != ARMOUR_OK) return rc;
        for (int b = 0; b < B; b++) {
            ProblemState& p = s.st[b];
            if (!p.searching) continue;
            p.evals++;
            const double v = s.viol[b];
            const double phi = s.f[b] + p.mu * v;
            if (phi <= p.phi0 + 1e-4 * p.alpha * p.dphi || ls == max_ls) {
                if (ls == max_ls && phi > p.phi0) { p.done = true; p.status = 4; p.searching = false; continue; }
                for (int j = 0; j < n; j++) p.x[j] = s.hk[b * n + j];
                p.f = s.f[b]; p.viol = v; p.searching = false; p.iters++;
            } else {
                p.alpha *= 0.5;
                *linearised = false;   // (this problem moves to another point: the linearisation taken at the full step is not its)
            }
        }
    }
    return ARMOUR_OK;
}

// finalize_solution: the feasibility re-check with the reference's slack thresholds (the per-row test runs on the device), then the results
static int finish_host_solve(HostSolve& s, ArmourSolveResult* results, Clock::time_point t_begin) {
    const int B = s.B, n = s.n, nseg = s.nseg;
    int rc;
    for (int b = 0; b < B; b++) for (int j = 0; j < n; j++) s.hk[b * n + j] = s.st[b].x[j];
    if ((rc = evaluate(s, Scan::Verdict)) != ARMOUR_OK) return rc;
    if ((rc = armour_eval_f(s.h, s.hk, s.f.data())) != ARMOUR_OK) return rc;
    const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t_begin).count();
    if (armour_trace_solve()) fprintf(stderr, "[armour_solve] B=%d total %.3f ms: evaluations+scan %.3f ms, QP %.3f ms, rows of problem 0, segment 0: %d (cap %d, %d segments)\n", B, ms, s.t_eval, s.t_qp, s.hcount[0], s.cap_rows, nseg);
    for (int b = 0; b < B; b++) {
        int bad = 0;
        for (int sg = 0; sg < nseg; sg++) bad += s.hcount[(size_t)b * nseg + sg];
        ArmourSolveResult& r = results[b];
        memset(&r, 0, sizeof(r));
        for (int j = 0; j < n; j++) r.k_opt[j] = s.st[b].x[j];
        r.cost = s.f[b];
        r.max_violation = s.viol[b];
        r.feasible = bad == 0 ? 1 : 0;
        r.iterations = s.st[b].iters;
        r.evaluations = s.st[b].evals + 1;
        r.status = s.st[b].done ? s.st[b].status : 2;
        r.time_ms = ms;
    }
    return ARMOUR_OK;
}

// SQP from the start point (x = 0 unless the caller gave one): QP steps on host threads, the evaluations (with the scan of what the QPs need) on the device
static int solve_on_host(ArmourPlanner* h, const ArmourSolveOptions& opt, const double* k_start, ArmourSolveResult* results, Clock::time_point t_begin) {
    HostSolve s;
    int rc;
    if ((rc = setup_host_solve(h, opt, k_start, s)) != ARMOUR_OK) return rc;
    const int B = s.B, n = s.n;
    if ((rc = evaluate(s, Scan::Rows)) != ARMOUR_OK) return rc;
    if ((rc = armour_eval_f(h, s.hk, s.f.data())) != ARMOUR_OK) return rc;
    if ((rc = armour_eval_grad_f(h, s.hk, s.gradf.data())) != ARMOUR_OK) return rc;
    for (int b = 0; b < B; b++) {
        s.st[b].f = s.f[b];
        for (int j = 0; j < n; j++) s.st[b].gradf[j] = s.gradf[(size_t)b * n + j];
        s.st[b].viol = s.viol[b];
        s.st[b].evals = 1;
    }
    // the QPs are small now (tens to hundreds of rows each): a host thread per 32 problems
    const unsigned nthreads = std::max(1u, std::min(std::thread::hardware_concurrency(), (unsigned)B / 32u));
    for (int it = 0; it < opt.max_iterations; it++) {
        bool any = false;
        for (int b = 0; b < B; b++) any = any || !s.st[b].done;
        if (!any) break;
        if (opt.max_wall_time_s > 0 && std::chrono::duration<double>(Clock::now() - t_begin).count() >= opt.max_wall_time_s) {
            for (int b = 0; b < B; b++) if (!s.st[b].done) { s.st[b].done = true; s.st[b].status = 5; }
            break;
        }
        for (int b = 0; b < B; b++) s.st[b].searching = false;
        const auto q0 = Clock::now();
        if (nthreads <= 1) qp_step(s, it, 0, B);
        else {
            std::vector<std::thread> th;
            const int per = (B + (int)nthreads - 1) / (int)nthreads;
            for (unsigned tI = 0; tI < nthreads; tI++) { const int b0 = (int)tI * per, b1 = std::min(B, b0 + per); if (b0 < b1) th.emplace_back(qp_step, std::ref(s), it, b0, b1); }
            for (auto& t : th) t.join();
        }
        s.t_qp += std::chrono::duration<double, std::milli>(Clock::now() - q0).count();
        bool linearised = false;
        if ((rc = line_search(s, &linearised)) != ARMOUR_OK) return rc;
        // new linearisation at the accepted points (already there if every searching problem took its full step)
        for (int b = 0; b < B; b++) for (int j = 0; j < n; j++) s.hk[b * n + j] = s.st[b].x[j];
        if (!linearised && (rc = evaluate(s, Scan::Rows)) != ARMOUR_OK) return rc;
        if ((rc = armour_eval_grad_f(h, s.hk, s.gradf.data())) != ARMOUR_OK) return rc;
        for (int b = 0; b < B; b++) {
            if (s.st[b].done) continue;
            s.st[b].evals++;
            for (int j = 0; j < n; j++) s.st[b].gradf[j] = s.gradf[(size_t)b * n + j];
            s.st[b].viol = s.viol[b];
        }
    }
    return finish_host_solve(s, results, t_begin);
}

extern "C" int armour_solve(ArmourPlanner* h, const ArmourSolveOptions* opt_in, ArmourSolveResult* results) { return armour_solve_from(h, opt_in, nullptr, results); }

extern "C" int armour_solve_from(ArmourPlanner* h, const ArmourSolveOptions* opt_in, const double* k_start, ArmourSolveResult* results) {
    if (!results) { armour_set_error("null argument"); return ARMOUR_EINVAL; }
    NEED_READY(h);
    if (k_start)   // the variables' box (and the box the culled form's row lists hold in): checked before the device is touched
        for (size_t i = 0; i < (size_t)h->B * h->n; i++)
            if (!(std::fabs(k_start[i]) <= 1.0)) { armour_set_error("armour_solve_from: k_start[%zu] = %g is outside [-1, 1]", i, k_start[i]); return ARMOUR_EINVAL; }
    ArmourSolveOptions opt;
    if (opt_in) opt = *opt_in; else armour_solve_options_default(&opt);
    const auto t_begin = Clock::now();
    // The device-resident form is the automatic choice for every batch size: with the QP's box-clipped first try (solver_common.h) it beats the
    // host form for one problem too (0.070 against 0.120 ms, medians of the reference's 107 worlds).  force_host_qp > 0 and
    // ARMOUR_OPT_SOLVE_DEVICE = 0 hold a call / a handle to the host form, force_host_qp < 0 to the device form.  Both give the same iterates,
    // and the host form also solves every batch the device form hands back.
    const int dev_env = h->tune(ARMOUR_OPT_SOLVE_DEVICE);
    const bool want_device = opt.force_host_qp > 0.0 ? false : opt.force_host_qp < 0.0 ? true : dev_env != 0;
    HIPCHK(hipSetDevice(h->device));
    if (want_device) {
        DeviceOutcome out;
        const int rc = solve_on_device(h, opt, k_start, results, t_begin, &out);
        if (rc != ARMOUR_OK || out == DeviceOutcome::Solved) return rc;
    }
    return solve_on_host(h, opt, k_start, results, t_begin);
}
