// armour_robust_controller: the reference's tracking controller for a BATCH of states -- nominal and interval passivity
// RNEA and the ARMOUR robust input.
//
// Replaces kinova_controller.cpp:19-84 (the MEX gateway: builds the model and a RobustController, calls update once)
// for B states at a time: one thread per state, everything in registers / thread-local memory.  The model preparation
// (model file -> CoM frames -> interval model, robot_models.cpp:124-255) is host arithmetic done once per call from
// the ArmourRobot constants; the per-state arithmetic is controller_core.h.
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "controller_core.h"
#include "controller_models.h"

namespace {

using namespace ctl;

struct CtlArgs {
    Model<double> md;
    Model<Itv> imd;
    double Kr[ARMOUR_MAX_FACTORS];
    double alpha, V_max, r_norm_threshold;
};

__global__ __launch_bounds__(64) void armour_controller_kernel(const CtlArgs* __restrict__ ap, int B, const double* __restrict__ q, const double* __restrict__ qd,
                                                               const double* __restrict__ q_des, const double* __restrict__ qd_des,
                                                               const double* __restrict__ qdd_des, double* __restrict__ u, double* __restrict__ tau,
                                                               double* __restrict__ v, int* __restrict__ status) {
    // the models go to LDS first: a lone state is one lane working through ~10^4 dependent operations, and every model
    // entry read from global memory would be a full-latency miss on that chain
    __shared__ CtlArgs sa;
    static_assert(sizeof(CtlArgs) % sizeof(double) == 0, "CtlArgs is copied as doubles");
    for (unsigned i2 = threadIdx.x; i2 < sizeof(CtlArgs) / sizeof(double); i2 += blockDim.x)
        reinterpret_cast<double*>(&sa)[i2] = reinterpret_cast<const double*>(ap)[i2];
    __syncthreads();
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const CtlArgs& a = sa;
    const int n = a.md.n;
    double lq[ARMOUR_MAX_FACTORS], lqd[ARMOUR_MAX_FACTORS], lqdes[ARMOUR_MAX_FACTORS], lqddes[ARMOUR_MAX_FACTORS], lqdddes[ARMOUR_MAX_FACTORS];
    double lu[ARMOUR_MAX_FACTORS], lt[ARMOUR_MAX_FACTORS], lv[ARMOUR_MAX_FACTORS];
    for (int i = 0; i < n; i++) {
        lq[i] = q[(size_t)b * n + i]; lqd[i] = qd[(size_t)b * n + i];
        lqdes[i] = q_des[(size_t)b * n + i]; lqddes[i] = qd_des[(size_t)b * n + i]; lqdddes[i] = qdd_des[(size_t)b * n + i];
    }
    const bool ok = robust_update(a.md, a.imd, a.Kr, a.alpha, a.V_max, a.r_norm_threshold, lq, lqd, lqdes, lqddes, lqdddes, lu, lt, lv);
    for (int i = 0; i < n; i++) { u[(size_t)b * n + i] = lu[i]; tau[(size_t)b * n + i] = lt[i]; v[(size_t)b * n + i] = lv[i]; }
    if (!ok) atomicOr(status, 1);
}

// Latency form for few states -- the simulator's own call pattern is ONE state per ODE step (kinova_controller.cpp:19-84), and one lane
// working through robust_update is 1.35 ms of dependent interval arithmetic.  A block of four waves, lane = state in every wave:
//   wave 0  the nominal RNEA, and at the end the robust input from everybody's torques;
//   wave 3  the interval kinematics (Xli_i, Sb_i), published joint by joint through LDS;
//   wave 1  the interval dynamics of the torque enclosure, wave 2 those of M r, both reading the kinematics as they appear.
// Every quantity is computed by the same code in the same order as in the one-thread form: results are bit-identical
// (tests/test_controller.py).  Lanes past the last state shadow it, so that every wave runs its loops whole.  16 states per block: the
// kinematics of 64 would need 130 KB of LDS (and the first version, with a 154 KB dynamic allocation, ended in a memory-aperture violation
// that the core dump did not explain); with 16 everything is static and below 64 KB.
#define CTL_LDS __attribute__((address_space(3)))
constexpr int kSplitStates = 16;
constexpr int kKinWords = 18;   // Xli: R 9 + p 3, Sb: w 3 + v 3 intervals per joint
struct SplitLds {
    double u_nom[ARMOUR_MAX_FACTORS][kSplitStates];
    double u_int[ARMOUR_MAX_FACTORS][2][kSplitStates], Mr[ARMOUR_MAX_FACTORS][2][kSplitStates];   // intervals as {lo, hi} planes
    double kin[ARMOUR_MAX_FACTORS][kKinWords][2][kSplitStates];
    int joints_published;
};
__device__ inline void lds_put(CTL_LDS double (*p)[kSplitStates], int lane, Itv v) { p[0][lane] = v.lo; p[1][lane] = v.hi; }
__device__ inline Itv lds_get(const CTL_LDS double (*p)[kSplitStates], int lane) { return Itv{p[0][lane], p[1][lane]}; }
__global__ __launch_bounds__(256) void armour_controller_split_kernel(const CtlArgs* __restrict__ ap, int B, const double* __restrict__ q,
                                                                      const double* __restrict__ qd, const double* __restrict__ q_des,
                                                                      const double* __restrict__ qd_des, const double* __restrict__ qdd_des,
                                                                      double* __restrict__ u, double* __restrict__ tau, double* __restrict__ v,
                                                                      int* __restrict__ status) {
    __shared__ CtlArgs sa;
    __shared__ SplitLds xs;
    CTL_LDS SplitLds& x = *(CTL_LDS SplitLds*)&xs;   // (LDS-typed: ds instructions, no generic pointers into the exchange area)
    for (unsigned i2 = threadIdx.x; i2 < sizeof(CtlArgs) / sizeof(double); i2 += blockDim.x)
        reinterpret_cast<double*>(&sa)[i2] = reinterpret_cast<const double*>(ap)[i2];
    if (threadIdx.x == 0) x.joints_published = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b0 = blockIdx.x * kSplitStates + lane;
    const bool active = lane < kSplitStates && b0 < B;
    const int slot = lane < kSplitStates ? lane : kSplitStates - 1;   // (idle lanes shadow the last state of the block; only lanes < kSplitStates write)
    const bool own = lane < kSplitStates;
    const int b = min(blockIdx.x * kSplitStates + slot, B - 1);
    const CtlArgs& a = sa;
    const int n = a.md.n;
    double lq[ARMOUR_MAX_FACTORS], lqd[ARMOUR_MAX_FACTORS], lqdes[ARMOUR_MAX_FACTORS], lqddes[ARMOUR_MAX_FACTORS], lqdddes[ARMOUR_MAX_FACTORS];
    double qa_d[ARMOUR_MAX_FACTORS], qa_dd[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_FACTORS];
    for (int i = 0; i < n; i++) {
        lq[i] = q[(size_t)b * n + i]; lqd[i] = qd[(size_t)b * n + i];
        lqdes[i] = q_des[(size_t)b * n + i]; lqddes[i] = qd_des[(size_t)b * n + i]; lqdddes[i] = qdd_des[(size_t)b * n + i];
    }
    const double r_norm = robust_prepare(n, a.Kr, lq, lqd, lqdes, lqddes, lqdddes, qa_d, qa_dd, r);   // (every wave for itself: a few dozen operations)
    // the kinematics of joint i are in LDS once joints_published > i
    CTL_LDS SplitLds* const xp = &x;   // (the lambdas below capture by value: nothing of this frame is reached through a pointer)
    auto get = [xp, slot](int i, Xf<Itv>& Xli, Tw<Itv>& Sb) {
        CTL_LDS SplitLds& x = *xp;
        while (__hip_atomic_load(&x.joints_published, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) <= i) __builtin_amdgcn_s_sleep(1);
        for (int e = 0; e < 9; e++) Xli.R.a[e] = lds_get(x.kin[i][e], slot);
        for (int e = 0; e < 3; e++) { Xli.p.x[e] = lds_get(x.kin[i][9 + e], slot); Sb.w.x[e] = lds_get(x.kin[i][12 + e], slot); Sb.v.x[e] = lds_get(x.kin[i][15 + e], slot); }
    };
    if (wave == 0) {
        double t[ARMOUR_MAX_FACTORS];
        pass_rnea<double>(a.md, lq, lqd, qa_d, qa_dd, false, true, t);
        if (own) for (int i = 0; i < n; i++) x.u_nom[i][lane] = t[i];
    } else if (wave == 3) {
        rnea_kinematics(a.imd, lq, [xp, own, lane](int i, const Xf<Itv>& Xli, const Tw<Itv>& Sb) {
            CTL_LDS SplitLds& x = *xp;
            if (own) {
                for (int e = 0; e < 9; e++) lds_put(x.kin[i][e], lane, Xli.R.a[e]);
                for (int e = 0; e < 3; e++) { lds_put(x.kin[i][9 + e], lane, Xli.p.x[e]); lds_put(x.kin[i][12 + e], lane, Sb.w.x[e]); lds_put(x.kin[i][15 + e], lane, Sb.v.x[e]); }
            }
            // (the wave runs in lockstep: lane 0's release store follows every lane's writes of this joint)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0) __hip_atomic_store(&x.joints_published, i + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        });
    } else if (wave == 1) {
        Itv t[ARMOUR_MAX_FACTORS];
        rnea_dynamics(a.imd, get, lqd, qa_d, qa_dd, false, true, t);
        if (own) for (int i = 0; i < n; i++) lds_put(x.u_int[i], lane, t[i]);
    } else if (__ballot(r_norm > a.r_norm_threshold) != 0) {   // (no lane needs M r: nothing to do)
        Itv t[ARMOUR_MAX_FACTORS];
        double zero[ARMOUR_MAX_FACTORS];
        for (int i = 0; i < n; i++) zero[i] = 0.0;
        rnea_dynamics(a.imd, get, zero, zero, r, false, false, t);
        if (own) for (int i = 0; i < n; i++) lds_put(x.Mr[i], lane, t[i]);
    }
    __syncthreads();
    if (wave == 0 && active) {
        double lt[ARMOUR_MAX_FACTORS], lu[ARMOUR_MAX_FACTORS], lv[ARMOUR_MAX_FACTORS];
        Itv ui[ARMOUR_MAX_FACTORS], mr[ARMOUR_MAX_FACTORS];
        for (int i = 0; i < n; i++) { lt[i] = x.u_nom[i][lane]; ui[i] = lds_get(x.u_int[i], lane); mr[i] = lds_get(x.Mr[i], lane); }
        const bool ok = robust_combine(n, a.alpha, a.V_max, a.r_norm_threshold, r, r_norm, lt, ui, mr, lu, lv);
        for (int i = 0; i < n; i++) { u[(size_t)b * n + i] = lu[i]; tau[(size_t)b * n + i] = lt[i]; v[(size_t)b * n + i] = lv[i]; }
        if (!ok) atomicOr(status, 1);
    }
}

// Per-thread cache across calls: the MEX gateway this replaces is called once per ODE step with ONE state, so the fixed
// cost of a call matters more than the kernel.  Kept: the prepared models on the device (rebuilt only when the robot or the
// controller parameters change), the device buffer, and a page-locked staging buffer so that a small call is one H2D
// copy, one launch and one D2H copy on a private stream (first version: three hipMalloc / hipFree and ten blocking
// copies per call, 1.7 ms; now tens of microseconds).
struct CtlCache {
    bool have_model = false;
    ArmourRobot rb;
    double eps = 0, Kr[ARMOUR_MAX_FACTORS] = {0}, alpha = 0, V_max = 0, r_thr = 0;
    int n = 0, device = -1;
    // (the owners' destructors run at thread or process exit, when the runtime may already be gone: errors are ignored)
    DevStream stream;
    DevBuf<CtlArgs> d_args;
    DevBuf<double> d_buf;
    PinBuf<double> h_pin;
};
thread_local CtlCache g_ctl;

constexpr int kSplitMaxStates = kSplitStates * 256;   // up to one four-wave block per CU
constexpr size_t kStagedDoubles = (size_t)1 << 20;  // calls up to this many input doubles go through the page-locked buffer

}  // namespace

// C ABI: see include/armour_hip.h.  Host pointers; B states of n = robot->num_factors joints each, row-major [B][n].
static std::atomic<int> g_ctl_kernel{-1};
extern "C" int armour_controller_set_kernel(int32_t which) {
    if (which < -1 || which > 1) { armour_set_error("armour_controller_set_kernel: -1 (automatic), 0 or 1"); return ARMOUR_EINVAL; }
    g_ctl_kernel.store(which, std::memory_order_relaxed);
    return ARMOUR_OK;
}

extern "C" int armour_robust_controller(const ArmourRobot* robot, double model_uncertainty, const double* Kr, double alpha, double V_max,
                                        double r_norm_threshold, int32_t B, const double* q, const double* qd, const double* q_des,
                                        const double* qd_des, const double* qdd_des, double* u, double* tau, double* v) {
    if (!robot || !Kr || !q || !qd || !q_des || !qd_des || !qdd_des || !u || !tau || !v || B < 1) { armour_set_error("null or empty argument"); return ARMOUR_EINVAL; }
    // ---- arguments, before the device is touched (a non-finite state in a kernel is ~10^4 operations on NaN at best)
    const int nf = robot->num_factors;
    if (nf < 1 || nf > ARMOUR_MAX_FACTORS) { armour_set_error("armour_robust_controller: num_factors out of range"); return ARMOUR_EINVAL; }
    if (!finite_all(Kr, nf) || !std::isfinite(alpha) || !std::isfinite(V_max) || !std::isfinite(r_norm_threshold) || !(model_uncertainty >= 0) ||
        !std::isfinite(model_uncertainty)) {
        armour_set_error("armour_robust_controller: non-finite controller constant, or a model uncertainty that is negative or non-finite");
        return ARMOUR_EINVAL;
    }
    for (const double* x : {q, qd, q_des, qd_des, qdd_des})
        if (!finite_all(x, (size_t)B * nf)) { armour_set_error("armour_robust_controller: non-finite state or reference"); return ARMOUR_EINVAL; }
    CtlCache& c = g_ctl;
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (c.device != dev) {  // first call of this thread, or the caller switched devices: start over
        c.d_args.release();
        c.d_buf.release();
        c.stream.release();
        c.have_model = false;
        c.device = dev;
    }
    ARMOUR_TRY(c.stream.create());
    ARMOUR_TRY(c.d_args.reserve(1));
    bool same = c.have_model && memcmp(&c.rb, robot, sizeof(ArmourRobot)) == 0 && c.eps == model_uncertainty && c.alpha == alpha && c.V_max == V_max &&
                c.r_thr == r_norm_threshold;
    for (int i = 0; same && i < nf; i++) same = c.Kr[i] == Kr[i];
    if (!same) {
        CtlArgs args;
        memset(&args, 0, sizeof(args));
        if (build_models(*robot, model_uncertainty, args.md, args.imd) != 0) { armour_set_error("unsupported robot model (joint axes / count)"); return ARMOUR_EINVAL; }
        for (int i = 0; i < args.md.n; i++) args.Kr[i] = Kr[i];
        args.alpha = alpha; args.V_max = V_max; args.r_norm_threshold = r_norm_threshold;
        HIPCHK(hipMemcpy(c.d_args, &args, sizeof(args), hipMemcpyHostToDevice));
        c.rb = *robot; c.eps = model_uncertainty; c.alpha = alpha; c.V_max = V_max; c.r_thr = r_norm_threshold; c.n = args.md.n;
        for (int i = 0; i < c.n; i++) c.Kr[i] = Kr[i];
        c.have_model = true;
    }
    const int n = c.n;
    const size_t bn = (size_t)B * n, total = 8 * bn + 1;  // 5 inputs | 3 outputs | status word
    ARMOUR_TRY(c.d_buf.reserve(total));
    double* d_in = c.d_buf;
    double* d_out = c.d_buf + 5 * bn;
    int* d_status = reinterpret_cast<int*>(c.d_buf + 8 * bn);
    const double* in[5] = {q, qd, q_des, qd_des, qdd_des};
    double* out[3] = {u, tau, v};
    const bool staged = 5 * bn <= kStagedDoubles;
    if (staged) {
        ARMOUR_TRY(c.h_pin.reserve(total));
        for (int k = 0; k < 5; k++) memcpy(c.h_pin + (size_t)k * bn, in[k], bn * sizeof(double));
        HIPCHK(hipMemcpyAsync(d_in, c.h_pin, 5 * bn * sizeof(double), hipMemcpyHostToDevice, c.stream));
    } else {
        for (int k = 0; k < 5; k++) HIPCHK(hipMemcpyAsync(d_in + (size_t)k * bn, in[k], bn * sizeof(double), hipMemcpyHostToDevice, c.stream));
    }
    HIPCHK(hipMemsetAsync(d_status, 0, sizeof(double), c.stream));
    // few states: four waves per 16 states (latency); many: one lane per state (throughput) -- bit-identical results
    const int split_env = g_ctl_kernel.load(std::memory_order_relaxed);   // armour_controller_set_kernel: -1 automatic, 0 never, 1 always
    const bool split = split_env >= 0 ? split_env != 0 : B <= kSplitMaxStates;
    if (split)
        hipLaunchKernelGGL(armour_controller_split_kernel, dim3((B + kSplitStates - 1) / kSplitStates), dim3(256), 0, c.stream, c.d_args, B, d_in,
                           d_in + bn, d_in + 2 * bn, d_in + 3 * bn, d_in + 4 * bn, d_out, d_out + bn, d_out + 2 * bn, d_status);
    else
        hipLaunchKernelGGL(armour_controller_kernel, dim3((B + 63) / 64), dim3(64), 0, c.stream, c.d_args, B, d_in, d_in + bn, d_in + 2 * bn, d_in + 3 * bn, d_in + 4 * bn,
                           d_out, d_out + bn, d_out + 2 * bn, d_status);
    HIPCHK(hipGetLastError());
    int st = 0;
    if (staged) {
        HIPCHK(hipMemcpyAsync(c.h_pin + 5 * bn, d_out, (3 * bn + 1) * sizeof(double), hipMemcpyDeviceToHost, c.stream));
        if (armour_spin_on_stream(c.stream) != ARMOUR_OK) return ARMOUR_EDEVICE;
        for (int k = 0; k < 3; k++) memcpy(out[k], c.h_pin + (5 + (size_t)k) * bn, bn * sizeof(double));
        memcpy(&st, c.h_pin + 8 * bn, sizeof(int));
    } else {
        for (int k = 0; k < 3; k++) HIPCHK(hipMemcpyAsync(out[k], d_out + (size_t)k * bn, bn * sizeof(double), hipMemcpyDeviceToHost, c.stream));
        HIPCHK(hipMemcpyAsync(&st, d_status, sizeof(int), hipMemcpyDeviceToHost, c.stream));
        HIPCHK(hipStreamSynchronize(c.stream));
    }
    if (st) { armour_set_error("nominal model output falls outside interval output (robust_controller.cpp:88-94)"); return ARMOUR_ESTATE; }
    return ARMOUR_OK;
}
