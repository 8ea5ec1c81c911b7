// armour_althoff_controller: the reference's tracking controller with the robust input of Giusti and Althoff, for a BATCH of states.
//
// Replaces kinova_controller_ALTHOFF.cpp:19-90 (the MEX gateway: builds the model and a RobustController with (Kr, Kp, Ki, maxError),
// calls update once) for B states at a time -- the call pattern of kinova_compare_robust_controller.m's get_control_inputs loop, which
// asks for the input at every recorded node of every rollout.  One lane per state; the per-state arithmetic is controller_core.h's
// althoff_update (robust_controller.cpp:63-128), the models are those of armour_robust_controller (controller_models.h).
//
// A unit of its own: controller.o holds exactly the ARMOUR method's two kernels (tools/check_controller_codegen.py's default), and this
// kernel is held to the same rule -- one function, static stack -- by the Makefile's check on althoff.resources.txt.  There is no four-wave
// latency form and no cache across calls: a lone state is slower here than on one CPU core for the ARMOUR method already (DESIGN.md 8
// item 9), and the study calls this entry with tens of thousands of states, where the allocations of a call are noise.
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "controller_core.h"
#include "controller_models.h"

namespace {

using namespace ctl;

struct AlthoffArgs {
    Model<double> md;
    Model<Itv> imd;
    double Kr[ARMOUR_MAX_FACTORS];
    double Kp[2], Ki[2];
};

__global__ __launch_bounds__(64) void armour_althoff_kernel(const AlthoffArgs* __restrict__ ap, int B, const double* __restrict__ e_acc,
                                                            const double* __restrict__ q, const double* __restrict__ qd,
                                                            const double* __restrict__ q_des, const double* __restrict__ qd_des,
                                                            const double* __restrict__ qdd_des, double* __restrict__ u, double* __restrict__ tau,
                                                            double* __restrict__ v, int* __restrict__ status) {
    // the models go to LDS first, as in armour_controller_kernel: every entry is read on a chain of ~10^4 dependent operations
    __shared__ AlthoffArgs sa;
    static_assert(sizeof(AlthoffArgs) % sizeof(double) == 0, "AlthoffArgs is copied as doubles");
    for (unsigned i2 = threadIdx.x; i2 < sizeof(AlthoffArgs) / sizeof(double); i2 += blockDim.x)
        reinterpret_cast<double*>(&sa)[i2] = reinterpret_cast<const double*>(ap)[i2];
    __syncthreads();
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const AlthoffArgs& a = sa;
    const int n = a.md.n;
    double lq[ARMOUR_MAX_FACTORS], lqd[ARMOUR_MAX_FACTORS], lqdes[ARMOUR_MAX_FACTORS], lqddes[ARMOUR_MAX_FACTORS], lqdddes[ARMOUR_MAX_FACTORS];
    double lu[ARMOUR_MAX_FACTORS], lt[ARMOUR_MAX_FACTORS], lv[ARMOUR_MAX_FACTORS];
    for (int i = 0; i < n; i++) {
        lq[i] = q[(size_t)b * n + i]; lqd[i] = qd[(size_t)b * n + i];
        lqdes[i] = q_des[(size_t)b * n + i]; lqddes[i] = qd_des[(size_t)b * n + i]; lqdddes[i] = qdd_des[(size_t)b * n + i];
    }
    const bool ok = althoff_update(a.md, a.imd, a.Kr, a.Kp, a.Ki, e_acc[b], lq, lqd, lqdes, lqddes, lqdddes, lu, lt, lv);
    for (int i = 0; i < n; i++) { u[(size_t)b * n + i] = lu[i]; tau[(size_t)b * n + i] = lt[i]; v[(size_t)b * n + i] = lv[i]; }
    if (!ok) atomicOr(status, 1);
}

}  // namespace

// C ABI: see include/armour_hip.h.  Host pointers; B states of n = robot->num_factors joints each, row-major [B][n].
extern "C" int armour_althoff_controller(const ArmourRobot* robot, double model_uncertainty, const double* Kr, const double Kp[2], const double Ki[2],
                                         const double* e_acc, int32_t B, const double* q, const double* qd, const double* q_des,
                                         const double* qd_des, const double* qdd_des, double* u, double* tau, double* v) {
    // ---- arguments, before the device is touched
    if (!robot || !Kr || !Kp || !Ki || !q || !qd || !q_des || !qd_des || !qdd_des || !u || !tau || !v || B < 1) {
        armour_set_error("armour_althoff_controller: null or empty argument");
        return ARMOUR_EINVAL;
    }
    const int nf = robot->num_factors;
    if (nf < 1 || nf > ARMOUR_MAX_FACTORS) { armour_set_error("armour_althoff_controller: num_factors out of range"); return ARMOUR_EINVAL; }
    if (!finite_all(Kr, nf) || !finite_all(Kp, 2) || !finite_all(Ki, 2) || !(model_uncertainty >= 0) || !std::isfinite(model_uncertainty)) {
        armour_set_error("armour_althoff_controller: non-finite gain, or a model uncertainty that is negative or non-finite");
        return ARMOUR_EINVAL;
    }
    const size_t bn = (size_t)B * nf;
    for (const double* x : {q, qd, q_des, qd_des, qdd_des})
        if (!finite_all(x, bn)) { armour_set_error("armour_althoff_controller: non-finite state or reference"); return ARMOUR_EINVAL; }
    if (e_acc && !finite_all(e_acc, B)) { armour_set_error("armour_althoff_controller: non-finite e_acc"); return ARMOUR_EINVAL; }
    std::vector<AlthoffArgs> args(1);   // (on the heap: the two models are tens of KB)
    AlthoffArgs& aa = args[0];
    memset(&aa, 0, sizeof(aa));
    if (build_models(*robot, model_uncertainty, aa.md, aa.imd) != 0) { armour_set_error("armour_althoff_controller: unsupported robot model (joint axes / count)"); return ARMOUR_EINVAL; }
    for (int i = 0; i < nf; i++) aa.Kr[i] = Kr[i];
    for (int i = 0; i < 2; i++) { aa.Kp[i] = Kp[i]; aa.Ki[i] = Ki[i]; }
    // ---- the device
    if (!armour_device_available()) { armour_set_error("armour_althoff_controller: no HIP device visible (there is no CPU path)"); return ARMOUR_EDEVICE; }
    DevStream stream;
    DevBuf<AlthoffArgs> d_args;
    DevBuf<double> d_buf;   // e_acc [B] | 5 inputs [B][n] | 3 outputs [B][n] | status word
    ARMOUR_TRY(stream.create());
    ARMOUR_TRY(d_args.reserve(1));
    ARMOUR_TRY(d_buf.reserve((size_t)B + 8 * bn + 1));
    double* d_e = d_buf;
    double* d_in = d_buf + B;
    double* d_out = d_in + 5 * bn;
    int* d_status = reinterpret_cast<int*>(d_out + 3 * bn);
    HIPCHK(hipMemcpyAsync(d_args, &aa, sizeof(AlthoffArgs), hipMemcpyHostToDevice, stream));
    if (e_acc) HIPCHK(hipMemcpyAsync(d_e, e_acc, (size_t)B * sizeof(double), hipMemcpyHostToDevice, stream));
    else HIPCHK(hipMemsetAsync(d_e, 0, (size_t)B * sizeof(double), stream));   // (all-zero bytes: +0.0)
    const double* in[5] = {q, qd, q_des, qd_des, qdd_des};
    for (int k = 0; k < 5; k++) HIPCHK(hipMemcpyAsync(d_in + (size_t)k * bn, in[k], bn * sizeof(double), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(d_status, 0, sizeof(double), stream));
    hipLaunchKernelGGL(armour_althoff_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, d_args, B, d_e, d_in, d_in + bn, d_in + 2 * bn, d_in + 3 * bn,
                       d_in + 4 * bn, d_out, d_out + bn, d_out + 2 * bn, d_status);
    HIPCHK(hipGetLastError());
    double* out[3] = {u, tau, v};
    int st = 0;
    for (int k = 0; k < 3; k++) HIPCHK(hipMemcpyAsync(out[k], d_out + (size_t)k * bn, bn * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(&st, d_status, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (st) { armour_set_error("armour_althoff_controller: nominal model output falls outside interval output (robust_controller.cpp:94-101)"); return ARMOUR_ESTATE; }
    return ARMOUR_OK;
}
