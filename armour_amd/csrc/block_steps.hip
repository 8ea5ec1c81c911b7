// Test hooks (include/armour_hip.h, armour_debug_block_steps / _split / _owner): tree_block.h's block steps on the caller's values, in a launch
// of one block that touches no planner state, and the two host-callable ones as they stand.
#include "common.h"
#include "tree_block.h"

using namespace treeblk;

namespace {

// ints: min_v | first | any | total, then sums [TP_BLOCK]
__global__ __launch_bounds__(TP_BLOCK) void block_steps_kernel(const double* d, const int32_t* v, const int32_t* flag, const int32_t* n, double* min_d, int32_t* ints) {
    __shared__ BlockKeys keys;
    __shared__ BlockWords words;
    const int t = threadIdx.x;
    double bd = d[t];
    int bv = v[t];
    block_argmin(keys, &bd, &bv);
    const int first = block_first(words, flag[t] != 0);
    const bool any = block_any(words, flag[t] != 0);
    int total;
    ints[4 + t] = block_scan(words, n[t], &total);
    if (t == 0) {
        *min_d = bd;
        ints[0] = bv; ints[1] = first; ints[2] = any ? 1 : 0; ints[3] = total;
    }
}

}  // namespace

extern "C" int armour_debug_block_steps(const double* d, const int32_t* v, const int32_t* flag, const int32_t* n, double* min_d, int32_t* min_v, int32_t* first,
                                        int32_t* any, int32_t* sums, int32_t* total) {
    const char* who = "armour_debug_block_steps";
    if (!d || !v || !flag || !n || !min_d || !min_v || !first || !any || !sums || !total) { armour_set_error("%s: null argument", who); return ARMOUR_EINVAL; }
    if (!armour_device_available()) { armour_set_error("%s: no HIP device visible", who); return ARMOUR_EDEVICE; }
    DevStream st;
    DevBuf<double> d_d, d_min;
    DevBuf<int32_t> d_in[3], d_ints;
    const int32_t* in[3] = {v, flag, n};
    int32_t ints[4 + TP_BLOCK];
    ARMOUR_TRY(st.create());
    ARMOUR_TRY(d_d.upload(d, TP_BLOCK, st));
    for (int k = 0; k < 3; k++) ARMOUR_TRY(d_in[k].upload(in[k], TP_BLOCK, st));
    ARMOUR_TRY(d_min.reserve(1));
    ARMOUR_TRY(d_ints.reserve(4 + TP_BLOCK));
    hipLaunchKernelGGL(block_steps_kernel, dim3(1), dim3(TP_BLOCK), 0, st, d_d.p, d_in[0].p, d_in[1].p, d_in[2].p, d_min.p, d_ints.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(min_d, d_min, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(ints, d_ints, sizeof(ints), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *min_v = ints[0]; *first = ints[1]; *any = ints[2]; *total = ints[3];
    std::memcpy(sums, ints + 4, TP_BLOCK * sizeof(int32_t));
    return ARMOUR_OK;
}

extern "C" int armour_debug_block_split(int32_t items, int32_t O, int32_t allowed, int32_t* split) {
    if (items < 1 || O < 0 || !split) { armour_set_error("armour_debug_block_split: items = %d (>= 1), O = %d (>= 0), or a null output", items, O); return ARMOUR_EINVAL; }
    for (int t = 0; t < TP_BLOCK; t++) {
        const ObstacleSplit sp = obstacle_split(items, O, allowed != 0, t);
        const int32_t row[4] = {sp.G, sp.per, sp.o0, sp.o1};
        std::memcpy(split + 4 * t, row, sizeof(row));
    }
    return ARMOUR_OK;
}

extern "C" int armour_debug_block_owner(const int32_t* end, int32_t n, int32_t count, const int32_t* item, int32_t* owner) {
    if (n < 0 || n > TP_BLOCK || count < 0 || (n > 0 && !end) || (count > 0 && (!item || !owner))) {
        armour_set_error("armour_debug_block_owner: n = %d (0..%d), count = %d, or a null argument", n, TP_BLOCK, count);
        return ARMOUR_EINVAL;
    }
    for (int32_t i = 0; i < count; i++) owner[i] = item_owner(end, n, item[i]);
    return ARMOUR_OK;
}
