// Host-side owners of what every entry point holds on the device -- buffers, page-locked host buffers, a stream, a pair of timing
// events, an instantiated graph -- and the argument checks the entries share.  Host code only: nothing here is seen by a kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/armour_hip.h"

void armour_set_error(const char* fmt, ...);

#define HIPCHK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e__ = (expr);                                                                         \
        if (e__ != hipSuccess) {                                                                         \
            armour_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return ARMOUR_EDEVICE;                                                                       \
        }                                                                                                \
    } while (0)

// for the calls that have reported their error already (reserve, upload, the event pair, ...)
#define ARMOUR_TRY(expr)                            \
    do {                                            \
        const int rc__ = (expr);                    \
        if (rc__ != ARMOUR_OK) return rc__;         \
    } while (0)

// An owning device buffer of `cap` elements; converts to its pointer wherever one is expected.  The ONE way to size a device buffer:
// reserve() keeps the buffer when need <= cap and otherwise frees it and allocates max(need, 1) elements (the contents are lost; a buffer
// that was never allocated counts as too small for any need, so the pointer is not null after a reserve that succeeded).
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    operator T*() const { return p; }
    template <class U> U* as() const { return reinterpret_cast<U*>(p); }   // a block of bytes that holds records
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
    // `fresh`, if given: set when the buffer was allocated anew
    int reserve(size_t need, bool* fresh = nullptr) {
        if (p && need <= cap) return ARMOUR_OK;
        release();
        const size_t count = need ? need : 1;
        HIPCHK(hipMalloc((void**)&p, count * sizeof(T)));
        cap = count;
        if (fresh) *fresh = true;
        return ARMOUR_OK;
    }
    int upload(const T* src, size_t count, hipStream_t st) {
        ARMOUR_TRY(reserve(count));
        if (count && src) HIPCHK(hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, st));
        return ARMOUR_OK;
    }
};

// An owning page-locked host buffer under the same reserve() contract.  From armour_alloc_pinned (api.hip): allocated with the default flags, so
// that kernels may write it in place, and listed in the registry of page-locked ranges the synchronous evaluation consults.  Only a unit
// that instantiates a PinBuf refers to those two functions.
template <class T>
struct PinBuf {
    T* p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(PinBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    PinBuf& operator=(PinBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~PinBuf() { release(); }
    operator T*() const { return p; }
    template <class U> U* as() const { return reinterpret_cast<U*>(p); }   // a block of bytes that holds records
    void release() {
        if (p) armour_free_pinned(p);
        p = nullptr; cap = 0;
    }
    int reserve(size_t need) {
        if (p && need <= cap) return ARMOUR_OK;
        release();
        const size_t count = need ? need : 1;
        void* q = nullptr;
        ARMOUR_TRY(armour_alloc_pinned(count * sizeof(T), &q));
        p = static_cast<T*>(q);
        cap = count;
        return ARMOUR_OK;
    }
};

// a non-blocking stream of the one-shot entries, of the planner handle and of the handles that are not planners
struct DevStream {
    hipStream_t s = nullptr;
    DevStream() = default;
    DevStream(const DevStream&) = delete;
    DevStream& operator=(const DevStream&) = delete;
    ~DevStream() { release(); }
    operator hipStream_t() const { return s; }
    void release() {
        if (s) (void)hipStreamDestroy(s);
        s = nullptr;
    }
    int create() {
        if (!s) HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return ARMOUR_OK;
    }
};

// two events around a piece of a stream's work, created on first use
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventPair() = default;
    EventPair(const EventPair&) = delete;
    EventPair& operator=(const EventPair&) = delete;
    ~EventPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    int record_start(hipStream_t st) {
        if (!e0) HIPCHK(hipEventCreate(&e0));
        if (!e1) HIPCHK(hipEventCreate(&e1));
        HIPCHK(hipEventRecord(e0, st));
        return ARMOUR_OK;
    }
    int record_stop(hipStream_t st) {
        HIPCHK(hipEventRecord(e1, st));
        return ARMOUR_OK;
    }
    // (both events must have completed: the caller has synchronised the stream)
    int elapsed_ms(double* ms) {
        float f = 0.f;
        HIPCHK(hipEventElapsedTime(&f, e0, e1));
        *ms = f;
        return ARMOUR_OK;
    }
};

// an instantiated graph: move-only, so that a vector of them destroys what it erases or clears
struct GraphExec {
    hipGraphExec_t g = nullptr;
    GraphExec() = default;
    explicit GraphExec(hipGraphExec_t g_) : g(g_) {}
    GraphExec(GraphExec&& o) noexcept : g(o.g) { o.g = nullptr; }
    GraphExec& operator=(GraphExec&& o) noexcept {
        if (this != &o) { release(); g = o.g; o.g = nullptr; }
        return *this;
    }
    ~GraphExec() { release(); }
    operator hipGraphExec_t() const { return g; }
    void release() {
        if (g) (void)hipGraphExecDestroy(g);
        g = nullptr;
    }
};

// ---- argument checks (no device call: they run before an entry touches the device)
// index of the first entry that is not finite, `count` if there is none
inline size_t first_nonfinite(const double* x, size_t count) {
    size_t i = 0;
    while (i < count && std::isfinite(x[i])) i++;
    return i;
}
inline bool finite_all(const double* x, size_t count) { return first_nonfinite(x, count) == count; }

// joints and factors a robot may have: 1 <= factors <= joints, within the compiled maxima
inline bool armour_robot_shape_ok(const ArmourRobot* robot) {
    return robot->num_factors >= 1 && robot->num_factors <= ARMOUR_MAX_FACTORS && robot->num_joints >= robot->num_factors && robot->num_joints <= ARMOUR_MAX_JOINTS;
}
inline int armour_check_robot_shape(const char* who, const ArmourRobot* robot) {
    if (armour_robot_shape_ok(robot)) return ARMOUR_OK;
    armour_set_error("%s: robot has %d joints, %d factors", who, robot->num_joints, robot->num_factors);
    return ARMOUR_EINVAL;
}
// W worlds of O obstacles each, as the roadmap check and the path audit take them
inline int armour_check_world_counts(const char* who, int32_t W, int32_t O, const double* obstacles) {
    if (W >= 0 && W <= 65535 && O >= 0 && O <= ARMOUR_ROADMAP_MAX_OBSTACLES && !(W > 0 && O > 0 && !obstacles)) return ARMOUR_OK;
    armour_set_error("%s: W = %d (0..65535), O = %d (0..%d)", who, W, O, ARMOUR_ROADMAP_MAX_OBSTACLES);
    return ARMOUR_EINVAL;
}
// the roadmap entries' capacity rule: points [W] is complete; a path longer than max_points was not written.  `wanted`: the rule applies
// (the tree planners': the caller gave a path array; the shortener's: always)
inline int armour_check_path_capacity(const char* who, int32_t W, const int32_t* points, int32_t max_points, bool wanted) {
    for (int32_t w = 0; wanted && w < W; w++)
        if (points[w] > max_points) { armour_set_error("%s: world %d's path of %d points, room for %d", who, w, points[w], max_points); return ARMOUR_ECAPACITY; }
    return ARMOUR_OK;
}
// a box [lb, ub] of n components: finite and ordered.  `what`: how the message names it ("sampling box", "box"); `noun`: a component ("joint", "axis")
inline int armour_check_box(const char* who, const char* what, const char* noun, int n, const double* lb, const double* ub) {
    for (int j = 0; j < n; j++)
        if (!std::isfinite(lb[j]) || !std::isfinite(ub[j]) || !(lb[j] <= ub[j])) { armour_set_error("%s: %s [%g, %g] of %s %d", who, what, lb[j], ub[j], noun, j); return ARMOUR_EINVAL; }
    return ARMOUR_OK;
}

// k result columns of W elements each, packed in one device buffer so that one copy brings all of them back: reserve, hand column i to the
// kernel, fetch (the caller synchronises the stream), copy column i -- or `span` columns from i, for a result of [W][span] -- to the caller's array
template <class T>
struct DevColumns {
    DevBuf<T> dev;
    std::vector<T> host;
    size_t W = 0;
    int reserve(int k, size_t W_) { W = W_; host.resize((size_t)k * W); return dev.reserve(host.size()); }
    T* column(int i) const { return dev.p + (size_t)i * W; }
    int fetch(hipStream_t st) {
        HIPCHK(hipMemcpyAsync(host.data(), dev, host.size() * sizeof(T), hipMemcpyDeviceToHost, st));
        return ARMOUR_OK;
    }
    const T* fetched(int i) const { return host.data() + (size_t)i * W; }
    void copy_out(int i, T* to, int span = 1) const {
        if (to) std::memcpy(to, fetched(i), (size_t)span * W * sizeof(T));
    }
};
