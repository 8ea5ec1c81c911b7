// What the tree planner (tree_plan.hip) and the path shortener (path_shortcut.hip) share, one copy: the block shape, the scalar steps of the
// tree planner's rule that both apply to an edge a -> b (the wrapped joint difference, S of a prefix, one sub-segment's verdict, the node rule,
// the cut point), and the host twins' prefix with its margin.  include/armour_hip.h states the rule; everything here is the roadmap's
// geometry (roadmap_handle.h) called the same way by a kernel's lanes and by a host loop.
// The block shape and the counter hash u(seed, i, j) are also what the inverse kinematics (ik.hip) takes from here.
#pragma once
#include <climits>
#include <cmath>

#include "common.h"
#include "roadmap_handle.h"

namespace treeblk {

using namespace rmgeo;

constexpr int TP_BLOCK = 256;                 // four waves; a block is one world (its obstacles are staged in LDS)
constexpr int TP_WAVES = TP_BLOCK / 64;
constexpr int TP_NONE = INT_MAX;              // "no sub-segment collides" / the index of "no node"

// u(seed, i, j) of the header (the tree planner's samples, the inverse kinematics' start points): a splitmix64 finaliser of the counter, 53 bits -> [0, 1)
__host__ __device__ inline double tree_u(uint64_t seed, uint64_t i, uint64_t j) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (((i << 8) | j) + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1p-53;
}
__host__ __device__ inline double joint_diff(const RmRobot& rb, int j, double a, double b) { return rb.cont[j] ? wrap_diff(a, b) : b - a; }
// joint j of the point that ends the free prefix of m of S sub-segments of the edge a -> b
__host__ __device__ inline double cut_joint(const RmRobot& rb, int j, double a, double b, int m, int S) { return a + ((double)m / (double)S) * joint_diff(rb, j, a, b); }

// S of the edge a -> b as a prefix walks it (the argument checks keep every edge of a run below the cap; the clamp bounds the loop regardless)
__host__ __device__ inline int prefix_segments(const RmRobot& rb, const double* a, const double* b, double edge_step) {
    const int64_t S = edge_segments(rb, a, b, edge_step);
    return S > ARMOUR_TREE_MAX_SEGMENTS ? ARMOUR_TREE_MAX_SEGMENTS : (int)S;
}
// sub-segment s of S of the edge a -> b against the staged obstacles: the edge rule's enlarged test, verdict mode
__host__ __device__ inline bool segment_free(const RmRobot& rb, const double* a, const double* b, int s, int S, const double* obs, int O) {
    double q[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS];
    edge_sample(rb, a, b, s, S, q, r);
    return config_free(rb, q, r, obs, O, false, nullptr);
}
__host__ __device__ inline bool node_free(const RmRobot& rb, const double* x, const double* obs, int O) {
    double q[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS];
#pragma unroll
    for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q[j] = j < rb.n ? x[j] : 0.0;
#pragma unroll
    for (int l = 0; l < ARMOUR_MAX_JOINTS; l++) r[l] = 0.0;
    return config_free(rb, q, r, obs, O, false, nullptr);
}

// ---- the host twins' steps: the same functions in a loop.  margin (may be null): min |clearance| over the checks that decide.
struct HostWorld {
    const RmRobot& rb;
    const double* obs;
    int O;
    double edge_step;
    double* margin;

    void note(double (&q)[ARMOUR_MAX_FACTORS], double (&r)[ARMOUR_MAX_JOINTS]) const {
        double cl;
        config_free(rb, q, r, obs, O, true, &cl);
        *margin = std::fmin(*margin, std::fabs(cl));
    }
    bool node(const double* x) const {
        if (margin) {
            double q[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS] = {};
            for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q[j] = j < rb.n ? x[j] : 0.0;
            note(q, r);
        }
        return node_free(rb, x, obs, O);
    }
    int prefix(const double* a, const double* b, int* S_out) const {
        const int S = prefix_segments(rb, a, b, edge_step);
        *S_out = S;
        for (int s = 0; s < S; s++) {
            if (margin) {
                double q[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS];
                edge_sample(rb, a, b, s, S, q, r);
                note(q, r);
            }
            if (!segment_free(rb, a, b, s, S, obs, O)) return s;
        }
        return S;
    }
};

}  // namespace treeblk
