// Build check of the self-collision host entries (armour_amd/csrc/self_check.hip) under the host sanitizers: a program of its own that
// calls armour_self_check_host, armour_self_edges_host and armour_path_audit_self_host on 257 configurations of the Kinova (of fetch8 with -DARMOUR_KEY128: make selfhost8) and prints what it found.
//   make -C armour_amd/csrc selfhost      (hipcc -Xarch_host -fsanitize=address,undefined; no GPU is used)
// It supplies the two symbols self_check.hip takes from api.hip, so that nothing else of the library is linked.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/armour_hip.h"
#include "host_check_robot.h"

static char g_error[512];
void armour_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
extern "C" int armour_device_available(void) { return 0; }

#define CHECK(expr)                                                               \
    do {                                                                          \
        if ((expr) != ARMOUR_OK) { printf("FAILED %s: %s\n", #expr, g_error); return 1; } \
    } while (0)

int main() {
    ArmourRobot robot;
    host_check_robot(&robot);
    const int n = robot.num_factors, J = robot.num_joints, N = 257;
    uint64_t seed = 12345;
    auto unit = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (double)(seed >> 11) / 9007199254740992.0; };
    std::vector<double> q((size_t)N * n), qb((size_t)N * n);
    for (size_t i = 0; i < q.size(); i++) {
        q[i] = -3.0 + 6.0 * unit();
        qb[i] = q[i] + 0.4 * (unit() - 0.5);
    }
    for (int j = 0; j < n; j++) q[j] = HC_FOLDED[j];
    std::vector<uint8_t> pairs((size_t)J * J), free_(N), edge_free(N);
    std::vector<double> shrink((size_t)J * J, 0.002), clearance(N), t_hit(N), piece_clear(N), z((size_t)N * n, 0.0), k((size_t)N * n), ta(N, 0.0), tb(N, 0.5),
        tube((size_t)N * n, 0.001), k_range(n, 3.141592653589793 / 48);
    std::vector<int32_t> worst(N), verdict(N);
    for (auto& x : k) x = 2.0 * unit() - 1.0;
    CHECK(armour_self_pairs_default(&robot, pairs.data()));
    CHECK(armour_self_check_host(&robot, nullptr, nullptr, N, q.data(), free_.data(), nullptr, worst.data()));
    int hits = 0;
    for (int i = 0; i < N; i++) hits += !free_[i];
    CHECK(armour_self_check_host(&robot, pairs.data(), shrink.data(), N, q.data(), free_.data(), clearance.data(), worst.data()));
    CHECK(armour_self_edges_host(&robot, nullptr, 0.05, pairs.data(), shrink.data(), N, q.data(), qb.data(), edge_free.data()));
    CHECK(armour_path_audit_self_host(&robot, pairs.data(), shrink.data(), N, q.data(), z.data(), z.data(), k.data(), k_range.data(), 1.0, ta.data(), tb.data(),
                                      tube.data(), 0.01, verdict.data(), t_hit.data(), piece_clear.data()));
    int efree = 0, v[3] = {0, 0, 0};
    for (int i = 0; i < N; i++) {
        efree += edge_free[i];
        v[verdict[i]]++;
    }
    // by rule, on any robot: the verdict is the clearance's sign, and the same call again gives the same bytes
    std::vector<uint8_t> free2(N);
    std::vector<double> clearance2(N);
    std::vector<int32_t> worst2(N);
    CHECK(armour_self_check_host(&robot, pairs.data(), shrink.data(), N, q.data(), free2.data(), clearance2.data(), worst2.data()));
    for (int i = 0; i < N; i++)
        if (free_[i] != (clearance[i] > 0.0) || free2[i] != free_[i] || worst2[i] != worst[i] || std::memcmp(&clearance2[i], &clearance[i], sizeof(double))) {
            printf("FAILED: configuration %d: free %d with clearance %g, or the second call differs\n", i, free_[i], clearance[i]);
            return 1;
        }
    if ((HC_KINOVA_SCENE && (free_[0] || !(clearance[0] < 0.0) || verdict[0] != 1)) || armour_self_check_host(&robot, nullptr, nullptr, -1, nullptr, nullptr, nullptr, nullptr) != ARMOUR_EINVAL) {
        printf("FAILED: the folded configuration is free (clearance %g, verdict %d), or a bad argument passed\n", clearance[0], verdict[0]);
        return 1;
    }
    printf("self host check ok: %d of %d configurations collide, %d self-free edges, pieces free / hit / undecided = %d / %d / %d\n", hits, N, efree, v[0], v[1], v[2]);
    return 0;
}
