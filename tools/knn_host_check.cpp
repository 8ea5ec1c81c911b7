// Build check of the roadmap search's host half (armour_amd/csrc/roadmap_knn.hip, roadmap_field.hip) under the host sanitizers: a program
// of its own that calls armour_roadmap_knn_host on a host handle (armour_roadmap_create_host) and the descend walk on a hand-built field,
// compares the search with a plain sort, runs the window rule's host twin (armour_roadmap_check_moving_host) and armour_roadmap_plan after it
// on a three-node roadmap, and prints what it found.
//   make -C armour_amd/csrc knnhost      (hipcc -Xarch_host -fsanitize=address,undefined; no GPU is used)
// It supplies the symbol the roadmap units take from api.hip, so that nothing else of the library is linked.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../armour_amd/csrc/roadmap_handle.h"
#include "host_check_robot.h"

static char g_error[512];
void armour_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

#define CHECK(expr)                                                               \
    do {                                                                          \
        if ((expr) != ARMOUR_OK) { printf("FAILED %s: %s\n", #expr, g_error); return 1; } \
    } while (0)

int main() {
    ArmourRobot robot;
    host_check_robot(&robot);
    const int n = robot.num_factors, N = 301, Q = 67;
    uint64_t seed = 2024;
    auto unit = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (double)(seed >> 11) / 9007199254740992.0; };
    std::vector<double> nodes((size_t)N * n), queries((size_t)Q * n);
    for (auto& x : nodes) x = -3.141592653589793 + 6.283185307179586 * unit();
    for (int j = 0; j < n; j++) nodes[(size_t)(N - 1) * n + j] = nodes[j];   // node N - 1 repeats node 0: a tie for the index to break
    for (auto& x : queries) x = -3.0 + 6.0 * unit();
    ArmourRoadmap* rm = nullptr;
    CHECK(armour_roadmap_create_host(&robot, N, nodes.data(), 0, nullptr, nullptr, 0.05, &rm));
    int checked = 0;
    for (int k : {1, 8, ARMOUR_ROADMAP_KNN_MAX}) {
        for (double radius : {(double)INFINITY, 4.0}) {
            std::vector<int32_t> index((size_t)Q * k), count(Q), excl(Q);
            std::vector<double> dist((size_t)Q * k);
            for (int i = 0; i < Q; i++) excl[i] = i % 3 ? i : -1;
            CHECK(armour_roadmap_knn_host(rm, Q, queries.data(), nullptr, excl.data(), k, radius, index.data(), dist.data(), count.data(), nullptr));
            for (int i = 0; i < Q; i++) {
                std::vector<std::pair<double, int>> all;
                for (int v = 0; v < N; v++) {
                    const double d = rmhost::wrapped_distance(rm->rb, &queries[(size_t)i * n], &nodes[(size_t)v * n]);
                    if (v != excl[i] && d <= radius) all.push_back({d, v});
                }
                std::sort(all.begin(), all.end());
                const int want = (int)std::min<size_t>(all.size(), (size_t)k);
                bool same = count[i] == want;
                for (int c = 0; same && c < k; c++)
                    same = c < want ? (index[(size_t)i * k + c] == all[c].second && dist[(size_t)i * k + c] == all[c].first)
                                    : (index[(size_t)i * k + c] == -1 && std::isinf(dist[(size_t)i * k + c]));
                if (!same) { printf("FAILED: query %d, k %d, radius %g differs from the plain sort\n", i, k, radius); return 1; }
                checked++;
            }
        }
    }
    int32_t idx[2], cnt[1];
    double dd[2];
    if (armour_roadmap_knn_host(rm, 1, queries.data(), nullptr, nullptr, 0, 1.0, idx, dd, cnt, nullptr) != ARMOUR_EINVAL ||
        armour_roadmap_knn_host(rm, 1, queries.data(), nullptr, nullptr, 2, -1.0, idx, dd, cnt, nullptr) != ARMOUR_EINVAL ||
        armour_roadmap_knn_host(rm, 1, queries.data(), cnt, nullptr, 2, 1.0, idx, dd, (cnt[0] = 0, cnt), nullptr) != ARMOUR_ESTATE) {
        printf("FAILED: a bad argument passed\n");
        return 1;
    }
    armour_roadmap_destroy(rm);
    // the window rule on the host: a box that reaches the end of the arm at t = 2 leaves the edge 0 -> 1 free in [0, 1] and blocks it in [0, 3]
    {
        std::vector<double> three((size_t)3 * n, 0.0);
        three[1] = three[n + 1] = three[2 * n + 1] = 0.6;
        three[n] = 0.5;
        three[2 * n] = 0.25;
        three[2 * n + 1] = -0.6;
        const int32_t edges[6] = {0, 1, 0, 2, 2, 1};
        const double box[24] = {0.0, 0.0, 3.5, 0.05, 0, 0, 0, 0.05, 0, 0, 0, 0.05,      // falls onto the arm's top at 1 m/s
                                50.0, 0.0, 0.0, 0.05, 0, 0, 0, 0.05, 0, 0, 0, 0.05};     // far away, at rest
        const double vel[6] = {0.0, 0.0, -1.0, 0.0, 0.0, 0.0}, from[1] = {0.0}, early[1] = {1.0}, late[1] = {3.0};
        uint8_t nf[3], ef[3];
        double cl[3], path[5 * ARMOUR_MAX_FACTORS];
        int32_t points = 0;
        CHECK(armour_roadmap_create_host(&robot, 3, three.data(), 3, edges, nullptr, 0.1, &rm));
        CHECK(armour_roadmap_check_moving_host(rm, 1, 2, box, vel, from, early, nf, ef, cl));
        CHECK(armour_roadmap_plan(rm, 0, three.data(), three.data() + n, 2, 5, path, &points));
        if (!ef[0] || points != 2) { printf("FAILED: window [0, 1]: edge %d, %d points\n", ef[0], points); return 1; }
        CHECK(armour_roadmap_check_moving_host(rm, 1, 2, box, vel, from, late, nf, ef, nullptr));
        CHECK(armour_roadmap_plan(rm, 0, three.data(), three.data() + n, 2, 5, path, &points));
        if (ef[0] || points == 2) { printf("FAILED: window [0, 3]: edge %d, %d points\n", ef[0], points); return 1; }
        if (armour_roadmap_check_moving_host(rm, 1, 2, box, vel, late, from, nf, ef, nullptr) != ARMOUR_EINVAL ||
            armour_roadmap_check_moving_host(rm, 1, 2, box, nullptr, from, late, nf, ef, nullptr) != ARMOUR_EINVAL) {
            printf("FAILED: a bad window or a null velocity passed\n");
            return 1;
        }
        armour_roadmap_destroy(rm);
    }
    // the descend walk on a chain 4 -> 3 -> 2 -> 1 -> 0 -> goal, joined at 4 (far) and 2 (near), and on successors that never arrive
    const double cost[5] = {1.0, 2.0, 3.0, 4.0, 5.0};
    const int32_t next[5] = {ARMOUR_ROADMAP_NEXT_GOAL, 0, 1, 2, 3}, loop[5] = {1, 0, 1, 2, 3};
    std::vector<int> seq;
    double total;
    CHECK(rmhost::descend_walk("knn_host_check", 5, 0, cost, next, {{0.5, 4}, {0.75, 2}}, &seq, &total));
    if (seq != std::vector<int>({2, 1, 0}) || total != 3.75) { printf("FAILED: walk of %zu nodes, length %g\n", seq.size(), total); return 1; }
    CHECK(rmhost::descend_walk("knn_host_check", 5, 0, cost, next, {}, &seq, &total));
    if (!seq.empty() || !std::isinf(total) || rmhost::descend_walk("knn_host_check", 5, 0, cost, loop, {{0.5, 4}}, &seq, &total) != ARMOUR_ESTATE) {
        printf("FAILED: the empty join or the walk without an end\n");
        return 1;
    }
    printf("knn host check ok: %d result lists equal a plain sort, the window rule frees and blocks the edge, the walk gives 2 1 0 and refuses a cycle\n", checked);
    return 0;
}
