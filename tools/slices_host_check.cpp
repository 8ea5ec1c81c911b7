// Build check of the time slices' host half (armour_amd/csrc/roadmap_slices.hip) under the host sanitizers: a program of its own that runs
// armour_roadmap_check_slices_host on a small random roadmap with a falling box, compares every bit with armour_roadmap_check_moving_host on
// that slice's window (K = 1, 33 and 64: the full-width mask), then runs armour_roadmap_arrival_host and follows the path it returns, and
// prints what it found.
//   make -C armour_amd/csrc sliceshost      (hipcc -Xarch_host -fsanitize=address,undefined; no GPU is used)
// It supplies the symbol the roadmap units take from api.hip, so that nothing else of the library is linked.
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
    const int n = robot.num_factors, N = 24, W = 2, O = 2;
    uint64_t seed = 77;
    auto unit = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (double)(seed >> 11) / 9007199254740992.0; };
    std::vector<double> nodes((size_t)N * n);
    for (auto& x : nodes) x = -1.0 + 2.0 * unit();
    std::vector<int32_t> edges;
    for (int i = 0; i < N; i++)
        for (int d : {1, 5}) { edges.push_back(i); edges.push_back((i + d) % N); }
    const int E = (int)edges.size() / 2;
    // per world: a box that falls onto the arm at 1 m/s (from another height in world 1) and a box at rest far away
    const double box[W * O * 12] = {0.0, 0.0, 2.5, 0.05, 0, 0, 0, 0.05, 0, 0, 0, 0.05, 50.0, 0.0, 0.0, 0.05, 0, 0, 0, 0.05, 0, 0, 0, 0.05,
                                    0.1, 0.0, 3.0, 0.05, 0, 0, 0, 0.05, 0, 0, 0, 0.05, 50.0, 0.0, 0.0, 0.05, 0, 0, 0, 0.05, 0, 0, 0, 0.05};
    const double vel[W * O * 3] = {0, 0, -1.0, 0, 0, 0, 0, 0, -1.0, 0, 0, 0}, t0[W] = {0.0, 0.25};
    ArmourRoadmap* rm = nullptr;
    CHECK(armour_roadmap_create_host(&robot, N, nodes.data(), E, edges.data(), nullptr, 0.2, &rm));
    // the extras: start (node 0's configuration, moved a little) and goal (node 12's) joined to two nodes each, and the two degenerate edges
    std::vector<double> start(nodes.begin(), nodes.begin() + n), goal(nodes.begin() + 12 * n, nodes.begin() + 13 * n);
    for (int j = 0; j < n; j++) { start[j] += 0.05; goal[j] -= 0.05; }
    const int Q = W * 6;
    std::vector<int32_t> xw(Q), xu, xv;
    std::vector<double> xa((size_t)Q * n), xb((size_t)Q * n), xl;
    for (int w = 0; w < W; w++) {
        const double* a[6] = {start.data(), start.data(), goal.data(), goal.data(), start.data(), goal.data()};
        const double* b[6] = {&nodes[0], &nodes[(size_t)1 * n], &nodes[(size_t)12 * n], &nodes[(size_t)11 * n], start.data(), goal.data()};
        for (int i = 0; i < 6; i++) {
            xw[w * 6 + i] = w;
            for (int j = 0; j < n; j++) { xa[((size_t)w * 6 + i) * n + j] = a[i][j]; xb[((size_t)w * 6 + i) * n + j] = b[i][j]; }
        }
    }
    for (int w = 0; w < W; w++) {
        const int ends[4] = {0, 1, 12, 11};
        for (int i = 0; i < 4; i++) {
            xu.push_back(i < 2 ? N : N + 1);
            xv.push_back(ends[i]);
            xl.push_back(rmhost::wrapped_distance(rm->rb, &xa[((size_t)w * 6 + i) * n], &xb[((size_t)w * 6 + i) * n]));
        }
    }
    long bits = 0, differing = 0;
    for (int K : {1, 33, 64}) {
        const double dt = 2.5 / K;
        std::vector<uint64_t> ns((size_t)W * N), es((size_t)W * E), xs(Q);
        std::vector<double> times((size_t)W * (K + 1));
        CHECK(armour_roadmap_check_slices_host(rm, W, O, box, vel, t0, dt, K, Q, xw.data(), xa.data(), xb.data(), ns.data(), es.data(), xs.data(), times.data()));
        std::vector<uint8_t> nf((size_t)W * N), ef((size_t)W * E);
        for (int k = 0; k < K; k++) {
            double from[W], to[W];
            for (int w = 0; w < W; w++) { from[w] = times[(size_t)w * (K + 1) + k]; to[w] = times[(size_t)w * (K + 1) + k + 1]; }
            CHECK(armour_roadmap_check_moving_host(rm, W, O, box, vel, from, to, nf.data(), ef.data(), nullptr));
            for (size_t i = 0; i < ns.size(); i++, bits++)
                if (((ns[i] >> k) & 1) != nf[i]) { printf("FAILED: K %d slice %d node row %zu\n", K, k, i); return 1; }
            for (size_t i = 0; i < es.size(); i++, bits++)
                if (((es[i] >> k) & 1) != ef[i]) { printf("FAILED: K %d slice %d edge row %zu\n", K, k, i); return 1; }
        }
        for (uint64_t m : ns) {
            if (K < 64 && (m >> K)) { printf("FAILED: K %d: a bit past the last slice\n", K); return 1; }
            differing += m != 0 && m != (K < 64 ? (1ull << K) - 1 : ~0ull);
        }
        // the search: start N, goal N + 1, joined as above; the path must start at N, end at N + 1 at goal_slice, with rising slices
        std::vector<int32_t> aw;
        std::vector<uint64_t> am, sm(W), gm(W);
        for (int w = 0; w < W; w++) {
            for (int i = 0; i < 4; i++) { aw.push_back(w); am.push_back(xs[(size_t)w * 6 + i]); }
            sm[w] = xs[(size_t)w * 6 + 4];
            gm[w] = xs[(size_t)w * 6 + 5];
        }
        std::vector<uint64_t> reach((size_t)W * (N + 2));
        std::vector<int32_t> gs(W), pl(W), pn((size_t)W * 64), ps((size_t)W * 64), sweeps(W);
        CHECK(armour_roadmap_arrival_host(rm, 0.4, (int)aw.size(), aw.data(), xu.data(), xv.data(), xl.data(), am.data(), sm.data(), gm.data(), reach.data(), gs.data(),
                                          pl.data(), pn.data(), ps.data(), sweeps.data()));
        for (int w = 0; w < W; w++) {
            if (sweeps[w] < 1 || sweeps[w] > K + 1) { printf("FAILED: K %d world %d: %d sweeps\n", K, w, sweeps[w]); return 1; }
            if (gs[w] < 0) { if (pl[w] != 0) { printf("FAILED: a path without a goal slice\n"); return 1; } continue; }
            const int32_t *p = &pn[(size_t)w * 64], *s = &ps[(size_t)w * 64];
            bool ok = pl[w] >= 2 && p[0] == N && p[pl[w] - 1] == N + 1 && s[pl[w] - 1] == gs[w] && ((reach[(size_t)w * (N + 2) + N + 1] >> gs[w]) & 1);
            for (int i = 1; ok && i < pl[w]; i++) ok = s[i] > s[i - 1] && ((reach[(size_t)w * (N + 2) + p[i]] >> s[i]) & 1);
            if (!ok) { printf("FAILED: K %d world %d: the path of %d entries\n", K, w, pl[w]); return 1; }
            printf("K %d world %d: goal slice %d, %d path entries, %d sweeps\n", K, w, gs[w], pl[w], sweeps[w]);
        }
    }
    if (differing == 0) { printf("FAILED: no node's slices differ: the falling box never arrives\n"); return 1; }
    // refusals
    if (armour_roadmap_check_slices_host(rm, W, O, box, vel, t0, 0.1, 65, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != ARMOUR_EINVAL ||
        armour_roadmap_check_slices_host(rm, W, O, box, vel, t0, 0.0, 4, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != ARMOUR_EINVAL ||
        armour_roadmap_arrival_host(rm, 0.0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != ARMOUR_EINVAL) {
        printf("FAILED: a bad argument passed\n");
        return 1;
    }
    armour_roadmap_destroy(rm);
    printf("slices host check ok: %ld bits equal the window rule slice by slice, %ld node rows change between slices, the paths rise from start to goal\n", bits,
           differing);
    return 0;
}
