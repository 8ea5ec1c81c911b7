// Build check of the workspace tree's host twin (armour_amd/csrc/ws_tree.hip) under the host sanitizers: a program of its own that calls
// armour_ws_tree_plan_host on a wall with a window (the straight segment collides, so the tree has to go through the window or around), with
// and without an initial chain, at the node cap and with every optional output absent, checks what every run must satisfy -- every parent
// chain reaches the root within count steps, cost_k = cost_parent + |x_k - x_parent| bit for bit, the path runs from the start to a node
// whose distance to the goal is goal_dist, the same seed gives the same bytes -- and the refusals, and prints what it found.
// Then the resident trees' host handle (armour_ws_trees_create_host / _grow / _read / _destroy): instalments of a permuted subset and of
// every world must leave each world with the bytes of one plan of its own sum; a blocked start, ECAPACITY by slot, the refusals.
// And the moving twin (armour_ws_tree_plan_moving_host): zero velocity against the static call for two sets of windows, a drifting wall, one
// box that arrives at the start point, the refusals.
//   make -C armour_amd/csrc wshost      (hipcc -Xarch_host -fsanitize=address,undefined; no GPU is used)
// It supplies the symbols ws_tree.hip takes from api.hip, so that nothing else of the library is linked.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/armour_hip.h"

static char g_error[512];
void armour_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
extern "C" int armour_device_available(void) { return 0; }

static void box(std::vector<double>* out, double cx, double cy, double cz, double hx, double hy, double hz) {
    const double Z[12] = {cx, cy, cz, hx, 0, 0, 0, hy, 0, 0, 0, hz};
    out->insert(out->end(), Z, Z + 12);
}

struct Out {
    std::vector<int32_t> status, iterations, points, rewires, kept, count, parent;
    std::vector<double> path_cost, goal_dist, path, nodes, cost, margin;
};

int main() {
    const int W = 3, O = 4, cap = 512, iters = 300, max_init = 4;
    const double lb[3] = {-0.1, -0.7, -0.1}, ub[3] = {1.1, 0.7, 1.1}, start[3] = {0.1, -0.3, 0.2}, goal[3] = {0.9, 0.3, 0.8};
    std::vector<double> obstacles, starts, goals;
    for (int w = 0; w < W; w++) {
        box(&obstacles, 0.5, -0.35, 0.5, 0.02, 0.25, 0.5);
        box(&obstacles, 0.5, 0.35, 0.5, 0.02, 0.25, 0.5);
        box(&obstacles, 0.5, 0.0, 0.2, 0.02, 0.1, 0.2);
        box(&obstacles, 0.5, 0.0, 0.8, 0.02, 0.1, 0.2);
        starts.insert(starts.end(), start, start + 3);
        goals.insert(goals.end(), goal, goal + 3);
    }
    // world 1's chain: its third edge crosses the wall beside the window; world 2's goes through the window to the goal
    const double chains[W][max_init][3] = {{}, {{0.2, -0.2, 0.3}, {0.4, 0.0, 0.5}, {0.6, 0.3, 0.5}, {0.8, 0.3, 0.7}}, {{0.4, 0.0, 0.5}, {0.6, 0.0, 0.5}, {0.9, 0.3, 0.8}}};
    const int32_t chain_count[W] = {0, 4, 3};
    const uint64_t seeds[W] = {1, 2, 3};
    auto run = [&](Out* o, int32_t nodes_cap, int32_t room, bool with_chain, double radius) {
        o->status.assign(W, -1); o->iterations.assign(W, -1); o->points.assign(W, -1); o->rewires.assign(W, -1); o->kept.assign(W, -1); o->count.assign(W, -1);
        o->parent.assign((size_t)W * nodes_cap, -7); o->path_cost.assign(W, -1.0); o->goal_dist.assign(W, -1.0); o->path.assign((size_t)W * (room ? room : 1) * 3, 0.0);
        o->nodes.assign((size_t)W * nodes_cap * 3, 0.0); o->cost.assign((size_t)W * nodes_cap, 0.0); o->margin.assign(W, 0.0);
        return armour_ws_tree_plan_host(lb, ub, W, O, obstacles.data(), starts.data(), goals.data(), seeds, max_init, with_chain ? &chains[0][0][0] : nullptr,
                                        with_chain ? chain_count : nullptr, 0.1, 0.01, radius, 0.1, 0.01, 0.01, iters, nodes_cap, room, o->status.data(),
                                        o->iterations.data(), o->points.data(), o->rewires.data(), o->kept.data(), o->path_cost.data(), o->goal_dist.data(),
                                        o->path.data(), o->count.data(), o->nodes.data(), o->parent.data(), o->cost.data(), o->margin.data());
    };
    auto check_trees = [&](const Out& a, int32_t nodes_cap, int32_t room) {
        for (int w = 0; w < W; w++) {
            const int c = a.count[w], P = a.points[w];
            const double* x = &a.nodes[(size_t)w * nodes_cap * 3];
            const int32_t* par = &a.parent[(size_t)w * nodes_cap];
            const double* cost = &a.cost[(size_t)w * nodes_cap];
            if (c < 1 || c > nodes_cap || par[0] != -1 || cost[0] != 0.0 || std::memcmp(x, start, sizeof(start))) { printf("FAILED: world %d: the root\n", w); return false; }
            for (int k = 1; k < c; k++) {
                int steps = 0;
                for (int v = k; v != 0; v = par[v])
                    if (par[v] < 0 || par[v] >= c || ++steps >= c) { printf("FAILED: world %d: node %d does not reach the root\n", w, k); return false; }
                const double* p = x + (size_t)par[k] * 3;
                const double D[3] = {x[3 * k] - p[0], x[3 * k + 1] - p[1], x[3 * k + 2] - p[2]};
                if (cost[k] != cost[par[k]] + std::sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2])) { printf("FAILED: world %d: the cost of node %d\n", w, k); return false; }
            }
            const double* path = &a.path[(size_t)w * room * 3];
            if (P < 1 || P > c || std::memcmp(path, start, sizeof(start))) { printf("FAILED: world %d: a path of %d points\n", w, P); return false; }
            const double* e = path + (size_t)(P - 1) * 3;
            const double D[3] = {goal[0] - e[0], goal[1] - e[1], goal[2] - e[2]};
            if (a.goal_dist[w] != std::sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]) || (a.status[w] == ARMOUR_WS_REACHED) != (a.goal_dist[w] <= 0.01)) {
                printf("FAILED: world %d: status %d, goal_dist %g\n", w, a.status[w], a.goal_dist[w]);
                return false;
            }
            if (!(a.margin[w] > 0.0)) { printf("FAILED: world %d: margin %g\n", w, a.margin[w]); return false; }
        }
        return true;
    };
    Out a, b, c;
    if (run(&a, cap, cap, true, 0.2) != ARMOUR_OK || run(&b, cap, cap, true, 0.2) != ARMOUR_OK) { printf("FAILED: %s\n", g_error); return 1; }
    if (a.status != b.status || a.iterations != b.iterations || a.points != b.points || a.rewires != b.rewires || a.count != b.count || a.parent != b.parent ||
        std::memcmp(a.path.data(), b.path.data(), a.path.size() * sizeof(double)) || std::memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * sizeof(double)) ||
        std::memcmp(a.cost.data(), b.cost.data(), a.cost.size() * sizeof(double))) {
        printf("FAILED: the same call twice gave different results\n");
        return 1;
    }
    if (!check_trees(a, cap, cap)) return 1;
    if (a.kept[0] != 0 || a.kept[1] != 2 || a.kept[2] != 3 || a.status[2] != ARMOUR_WS_REACHED || a.rewires[0] <= 0) {
        printf("FAILED: chains kept %d %d %d, status %d, rewires %d\n", a.kept[0], a.kept[1], a.kept[2], a.status[2], a.rewires[0]);
        return 1;
    }
    // plain RRT, no chain; a tree at its cap of 8 nodes (the chain of world 1 stops there or before)
    if (run(&c, cap, cap, false, 0.0) != ARMOUR_OK || !check_trees(c, cap, cap) || c.rewires[0] || c.rewires[1] || c.rewires[2]) { printf("FAILED: plain RRT: %s\n", g_error); return 1; }
    if (run(&c, 8, 8, true, 0.2) != ARMOUR_OK || !check_trees(c, 8, 8) || c.count[0] != 8 || c.iterations[0] >= iters) { printf("FAILED: the full tree: %s\n", g_error); return 1; }
    // too little room for a path: ECAPACITY with the points complete; the optional outputs may all be absent
    if (run(&b, cap, 2, true, 0.2) != ARMOUR_ECAPACITY || b.points != a.points) { printf("FAILED: a path longer than max_points was not refused\n"); return 1; }
    std::vector<int32_t> st(W), it(W), pt(W), rw(W), kp(W);
    std::vector<double> pc(W), gd(W);
    auto bare = [&](double step, double edge_step, double radius, double rate, double buffer, int32_t n_iter, int32_t nodes_cap) {
        return armour_ws_tree_plan_host(lb, ub, W, O, obstacles.data(), starts.data(), goals.data(), seeds, max_init, &chains[0][0][0], chain_count, step, edge_step, radius,
                                        rate, buffer, 0.01, n_iter, nodes_cap, 0, st.data(), it.data(), pt.data(), rw.data(), kp.data(), pc.data(), gd.data(), nullptr,
                                        nullptr, nullptr, nullptr, nullptr, nullptr);
    };
    if (bare(0.1, 0.01, 0.2, 0.1, 0.01, iters, cap) != ARMOUR_OK || st != a.status || it != a.iterations || pt != a.points || rw != a.rewires ||
        std::memcmp(pc.data(), a.path_cost.data(), W * sizeof(double))) {
        printf("FAILED: the call without optional outputs: %s\n", g_error);
        return 1;
    }
    if (bare(0.0, 0.01, 0.2, 0.1, 0.0, iters, cap) != ARMOUR_EINVAL || bare(0.1, -1.0, 0.2, 0.1, 0.0, iters, cap) != ARMOUR_EINVAL ||
        bare(0.1, 0.01, -0.2, 0.1, 0.0, iters, cap) != ARMOUR_EINVAL || bare(0.1, 0.01, 0.2, 1.5, 0.0, iters, cap) != ARMOUR_EINVAL ||
        bare(0.1, 0.01, 0.2, 0.1, -0.1, iters, cap) != ARMOUR_EINVAL || bare(0.1, 0.01, 0.2, 0.1, 0.0, -1, cap) != ARMOUR_EINVAL ||
        bare(0.1, 0.01, 0.2, 0.1, 0.0, iters, 0) != ARMOUR_EINVAL || bare(0.1, 0.01, 0.2, 0.1, 0.0, iters, ARMOUR_WS_MAX_NODES + 1) != ARMOUR_EINVAL ||
        bare(0.1, 0.00001, 0.2, 0.1, 0.0, iters, cap) != ARMOUR_EINVAL) {
        printf("FAILED: a bad argument passed\n");
        return 1;
    }
    // ---- resident trees on the host handle: create_host / grow / read / destroy.  Three instalments (100 + 0 + 200; the second empty) of
    // a subset in permuted order, then of everyone, must leave every world with the bytes of ONE plan of its own sum from the same start.
    {
        ArmourWsTrees* h = nullptr;
        if (armour_ws_trees_create_host(lb, ub, W, O, obstacles.data(), goals.data(), seeds, 0.1, 0.01, 0.2, 0.1, 0.01, 0.01, cap, &h) != ARMOUR_OK || !h) {
            printf("FAILED: create_host: %s\n", g_error);
            return 1;
        }
        Out g;
        auto grow = [&](int32_t L, const int32_t* worlds, const double* from, int32_t n, int32_t room) {
            g.status.assign(W, -1); g.iterations.assign(W, -1); g.points.assign(W, -1); g.rewires.assign(W, -1); g.count.assign(W, -1);
            g.path_cost.assign(W, -1.0); g.goal_dist.assign(W, -1.0); g.path.assign((size_t)W * (room > 0 ? room : 1) * 3, 0.0); g.margin.assign(W, 0.0);
            double ms = -1.0;
            const int rc = armour_ws_trees_grow(h, L, worlds, from, n, room, g.status.data(), g.iterations.data(), g.points.data(), g.rewires.data(), g.path_cost.data(),
                                                g.goal_dist.data(), g.path.data(), g.count.data(), &ms, g.margin.data());
            return ms == 0.0 || rc == ARMOUR_EINVAL ? rc : -100;
        };
        const int32_t two[2] = {2, 0}, all[3] = {0, 1, 2}, twice[2] = {1, 1}, outside[1] = {3};
        const double inside[3] = {0.5, 0.35, 0.5}, nan3[3] = {NAN, 0.0, 0.0};
        if (grow(1, all, inside, 50, cap) != ARMOUR_OK || g.status[0] != ARMOUR_WS_START_BLOCKED || g.count[0] != 0 || g.iterations[0] != 0) {
            printf("FAILED: a blocked start planted a tree: %s\n", g_error);
            return 1;
        }
        if (grow(2, two, starts.data(), 100, cap) != ARMOUR_OK || grow(2, two, nullptr, 0, cap) != ARMOUR_OK || grow(3, all, starts.data(), 200, cap) != ARMOUR_OK) {
            printf("FAILED: grow: %s\n", g_error);
            return 1;
        }
        Out nc;
        if (run(&nc, cap, cap, false, 0.2) != ARMOUR_OK) { printf("FAILED: %s\n", g_error); return 1; }    // 300 iterations, no chain: worlds 0 and 2
        Out one;                                                                                                 // world 1: 200 iterations
        one.status.assign(W, 0); one.iterations.assign(W, 0); one.points.assign(W, 0); one.rewires.assign(W, 0); one.kept.assign(W, 0); one.count.assign(W, 0);
        one.path_cost.assign(W, 0.0); one.goal_dist.assign(W, 0.0); one.path.assign((size_t)W * cap * 3, 0.0); one.nodes.assign((size_t)W * cap * 3, 0.0);
        one.parent.assign((size_t)W * cap, -7); one.cost.assign((size_t)W * cap, 0.0);
        if (armour_ws_tree_plan_host(lb, ub, W, O, obstacles.data(), starts.data(), goals.data(), seeds, 0, nullptr, nullptr, 0.1, 0.01, 0.2, 0.1, 0.01, 0.01, 200, cap, cap,
                                     one.status.data(), one.iterations.data(), one.points.data(), one.rewires.data(), one.kept.data(), one.path_cost.data(),
                                     one.goal_dist.data(), one.path.data(), one.count.data(), one.nodes.data(), one.parent.data(), one.cost.data(), nullptr) != ARMOUR_OK) {
            printf("FAILED: %s\n", g_error);
            return 1;
        }
        std::vector<double> rn((size_t)W * cap * 3, 0.0), rc_((size_t)W * cap, 0.0);
        std::vector<int32_t> rp((size_t)W * cap, -7), rcount(W, -1);
        if (armour_ws_trees_read(h, 3, all, rn.data(), rp.data(), rc_.data(), rcount.data()) != ARMOUR_OK) { printf("FAILED: read: %s\n", g_error); return 1; }
        for (int w = 0; w < W; w++) {
            const Out& ref = w == 1 ? one : nc;
            const size_t c = (size_t)ref.count[w], row = (size_t)w * cap;
            if (g.status[w] != ref.status[w] || g.iterations[w] != ref.iterations[w] || g.points[w] != ref.points[w] || g.rewires[w] != ref.rewires[w] ||
                g.count[w] != ref.count[w] || rcount[w] != ref.count[w] || std::memcmp(&g.path_cost[w], &ref.path_cost[w], sizeof(double)) ||
                std::memcmp(&g.goal_dist[w], &ref.goal_dist[w], sizeof(double)) ||
                std::memcmp(&g.path[row * 3], &ref.path[row * 3], (size_t)ref.points[w] * 3 * sizeof(double)) || std::memcmp(&rn[row * 3], &ref.nodes[row * 3], c * 3 * sizeof(double)) ||
                std::memcmp(&rp[row], &ref.parent[row], c * sizeof(int32_t)) || std::memcmp(&rc_[row], &ref.cost[row], c * sizeof(double)) || rp[row + c] != -7) {
                printf("FAILED: world %d grown in instalments differs from one plan of %d iterations\n", w, ref.iterations[w]);
                return 1;
            }
        }
        // the refusals, and the read of a subset with every array absent but the counts
        if (grow(2, twice, starts.data(), 1, cap) != ARMOUR_EINVAL || grow(1, outside, starts.data(), 1, cap) != ARMOUR_EINVAL || grow(1, all, starts.data(), -1, cap) != ARMOUR_EINVAL ||
            grow(1, all, starts.data(), ARMOUR_TREE_MAX_ITERATIONS + 1, cap) != ARMOUR_EINVAL || grow(1, all, starts.data(), 1, -1) != ARMOUR_EINVAL ||
            armour_ws_trees_read(h, 1, outside, nullptr, nullptr, nullptr, nullptr) != ARMOUR_EINVAL) {
            printf("FAILED: a bad argument of grow or read passed\n");
            return 1;
        }
        // too little room, no iterations, planted trees (their starts are not read): ECAPACITY with every world's own points complete
        if (grow(3, all, nan3, 0, 2) != ARMOUR_ECAPACITY || g.points[0] != nc.points[0] || g.points[1] != one.points[1] || g.points[2] != nc.points[2]) {
            printf("FAILED: ECAPACITY of a grow\n");
            return 1;
        }
        int32_t c2[2] = {-1, -1};
        if (armour_ws_trees_read(h, 2, two, nullptr, nullptr, nullptr, c2) != ARMOUR_OK || c2[0] != nc.count[2] || c2[1] != nc.count[0]) { printf("FAILED: read of a subset\n"); return 1; }
        ArmourWsTrees* fresh = nullptr;
        if (armour_ws_trees_create_host(lb, ub, W, O, obstacles.data(), goals.data(), seeds, 0.1, 0.01, 0.2, 0.1, 0.01, 0.01, cap, &fresh) != ARMOUR_OK ||
            armour_ws_trees_grow(fresh, 1, all, nan3, 1, 0, g.status.data(), g.iterations.data(), g.points.data(), g.rewires.data(), g.path_cost.data(), g.goal_dist.data(), nullptr,
                                 nullptr, nullptr, nullptr) != ARMOUR_EINVAL) {
            printf("FAILED: the non-finite start of an empty tree passed\n");
            return 1;
        }
        armour_ws_trees_destroy(fresh);
        if (armour_ws_trees_create_host(lb, ub, W, O, obstacles.data(), goals.data(), seeds, 0.0, 0.01, 0.2, 0.1, 0.01, 0.01, cap, &fresh) != ARMOUR_EINVAL || fresh) {
            printf("FAILED: a bad argument of create passed\n");
            return 1;
        }
        armour_ws_trees_destroy(h);
        armour_ws_trees_destroy(nullptr);
        printf("ws trees host check ok: 100 + 0 + 200 / 200 / 100 + 0 + 200 iterations in instalments equal one plan each: %d / %d / %d nodes\n", rcount[0], rcount[1], rcount[2]);
    }
    // ---- moving obstacles (armour_ws_tree_plan_moving_host): zero velocity against the static call `a`, for two sets of windows; one box that
    // arrives at the start point (free on [0, 1], START_BLOCKED on [0, 3]); the refusals
    {
        Out m;
        auto run_moving = [&](Out* o, const double* vel, const double* t0, const double* t1) {
            o->status.assign(W, -1); o->iterations.assign(W, -1); o->points.assign(W, -1); o->rewires.assign(W, -1); o->kept.assign(W, -1); o->count.assign(W, -1);
            o->parent.assign((size_t)W * cap, -7); o->path_cost.assign(W, -1.0); o->goal_dist.assign(W, -1.0); o->path.assign((size_t)W * cap * 3, 0.0);
            o->nodes.assign((size_t)W * cap * 3, 0.0); o->cost.assign((size_t)W * cap, 0.0); o->margin.assign(W, 0.0);
            return armour_ws_tree_plan_moving_host(lb, ub, W, O, obstacles.data(), vel, t0, t1, starts.data(), goals.data(), seeds, max_init, &chains[0][0][0], chain_count,
                                                   0.1, 0.01, 0.2, 0.1, 0.01, 0.01, iters, cap, cap, o->status.data(), o->iterations.data(), o->points.data(),
                                                   o->rewires.data(), o->kept.data(), o->path_cost.data(), o->goal_dist.data(), o->path.data(), o->count.data(),
                                                   o->nodes.data(), o->parent.data(), o->cost.data(), o->margin.data());
        };
        const std::vector<double> zero((size_t)W * O * 3, 0.0);
        const double windows[2][2][W] = {{{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, {{-3.0, 0.25, 7.0}, {4.0, 0.25, 11.5}}};
        for (int k = 0; k < 2; k++) {
            if (run_moving(&m, zero.data(), windows[k][0], windows[k][1]) != ARMOUR_OK) { printf("FAILED: moving, zero velocity: %s\n", g_error); return 1; }
            if (m.status != a.status || m.iterations != a.iterations || m.points != a.points || m.rewires != a.rewires || m.kept != a.kept || m.count != a.count ||
                m.parent != a.parent || std::memcmp(m.path.data(), a.path.data(), a.path.size() * sizeof(double)) ||
                std::memcmp(m.nodes.data(), a.nodes.data(), a.nodes.size() * sizeof(double)) || std::memcmp(m.cost.data(), a.cost.data(), a.cost.size() * sizeof(double)) ||
                std::memcmp(m.path_cost.data(), a.path_cost.data(), W * sizeof(double)) || std::memcmp(m.goal_dist.data(), a.goal_dist.data(), W * sizeof(double)) ||
                std::memcmp(m.margin.data(), a.margin.data(), W * sizeof(double))) {
                printf("FAILED: zero velocity differs from the static entry (windows %d)\n", k);
                return 1;
            }
        }
        // a drifting wall and windows of three kinds: the trees must keep the static entry's invariants
        std::vector<double> drift((size_t)W * O * 3, 0.0);
        for (size_t i = 0; i < drift.size(); i += 3) { drift[i] = 0.01; drift[i + 1] = -0.02; drift[i + 2] = 0.005; }
        const double d0[W] = {0.0, 1.25, -0.1}, d1[W] = {0.5, 1.25, 0.2};
        if (run_moving(&m, drift.data(), d0, d1) != ARMOUR_OK || !check_trees(m, cap, cap)) { printf("FAILED: moving, drifting wall: %s\n", g_error); return 1; }
        // one box 1 m above the start point, coming down at 0.5 m/s
        std::vector<double> one_box;
        box(&one_box, start[0], start[1], start[2] + 1.0, 0.05, 0.05, 0.05);
        const double v[3] = {0.0, 0.0, -0.5}, from[1] = {0.0}, early[1] = {1.0}, late[1] = {3.0};
        int32_t s1, i1, p1, r1, k1, c1;
        double pc1, gd1, mg1;
        auto arriving = [&](const double* vel, const double* t0, const double* t1, const double* obs) {
            return armour_ws_tree_plan_moving_host(lb, ub, 1, 1, obs, vel, t0, t1, start, goal, seeds, 0, nullptr, nullptr, 0.1, 0.01, 0.2, 0.1, 0.0, 0.01, 40, cap, 0, &s1, &i1,
                                                   &p1, &r1, &k1, &pc1, &gd1, nullptr, &c1, nullptr, nullptr, nullptr, &mg1);
        };
        if (arriving(v, from, early, one_box.data()) != ARMOUR_OK || s1 == ARMOUR_WS_START_BLOCKED || c1 < 2) { printf("FAILED: the early window: status %d, %d nodes\n", s1, c1); return 1; }
        if (arriving(v, from, late, one_box.data()) != ARMOUR_OK || s1 != ARMOUR_WS_START_BLOCKED || c1 != 0 || !(mg1 > 0.0)) { printf("FAILED: the late window: status %d, %d nodes\n", s1, c1); return 1; }
        const double nanv[3] = {0.0, NAN, 0.0}, inf1[1] = {INFINITY};
        if (arriving(nullptr, from, early, one_box.data()) != ARMOUR_EINVAL || arriving(nanv, from, early, one_box.data()) != ARMOUR_EINVAL ||
            arriving(v, nullptr, early, one_box.data()) != ARMOUR_EINVAL || arriving(v, from, nullptr, one_box.data()) != ARMOUR_EINVAL ||
            arriving(v, from, inf1, one_box.data()) != ARMOUR_EINVAL || arriving(v, late, early, one_box.data()) != ARMOUR_EINVAL ||
            arriving(v, from, early, nullptr) != ARMOUR_EINVAL) {
            printf("FAILED: a bad argument of the moving entry passed\n");
            return 1;
        }
        printf("ws tree moving host check ok: zero velocity equals the static call for two sets of windows; drifting wall %d / %d / %d nodes\n", m.count[0], m.count[1], m.count[2]);
    }
    printf("ws tree host check ok: %d / %d / %d nodes, %d / %d / %d rewires, path costs %.4f %.4f %.4f, chains kept %d %d %d, margins %.3g %.3g %.3g\n", a.count[0],
           a.count[1], a.count[2], a.rewires[0], a.rewires[1], a.rewires[2], a.path_cost[0], a.path_cost[1], a.path_cost[2], a.kept[0], a.kept[1], a.kept[2], a.margin[0],
           a.margin[1], a.margin[2]);
    return 0;
}
