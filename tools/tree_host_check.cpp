// Build check of the tree planner's host twin (armour_amd/csrc/tree_plan.hip) under the host sanitizers: a program of its own that calls
// armour_tree_plan_host on a wall world (the straight segment collides, so the trees have to grow) and on an empty one, checks what every
// run must satisfy -- the path runs from start to goal, a parent precedes its child, the same seed gives the same bytes, every edge of a
// found path is free by the node rule at the midpoints of its sub-segments -- and the refusals, and prints what it found.  Then
// armour_tree_plan_moving_host: at zero velocity against the static call, and with the wall arriving.
//   make -C armour_amd/csrc treehost      (hipcc -Xarch_host -fsanitize=address,undefined; no GPU is used)
// It supplies the symbols tree_plan.hip takes from api.hip, so that nothing else of the library is linked.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
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
extern "C" int armour_device_available(void) { return 0; }

using namespace rmgeo;

int main() {
    ArmourRobot robot;
    host_check_robot(&robot);
    RmRobot rb;
    fill_rm_robot(&robot, nullptr, &rb);
    const int n = rb.n, W = 3, O = 1, cap = 512, max_points = 2 * cap;
    const double *start = HC_START, *goal = HC_GOAL;
    // the wall: a thin box through the centre of link 5 (fetch8: 6) halfway along the straight segment
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0}, x[3], u[3][3];
    for (int l = 0; l <= HC_WALL_LINK; l++) link_frame(rb, l, l < n ? 0.5 * (start[l] + goal[l]) : 0.0, R, p);
    link_box(rb, HC_WALL_LINK, R, p, x, u);
    const double wall[12] = {x[0], x[1], x[2], HC_WALL_HALF[0], 0, 0, 0, HC_WALL_HALF[1], 0, 0, 0, HC_WALL_HALF[2]}, far_box[12] = {0, 0, -50, 0.005, 0, 0, 0, 0.005, 0, 0, 0, 0.005};
    std::vector<double> obstacles, starts, goals, lb(n), ub(n);
    for (int w = 0; w < W; w++) {
        obstacles.insert(obstacles.end(), w < 2 ? wall : far_box, (w < 2 ? wall : far_box) + 12);
        starts.insert(starts.end(), start, start + n);
        goals.insert(goals.end(), goal, goal + n);
    }
    for (int j = 0; j < n; j++) {
        lb[j] = rb.cont[j] ? -RM_PI : robot.state_limits_lb[j];
        ub[j] = rb.cont[j] ? RM_PI : robot.state_limits_ub[j];
    }
    const uint64_t seeds[W] = {1, 2, 1};
    struct Out {
        std::vector<int32_t> status, iterations, points, count, parent;
        std::vector<double> path, nodes, margin;
    };
    auto run = [&](Out* o, int32_t room) {
        o->status.assign(W, -1); o->iterations.assign(W, -1); o->points.assign(W, -1); o->count.assign(2 * W, -1);
        o->parent.assign((size_t)W * 2 * cap, -7); o->path.assign((size_t)W * max_points * n, 0.0); o->nodes.assign((size_t)W * 2 * cap * n, 0.0);
        o->margin.assign(W, 0.0);
        return armour_tree_plan_host(&robot, nullptr, lb.data(), ub.data(), W, O, obstacles.data(), starts.data(), goals.data(), seeds, 0.5, 0.05, 400, cap, room,
                                     o->status.data(), o->iterations.data(), o->points.data(), o->path.data(), o->count.data(), o->nodes.data(), o->parent.data(),
                                     o->margin.data());
    };
    Out a, b;
    if (run(&a, max_points) != ARMOUR_OK || run(&b, max_points) != ARMOUR_OK) { printf("FAILED: %s\n", g_error); return 1; }
    if (a.status != b.status || a.iterations != b.iterations || a.points != b.points || a.count != b.count || a.parent != b.parent ||
        std::memcmp(a.path.data(), b.path.data(), a.path.size() * sizeof(double)) || std::memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * sizeof(double))) {
        printf("FAILED: the same call twice gave different results\n");
        return 1;
    }
    std::vector<double> staged((size_t)RM_OBS_STRIDE);
    int edges = 0;
    for (int w = 0; w < W; w++) {
        const double* path = &a.path[(size_t)w * max_points * n];
        const int P = a.points[w];
        if (a.status[w] != ARMOUR_TREE_FOUND || P < 2 || std::memcmp(path, start, n * sizeof(double)) || std::memcmp(path + (size_t)(P - 1) * n, goal, n * sizeof(double))) {
            printf("FAILED: world %d: status %d, %d points, or the path's ends are not start and goal\n", w, a.status[w], P);
            return 1;
        }
        if (w < 2 ? (P <= 2 || a.iterations[w] < 1 || a.count[2 * w] < 2) : (P != 2 || a.iterations[w] != 0 || a.count[2 * w] != 0 || a.count[2 * w + 1] != 0)) {
            printf("FAILED: world %d: %d points after %d iterations, trees %d / %d\n", w, P, a.iterations[w], a.count[2 * w], a.count[2 * w + 1]);
            return 1;
        }
        for (int k = 0; k < 2; k++)
            for (int v = 0; v < a.count[2 * w + k]; v++) {
                const int par = a.parent[((size_t)w * 2 + k) * cap + v];
                if (v == 0 ? par != -1 : (par < 0 || par >= v)) { printf("FAILED: world %d tree %d: node %d has parent %d\n", w, k, v, par); return 1; }
            }
        stage_obstacles(&obstacles[(size_t)w * 12], 1, staged.data());
        for (int e = 0; e + 1 < P; e++, edges++) {
            const double *qa = path + (size_t)e * n, *qb = qa + n;
            const int64_t S = edge_segments(rb, qa, qb, 0.05);
            for (int64_t s = 0; s < S; s++) {
                double q[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS];
                for (int l = 0; l < ARMOUR_MAX_JOINTS; l++) r[l] = 0.0;
                const double t = ((double)s + 0.5) / (double)S;
                for (int j = 0; j < ARMOUR_MAX_FACTORS; j++) q[j] = j < n ? qa[j] + t * (rb.cont[j] ? wrap_diff(qa[j], qb[j]) : qb[j] - qa[j]) : 0.0;
                if (!config_free(rb, q, r, staged.data(), 1, false, nullptr)) { printf("FAILED: world %d: the path's edge %d collides at sample %lld\n", w, e, (long long)s); return 1; }
            }
        }
        if (!(a.margin[w] > 0.0)) { printf("FAILED: world %d: margin %g\n", w, a.margin[w]); return 1; }
    }
    // too little room for a path: ECAPACITY with the points complete; the optional outputs may all be absent
    if (run(&b, 2) != ARMOUR_ECAPACITY || b.points != a.points) { printf("FAILED: a path longer than max_points was not refused\n"); return 1; }
    std::vector<int32_t> st(W), it(W), pt(W);
    if (armour_tree_plan_host(&robot, nullptr, lb.data(), ub.data(), W, O, obstacles.data(), starts.data(), goals.data(), seeds, 0.5, 0.05, 400, cap, 0, st.data(),
                              it.data(), pt.data(), nullptr, nullptr, nullptr, nullptr, nullptr) != ARMOUR_OK || st != a.status || it != a.iterations || pt != a.points) {
        printf("FAILED: the call without optional outputs: %s\n", g_error);
        return 1;
    }
    auto refused = [&](double step, double edge_step, int32_t iters, int32_t nodes_cap) {
        return armour_tree_plan_host(&robot, nullptr, lb.data(), ub.data(), W, O, obstacles.data(), starts.data(), goals.data(), seeds, step, edge_step, iters, nodes_cap, 0,
                                     st.data(), it.data(), pt.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == ARMOUR_EINVAL;
    };
    if (!refused(0.0, 0.05, 400, cap) || !refused(0.5, -1.0, 400, cap) || !refused(0.5, 0.05, -1, cap) || !refused(0.5, 0.05, 400, 1) ||
        !refused(0.5, 0.05, 400, ARMOUR_TREE_MAX_NODES + 1) || !refused(0.5, 0.05, ARMOUR_TREE_MAX_ITERATIONS + 1, cap)) {
        printf("FAILED: a bad argument passed\n");
        return 1;
    }
    // moving obstacles.  Zero velocity on any window is the static call bit for bit; then the wall 1 m further out at t = 0 and moving in at
    // 0.5 m/s: the direct edge is the path while the window ends before the wall is near, and trees grow in a window about its arrival
    auto run_moving = [&](Out* o, const double* obs, const double* vel, const double* t_from, const double* t_to) {
        o->status.assign(W, -1); o->iterations.assign(W, -1); o->points.assign(W, -1); o->count.assign(2 * W, -1);
        o->parent.assign((size_t)W * 2 * cap, -7); o->path.assign((size_t)W * max_points * n, 0.0); o->nodes.assign((size_t)W * 2 * cap * n, 0.0);
        o->margin.assign(W, 0.0);
        return armour_tree_plan_moving_host(&robot, nullptr, lb.data(), ub.data(), W, O, obs, vel, t_from, t_to, starts.data(), goals.data(), seeds, 0.5, 0.05, 400, cap,
                                            max_points, o->status.data(), o->iterations.data(), o->points.data(), o->path.data(), o->count.data(), o->nodes.data(),
                                            o->parent.data(), o->margin.data());
    };
    const std::vector<double> zero((size_t)W * O * 3, 0.0);
    const double t_from[W] = {-3.0, 0.25, 7.0}, t_to[W] = {4.0, 0.25, 11.5};
    if (run_moving(&b, obstacles.data(), zero.data(), t_from, t_to) != ARMOUR_OK) { printf("FAILED: the moving call: %s\n", g_error); return 1; }
    if (a.status != b.status || a.iterations != b.iterations || a.points != b.points || a.count != b.count || a.parent != b.parent || a.margin != b.margin ||
        std::memcmp(a.path.data(), b.path.data(), a.path.size() * sizeof(double)) || std::memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * sizeof(double))) {
        printf("FAILED: zero velocity is not the static call\n");
        return 1;
    }
    const double out_dir[3] = {x[0] / std::hypot(x[0], x[1]), x[1] / std::hypot(x[0], x[1]), 0.0};
    std::vector<double> away = obstacles, vel((size_t)W * O * 3, 0.0);
    for (int w = 0; w < 2; w++)
        for (int i = 0; i < 3; i++) {
            away[(size_t)w * 12 + i] += 1.0 * out_dir[i];
            vel[(size_t)w * 3 + i] = -0.5 * out_dir[i];
        }
    const double m_from[W] = {0.0, HC_LATE[0], 0.0}, m_to[W] = {0.2, HC_LATE[1], 1.0};
    if (run_moving(&b, away.data(), vel.data(), m_from, m_to) != ARMOUR_OK) { printf("FAILED: the moving call: %s\n", g_error); return 1; }
    if (b.status[0] != ARMOUR_TREE_FOUND || b.points[0] != 2 || b.iterations[0] != 0 || b.status[1] != ARMOUR_TREE_FOUND || b.points[1] <= 2 || b.iterations[1] < 1 ||
        !(b.margin[0] > 0.0) || !(b.margin[1] > 0.0)) {
        printf("FAILED: the arriving wall: status %d / %d, %d / %d points after %d / %d iterations\n", b.status[0], b.status[1], b.points[0], b.points[1], b.iterations[0],
               b.iterations[1]);
        return 1;
    }
    // every sub-segment midpoint of the grown path, at both ends and the middle of its window, against the wall where it then is
    std::vector<double> moved((size_t)RM_MOV_STRIDE);
    int moving_edges = 0;
    for (int e = 0; e + 1 < b.points[1]; e++, moving_edges++) {
        const double *qa = &b.path[((size_t)1 * max_points + e) * n], *qb = qa + n;
        const int64_t S = edge_segments(rb, qa, qb, 0.05);
        stage_obstacles_moving(&away[12], &vel[3], 1, moved.data());
        for (int64_t s = 0; s < S; s++)
            for (int k = 0; k < 3; k++) {
                double q[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS], none[ARMOUR_MAX_JOINTS] = {};
                edge_sample(rb, qa, qb, s, S, q, r);
                if (!config_free_moving(rb, q, none, moved.data(), 1, m_from[1] + 0.5 * k * (m_to[1] - m_from[1]), 0.0, false, nullptr)) {
                    printf("FAILED: the grown path's edge %d meets the wall in its window\n", e);
                    return 1;
                }
            }
    }
    const int grown_points = b.points[1], grown_iterations = b.iterations[1];
    const double reversed[W] = {0.0, HC_LATE[1] + 0.1, 0.0}, nan_t[W] = {0.0, NAN, 0.0};
    vel[4] = INFINITY;
    if (run_moving(&b, away.data(), nullptr, m_from, m_to) != ARMOUR_EINVAL || run_moving(&b, away.data(), vel.data(), m_from, m_to) != ARMOUR_EINVAL ||
        run_moving(&b, away.data(), zero.data(), reversed, m_to) != ARMOUR_EINVAL || run_moving(&b, away.data(), zero.data(), m_from, nan_t) != ARMOUR_EINVAL ||
        run_moving(&b, away.data(), zero.data(), nullptr, m_to) != ARMOUR_EINVAL) {
        printf("FAILED: a bad velocity or window passed\n");
        return 1;
    }
    printf("moving: zero velocity equals the static call; the arriving wall: direct edge on [0, 0.2], %d points after %d iterations on [%g, %g], %d edges free over it\n",
           grown_points, grown_iterations, HC_LATE[0], HC_LATE[1], moving_edges);
    printf("tree host check ok: wall world found after %d / %d iterations with %d / %d points, %d path edges free by the rule, margins %.3g %.3g %.3g\n",
           a.iterations[0], a.iterations[1], a.points[0], a.points[1], edges, a.margin[0], a.margin[1], a.margin[2]);
    return 0;
}
