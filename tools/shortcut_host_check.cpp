// Build check of the path shortener's host twin (armour_amd/csrc/path_shortcut.hip) under the host sanitizers: a program of its own that
// calls armour_path_shortcut_host on a wall world -- a hand-placed detour with every edge cut into pieces, the same detour with repeated
// points, the straight segment through the wall (invalid) and a two-point path in an empty world -- checks what every run must satisfy
// (the ends are kept, one pass returns a subsequence, the output is not longer, every output edge is free by the node rule at the
// midpoints of its sub-segments, rows of an invalid world and rows past `points` are untouched, the same call twice gives the same bytes)
// and the refusals, and prints what it found.  Then armour_path_shortcut_moving_host: at zero velocity against the static call, and with
// the wall arriving.
//   make -C armour_amd/csrc shortcuthost      (hipcc -Xarch_host -fsanitize=address,undefined; no GPU is used)
// It supplies the symbols path_shortcut.hip takes from api.hip, so that nothing else of the library is linked.
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

static const double SENTINEL = -7.25;

int main() {
    ArmourRobot robot;
    host_check_robot(&robot);
    RmRobot rb;
    fill_rm_robot(&robot, nullptr, &rb);
    const int n = rb.n, W = 4, O = 1;
    const double edge_step = 0.05;
    const double *start = HC_START, *goal = HC_GOAL;
    // the wall: a thin box through the centre of link 5 (fetch8: 6) halfway along the straight segment
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0}, x[3], u[3][3];
    for (int l = 0; l <= HC_WALL_LINK; l++) link_frame(rb, l, l < n ? 0.5 * (start[l] + goal[l]) : 0.0, R, p);
    link_box(rb, HC_WALL_LINK, R, p, x, u);
    const double wall[12] = {x[0], x[1], x[2], HC_WALL_HALF[0], 0, 0, 0, HC_WALL_HALF[1], 0, 0, 0, HC_WALL_HALF[2]}, far_box[12] = {0, 0, -50, 0.005, 0, 0, 0, 0.005, 0, 0, 0, 0.005};
    // the detour: halfway, with the shoulder swung 2 rad back; each leg cut into 8 pieces
    double corner[ARMOUR_MAX_FACTORS];
    for (int j = 0; j < n; j++) corner[j] = 0.5 * (start[j] + goal[j]);
    corner[HC_SWING_JOINT] += HC_SWING;
    std::vector<std::vector<double>> in(W);
    auto push = [&](std::vector<double>& v, const double* q) { v.insert(v.end(), q, q + n); };
    for (int leg = 0; leg < 2; leg++)
        for (int k = 0; k < 8; k++) {
            double q[ARMOUR_MAX_FACTORS];
            const double* a = leg ? corner : start;
            const double* b = leg ? goal : corner;
            for (int j = 0; j < n; j++) q[j] = a[j] + (k / 8.0) * (b[j] - a[j]);
            push(in[0], q);
            push(in[1], q);
            if (k % 3 == 1) { push(in[1], q); push(in[1], q); }          // repeated points
        }
    push(in[0], goal); push(in[1], goal);
    push(in[2], start); push(in[2], goal);                                // through the wall
    push(in[3], start); push(in[3], goal);                                // the empty world
    int max_in = 0;
    std::vector<int32_t> counts(W);
    for (int w = 0; w < W; w++) { counts[w] = (int32_t)(in[w].size() / n); max_in = counts[w] > max_in ? counts[w] : max_in; }
    std::vector<double> paths((size_t)W * max_in * n, 0.0), obstacles;
    for (int w = 0; w < W; w++) {
        std::memcpy(&paths[(size_t)w * max_in * n], in[w].data(), in[w].size() * sizeof(double));
        obstacles.insert(obstacles.end(), w < 3 ? wall : far_box, (w < 3 ? wall : far_box) + 12);
    }
    const int max_points = 2 * max_in - 1;
    struct Out {
        std::vector<int32_t> status, points, first_bad, passes_done;
        std::vector<double> out, length_in, length_out, margin;
    };
    auto run = [&](Out* o, int32_t passes, int32_t room) {
        o->status.assign(W, -1); o->points.assign(W, -1); o->first_bad.assign(W, -9); o->passes_done.assign(W, -1);
        o->out.assign((size_t)W * room * n, SENTINEL); o->length_in.assign(W, -1.0); o->length_out.assign(W, -1.0); o->margin.assign(W, 0.0);
        return armour_path_shortcut_host(&robot, nullptr, W, O, obstacles.data(), max_in, paths.data(), counts.data(), edge_step, passes, room, o->status.data(),
                                         o->points.data(), o->first_bad.data(), o->passes_done.data(), o->out.data(), o->length_in.data(), o->length_out.data(),
                                         o->margin.data());
    };
    std::vector<double> staged((size_t)RM_OBS_STRIDE);
    int edges = 0;
    for (int passes = 1; passes <= 3; passes++) {
        Out a, b;
        if (run(&a, passes, max_points) != ARMOUR_OK || run(&b, passes, max_points) != ARMOUR_OK) { printf("FAILED: %s\n", g_error); return 1; }
        if (a.status != b.status || a.points != b.points || a.first_bad != b.first_bad || a.passes_done != b.passes_done ||
            std::memcmp(a.out.data(), b.out.data(), a.out.size() * sizeof(double)) || std::memcmp(a.length_out.data(), b.length_out.data(), W * sizeof(double))) {
            printf("FAILED: the same call twice gave different results\n");
            return 1;
        }
        for (int w = 0; w < W; w++) {
            const double* out = &a.out[(size_t)w * max_points * n];
            const int P = a.points[w];
            if (w == 2) {
                bool clean = true;
                for (int i = 0; i < max_points * n; i++) clean = clean && out[i] == SENTINEL;
                if (a.status[w] != ARMOUR_SHORTCUT_INVALID || a.first_bad[w] != 0 || P != 0 || a.passes_done[w] != 0 || !clean) {
                    printf("FAILED: the path through the wall: status %d, first_bad %d, %d points, or its rows were written\n", a.status[w], a.first_bad[w], P);
                    return 1;
                }
                continue;
            }
            if (a.status[w] != ARMOUR_SHORTCUT_OK || a.first_bad[w] != -1 || P < 2 || P > max_points || a.passes_done[w] < 1 || a.passes_done[w] > passes ||
                std::memcmp(out, start, n * sizeof(double)) || std::memcmp(out + (size_t)(P - 1) * n, goal, n * sizeof(double))) {
                printf("FAILED: world %d, %d passes: status %d, %d points, or the ends are not start and goal\n", w, passes, a.status[w], P);
                return 1;
            }
            if (!(a.length_out[w] <= a.length_in[w] * (1 + 1e-12)) || !(a.margin[w] > 0.0)) {
                printf("FAILED: world %d: length %g -> %g, margin %g\n", w, a.length_in[w], a.length_out[w], a.margin[w]);
                return 1;
            }
            for (int i = P * n; i < max_points * n; i++)
                if (out[i] != SENTINEL) { printf("FAILED: world %d: a row past its %d points was written\n", w, P); return 1; }
            if (passes == 1) {                                            // a subsequence of the input, bit for bit
                int k = 0;
                for (int i = 0; i < P; i++) {
                    while (k < counts[w] && std::memcmp(out + (size_t)i * n, &paths[((size_t)w * max_in + k) * n], n * sizeof(double))) k++;
                    if (k++ >= counts[w]) { printf("FAILED: world %d: point %d of the pruned path is not a later point of the input\n", w, i); return 1; }
                }
            }
            if (w == 3 ? P != 2 : (P < 3 || P >= counts[w])) { printf("FAILED: world %d: %d of %d points kept\n", w, P, counts[w]); return 1; }
            stage_obstacles(&obstacles[(size_t)w * 12], 1, staged.data());
            for (int i = 0; i + 1 < P; i++) {
                const double* qa = out + (size_t)i * n;
                const double* qb = qa + n;
                const int64_t S = edge_segments(rb, qa, qb, edge_step);
                for (int64_t s = 0; s < S; s++) {
                    double q[ARMOUR_MAX_FACTORS], r[ARMOUR_MAX_JOINTS], zero[ARMOUR_MAX_JOINTS] = {};
                    edge_sample(rb, qa, qb, s, S, q, r);
                    if (!config_free(rb, q, zero, staged.data(), 1, false, nullptr)) { printf("FAILED: world %d: edge %d of the output collides\n", w, i); return 1; }
                }
                edges++;
            }
        }
        if (passes == 2 && !(a.length_out[0] < 0.95 * a.length_in[0])) { printf("FAILED: refine did not cut the corner: %g -> %g\n", a.length_in[0], a.length_out[0]); return 1; }
        printf("passes %d: points %d %d - %d (of %d %d 2 2), passes done %d %d %d %d, length %.4f -> %.4f, margin %.2e\n", passes, a.points[0], a.points[1], a.points[3],
               counts[0], counts[1], a.passes_done[0], a.passes_done[1], a.passes_done[2], a.passes_done[3], a.length_in[0], a.length_out[0], a.margin[0]);
        // capacity: one row fewer than world 0's pruned path needs
        if (passes == 1) {
            Out c;
            const int rc = run(&c, 1, a.points[0] - 1 < 2 ? 2 : a.points[0] - 1);
            if (a.points[0] > 2 && (rc != ARMOUR_ECAPACITY || c.points != a.points || c.out[0] != SENTINEL)) { printf("FAILED: capacity: rc %d\n", rc); return 1; }
        }
    }
    // moving obstacles.  Zero velocity on any window is the static call bit for bit, every column; then the wall 1 m further out at t = 0
    // and moving in at 0.5 m/s: the straight segment of world 2 is free while the window ends before the wall is near and invalid in a
    // window about its arrival, where the detour of world 0 is still shortened
    {
        auto run_moving = [&](Out* o, const double* obs, const double* vel, const double* t_from, const double* t_to) {
            o->status.assign(W, -1); o->points.assign(W, -1); o->first_bad.assign(W, -9); o->passes_done.assign(W, -1);
            o->out.assign((size_t)W * max_points * n, SENTINEL); o->length_in.assign(W, -1.0); o->length_out.assign(W, -1.0); o->margin.assign(W, 0.0);
            return armour_path_shortcut_moving_host(&robot, nullptr, W, O, obs, vel, t_from, t_to, max_in, paths.data(), counts.data(), edge_step, 2, max_points,
                                                    o->status.data(), o->points.data(), o->first_bad.data(), o->passes_done.data(), o->out.data(), o->length_in.data(),
                                                    o->length_out.data(), o->margin.data());
        };
        Out a, b;
        const std::vector<double> zero((size_t)W * O * 3, 0.0);
        const double t_from[W] = {-3.0, 0.25, 7.0, 0.0}, t_to[W] = {4.0, 0.25, 11.5, 0.0};
        if (run(&a, 2, max_points) != ARMOUR_OK || run_moving(&b, obstacles.data(), zero.data(), t_from, t_to) != ARMOUR_OK) { printf("FAILED: %s\n", g_error); return 1; }
        if (a.status != b.status || a.points != b.points || a.first_bad != b.first_bad || a.passes_done != b.passes_done || a.length_in != b.length_in ||
            a.length_out != b.length_out || a.margin != b.margin || std::memcmp(a.out.data(), b.out.data(), a.out.size() * sizeof(double))) {
            printf("FAILED: zero velocity is not the static call\n");
            return 1;
        }
        const double out_dir[3] = {x[0] / std::hypot(x[0], x[1]), x[1] / std::hypot(x[0], x[1]), 0.0};
        std::vector<double> away = obstacles, vel((size_t)W * O * 3, 0.0);
        for (int w = 0; w < 3; w++)
            for (int i = 0; i < 3; i++) {
                away[(size_t)w * 12 + i] += 1.0 * out_dir[i];
                vel[(size_t)w * 3 + i] = -0.5 * out_dir[i];
            }
        const double early_from[W] = {0.0, 0.0, 0.0, 0.0}, early_to[W] = {0.2, 0.2, 0.2, 0.2}, late_from[W] = {HC_LATE[0], HC_LATE[0], HC_LATE[0], HC_LATE[0]},
                     late_to[W] = {HC_LATE[1], HC_LATE[1], HC_LATE[1], HC_LATE[1]};
        Out early, late;
        if (run_moving(&early, away.data(), vel.data(), early_from, early_to) != ARMOUR_OK || run_moving(&late, away.data(), vel.data(), late_from, late_to) != ARMOUR_OK) {
            printf("FAILED: the moving call: %s\n", g_error);
            return 1;
        }
        if (early.status[2] != ARMOUR_SHORTCUT_OK || early.points[2] != 2 || early.points[0] != 2 || late.status[2] != ARMOUR_SHORTCUT_INVALID || late.first_bad[2] != 0 ||
            late.status[0] != ARMOUR_SHORTCUT_OK || late.points[0] < 3 || late.points[0] >= counts[0] || !(late.margin[0] > 0.0)) {
            printf("FAILED: the arriving wall: early status %d with %d / %d points, late status %d / %d with %d points\n", early.status[2], early.points[2], early.points[0],
                   late.status[2], late.status[0], late.points[0]);
            return 1;
        }
        const double reversed[W] = {0.0, HC_LATE[1] + 0.1, 0.0, 0.0};
        vel[4] = NAN;
        if (run_moving(&b, away.data(), nullptr, late_from, late_to) != ARMOUR_EINVAL || run_moving(&b, away.data(), vel.data(), late_from, late_to) != ARMOUR_EINVAL ||
            run_moving(&b, away.data(), zero.data(), reversed, late_to) != ARMOUR_EINVAL || run_moving(&b, away.data(), zero.data(), late_from, nullptr) != ARMOUR_EINVAL) {
            printf("FAILED: a bad velocity or window passed\n");
            return 1;
        }
        printf("moving: zero velocity equals the static call; the arriving wall: the straight segment is free on [0, 0.2] and invalid on [%g, %g], the detour %d -> %d points\n",
               HC_LATE[0], HC_LATE[1], counts[0], late.points[0]);
    }
    // refusals
    Out r;
    struct Bad { int32_t passes, room; double es; } bad[] = {{0, 8, 0.05}, {9, 8, 0.05}, {1, 1, 0.05}, {1, 1025, 0.05}, {1, 8, 0.0}, {1, 8, NAN}};
    for (const Bad& c : bad) {
        r.status.assign(W, 0); r.points.assign(W, 0); r.first_bad.assign(W, 0); r.passes_done.assign(W, 0);
        r.out.assign((size_t)W * 1025 * n, 0.0); r.length_in.assign(W, 0.0); r.length_out.assign(W, 0.0); r.margin.assign(W, 0.0);
        const int rc = armour_path_shortcut_host(&robot, nullptr, W, O, obstacles.data(), max_in, paths.data(), counts.data(), c.es, c.passes, c.room, r.status.data(),
                                                 r.points.data(), r.first_bad.data(), r.passes_done.data(), r.out.data(), r.length_in.data(), r.length_out.data(),
                                                 r.margin.data());
        if (rc != ARMOUR_EINVAL) { printf("FAILED: passes %d, max_points %d, edge_step %g was not refused (rc %d)\n", c.passes, c.room, c.es, rc); return 1; }
    }
    counts[1] = 1;
    if (armour_path_shortcut_host(&robot, nullptr, W, O, obstacles.data(), max_in, paths.data(), counts.data(), edge_step, 1, max_points, r.status.data(), r.points.data(),
                                  r.first_bad.data(), r.passes_done.data(), r.out.data(), r.length_in.data(), r.length_out.data(), r.margin.data()) != ARMOUR_EINVAL) {
        printf("FAILED: a path of one point was not refused\n");
        return 1;
    }
    if (armour_path_shortcut(&robot, nullptr, 0, O, nullptr, max_in, nullptr, nullptr, edge_step, 1, max_points, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                             nullptr) != ARMOUR_OK) {
        printf("FAILED: W = 0 is not a success\n");
        return 1;
    }
    printf("shortcut_host_check: ok (%d output edges re-checked)\n", edges);
    return 0;
}
