// Build check of the inverse kinematics' host entries (armour_amd/csrc/ik.hip) under the host sanitizers: a program of its own that calls
// armour_ik_host on four targets -- one in an empty world, one in a world whose box stands clear of the arm, one whose target sits inside a box
// that holds the whole last link, one out of reach -- and armour_ik_end_effector_host, checks what every run must satisfy -- a found
// configuration reaches its target by the entry's own forward kinematics, stays inside the box on the non-continuous joints, is the flagged
// item with the smallest (distance, seed), the same call twice gives the same bytes, the Jacobian matches central differences -- and the
// refusals, and prints what it found.  Then the moving twin (armour_ik_moving_host): zero velocity against the static call for two sets of
// windows, the blocking box arriving on its target, the refusals.
//   make -C armour_amd/csrc ikhost      (hipcc -Xarch_host -fsanitize=address,undefined; no GPU is used)
// It supplies the symbols ik.hip takes from api.hip, so that nothing else of the library is linked.
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
    const int n = rb.n, N = 4, S = 16, W = 2, O = 1;
    const double *q_goal = HC_IK_GOAL, *q_ref = HC_IK_REF, tool[3] = {0.0, 0.0, 0.0};
    double pg[3], jac[3 * ARMOUR_MAX_FACTORS];
    if (armour_ik_end_effector_host(&robot, 1, q_goal, tool, pg, jac) != ARMOUR_OK) { printf("FAILED: %s\n", g_error); return 1; }
    // the Jacobian against central differences of the point
    double worst_fd = 0.0;
    for (int j = 0; j < n; j++) {
        double qa[ARMOUR_MAX_FACTORS], qb[ARMOUR_MAX_FACTORS], pa[3], pb[3];
        std::memcpy(qa, q_goal, sizeof(qa));
        std::memcpy(qb, q_goal, sizeof(qb));
        qa[j] -= 1e-6; qb[j] += 1e-6;
        if (armour_ik_end_effector_host(&robot, 1, qa, tool, pa, nullptr) != ARMOUR_OK || armour_ik_end_effector_host(&robot, 1, qb, tool, pb, nullptr) != ARMOUR_OK) {
            printf("FAILED: %s\n", g_error);
            return 1;
        }
        for (int r = 0; r < 3; r++) worst_fd = std::fmax(worst_fd, std::fabs(jac[r * n + j] - (pb[r] - pa[r]) / 2e-6));
    }
    if (!(worst_fd <= 1e-8)) { printf("FAILED: the Jacobian is %g away from central differences\n", worst_fd); return 1; }
    // world 0: a box far below the base; world 1: a cube about the target that holds the whole last link that has a box (fetch8 ends in one without)
    int boxed = rb.J - 1;
    while (boxed > 0 && dot3(rb.h[boxed], rb.h[boxed]) == 0.0) boxed--;
    double rr = std::sqrt(dot3(rb.c[boxed], rb.c[boxed])) + std::sqrt(dot3(rb.h[boxed], rb.h[boxed])) + 0.01;
    for (int l = boxed + 1; l < rb.J; l++) rr += std::sqrt(dot3(rb.trans[l], rb.trans[l]));
    const double obstacles[W * O * 12] = {0, 0, -50, 0.005, 0, 0, 0, 0.005, 0, 0, 0, 0.005, pg[0], pg[1], pg[2], rr, 0, 0, 0, rr, 0, 0, 0, rr};
    const int32_t world[N] = {-1, 0, 1, 0};
    std::vector<double> targets, refs, lb(n), ub(n);
    for (int t = 0; t < N; t++) {
        const double far_point[3] = {3.0, 0.0, 0.0};
        targets.insert(targets.end(), t == 3 ? far_point : pg, (t == 3 ? far_point : pg) + 3);
        refs.insert(refs.end(), q_ref, q_ref + n);
    }
    for (int j = 0; j < n; j++) {
        lb[j] = rb.cont[j] ? -RM_PI : robot.state_limits_lb[j];
        ub[j] = rb.cont[j] ? RM_PI : robot.state_limits_ub[j];
    }
    const uint64_t seeds[N] = {1, 2, 3, 4};
    struct Out {
        std::vector<int32_t> status, best, iterations, flags;
        std::vector<double> q_best, q, err, margin;
    };
    auto run = [&](Out* o, int32_t max_iterations) {
        o->status.assign(N, -7); o->best.assign(N, -7); o->iterations.assign((size_t)N * S, -7); o->flags.assign((size_t)N * S, -7);
        o->q_best.assign((size_t)N * n, -7.0); o->q.assign((size_t)N * S * n, 0.0); o->err.assign((size_t)N * S, 0.0); o->margin.assign(N, 0.0);
        return armour_ik_host(&robot, nullptr, lb.data(), ub.data(), tool, N, S, W, O, obstacles, world, targets.data(), refs.data(), seeds, 0.05, 0.1, 1e-9,
                              max_iterations, o->status.data(), o->best.data(), o->q_best.data(), o->q.data(), o->err.data(), o->iterations.data(), o->flags.data(),
                              o->margin.data());
    };
    Out a, b;
    if (run(&a, 200) != ARMOUR_OK || run(&b, 200) != ARMOUR_OK) { printf("FAILED: %s\n", g_error); return 1; }
    if (a.status != b.status || a.best != b.best || a.iterations != b.iterations || a.flags != b.flags || std::memcmp(a.q.data(), b.q.data(), a.q.size() * sizeof(double)) ||
        std::memcmp(a.q_best.data(), b.q_best.data(), a.q_best.size() * sizeof(double)) || std::memcmp(a.err.data(), b.err.data(), a.err.size() * sizeof(double))) {
        printf("FAILED: the same call twice gave different results\n");
        return 1;
    }
    const int32_t want[N] = {ARMOUR_IK_FOUND, ARMOUR_IK_FOUND, ARMOUR_IK_ALL_BLOCKED, ARMOUR_IK_NONE_CONVERGED};
    int converged = 0;
    for (int t = 0; t < N; t++) {
        if (a.status[t] != want[t]) { printf("FAILED: target %d has status %d, expected %d\n", t, a.status[t], want[t]); return 1; }
        double bd = INFINITY;
        int bv = -1;
        for (int s = 0; s < S; s++) {
            const size_t item = (size_t)t * S + s;
            const int f = a.flags[item];
            const double* q = &a.q[item * n];
            if (f < 0 || f > 3 || f == 2 || a.iterations[item] < 0 || a.iterations[item] > 200 || ((f & 1) != 0) != (a.err[item] <= 1e-9)) {
                printf("FAILED: item (%d, %d): flags %d, %d iterations, err %g\n", t, s, f, a.iterations[item], a.err[item]);
                return 1;
            }
            for (int j = 0; j < n; j++)
                if (!rb.cont[j] && !(q[j] >= lb[j] && q[j] <= ub[j])) { printf("FAILED: item (%d, %d): joint %d = %g leaves [%g, %g]\n", t, s, j, q[j], lb[j], ub[j]); return 1; }
            converged += f & 1;
            if (f == 3) {
                const double d = wrapped_sq(rb, q_ref, q);
                if (key_less(d, s, bd, bv < 0 ? INT32_MAX : bv)) { bd = d; bv = s; }
            }
        }
        if (a.best[t] != bv) { printf("FAILED: target %d: best %d, the flagged items give %d\n", t, a.best[t], bv); return 1; }
        const double* qb = &a.q_best[(size_t)t * n];
        if (bv < 0) {
            for (int j = 0; j < n; j++)
                if (qb[j] != -7.0) { printf("FAILED: target %d has no pick but its row was written\n", t); return 1; }
        } else {
            double p[3];
            if (std::memcmp(qb, &a.q[((size_t)t * S + bv) * n], n * sizeof(double)) || armour_ik_end_effector_host(&robot, 1, qb, tool, p, nullptr) != ARMOUR_OK) {
                printf("FAILED: target %d: q_best is not the picked item's q\n", t);
                return 1;
            }
            const double d[3] = {p[0] - pg[0], p[1] - pg[1], p[2] - pg[2]};
            if (!(std::sqrt(dot3(d, d)) <= 1e-9)) { printf("FAILED: target %d: the pick misses its target by %g\n", t, std::sqrt(dot3(d, d))); return 1; }
        }
    }
    if (!(a.margin[0] == INFINITY) || !(a.margin[1] > 1.0) || !(a.margin[2] > 0.0) || !(a.margin[3] == INFINITY)) {
        printf("FAILED: margins %g %g %g %g\n", a.margin[0], a.margin[1], a.margin[2], a.margin[3]);
        return 1;
    }
    // the optional outputs may all be absent; max_iterations = 0 leaves every item at its start point
    std::vector<int32_t> st(N), be(N);
    std::vector<double> qb((size_t)N * n, -7.0);
    if (armour_ik_host(&robot, nullptr, lb.data(), ub.data(), tool, N, S, W, O, obstacles, world, targets.data(), refs.data(), seeds, 0.05, 0.1, 1e-9, 200, st.data(),
                       be.data(), qb.data(), nullptr, nullptr, nullptr, nullptr, nullptr) != ARMOUR_OK || st != a.status || be != a.best) {
        printf("FAILED: the call without optional outputs: %s\n", g_error);
        return 1;
    }
    if (run(&b, 0) != ARMOUR_OK || b.status[0] != ARMOUR_IK_NONE_CONVERGED || std::memcmp(&b.q[0], q_ref, n * sizeof(double))) { printf("FAILED: max_iterations = 0\n"); return 1; }
    auto refused = [&](int32_t seeds_per_target, double lambda, double e_max, double tol, int32_t iters, int32_t world0) {
        const int32_t wd[N] = {world0, 0, 1, 0};
        return armour_ik_host(&robot, nullptr, lb.data(), ub.data(), tool, N, seeds_per_target, W, O, obstacles, wd, targets.data(), refs.data(), seeds, lambda, e_max, tol,
                              iters, st.data(), be.data(), qb.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == ARMOUR_EINVAL;
    };
    if (!refused(0, 0.05, 0.1, 1e-9, 200, 0) || !refused(ARMOUR_IK_MAX_SEEDS + 1, 0.05, 0.1, 1e-9, 200, 0) || !refused(S, 0.0, 0.1, 1e-9, 200, 0) ||
        !refused(S, 0.05, -0.1, 1e-9, 200, 0) || !refused(S, 0.05, 0.1, NAN, 200, 0) || !refused(S, 0.05, 0.1, 1e-9, -1, 0) ||
        !refused(S, 0.05, 0.1, 1e-9, ARMOUR_IK_MAX_ITERATIONS + 1, 0) || !refused(S, 0.05, 0.1, 1e-9, 200, W) || !refused(S, 0.05, 0.1, 1e-9, 200, -2)) {
        printf("FAILED: a bad argument passed\n");
        return 1;
    }
    // ---- moving obstacles (armour_ik_moving_host): zero velocity against the static call `a`, for two sets of windows; the blocking cube
    // of world 1 starting 2 m above the target and coming down at 1 m/s (FOUND on [0, 0.5], ALL_BLOCKED about t = 2); the refusals
    {
        Out m;
        auto run_moving = [&](Out* o, const double* obs, const double* vel, const double* t0, const double* t1) {
            o->status.assign(N, -7); o->best.assign(N, -7); o->iterations.assign((size_t)N * S, -7); o->flags.assign((size_t)N * S, -7);
            o->q_best.assign((size_t)N * n, -7.0); o->q.assign((size_t)N * S * n, 0.0); o->err.assign((size_t)N * S, 0.0); o->margin.assign(N, 0.0);
            return armour_ik_moving_host(&robot, nullptr, lb.data(), ub.data(), tool, N, S, W, O, obs, vel, t0, t1, world, targets.data(), refs.data(), seeds, 0.05, 0.1,
                                         1e-9, 200, o->status.data(), o->best.data(), o->q_best.data(), o->q.data(), o->err.data(), o->iterations.data(), o->flags.data(),
                                         o->margin.data());
        };
        const double zero[W * O * 3] = {0, 0, 0, 0, 0, 0};
        const double windows[2][2][W] = {{{0.0, 0.0}, {0.0, 0.0}}, {{-3.0, 7.0}, {4.0, 11.5}}};
        for (int k = 0; k < 2; k++) {
            if (run_moving(&m, obstacles, zero, windows[k][0], windows[k][1]) != ARMOUR_OK) { printf("FAILED: moving, zero velocity: %s\n", g_error); return 1; }
            if (m.status != a.status || m.best != a.best || m.iterations != a.iterations || m.flags != a.flags || std::memcmp(m.q.data(), a.q.data(), a.q.size() * sizeof(double)) ||
                std::memcmp(m.q_best.data(), a.q_best.data(), a.q_best.size() * sizeof(double)) || std::memcmp(m.err.data(), a.err.data(), a.err.size() * sizeof(double)) ||
                std::memcmp(m.margin.data(), a.margin.data(), a.margin.size() * sizeof(double))) {
                printf("FAILED: zero velocity differs from the static entry (windows %d)\n", k);
                return 1;
            }
        }
        double lifted[W * O * 12];
        std::memcpy(lifted, obstacles, sizeof(lifted));
        lifted[12 + 2] += 2.0;
        const double vel[W * O * 3] = {0, 0, 0, 0, 0, -1.0};
        const double e0[W] = {0.0, 0.0}, e1[W] = {0.5, 0.5}, l0[W] = {0.0, 1.9}, l1[W] = {0.5, 2.1};
        if (run_moving(&m, lifted, vel, e0, e1) != ARMOUR_OK || m.status[2] != ARMOUR_IK_FOUND || m.best[2] < 0 || m.status[1] != a.status[1]) {
            printf("FAILED: the early window: status %d, best %d: %s\n", m.status[2], m.best[2], g_error);
            return 1;
        }
        if (run_moving(&m, lifted, vel, l0, l1) != ARMOUR_OK || m.status[2] != ARMOUR_IK_ALL_BLOCKED || m.status[1] != a.status[1] || !(m.margin[2] > 0.0)) {
            printf("FAILED: the late window: status %d: %s\n", m.status[2], g_error);
            return 1;
        }
        const double nanv[W * O * 3] = {0, NAN, 0, 0, 0, 0}, inf2[W] = {0.5, INFINITY};
        if (run_moving(&m, lifted, nullptr, e0, e1) != ARMOUR_EINVAL || run_moving(&m, lifted, nanv, e0, e1) != ARMOUR_EINVAL || run_moving(&m, lifted, vel, nullptr, e1) != ARMOUR_EINVAL ||
            run_moving(&m, lifted, vel, e0, nullptr) != ARMOUR_EINVAL || run_moving(&m, lifted, vel, e0, inf2) != ARMOUR_EINVAL || run_moving(&m, lifted, vel, l1, l0) != ARMOUR_EINVAL ||
            run_moving(&m, nullptr, vel, e0, e1) != ARMOUR_EINVAL) {
            printf("FAILED: a bad argument of the moving entry passed\n");
            return 1;
        }
        printf("ik moving host check ok: zero velocity equals the static call for two sets of windows; the arriving cube blocks its target late\n");
    }
    printf("ik host check ok: %d of %d items converged, picks %d %d %d %d, margins %.3g %.3g, Jacobian within %.2g of central differences\n", converged, N * S, a.best[0],
           a.best[1], a.best[2], a.best[3], a.margin[1], a.margin[2], worst_fd);
    return 0;
}
