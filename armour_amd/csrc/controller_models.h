// The controller's models from the ArmourRobot constants: the model file -> CoM frames -> interval model preparation of the reference
// (robot_models.cpp:124-255), host arithmetic done once per call.  Shared by the controller (controller.hip) and the tracking
// simulator (tracking.hip), so that both run the same nominal and interval models.
#pragma once
#include <cmath>
#include <cstdlib>

#include "controller_core.h"

namespace ctl {

inline void rpy(double roll, double pitch, double yaw, double* c) {  // RT/PZsparse.cu:160-176 (the same convention as the planner)
    c[0] = cos(pitch) * cos(yaw);
    c[1] = -cos(pitch) * sin(yaw);
    c[2] = sin(pitch);
    c[3] = cos(roll) * sin(yaw) + cos(yaw) * sin(pitch) * sin(roll);
    c[4] = cos(roll) * cos(yaw) - sin(pitch) * sin(roll) * sin(yaw);
    c[5] = -cos(pitch) * sin(roll);
    c[6] = sin(roll) * sin(yaw) - cos(roll) * cos(yaw) * sin(pitch);
    c[7] = cos(yaw) * sin(roll) + cos(roll) * sin(pitch) * sin(yaw);
    c[8] = cos(pitch) * cos(roll);
}

// The model file of the reference (kinova_without_gripper.txt) holds, per joint: the joint twist (rotation about the
// joint's own axis), the spatial inertia at the joint frame, the parent-to-joint transform and the CoM offset.  The
// same quantities follow from ArmourRobot; Model::Model then re-expresses everything in CoM frames.
inline int build_models(const ArmourRobot& rb, double eps, Model<double>& md, Model<Itv>& imd) {
    const int n = rb.num_factors;
    if (n < 1 || n > ARMOUR_MAX_FACTORS) return -1;
    Tw<double> S[ARMOUR_MAX_FACTORS];
    Ri<double> I[ARMOUR_MAX_FACTORS];
    Xf<double> XT[ARMOUR_MAX_FACTORS], CoM[ARMOUR_MAX_FACTORS];
    for (int i = 0; i < n; i++) {
        const int ax = std::abs(rb.axes[i]);
        if (ax < 1 || ax > 3) return -1;
        S[i].w = vzero<double>(); S[i].v = vzero<double>();
        S[i].w.x[ax - 1] = rb.axes[i] > 0 ? 1.0 : -1.0;
        // RigidInertia(m, c, Ic), spatial.cpp:123-131
        V3<double> c{{rb.com[3 * i], rb.com[3 * i + 1], rb.com[3 * i + 2]}};
        M3<double> Ic;
        for (int e = 0; e < 9; e++) Ic.a[e] = rb.inertia[9 * i + e];
        const M3<double> ch = hat(c);
        I[i].m = rb.mass[i];
        I[i].m_c_hat = lscale(rb.mass[i], ch);
        I[i].I_bar = Ic - I[i].m_c_hat * ch;
        // parent-to-joint transform: E = R_rpy^T, r = trans (Featherstone's X = (E, r))
        double R[9];
        rpy(rb.rots[3 * i], rb.rots[3 * i + 1], rb.rots[3 * i + 2], R);
        M3<double> Rm;
        for (int e = 0; e < 9; e++) Rm.a[e] = R[e];
        XT[i].R = tr(Rm);
        XT[i].p = V3<double>{{rb.trans[3 * i], rb.trans[3 * i + 1], rb.trans[3 * i + 2]}};
        CoM[i].R = mident<double>();
        CoM[i].p = c;
    }
    md.n = n;
    for (int i = 0; i < n; i++) {  // robot_models.cpp:133-155
        Xf<double> Xwj = XT[i];
        for (int pind = i - 1; pind > -1; pind--) Xwj = apply(Xwj, XT[pind]);
        md.S_[i] = invapply(Xwj, S[i]);
        md.I[i] = apply(CoM[i], I[i]);
        const Xf<double> prev = i > 0 ? CoM[i - 1] : xf_identity<double>();
        md.XTree[i] = apply(prev, apply(inverse(XT[i]), inverse(CoM[i])));
        md.transI[i] = rb.armature[i];
        md.damping[i] = rb.damping[i];
        md.friction[i] = rb.friction[i];
    }
    md.gravity.w = vzero<double>();
    md.gravity.v = V3<double>{{0.0, 0.0, -rb.gravity}};
    // IntModel(model, eps), robot_models.cpp:176-255: point intervals, then mass and I_bar widened by 1 -+ eps
    imd.n = n;
    const double lowP = 1 - eps, highP = 1 + eps;
    for (int i = 0; i < n; i++) {
        for (int e = 0; e < 3; e++) { imd.S_[i].w.x[e] = Itv{md.S_[i].w.x[e], md.S_[i].w.x[e]}; imd.S_[i].v.x[e] = Itv{md.S_[i].v.x[e], md.S_[i].v.x[e]}; imd.XTree[i].p.x[e] = Itv{md.XTree[i].p.x[e], md.XTree[i].p.x[e]}; }
        for (int e = 0; e < 9; e++) {
            imd.XTree[i].R.a[e] = Itv{md.XTree[i].R.a[e], md.XTree[i].R.a[e]};
            imd.I[i].m_c_hat.a[e] = Itv{md.I[i].m_c_hat.a[e], md.I[i].m_c_hat.a[e]};
            const double val = md.I[i].I_bar.a[e];
            imd.I[i].I_bar.a[e] = val >= 0 ? Itv{val * lowP, val * highP} : Itv{val * highP, val * lowP};
        }
        imd.I[i].m = Itv{md.I[i].m * lowP, md.I[i].m * highP};
        imd.transI[i] = Itv{md.transI[i], md.transI[i]};
        imd.damping[i] = md.damping[i];
        imd.friction[i] = md.friction[i];
    }
    for (int e = 0; e < 3; e++) { imd.gravity.w.x[e] = Itv{0.0, 0.0}; imd.gravity.v.x[e] = Itv{md.gravity.v.x[e], md.gravity.v.x[e]}; }
    return 0;
}

}  // namespace ctl
