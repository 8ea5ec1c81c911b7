// The robot and the scene of the stand-alone host checks (tools/*_host_check.cpp).  In the shipped ABI: the Kinova Gen3, J = n = 7.  With
// -DARMOUR_KEY128 (the 8-factor ABI; make -C armour_amd/csrc k128host): fetch8, n = 8 = ARMOUR_MAX_FACTORS and J = 9 = ARMOUR_MAX_JOINTS, so
// that every q[ARMOUR_MAX_FACTORS] and r[ARMOUR_MAX_JOINTS] of the host twins is full under the sanitizers.  The fetch8 scene is that of
// tests/test_tree_plan.py _fetch_world("fetch8"): the shoulder pan turns by 1.2 rad through a thin wall about link 6.
#ifndef ARMOUR_HOST_CHECK_ROBOT_H
#define ARMOUR_HOST_CHECK_ROBOT_H

#include "../include/armour_robot_fetch.h"
#include "../include/armour_robot_kinova.h"

#if defined(ARMOUR_KEY128)
static_assert(ARMOUR_MAX_FACTORS == 8, "the 8-factor ABI");
static const bool HC_KINOVA_SCENE = false;      // assertions on a particular status or count of the Kinova's scene hold only there
static inline void host_check_robot(ArmourRobot* r) { armour_fill_fetch8(r); }
static const double HC_START[ARMOUR_MAX_FACTORS] = {0.0, 0.0, 0.4, 0.0, 0.8, 0.0, 0.0, 0.0}, HC_GOAL[ARMOUR_MAX_FACTORS] = {0.0, 1.2, 0.4, 0.0, 0.8, 0.0, 0.0, 0.0};
static const int HC_WALL_LINK = 6, HC_SWING_JOINT = 2;
static const double HC_WALL_HALF[3] = {0.05, 0.05, 0.10}, HC_SWING = -1.2, HC_LATE[2] = {1.9, 2.1};   // (the wall, 1 m out at t = 0, is back at t = 2)
static const double HC_FOLDED[ARMOUR_MAX_FACTORS] = {0.0, 0.0, 1.4, 0.0, 2.2, 0.0, 2.0, 0.0};
static const double HC_IK_GOAL[ARMOUR_MAX_FACTORS] = {0.2, 0.3, 0.4, -0.2, 0.8, 0.1, 0.6, 0.0}, HC_IK_REF[ARMOUR_MAX_FACTORS] = {0.0, 0.0, 0.3, 0.0, 0.6, 0.0, 0.4, 0.0};
#else
static const bool HC_KINOVA_SCENE = true;
static inline void host_check_robot(ArmourRobot* r) { armour_fill_kinova_gen3_no_gripper(r); }
static const double HC_START[ARMOUR_MAX_FACTORS] = {0.0, 0.6, 0.0, 1.2, 0.0, 0.6, 0.0}, HC_GOAL[ARMOUR_MAX_FACTORS] = {2.0, 0.6, 0.0, 1.2, 0.0, 0.6, 0.0};
static const int HC_WALL_LINK = 5, HC_SWING_JOINT = 1;
static const double HC_WALL_HALF[3] = {0.06, 0.06, 0.12}, HC_SWING = -2.0, HC_LATE[2] = {1.4, 1.6};
static const double HC_FOLDED[ARMOUR_MAX_FACTORS] = {0.0, 2.1, 0.0, 2.5, 0.0, 1.0, 0.0};
static const double HC_IK_GOAL[ARMOUR_MAX_FACTORS] = {0.3, 0.6, -0.2, 1.2, 0.1, 0.6, 0.0}, HC_IK_REF[ARMOUR_MAX_FACTORS] = {0.0, 0.3, 0.0, 0.9, 0.0, 0.4, 0.0};
#endif

#endif
