// armour_track under ARMOUR_TRACK_CTL_ALTHOFF: the steps of tracking_steps.h with controller_core.h's althoff_update as the controller
// (RobustController::update, ALTHOFF method, robust_controller.cpp:63-128; e_acc = 0 at every stage, as in the reference's runs).
// The host entry is tracking.hip's armour_track; this unit holds the mode's kernel alone (tracking_steps.h says why) under the same build
// check: one function, static stack.
#include "tracking_steps.h"

namespace {

using namespace trk;

__global__ __launch_bounds__(64) void armour_track_althoff_kernel(const TrackArgs* __restrict__ ap, int B, const TrackIn* __restrict__ inputs,
                                                                  ArmourTrackResult* __restrict__ state, double* __restrict__ trace, int steps) {
    track_steps<true>(ap, B, inputs, state, trace, steps);
}

}  // namespace

void trk::track_althoff_launch(hipStream_t stream, const TrackArgs* args, int B, const TrackIn* inputs, ArmourTrackResult* state, double* trace, int steps) {
    hipLaunchKernelGGL(armour_track_althoff_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, args, B, inputs, state, trace, steps);
}
