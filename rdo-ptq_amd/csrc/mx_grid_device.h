// The grid that the learned-rounding kernels on the MX block formats hand to ada_element (ada_device.h): shared by mx_round.hip (one
// tensor a launch) and mx_round_batch.hip (a unit a launch) so that both run the same arithmetic on an element.
#pragma once

namespace {

// The MX grid of one weight (ada_element's Grid): lo is on the grid and so is lo + gap -- no level clamp, dq/dh = gap everywhere
struct MxGrid {
    float lo, gap;
    __device__ __forceinline__ float q(float h) const { return lo + gap * h; }
    __device__ __forceinline__ float dq_dh(float g, float) const { return g * gap; }
};

}  // namespace
