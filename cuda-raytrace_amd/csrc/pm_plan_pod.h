/*
 * pm_plan_pod.h — the photon grid's descriptor and the radius histogram's
 * constants, read by the kernels (pm_kernels.h) and by the host-only pass
 * planning (pm_plan.h). Plain C++: no HIP header.
 */
#pragma once
#include <stdint.h>

namespace pm {

constexpr int R2_BINS = 64, R2_COPIES = 256, R2_PER_OCTAVE = 8; /* radius histogram (adaptive grid) */
struct GridDesc {
    float gx, gy, gz, inv_cs;
    int dx, dy, dz;
    uint32_t ncells;
};
static_assert(sizeof(GridDesc) == 32, "GridDesc is passed by value in kernel parameter blocks");

} // namespace pm
