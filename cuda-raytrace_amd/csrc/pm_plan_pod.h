/*
 * pm_plan_pod.h — the photon grid's descriptor, the radius histogram's
 * constants and the trace kernels' block geometry, read by the kernels
 * (pm_kernels.h) and by the host-only pass planning (pm_plan.h). Plain C++:
 * no HIP header.
 */
#pragma once
#include <stdint.h>

namespace pm {

/* the trace kernels' block and the held deposits' LDS (pm_trace.hip Held):
 * plan_trace (pm_plan.h) sizes the launch the kernels index with these */
constexpr int TRACE_BLOCK = 256;    /* k_trace: 4 waves compact paths together */
constexpr int HOLD_MPC = 4;         /* deposits are held only at the reference's 4 photons per path */
constexpr int HOLD_WORDS = 27;      /* LDS words per thread: slots 0..2: p, alpha, wi */

constexpr int R2_BINS = 64, R2_COPIES = 256, R2_PER_OCTAVE = 8; /* radius histogram (adaptive grid) */
struct GridDesc {
    float gx, gy, gz, inv_cs;
    int dx, dy, dz;
    uint32_t ncells;
};
static_assert(sizeof(GridDesc) == 32, "GridDesc is passed by value in kernel parameter blocks");

} // namespace pm
