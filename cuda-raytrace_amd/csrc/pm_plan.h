/*
 * pm_plan.h — pass planning: which photon grid a pass gets (the grid of a
 * radius, the adaptive radius and its state machine), which record bands
 * a device of a group gathers, and the trace launch's geometry (TracePlan).
 * Host code only, no HIP: pm_api_photons.cpp and pm_api_gather.cpp perform the
 * HIP call each answer asks for, and tests/native drives the same code on a CPU
 * (tests/test_pass_plan.py, tests/test_trace_plan.py).
 */
#pragma once
#include <stdint.h>

#include <stddef.h>

#include <functional>
#include <utility>
#include <vector>

#include "../../include/pm_api.h"
#include "pm_plan_pod.h"
#include "pm_scene_pod.h"

namespace pm {

/* photon-bucket grid over the scene box [lo, hi] for queries of radius^2
 * `radius2`. PPM: cell edge 2 r / (cell_span - 1), so a query box
 * [p - r', p + r'], r' <= r, spans <= cell_span cells per axis (span 2 by
 * default: at most 2x2x2 cells; env PM_CELL_SPAN 3..5 for finer cells,
 * DESIGN.md §5 sweep). kNN: r / 2 — the query visits rows nearest first and
 * prunes cells beyond the shrinking k-th distance (k_gather_knn). Cells grow
 * by 1.25 until the grid has at most 2^25 of them. */
GridDesc make_grid(const float lo[3], const float hi[3], int estimator, int cell_span, float radius2);

/* the grid radius^2 that covers `quantile` of the radii binned in hist
 * (bin b counts r^2 / init in (2^(-(b+1)/8), 2^(-b/8)], pm_gather.hip), at
 * most init; 0 for an empty histogram. *bin: the bin chosen. */
float quantile_radius2(const uint32_t hist[R2_BINS], float init, double quantile, int *bin = nullptr);

/* Adaptive grid radius (progressive PPM: radii shrink pass by pass). The
 * fused tile gather bins every updated r^2 (R2_BINS log bins per copy,
 * R2_COPIES copies) on the device; when the next pass chooses its grid the
 * bins are reduced into host-mapped memory behind an event and, once landed,
 * set the following passes' grid radius to the `quantile` of the records'
 * radii (the rest scan per lane). Staleness is safe (radii only shrink);
 * anything that can raise a radius (eye pass, reset, upload, set_radius2,
 * kNN radii) invalidates it. The grid only sets the cost of a gather, never
 * its sums. Streams are opaque identities. */
struct R2Plan {
    double quantile = 0.9;   /* env PM_GRID_QUANTILE; <= 0 disables. C5 step (same box, 3 runs each): 0.95 0.82-0.85 ms, 0.9 0.784-0.790, 0.8 0.826 */
    bool wanted = false;     /* a progressive pass asked for the radii (no histogram otherwise) */
    bool accum = false;      /* the device bins hold this pass's gathers (every band), not yet reduced */
    bool dirty = true;       /* the device bins hold nothing usable (never zeroed, or invalidated radii): zero before binning */
    bool pending = false;    /* a reduce in flight */
    bool valid = false;      /* the last landed / in-flight histogram describes the records */
    float accum_init = 0.f;  /* the r^2 the accumulated bins are relative to */
    float hist_init = 0.f;   /* the r^2 the histogram's bins are relative to */
    float design_r2 = 0.f;   /* grid radius^2 from the last landed histogram (0: the initial radius) */
    const void *stream = nullptr; /* the stream the last reduce ran on */

    /* false (kNN, or disabled): the grid radius is the initial radius and no event below is delivered */
    bool active(int estimator) const { return estimator != PM_ESTIMATOR_KNN && quantile > 0.0; }

    /* a new pass chooses its grid, in this order: */
    /* the pending reduce's event has fired: the R2_BINS host words set the
     * grid radius if they still describe the records of a pass with `init` */
    void landed(const uint32_t hist[R2_BINS], float init);
    /* the previous pass's gathers binned their radii: reduce them once (not
     * while a reduce is in flight: the host words are reused; the bins keep
     * accumulating, and older radii only overestimate) */
    bool reduce_due() const { return accum && !pending; }
    /* the reduce and its event were issued on `s` (both succeeded) */
    void reduce_issued(const void *s);
    /* a pass that continues a render (no reset pending) has its gathers bin their radii for the passes after it */
    void pass_began(bool rec_fresh) { wanted = !rec_fresh; }
    float radius2(float init, bool rec_fresh) const;

    /* a gather is about to bin radii relative to `init` on stream `s`.
     * wait: the pending reduce reads and re-zeroes the bins on another
     * stream — bin (and clear) only after its event. clear: zero the bins
     * first (whatever they hold is dropped). */
    struct BinPrep { bool wait, clear; };
    BinPrep before_bin(float init, const void *s);
    void binned(float init) { accum = true; accum_init = init; }

    /* the records' radii changed in a way that may raise them: back to the
     * initial radius; bins accumulated from the old radii are dropped */
    void invalidate();
};

/* the all-gather mode's record ranges (begin, count) of each device: 8-row
 * bands (`unit` records each) in runs dealt round-robin, about four runs per
 * device (pmrender/dist.py _bands; tests/test_pass_plan.py holds them equal) */
std::vector<std::vector<std::pair<int64_t, int64_t>>> device_bands(int64_t n, int64_t unit, int world);

/* ---- the trace launch ------------------------------------------------------
 * One trace call's launch geometry, decided once: pm_trace_photons
 * (pm_api_photons.cpp) fills TraceParams and sizes the spill buffer from it,
 * launch_trace (pm_trace.hip) takes its kernel, grid and LDS bytes from it.
 * The kernels index what it sizes: trace_lane_body / trace_pool_body
 * (pm_trace.hip) derive the same lstk from TraceParams::pool_stack and
 * S.stack_depth, lay the LDS out as [stacks][scene blob, per-lane LDS modes
 * only][pad to 16 B][held deposits] and address the spill area by
 * blockIdx.x * TRACE_BLOCK + threadIdx.x < spill_stride. */

/* the kernel family whose resident waves are asked for / that launches */
enum TraceFamily : int { TRACE_LANE_GLOBAL = 0, TRACE_LANE_LDS, TRACE_LANE_BRUTE, TRACE_LANE_INST, TRACE_POOL, TRACE_POOL8 };

struct TraceShape {
    int64_t path_count = 0;
    int mpc = HOLD_MPC;        /* max_photon_count of the call */
    bool slots_aligned = true; /* the slot buffer is 16-B aligned */
    int mode = MODE_GLOBAL;    /* scene_mode(S) */
    int wide = 0;              /* S.wide: 0 no wide tree, 2 the 4-wide one, 3 the 8-wide one */
    int stack_depth = 2;       /* S.stack_depth: the traversal stack's bound */
    uint32_t lds_bytes = 0;    /* S.lds_bytes */
    int pool_stack = 31;       /* the context's settings (env PM_POOL_STACK, PM_TRACE_POOL, PM_TRACE_HOLD) */
    bool trace_pool = true, trace_hold = true;
    int cus = 0;               /* compute units of the device (the context's env PM_TRACE_CUS in their place); <= 0: unknown, taken as 256 */
    bool mark = false;         /* pm_set_caustic_map: the launch marks caustic photons (the MARK instantiations) */
};

/* resident waves per CU of `family`'s HOLD (hold) or plain instantiation at
 * `lds` bytes of dynamic LDS per block, all of it (the held deposits' share
 * included); 0: unknown. The library asks the occupancy API
 * (trace_waves_per_cu, pm_trace.hip), the CPU test a table. */
using WavesPerCu = std::function<int(TraceFamily family, bool hold, size_t lds)>;

struct TracePlan {
    TraceFamily family = TRACE_LANE_GLOBAL; /* the kernel that launches */
    bool pooled = false;      /* family is TRACE_POOL / TRACE_POOL8: pool_paths paths per wave; else one path per lane */
    int lstk = 0;             /* TraceParams::pool_stack: LDS stack entries per lane of a scene with a wide tree
                               * (pool_stack when set and below stack_depth, else stack_depth); 0 without one */
    int64_t pool_paths = 0;   /* TraceParams::pool_paths */
    int64_t grid_blocks = 0;  /* blocks of TRACE_BLOCK threads */
    size_t lds = 0, lds_hold = 0; /* the launch's dynamic LDS bytes: per-deposit stores / held deposits */
    int hold = 0;             /* TraceParams::hold: held deposits wanted and free of resident waves; the fused
                               * counting's key layout and the lazy zero fill follow this one */
    bool hold_launch = false; /* the HOLD instantiation launches (with lds_hold): hold, mpc == HOLD_MPC, aligned slots */
    int spill_entries = 0;    /* stack entries per thread beyond lstk: TraceParams::spill holds spill_entries * spill_stride ints */
    uint32_t spill_stride = 0; /* TraceParams::spill_stride (0 with no spill) */
};

/* Oddities of the launch as it was measured, kept:
 *  - occupancy unknown (0) counts as 16 waves per CU, an unknown device as 256 CUs;
 *  - the 8-wide tree always takes the pooled kernel (its deeper stacks need the spill), whatever trace_pool says;
 *  - MODE_INST with a wide tree is planned like a pooled scene (lstk, pool_paths, hold, spill) but launches the
 *    per-lane kernel (the pooled one walks one level), which reads none of the four;
 * and where two sites disagreed, each keeps its value:
 *  - the pooled occupancy is asked at stacks + S.lds_bytes, the pooled launch reserves the stacks alone (a pooled
 *    launch has S.lds_bytes == 0: the two differ only where the per-lane kernel launches after all);
 *  - `hold` stays set at another mpc or a misaligned slot buffer, where the launch stores per deposit
 *    (hold_launch): the fused keys are then slot-major and not lazily zeroed, as for a held launch;
 *  - a per-lane MODE_INST launch asks the occupancy of TRACE_LANE_GLOBAL;
 *  - a wide scene launched per lane (MODE_INST, or trace_pool off) still gets the pooled geometry's spill_stride,
 *    which is not its grid's thread count: the per-lane kernel has no spill.
 * Marking (TraceShape::mark): the MARK instantiations store per deposit, so hold and hold_launch are 0 whatever
 * trace_hold says and no HOLD occupancy is asked; the pooled round is sized by the unmarked kernel's waves (the
 * occupancy attribute pins both to the same count). Everything else is the plan of trace_hold = 0. */
TracePlan plan_trace(const TraceShape &sh, const WavesPerCu &waves_per_cu);

} // namespace pm
