/*
 * pm_plan.cpp — pass planning (pm_plan.h). Host-only and free of HIP, like
 * pm_scene.cpp: tests/native compiles it with g++.
 */
#include "pm_plan.h"

#include <algorithm>
#include <cmath>

namespace pm {

GridDesc make_grid(const float lo[3], const float hi[3], int estimator, int cell_span, float radius2) {
    GridDesc g{};
    const float rq = sqrtf(radius2) * 1.0001f + 1e-4f;
    const float f = estimator == PM_ESTIMATOR_KNN ? 0.5f : 2.0f / (float)(cell_span - 1);
    float cs = f * rq * 1.001f;
    float ext[3];
    for (int a = 0; a < 3; ++a) ext[a] = std::max(hi[a] - lo[a], 1e-3f);
    int64_t dims[3];
    while (true) {
        for (int a = 0; a < 3; ++a) dims[a] = std::max<int64_t>(1, (int64_t)std::ceil(ext[a] / cs) + 1);
        if (dims[0] * dims[1] * dims[2] <= (int64_t)1 << 25) break;
        cs *= 1.25f;
    }
    g.gx = lo[0]; g.gy = lo[1]; g.gz = lo[2];
    g.inv_cs = 1.0f / cs;
    g.dx = (int)dims[0]; g.dy = (int)dims[1]; g.dz = (int)dims[2];
    g.ncells = (uint32_t)(dims[0] * dims[1] * dims[2]);
    return g;
}

float quantile_radius2(const uint32_t hist[R2_BINS], float init, double quantile, int *bin) {
    uint64_t total = 0;
    for (int b = 0; b < R2_BINS; ++b) total += hist[b];
    /* bins b.. hold t = r^2 / init <= 2^(-b/8): the largest b that still covers the quantile */
    int best = 0;
    uint64_t above = total;
    for (int b = 0; b < R2_BINS; ++b) {
        if ((double)above < quantile * (double)total) break;
        best = b;
        above -= hist[b];
    }
    if (bin) *bin = best;
    /* the bins come from an approximate log2: a small margin */
    return total ? std::min(init, (float)(init * std::exp2(-best / (double)R2_PER_OCTAVE) * 1.01)) : 0.f;
}

void R2Plan::landed(const uint32_t hist[R2_BINS], float init) {
    pending = false;
    if (valid && hist_init == init) design_r2 = quantile_radius2(hist, init, quantile);
}

void R2Plan::reduce_issued(const void *s) {
    pending = true;
    stream = s;
    accum = false; /* the reduce re-zeroes the bins */
    valid = true;
    hist_init = accum_init;
}

float R2Plan::radius2(float init, bool rec_fresh) const {
    if (rec_fresh || !valid || hist_init != init) return init;
    return design_r2 > 0.f ? design_r2 : init;
}

R2Plan::BinPrep R2Plan::before_bin(float init, const void *s) {
    const bool wait = pending && stream != s;
    if (accum && accum_init != init) { accum = false; dirty = true; }
    const bool clear = dirty;
    dirty = false;
    return {wait, clear};
}

void R2Plan::invalidate() {
    valid = false;
    design_r2 = 0.f;
    if (accum) { accum = false; dirty = true; }
}

std::vector<std::vector<std::pair<int64_t, int64_t>>> device_bands(int64_t n, int64_t unit, int world) {
    std::vector<std::vector<std::pair<int64_t, int64_t>>> owned(world);
    const int64_t units = (n + unit - 1) / unit;
    const int64_t runs = std::max<int64_t>(1, (units + (int64_t)world * 4 - 1) / ((int64_t)world * 4));
    int k = 0;
    for (int64_t u = 0; u < units; u += runs, ++k) {
        const int64_t b = u * unit, e = std::min(n, (u + runs) * unit);
        owned[k % world].push_back({b, e - b});
    }
    return owned;
}

/* the dynamic LDS of a trace block, the one place its bytes are written
 * down: a stack column per thread, then (per-lane kernels) the scene blob,
 * then (HOLD) the held deposits' columns from the next 16-B boundary */
static size_t stack_bytes(int entries) { return (size_t)entries * TRACE_BLOCK * 4; }
static size_t hold_bytes() { return (size_t)HOLD_WORDS * TRACE_BLOCK * 4; }
static size_t lane_lds(const TraceShape &sh, bool hold) {
    const size_t lds = stack_bytes(sh.stack_depth) + sh.lds_bytes;
    return hold ? lds + ((size_t)sh.lds_bytes + 15u) / 16u * 16u - sh.lds_bytes + hold_bytes() : lds;
}
static TraceFamily lane_family(int mode) {
    return mode == MODE_BRUTE ? TRACE_LANE_BRUTE : mode == MODE_LDS ? TRACE_LANE_LDS : mode == MODE_INST ? TRACE_LANE_INST : TRACE_LANE_GLOBAL;
}

TracePlan plan_trace(const TraceShape &sh, const WavesPerCu &waves_per_cu) {
    constexpr int64_t block_waves = TRACE_BLOCK / 64;
    TracePlan pl;
    pl.hold = sh.trace_hold && !sh.mark ? 1 : 0; /* marking stores per deposit: the mark bit is not carried through held_put */
    if (pl.hold && !sh.wide) { /* per-lane kernel: only when the held deposits' LDS costs no resident waves */
        const TraceFamily asked = sh.mode == MODE_INST ? TRACE_LANE_GLOBAL : lane_family(sh.mode);
        if (waves_per_cu(asked, true, lane_lds(sh, true)) < waves_per_cu(asked, false, lane_lds(sh, false))) pl.hold = 0;
    }
    if (sh.wide) {
        /* pooled kernel: one occupancy round (resident waves per CU: VGPRs
         * and the LDS stacks), each wave with a contiguous pool of paths. C3
         * sweep (1M paths, 256 CUs): 4096 waves 5.25 ms, 8192 (two rounds)
         * 5.81, 5462 (1.33 rounds) 6.73, 2048 7.22 */
        /* LDS stack entries per lane (pool_stack; 0 = the tree's exact
         * bound): below the bound, deeper entries spill to global memory and
         * the smaller LDS reservation admits more resident blocks */
        pl.lstk = sh.pool_stack > 0 && sh.pool_stack < sh.stack_depth ? sh.pool_stack : sh.stack_depth;
        const TraceFamily pool = sh.wide == 3 ? TRACE_POOL8 : TRACE_POOL;
        const size_t asked = stack_bytes(pl.lstk) + sh.lds_bytes; /* with S.lds_bytes: see pm_plan.h */
        int per_cu = waves_per_cu(pool, false, asked);
        if (pl.hold) { /* the held deposits' LDS must not cost resident waves */
            const int per_cu_h = waves_per_cu(pool, true, asked + hold_bytes());
            if (per_cu_h < per_cu) pl.hold = 0;
            else per_cu = per_cu_h;
        }
        const int64_t waves = (int64_t)(sh.cus > 0 ? sh.cus : 256) * (per_cu > 0 ? per_cu : 16);
        /* any pool size works (the wave's cursor hands out paths to dead lanes) */
        const int64_t per = std::max<int64_t>(1, (sh.path_count + waves - 1) / waves);
        pl.pool_paths = sh.trace_pool || sh.wide == 3 ? per : 0;
        pl.pooled = pl.pool_paths > 0 && sh.mode == MODE_GLOBAL;
        const int64_t pool_blocks = ((sh.path_count + per - 1) / per + block_waves - 1) / block_waves;
        if (pl.lstk < sh.stack_depth) {
            pl.spill_entries = sh.stack_depth - pl.lstk;
            pl.spill_stride = (uint32_t)(pool_blocks * TRACE_BLOCK);
        }
        if (pl.pooled) {
            pl.family = pool;
            pl.grid_blocks = pool_blocks;
            pl.lds = stack_bytes(pl.lstk);
            pl.lds_hold = pl.lds + hold_bytes();
        }
    }
    if (!pl.pooled) {
        pl.family = lane_family(sh.mode);
        pl.grid_blocks = (sh.path_count + TRACE_BLOCK - 1) / TRACE_BLOCK;
        pl.lds = lane_lds(sh, false);
        pl.lds_hold = lane_lds(sh, true);
    }
    pl.hold_launch = pl.hold && sh.mpc == HOLD_MPC && sh.slots_aligned;
    return pl;
}

} // namespace pm
