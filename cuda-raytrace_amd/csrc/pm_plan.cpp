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

} // namespace pm
