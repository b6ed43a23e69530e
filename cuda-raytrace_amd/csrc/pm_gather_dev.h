/*
 * pm_gather_dev.h — device-inline code shared by the gather and record units
 * (pm_gather.hip, pm_gather_knn.hip, pm_records.hip): the PPM update
 * (ppm_apply), the wave-level LDS ordering point and DPP scans / reductions,
 * the union cell box of a wave's lanes (union_box6), and the diagnostic
 * builds' hooks of the tile kernels (TILE_STAT, GProf). Only what more than
 * one of those units uses lives here.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "pm_kernels.h"

#pragma clang fp contract(off)

namespace pm {
/* gathering.cu:104-126 PPM update */
PMD void ppm_apply(float4 &st, float &N, int M, v3 L, float alpha) {
    if (M > 0) {
        int totalPhotons = N + alpha * M;
        float ratio = totalPhotons / (N + M);
        st.w = st.w * ratio;
        v3 flux = (xyz(st) + L) * ratio;
        st.x = flux.x; st.y = flux.y; st.z = flux.z;
        N = totalPhotons;
    }
}

/* LDS traffic between lanes of one wave: ds_* of a wave execute in order, so
 * a compiler-level ordering point is all the exchange needs */
PMD void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
/* inclusive wave scans on DPP (row_shr 1/2/4/8 inside rows of 16 lanes,
 * then row_bcast 15/31 into rows 1,3 / 2,3): VALU-rate cross-lane moves
 * instead of an LDS round trip per step (__shfl = ds_bpermute). A lane
 * whose DPP source is out of its row, or whose row the mask leaves out,
 * receives `id`, the operation's identity, so no lane guards are needed.
 * Every lane must be active. */
template <class Op>
PMD int wave_scan_dpp(int v, int id, Op op) {
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x111, 0xf, 0xf, false)); /* row_shr:1 */
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x112, 0xf, 0xf, false)); /* row_shr:2 */
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x114, 0xf, 0xf, false)); /* row_shr:4 */
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x118, 0xf, 0xf, false)); /* row_shr:8 */
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x142, 0xa, 0xf, false)); /* row_bcast:15 -> rows 1, 3 */
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x143, 0xc, 0xf, false)); /* row_bcast:31 -> rows 2, 3 */
    return v;
}
PMD uint32_t wave_incl_sum_u32(uint32_t v) {
    return (uint32_t)wave_scan_dpp((int)v, 0, [](int a, int b) { return (int)((uint32_t)a + (uint32_t)b); });
}
PMD int wave_incl_max_i32(int v) { return wave_scan_dpp(v, -1, [](int a, int b) { return max(a, b); }); }
/* wave-uniform min / max (the scan's last lane) */
PMD uint32_t wave_min_u32(uint32_t v) {
    const int m = wave_scan_dpp((int)v, -1, [](int a, int b) { return (int)min((uint32_t)a, (uint32_t)b); });
    return (uint32_t)__builtin_amdgcn_readlane(m, 63);
}
PMD uint32_t wave_max_u32(uint32_t v) {
    const int m = wave_scan_dpp((int)v, 0, [](int a, int b) { return (int)max((uint32_t)a, (uint32_t)b); });
    return (uint32_t)__builtin_amdgcn_readlane(m, 63);
}
/* two 16-bit minima at once (v_pk_min_u16) */
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
PMD uint32_t wave_min_2x16(uint32_t v) {
    const int m = wave_scan_dpp((int)v, -1, [](int a, int b) {
        return (int)__builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a),
                                                                          __builtin_bit_cast(u16x2, b)));
    });
    return (uint32_t)__builtin_amdgcn_readlane(m, 63);
}
PMD uint32_t uniform_u32(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

typedef float f2 __attribute__((ext_vector_type(2)));
/* PM_TILE_STATS builds (make variant VFLAGS=-DPM_TILE_STATS): per-wave event
 * counts of k_gather_tile into counters[8..15] (read with pm_trace_profile):
 * tile waves, windows, test pairs, hit iterations, direct lanes, chunks,
 * wide (> 64 rows) waves, staged photons */
#ifdef PM_TILE_STATS
#define TILE_STAT(k, v) do { const unsigned long long tv_ = (unsigned long long)(v); \
    if ((threadIdx.x & 63) == 0) atomicAdd(&P.counters[8 + (k)], tv_); } while (0)
#elif defined(PM_TILE_TIMES)
/* per-wave counts for the wave timeline records (k_gather_tile only) */
#define TILE_STAT(k, v) do { tstat[(k)] += (uint32_t)(v); } while (0)
#else
#define TILE_STAT(k, v) do { } while (0)
#endif

/* PM_GATHER_PROFILE builds (make variant VFLAGS=-DPM_GATHER_PROFILE): wave
 * clock (s_memtime) per phase of k_gather_tile, summed over waves into
 * counters[8..14] (record, group, stage, test, hits, direct, store) and the
 * wave count into counters[15] (tools/gather_profile.py). A phase's time
 * includes the memory waits of the loads it first consumes. */
struct GProf {
#ifdef PM_GATHER_PROFILE
    uint64_t last = 0, acc[7] = {0, 0, 0, 0, 0, 0, 0};
    PMD void begin() { last = __builtin_amdgcn_s_memtime(); }
    PMD void mark(int i) {
        const uint64_t t = __builtin_amdgcn_s_memtime();
        acc[i] += t - last;
        last = t;
    }
    PMD void flush(unsigned long long *out) {
        if (!out || (threadIdx.x & 63) != 0) return;
        for (int i = 0; i < 7; ++i) atomicAdd(&out[8 + i], (unsigned long long)acc[i]);
        atomicAdd(&out[15], 1ull);
    }
#else
    PMD void begin() {}
    PMD void mark(int) {}
    PMD void flush(unsigned long long *) {}
#endif
};

/* the cell box [X0, X1] x [Y0, Y1] x [Z0, Z1] of the lanes with `in` set */
PMD void union_box6(const GridDesc &g, bool in, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1, uint32_t z0,
                    uint32_t z1, uint32_t &X0, uint32_t &X1, uint32_t &Y0, uint32_t &Y1, uint32_t &Z0, uint32_t &Z1) {
    if (g.dx < 65536 && g.dy < 65536 && g.dz < 65536) {
        /* three packed 16-bit minima (maxima as minima of 0xffff - c) */
        const uint32_t m0 = wave_min_2x16(in ? (x0 << 16) | y0 : 0xffffffffu);
        const uint32_t m1 = wave_min_2x16(in ? ((0xffffu - x1) << 16) | (0xffffu - y1) : 0xffffffffu);
        const uint32_t m2 = wave_min_2x16(in ? (z0 << 16) | (0xffffu - z1) : 0xffffffffu);
        X0 = m0 >> 16; Y0 = m0 & 0xffffu; X1 = 0xffffu - (m1 >> 16); Y1 = 0xffffu - (m1 & 0xffffu);
        Z0 = m2 >> 16; Z1 = 0xffffu - (m2 & 0xffffu);
    } else {
        X0 = wave_min_u32(in ? x0 : 0xffffffffu); X1 = wave_max_u32(in ? x1 : 0u);
        Y0 = wave_min_u32(in ? y0 : 0xffffffffu); Y1 = wave_max_u32(in ? y1 : 0u);
        Z0 = wave_min_u32(in ? z0 : 0xffffffffu); Z1 = wave_max_u32(in ? z1 : 0u);
    }
}

} // namespace pm
