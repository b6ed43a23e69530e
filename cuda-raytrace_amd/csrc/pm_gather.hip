/*
 * pm_gather.hip — the PPM gathers: fixed-radius range query + fused PPM
 * update (gathering.cu:17-126) over photon buckets (k_gather_grid per lane,
 * k_gather_tile per 8x8 tile) or the reference kd-tree layout (k_gather_kd),
 * the radius histogram reduce of the adaptive grid, and launch_gather.
 * The kNN gathers are in pm_gather_knn.hip, the record kernels (PPM update of
 * reduced partials, final radiance, tile list, reset) in pm_records.hip, and
 * what they share in pm_gather_dev.h.
 *
 * wave64; 8x8 pixel tiles map onto one wave so a wave's gather points are
 * spatially coherent and share photon buckets in L1/L2.
 */
#include <hip/hip_runtime.h>

#include "pm_gather_dev.h"
#include "pm_kernels.h"

#pragma clang fp contract(off)

namespace pm {
/* Exact, order-independent flux sums for the bucket gather: each photon's
 * contribution is rounded once to a 64-bit fixed-point integer (scale 2^S
 * chosen per scene so that 2^23 maximal contributions fit, pm_api_gather.cpp
 * fx_scale) and integers add associatively. The bucket order (atomic
 * arrival order in pm_bucket.hip) and the number of GPUs that hold the
 * photons therefore never change a bit of the result. */
struct Fx3 { long long x, y, z; };
/* where record r's partial goes: its rank in the record view (active records
 * only, -1 = not in the view) or r itself (all-records view) */
PMD int64_t partial_index(const GatherParams &P, int64_t r) {
    if (!P.view_rank) return r;
    const uint32_t k = P.view_rank[r];
    return k == 0xffffffffu ? -1 : (int64_t)k;
}
PMD long long to_fx(float c, float scale) { return (long long)rintf(c * scale); }
/* partial of view record k: (M, L) as four int64, or split into an int32
 * count and three int64 flux words (the "reduce" exchange's layout) */
PMD void write_partial(const GatherParams &P, int64_t k, int M, Fx3 L) {
    if (k < 0) return;
    if (P.count) {
        P.count[k] = M;
        long long *f = P.flux + 3 * k;
        f[0] = L.x; f[1] = L.y; f[2] = L.z;
        return;
    }
    longlong2 *q = reinterpret_cast<longlong2 *>(P.partial + 4 * k);
    q[0] = make_longlong2((long long)M, L.x);
    q[1] = make_longlong2(L.y, L.z);
}

/* Fixed-radius query over photon buckets. Every photon with
 * d^2 < r^2 is inside the visited cells because the cell range is taken
 * over [p - r', p + r'] with r' slightly larger than sqrt(r^2). */
PMD void add_hit(Fx3 &Lf, v3 ns, v3 fv, float4 a, float4 b, float wz, float sc) {
    const v3 wi = mk(a.w, b.w, wz);
    const v3 c = fabsf(dot(ns, wi)) * fv * xyz(b); /* processPhoton, gathering.cu:17-23 */
    Lf.x += to_fx(c.x, sc); Lf.y += to_fx(c.y, sc); Lf.z += to_fx(c.z, sc);
}
PMD bool in_radius(v3 p, float4 a, float r2) { /* gathering.cu:32-36 (DistanceSquared < maxDist2) */
    const v3 diff = p - xyz(a);
    return diff.x * diff.x + diff.y * diff.y + diff.z * diff.z < r2;
}

#ifndef PM_SCAN_BATCH
#define PM_SCAN_BATCH 4 /* 6: 116 VGPRs, 8: 142 — the tile kernel drops to 4 / 3 waves per SIMD */
#endif
/* One lane scans its own cells [x0, x1] x [y0, y1] x [z0, z1] straight from
 * global memory: the census launches (their photons-tested count is the
 * per-record unit bench.py prices), lanes whose radius exceeds the grid's
 * design radius (uploaded records), and tiles whose row union is too wide for
 * k_gather_tile's LDS staging. All eight row bounds are loaded first; rows
 * are read in software-pipelined batches (PIPE, the tile kernel's lanes: C3
 * gather 0.51 -> 0.45 ms, C5 0.28 -> 0.25 ms, same box) or four photons at a
 * time (the census / per-lane kernel, whose 64-VGPR budget the pipeline
 * would spill). */
/* the lane's rows, each one contiguous run [b, e) of photons, passed to RANGE(b, e) */
#define PM_LANE_SCAN_CELLS(RANGE) \
    if (y1 <= y0 + 1 && z1 <= z0 + 1) {                                                     \
        /* all row bounds first: 8 independent loads in flight */                           \
        uint32_t rb[4], re[4];                                                              \
_Pragma("unroll")                                                                           \
        for (int k = 0; k < 4; ++k) {                                                       \
            const uint32_t cy = y0 + (k & 1), cz = z0 + (k >> 1);                           \
            const bool use = cy <= y1 && cz <= z1;                                          \
            const uint32_t row = (cz * (uint32_t)g.dy + cy) * (uint32_t)g.dx;               \
            rb[k] = use ? P.cell_start[row + x0] : 0u;                                      \
            re[k] = use ? P.cell_start[row + x1 + 1] : 0u;                                  \
            if (COUNT) { vis += re[k] - rb[k]; rows += use; }                               \
        }                                                                                   \
_Pragma("unroll")                                                                           \
        for (int k = 0; k < 4; ++k) RANGE(rb[k], re[k]);                                    \
    } else { /* radius above the grid's design radius (uploaded records) */                 \
        for (uint32_t cz = z0; cz <= z1; ++cz)                                              \
            for (uint32_t cy = y0; cy <= y1; ++cy) {                                        \
                const uint32_t row = (cz * (uint32_t)g.dy + cy) * (uint32_t)g.dx;           \
                const uint32_t b = P.cell_start[row + x0], e = P.cell_start[row + x1 + 1];  \
                if (COUNT) { vis += e - b; rows++; }                                        \
                RANGE(b, e);                                                                \
            }                                                                               \
    }                                                                                       \
    do { } while (0)
template <int COUNT, int PIPE>
PMD void lane_scan(const GatherParams &P, v3 p, float r2, v3 ns, v3 fv, uint32_t x0, uint32_t x1, uint32_t y0,
                   uint32_t y1, uint32_t z0, uint32_t z1, int &M, Fx3 &Lf, unsigned long long &vis,
                   unsigned long long &rows) {
    const GridDesc &g = P.grid;
    const float sc = P.fx_scale;
    const float *phb = reinterpret_cast<const float *>(P.ph_b);
    auto photon = [&](const float4 a, uint32_t j) {
        if (in_radius(p, a, r2)) {
            M++;
            add_hit(Lf, ns, fv, a, P.ph_b[2 * (size_t)j], phb[8 * (size_t)j + 4], sc);
        }
    };
    if constexpr (PIPE != 0) {
        (void)photon;
        constexpr int SB = PM_SCAN_BATCH;
        /* batches of PM_SCAN_BATCH photons, software-pipelined: the next batch's positions
         * are requested before this batch is tested, and the flux words of all
         * of a batch's hits are requested together before any is summed — one
         * memory round trip per batch instead of one for the positions plus one
         * per hit (dense cells: C5's caustic, the soup's incoherent lanes) */
        auto range = [&](uint32_t j, const uint32_t e) {
            if (j >= e) return;
            float4 a[SB];
#pragma unroll
            for (int i = 0; i < SB; ++i) a[i] = P.ph_a[min(j + (uint32_t)i, e - 1u)]; /* past e: masked below */
            for (; j < e; j += SB) {
                float4 cur[SB];
#pragma unroll
                for (int i = 0; i < SB; ++i) cur[i] = a[i];
                if (j + (uint32_t)SB < e) {
#pragma unroll
                    for (int i = 0; i < SB; ++i) a[i] = P.ph_a[min(j + (uint32_t)SB + (uint32_t)i, e - 1u)];
                }
                uint32_t m = 0u;
#pragma unroll
                for (int i = 0; i < SB; ++i) m |= (j + (uint32_t)i < e && in_radius(p, cur[i], r2)) ? 1u << i : 0u;
                float4 hb[SB];
                float hc[SB];
#pragma unroll
                for (int i = 0; i < SB; ++i) {
                    hb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                    hc[i] = 0.f;
                    if (m & (1u << i)) { hb[i] = P.ph_b[2 * (size_t)(j + i)]; hc[i] = phb[8 * (size_t)(j + i) + 4]; }
                }
#pragma unroll
                for (int i = 0; i < SB; ++i)
                    if (m & (1u << i)) { M++; add_hit(Lf, ns, fv, cur[i], hb[i], hc[i], sc); }
            }
        };
        PM_LANE_SCAN_CELLS(range);
    } else {
        auto range = [&](uint32_t j, const uint32_t e) {
            for (; j + 4 <= e; j += 4) { /* 4 photon loads in flight */
                const float4 a0 = P.ph_a[j], a1 = P.ph_a[j + 1], a2 = P.ph_a[j + 2], a3 = P.ph_a[j + 3];
                photon(a0, j); photon(a1, j + 1); photon(a2, j + 2); photon(a3, j + 3);
            }
            for (; j < e; ++j) photon(P.ph_a[j], j);
        };
        PM_LANE_SCAN_CELLS(range);
    }
}

/* r' of a record's cell box [p - r', p + r']: hardware sqrt (<= 1 ulp), the
 * 1e-4 relative margin covers it */
PMD float box_reach(float r2) { return __builtin_amdgcn_sqrtf(r2) * 1.0001f + 1e-4f; }

/* k_gather_tile requests a record's normal with its position (EARLY) and its
 * material as one 16-B load: C2 gather 43.7 -> 42.8 us against the normal
 * after the position and m.w before m.xyz (profiles/r05/tile_order). */
/* record prologue shared by the bucket kernels: flags, PPM state, BSDF, cell
 * box of [p - r', p + r'] (small: at most 2 x 2 rows, the grid's design case) */
struct GatherRec {
    bool live = false, small = false, big = false;
    float4 st = make_float4(0.f, 0.f, 0.f, 0.f);
    v3 p = mk(0.f, 0.f, 0.f), ns = mk(0.f, 0.f, 0.f), fv = mk(0.f, 0.f, 0.f);
    float r2 = 0.f;
    uint32_t x0 = 0, x1 = 0, y0 = 0, y1 = 0, z0 = 0, z1 = 0;
    float4 nrm = make_float4(0.f, 0.f, 0.f, 0.f);
    /* phase 1: position, PPM state and cell box. The state is read with the
     * position (speculatively, also for inactive records) so that the cell
     * box waits for one round trip only; the normal is requested here and
     * consumed by shade() */
    template <int PARTIAL, bool EARLY = false>
    PMD void load(const GatherParams &P, int64_t r) {
        if (r >= P.rec_end) return;
        const float4 pos = P.R.pos[r];
        const float4 st0 = P.fresh ? make_float4(0.f, 0.f, 0.f, P.r2init) : P.R.state[r];
        if (EARLY) { /* the normal requested with the position (one round trip fewer) */
            const float4 n0 = P.R.nrm[r];
            if (accept<PARTIAL>(P, r, pos, st0)) nrm = n0;
        } else if (accept<PARTIAL>(P, r, pos, st0)) {
            nrm = P.R.nrm[r];
        }
    }
    /* the flags, PPM state and cell box of record r < rec_end from its loaded
     * position and state; false: inactive (its partial written) */
    template <int PARTIAL>
    PMD bool accept(const GatherParams &P, int64_t r, float4 pos, float4 st0) {
        const uint32_t flags = (uint32_t)__float_as_int(pos.w);
        if (flags & (PM_REC_MISS | PM_REC_EXCEPTION | PM_REC_INVALID)) {
            if (PARTIAL) write_partial(P, partial_index(P, r), 0, Fx3{0, 0, 0});
            return false;
        }
        live = true;
        st = st0;
        r2 = st.w;
        p = xyz(pos);
        if (r2 > 0.f) {
            const GridDesc &g = P.grid;
            const float rq = box_reach(r2);
            /* cells overlapping [p - r', p + r']: cell edge >= 2 r_max, so at
             * most 2 per axis -> at most 4 (y, z) rows of <= 2 cells in x */
            x0 = cell_axis(p.x - rq, g.gx, g.inv_cs, g.dx); x1 = cell_axis(p.x + rq, g.gx, g.inv_cs, g.dx);
            y0 = cell_axis(p.y - rq, g.gy, g.inv_cs, g.dy); y1 = cell_axis(p.y + rq, g.gy, g.inv_cs, g.dy);
            z0 = cell_axis(p.z - rq, g.gz, g.inv_cs, g.dz); z1 = cell_axis(p.z + rq, g.gz, g.inv_cs, g.dz);
            small = y1 <= y0 + 1 && z1 <= z0 + 1;
            big = !small;
        }
        return true;
    }
    /* phase 2: shading normal and BSDF (Kd / pi for matte, processPhoton) */
    PMD void shade(const GatherParams &P) {
        if (!live) return;
        float4 m = P.materials[__float_as_int(nrm.w)];
        asm volatile("" : "+v"(m.x), "+v"(m.y), "+v"(m.z), "+v"(m.w)); /* one 16-B load, not m.w then m.xyz */
        fv = __float_as_int(m.w) == PM_MATTE ? xyz(m) * INV_PI : mk(0.f, 0.f, 0.f);
        ns = xyz(nrm);
    }
    /* fused PPM update (gathering.cu:104-126) from the fixed-point sums as
     * doubles (exact integers) */
    PMD void store_sum(const GatherParams &P, int64_t r, int M, double sx, double sy, double sz) {
        if (!live) return;
        const double inv = P.fx_inv;
        v3 L = mk((float)(sx * inv), (float)(sy * inv), (float)(sz * inv));
        float N = P.fresh ? 0.f : P.R.n[r];
        ppm_apply(st, N, M, L, P.ppm_alpha);
        if (M > 0 || P.fresh) { P.R.state[r] = st; P.R.n[r] = N; }
    }
    /* fused PPM update or the partial of the exchange */
    template <int PARTIAL>
    PMD void store(const GatherParams &P, int64_t r, int M, Fx3 Lf) {
        if (!live) return;
        if (PARTIAL) write_partial(P, partial_index(P, r), M, Lf);
        else store_sum(P, r, M, (double)Lf.x, (double)Lf.y, (double)Lf.z);
    }
};

/* Per-lane bucket gather: one lane per record, its own rows from global
 * memory. Census launches (COUNT) and the PM_GATHER_KERNEL=lane experiment. */
template <int PARTIAL, int COUNT>
__global__ __launch_bounds__(GATHER_BLOCK, 8) void k_gather_grid(GatherParams P) { /* 8 waves/SIMD: latency bound */
    const int64_t r = P.rec_begin + (int64_t)blockIdx.x * GATHER_BLOCK + threadIdx.x;
    unsigned long long vis = 0, hits = 0, rows = 0, act = 0;
    GatherRec R;
    R.load<PARTIAL>(P, r);
    R.shade(P);
    int M = 0;
    Fx3 Lf{0, 0, 0};
    if (R.live && R.r2 > 0.f)
        lane_scan<COUNT, 0>(P, R.p, R.r2, R.ns, R.fv, R.x0, R.x1, R.y0, R.y1, R.z0, R.z1, M, Lf, vis, rows);
    if (COUNT && R.live) { hits += (unsigned long long)M; act++; }
    R.store<PARTIAL>(P, r, M, Lf);
    if (COUNT) count4(P.counters, vis, hits, rows, act);
}

/* ---------------------------------------------------------------------- */
/* Tile gather (default): the 64 records of a wave are one 8x8 pixel tile, so
 * their cell boxes overlap almost entirely. The wave takes the union box of
 * its lanes' boxes (X0..X1 x Y0..Y1 x Z0..Z1 cells), and when it has at most
 * 64 (y, z) rows:
 *   1. lane u loads the bounds of union row u (cells X0..X1: one contiguous
 *      run of photons), a wave prefix sum concatenates the rows -> U photons;
 *   2. the concatenation is staged into this wave's LDS window, TILE_CAP
 *      photons at a time, with coalesced loads (positions lane and lane + 64:
 *      1 KiB per load instruction): ph_a (p, wi.x) and the flux half of ph_b
 *      (alpha, wi.y | wi.z); the row of each position comes from a wave
 *      max-scan over the row-start markers;
 *   3. every lane tests the whole union-x run of each of its <= 4 rows from
 *      LDS (lanes sharing a row read the same address: broadcast), its rows
 *      walked as one flattened sequence, two photons per step.
 * A lane tests a superset of its own cells (the union's x-range); every
 * photon with d^2 < r^2 still lies in exactly one visited run, and the sums
 * are exact fixed point, so M and L are bit-identical to k_gather_grid's.
 * Global memory sees one record read, one row-bounds load per union row and
 * ~3 coalesced loads per 64 photons per tile, instead of ~2 scattered loads
 * per photon per lane. Lanes with an oversized radius and
 * tiles with more than 64 union rows fall back to lane_scan. */
#ifndef PM_TILE_CAP
#define PM_TILE_CAP 128
#endif
constexpr int TILE_CAP = PM_TILE_CAP; /* photons per LDS window (two per lane) */
/* Positions are stored by aligned pairs, 32 B per pair (x0 x1 y0 y1 | z0 z1
 * . .), so a pair test reads one ds_read_b128 and one ds_read_b64 at
 * immediate offsets (no per-pair address arithmetic) straight into the
 * register pairs of the packed math; runs start at even positions (an odd
 * start masks its first bit). Against SoA x / y / z read with ds_read2: C2
 * gather 50.1-50.3 -> 49.3 us, C3 0.561 -> 0.529 ms (docs/HISTORY.md, "Paired
 * positions and sign-bit masks"; counters in profiles/r04). */
struct TileLds {
    /* TILE_CAP pairs: a run's aligned pairs reach at most one pair past
     * them (lanes beyond their run, masked): that read lands in b[] below,
     * inside the block's LDS. No padding pairs: 7,680 B per wave (the LDS
     * allocation granule makes 7,744 B fit 18 one-wave blocks per CU, 7,680
     * B 20, the VGPR limit): C2 gather 47.4-48.6 -> 44.4-46.3 us (same box) */
    float4 pr[2 * TILE_CAP];
    float4 b[TILE_CAP]; /* alpha.rgb, wi.y */
    float w[TILE_CAP];  /* wi.x */
    float c[TILE_CAP];  /* wi.z */
    int mark[TILE_CAP]; /* union row starting at this position, -1 = none */
};
/* one-wave blocks are dealt round-robin over the 8 XCDs: blocks b, b + 8, ...
 * (one XCD, dispatched close together) take PM_TILE_XCDG neighbouring entries
 * of the tile list, so neighbouring tiles share their photon rows in one L2
 * (C2 gather FETCH 141 -> 96 MB per launch at 8, 118 at 4, 82 at 16; time
 * within noise of each other, ~2 % below no grouping). A bijection on whole
 * groups of 8 x XCDG entries; the tail keeps its order. (The kNN tile kernel
 * measured 1.5 % slower with it: its passes re-stage unions a tile's own
 * wave re-reads, not its neighbours'.) */
#ifndef PM_TILE_XCDG
#define PM_TILE_XCDG 8
#endif
PMD int64_t xcd_tile(int64_t w, int64_t nt) {
#if PM_TILE_XCDG > 1
    constexpr int64_t GX = 8 * PM_TILE_XCDG;
    if (w < nt / GX * GX) w = w / GX * GX + (w % 8) * PM_TILE_XCDG + (w / 8) % PM_TILE_XCDG;
#endif
    return w;
}

/* integer-valued double in [0, 2^53) -> int64, exactly (two 32-bit halves) */
PMD long long d2ll(double d) {
    const uint32_t hi = (uint32_t)(d * 0x1p-32);
    const uint32_t lo = (uint32_t)fma((double)hi, -0x1p32, d);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

/* the default instance (span 2, non-negative sums) at 5 waves/SIMD, the
 * LDS limit (TileLds): unbounded, the compiler takes more than 102 VGPRs
 * since the cooperative direct scan (4 waves); bounded, none spill. The
 * other instances keep the compiler's choice (bounded they spill) */
#ifndef PM_TILE_WAVES
#define PM_TILE_WAVES 5
#endif
template <int NN, int KR>
constexpr int tile_waves() { return NN && KR == 2 ? PM_TILE_WAVES : 1; }
#define TILE_OCC __attribute__((amdgpu_waves_per_eu(tile_waves<NN, KR>(), 8)))
/* the union cell box (union_box6) of the records with `in` set */
PMD void union_box(const GridDesc &g, const GatherRec &R, bool in, uint32_t &X0, uint32_t &X1, uint32_t &Y0,
                   uint32_t &Y1, uint32_t &Z0, uint32_t &Z1) {
    union_box6(g, in, R.x0, R.x1, R.y0, R.y1, R.z0, R.z1, X0, X1, Y0, Y1, Z0, Z1);
}
#ifndef PM_GROUP_R
#define PM_GROUP_R 3
#endif
/* a group takes the lanes whose box starts within GROUP_R cells of the
 * leader's: y rows [ly - R, ly + R + 1] fit the row pitch 8, z layers x 8
 * rows fit the 64 lanes */
constexpr uint32_t GROUP_R = PM_GROUP_R;
/* C2 gather: 12 -> 51.9 us, 8 -> 51.3, 4 -> 48.5, 2 -> 48.8, 1 -> 48.9 (C3
 * unchanged): a small LDS group still beats its lanes scanning per lane.
 * Sparse maps are the exception: with under 1/SPARSE_CELLS photons per
 * cell (C1: 52K photons in 2.7M cells) a lane's own cells hold almost
 * nothing and a small group's staging overhead is the larger cost — C1 14.9
 * us with 12, 34.9 us with 4 — so they keep groups of >= 12 lanes. The
 * density is read on the device (cell_start[ncells] = photons in the map). */
#ifndef PM_GROUP_MIN
#define PM_GROUP_MIN 4
#endif
#ifndef PM_GROUP_MIN_SPARSE
#define PM_GROUP_MIN_SPARSE 12
#endif
constexpr int GROUP_MIN = PM_GROUP_MIN, GROUP_MIN_SPARSE = PM_GROUP_MIN_SPARSE;
constexpr uint32_t SPARSE_CELLS = 20;
#ifndef PM_TILE_UMAX
#define PM_TILE_UMAX 512
#endif
constexpr int TILE_UMAX = PM_TILE_UMAX; /* C5 (r02 grid): no cap 2.88 ms, 2048 0.44, 1024 0.41, 512 0.43; adaptive grid (r03): 2048 0.268, 1024 0.24, 512 0.205; C2 unchanged */
/* Dense maps (>= 2 photons per 5 cells: C5's caustic scene, 0.73; C2 0.20)
 * fall back to the per-lane scans from smaller unions on: C5 tile gather
 * 0.153-0.159 ms at 512, 0.145-0.148 at 256, 0.150-0.152 at 192, 0.158-0.161
 * at 128; C2 0.5 % slower at 256, C4 unchanged (round 6, same box,
 * profiles/r06/tile_umax). The density is read on the device, as for
 * GROUP_MIN_SPARSE. */
#ifndef PM_TILE_UMAX_DENSE
#define PM_TILE_UMAX_DENSE 256
#endif
constexpr int TILE_UMAX_DENSE = PM_TILE_UMAX_DENSE;
static_assert(2 * GROUP_R + 2 <= 8, "group rows exceed the 64-lane row map");
/* the updated radii of a wave into the adaptive-grid histogram
 * (GatherParams::r2hist): one atomic per distinct bin of the wave (a tile's
 * radii are alike), in one of R2_COPIES copies by block */
PMD void r2_histogram(const GatherParams &P, bool live, float r2) {
    int b = -1;
    if (live) {
        const float t = r2 * P.r2hist_inv;
        b = t >= 1.f ? 0 : !(t > 0.f) ? R2_BINS - 1 : min(R2_BINS - 1, (int)(-__log2f(t) * (float)R2_PER_OCTAVE));
    }
    unsigned long long pend = __ballot(b >= 0);
    uint32_t *h = P.r2hist + (blockIdx.x % (unsigned)R2_COPIES) * R2_BINS;
    while (pend) {
        const int l = __builtin_ctzll(pend);
        const int bb = __builtin_amdgcn_readlane(b, l);
        const unsigned long long same = __ballot(b == bb);
        if ((threadIdx.x & 63) == (unsigned)l) atomicAdd(&h[bb], (uint32_t)__builtin_popcountll(same));
        pend &= ~same;
    }
}
__global__ __launch_bounds__(R2_BINS) void k_r2hist_reduce(uint32_t *hist, uint32_t *out) {
    const int b = threadIdx.x;
    uint32_t t = 0u;
    for (int k = 0; k < R2_COPIES; ++k) {
        t += hist[k * R2_BINS + b];
        hist[k * R2_BINS + b] = 0u; /* ready for the next histogram */
    }
    out[b] = t;
}
hipError_t launch_r2hist_reduce(uint32_t *hist, uint32_t *out_mapped, hipStream_t s) {
    pm_launch(k_r2hist_reduce, dim3(1), dim3(R2_BINS), 0, s, hist, out_mapped);
    return hipGetLastError();
}
/* KR: cells per axis a lane's box [p - r', p + r'] spans at most, for the
 * grid's design radius (GatherParams::span: cell edge 2 r' / (KR - 1), the
 * cell-edge sweep of DESIGN.md §5). A lane reads KR z-layers, each one
 * contiguous run of <= KR rows of the union; its group radius keeps the union
 * inside the 64-lane row map (2 GR + KR <= 8 rows per axis). */
template <int KR>
constexpr uint32_t tile_group_r() { return KR == 2 ? GROUP_R : (8u - (uint32_t)KR) / 2u; }
struct TileLds;
/* The lanes of `sel` (small boxes: at most KR x KR rows each) all at once:
 * their rows are concatenated (row slot = lane, its owner from a max-scan
 * over the owners' first slots), the rows' photons concatenated again and
 * tested 64 per step, each against its owner's query (shuffled from the
 * owner); hits are added with add_hit — lane_scan's terms — into the
 * owner's int64 sums in LDS (exact, order-free), so M and L equal
 * lane_scan's bit for bit. A step costs the whole wave whatever the number
 * of owners: the cost is ~ the lanes' photons / 64. Every lane active. */
PMD void coop_batch(const GatherParams &P, TileLds &T, int lane, const GatherRec &R, bool &sel, int &M, Fx3 &Lf) {
    const GridDesc &g = P.grid;
    const float sc = P.fx_scale;
    const float *phb = reinterpret_cast<const float *>(P.ph_b);
    /* per-owner sums (M, L.x, L.y, L.z) in the idle staging array: 64 x 32 B */
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(T.b);
    static_assert(sizeof(T.b) >= 64 * 32, "owner sums fit the flux staging array");
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[4 * lane + q] = 0ull;
    const uint32_t ny = sel ? R.y1 - R.y0 + 1u : 0u, nr = sel ? ny * (R.z1 - R.z0 + 1u) : 0u;
    const uint32_t rin = wave_incl_sum_u32(nr), rpre = rin - nr;
    const uint32_t RT = uniform_u32(__builtin_amdgcn_readlane(rin, 63));
    for (uint32_t c0 = 0; c0 < RT; c0 += 64u) {
        /* row slot c0 + lane: its owner, the lane whose slots [rpre, rin) hold it */
        T.mark[lane] = -1;
        wave_lds_sync();
        if (nr > 0u) {
            if (rpre >= c0 && rpre < c0 + 64u) T.mark[rpre - c0] = lane;
            else if (rpre < c0 && rin > c0) T.mark[0] = lane;
        }
        wave_lds_sync();
        const int o = wave_incl_max_i32(T.mark[lane]);
        wave_lds_sync();
        const int os = max(o, 0);
        const uint32_t j = c0 + (uint32_t)lane;
        const uint32_t ox0 = (uint32_t)__shfl((int)R.x0, os), ox1 = (uint32_t)__shfl((int)R.x1, os);
        const uint32_t oy0 = (uint32_t)__shfl((int)R.y0, os), oz0 = (uint32_t)__shfl((int)R.z0, os);
        const uint32_t ony = (uint32_t)__shfl((int)ny, os), orp = (uint32_t)__shfl((int)rpre, os);
        uint32_t B = 0u, len = 0u;
        if (j < RT && o >= 0) {
            const uint32_t k = j - orp;
            const uint32_t cy = oy0 + k % ony, cz = oz0 + k / ony;
            const uint32_t row = (cz * (uint32_t)g.dy + cy) * (uint32_t)g.dx;
            B = P.cell_start[row + ox0];
            len = P.cell_start[row + ox1 + 1u] - B;
        }
        const uint32_t incl = wave_incl_sum_u32(len), pre = incl - len;
        const uint32_t U = uniform_u32(__builtin_amdgcn_readlane(incl, 63));
        const uint32_t gofs = B - pre;
        for (uint32_t t0 = 0; t0 < U; t0 += 64u) {
            T.mark[lane] = -1;
            wave_lds_sync();
            if (len > 0u) {
                if (pre >= t0 && pre < t0 + 64u) T.mark[pre - t0] = lane;
                else if (pre < t0 && pre + len > t0) T.mark[0] = lane;
            }
            wave_lds_sync();
            const int u = max(wave_incl_max_i32(T.mark[lane]), 0);
            wave_lds_sync();
            const uint32_t t = t0 + (uint32_t)lane;
            const uint32_t gi = t + (uint32_t)__shfl((int)gofs, u);
            const int ow = __shfl(os, u);
            const v3 p = mk(__shfl(R.p.x, ow), __shfl(R.p.y, ow), __shfl(R.p.z, ow));
            const float r2 = __shfl(R.r2, ow);
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            bool h = false;
            if (t < U) {
                a = P.ph_a[gi];
                h = in_radius(p, a, r2);
            }
            if (__ballot(h)) {
                const v3 ns = mk(__shfl(R.ns.x, ow), __shfl(R.ns.y, ow), __shfl(R.ns.z, ow));
                const v3 fv = mk(__shfl(R.fv.x, ow), __shfl(R.fv.y, ow), __shfl(R.fv.z, ow));
                if (h) {
                    Fx3 c{0, 0, 0};
                    add_hit(c, ns, fv, a, P.ph_b[2 * (size_t)gi], phb[8 * (size_t)gi + 4], sc);
                    atomicAdd(&acc[4 * ow], 1ull);
                    atomicAdd(&acc[4 * ow + 1], (unsigned long long)c.x);
                    atomicAdd(&acc[4 * ow + 2], (unsigned long long)c.y);
                    atomicAdd(&acc[4 * ow + 3], (unsigned long long)c.z);
                }
            }
        }
    }
    wave_lds_sync();
    if (sel) {
        M = (int)acc[4 * lane];
        Lf = Fx3{(long long)acc[4 * lane + 1], (long long)acc[4 * lane + 2], (long long)acc[4 * lane + 3]};
        sel = false;
    }
    wave_lds_sync(); /* the sums are read before anything else writes the array */
}

/* COST: record each wave's lifetime into P.tile_cost (the launch that
 * measures the tile list for k_tile_sort); a separate instance, since the
 * clock kept live across the kernel cost the timed instance 12 B of scratch */
template <int PARTIAL, int NN, int KR, bool COST>
__global__ __launch_bounds__(TILE_BLOCK) TILE_OCC void k_gather_tile(GatherParams P) {
    static_assert(KR >= 2 && KR <= 5 && 2 * tile_group_r<KR>() + KR <= 8, "lane box / group radius");
    constexpr uint32_t GR = tile_group_r<KR>();
    __shared__ TileLds tiles[TILE_BLOCK / 64];
    TileLds &T = tiles[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    int64_t r, w = 0;
    const unsigned long long tc0 = COST ? __builtin_amdgcn_s_memrealtime() : 0ull;
    if (P.tiles) { /* only tiles with an active record (no block-level barrier below: a wave may leave) */
        w = (int64_t)blockIdx.x * (TILE_BLOCK / 64) + (threadIdx.x >> 6);
        const int64_t nt = P.n_tiles_dev ? (int64_t)*P.n_tiles_dev : P.n_tiles;
        if (w >= nt) return;
        if (TILE_BLOCK == 64) w = xcd_tile(w, nt);
        /* wave-uniform entry through the scalar cache: a vector load of it cost an L2 round trip (profiles/r05/tile_order) */
        w = (int64_t)__builtin_amdgcn_readfirstlane((int)w);
        r = P.rec_begin + (int64_t)((const_u32_ptr)P.tiles)[w] * 64 + lane;
    } else {
        r = P.rec_begin + (int64_t)blockIdx.x * TILE_BLOCK + threadIdx.x;
    }
    const GridDesc &g = P.grid;
#ifdef PM_TILE_TIMES
    const unsigned long long tt0 = __builtin_amdgcn_s_memrealtime();
    uint32_t tstat[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
    GProf gp;
    gp.begin();
    GatherRec R;
    R.load<PARTIAL, true>(P, r);
    /* a box of <= KR cells per axis takes part in the LDS groups; larger
     * (radius above the grid's design radius) scans its own cells */
    const bool small = R.live && R.r2 > 0.f && R.y1 - R.y0 < (uint32_t)KR && R.z1 - R.z0 < (uint32_t)KR;
    int M = 0;
    Fx3 Lf{0, 0, 0};
    const float sc = P.fx_scale;
    unsigned long long nv = 0, nr = 0; /* lane_scan census (unused) */
    /* NN (no negative contribution possible, GatherParams::fx_nonneg): the
     * integer-valued contributions rint(c * 2^S) are summed in double — exact
     * while the sum stays below 2^53 (checked at the end; partial sums of
     * non-negative terms never exceed it), and 4 instructions per channel
     * instead of a float -> int64 conversion and a 64-bit add */
    double dx = 0.0, dy = 0.0, dz = 0.0;
    R.shade(P);
    const v3 fvs = R.fv * sc;
    const f2 px2 = {R.p.x, R.p.x}, py2 = {R.p.y, R.p.y}, pz2 = {R.p.z, R.p.z};
    const f2 r2v = {R.r2, R.r2};
    /* Groups: the first pending lane leads; every pending lane whose box
     * starts within GR cells of the leader's on each axis joins. A group's
     * union box is at most (2 GR + KR)^3 cells (<= 8 x 8 rows), so it always
     * fits the 64-lane row map; a coherent tile is one group, a tile across a
     * depth edge two or three, never one huge box. */
    bool pend = small;
    bool direct = R.live && R.r2 > 0.f && !small; /* lanes that scan their own cells from global memory */
    const uint64_t n_map = P.cell_start[g.ncells];
    const int group_min = n_map * SPARSE_CELLS < (uint64_t)g.ncells ? GROUP_MIN_SPARSE : GROUP_MIN;
    const uint32_t umax = n_map * 5u >= (uint64_t)g.ncells * 2u ? (uint32_t)TILE_UMAX_DENSE : (uint32_t)TILE_UMAX;
    gp.mark(0);
    while (true) {
        const unsigned long long pm = __ballot(pend);
        if (pm == 0ull) break;
        /* the box of all pending lanes when it fits the row map (the common,
         * coherent tile: one group), else the leader's neighbourhood */
        uint32_t X0, X1, Y0, Y1, Z0, Z1, LY;
        bool mine = pend;
        /* 1. union row u = lane: photons [B, B + len); u = (cz - Z0) * 2^LY +
         * (cy - Y0) (no lane divides; padding rows are empty) */
        uint32_t B = 0u, len = 0u;
        union_box(g, R, mine, X0, X1, Y0, Y1, Z0, Z1);
        /* row pitch: NY rounded up to a power of two, 2^LY */
        LY = Y1 > Y0 ? 32u - (uint32_t)__builtin_clz(Y1 - Y0) : 0u;
        if (LY > 6u || ((uint64_t)(Z1 - Z0 + 1u) << LY) > 64u) {
            const int leader = __builtin_ctzll(pm);
            const uint32_t lx = __builtin_amdgcn_readlane(R.x0, leader), ly = __builtin_amdgcn_readlane(R.y0, leader),
                           lz = __builtin_amdgcn_readlane(R.z0, leader);
            mine = pend && R.x0 + GR - lx <= 2u * GR && R.y0 + GR - ly <= 2u * GR && R.z0 + GR - lz <= 2u * GR;
            /* an incoherent tile (lanes on many far-apart surfaces, e.g. a
             * triangle soup) would need a group per few lanes: below
             * GROUP_MIN lanes the rest scan their own cells per lane */
            if (__builtin_popcountll(__ballot(mine)) < group_min) {
                direct = direct || pend;
                break;
            }
            union_box(g, R, mine, X0, X1, Y0, Y1, Z0, Z1);
            LY = 3u;
        }
        const uint32_t cy = Y0 + ((uint32_t)lane & ((1u << LY) - 1u)), cz = Z0 + ((uint32_t)lane >> LY);
        if (cy <= Y1 && cz <= Z1) {
            const uint32_t row = (cz * (uint32_t)g.dy + cy) * (uint32_t)g.dx;
            B = P.cell_start[row + X0];
            len = P.cell_start[row + X1 + 1u] - B;
        }
        pend = pend && !mine;
        TILE_STAT(0, 1);
        const uint32_t incl = wave_incl_sum_u32(len), pre = incl - len;
        const uint32_t U = uniform_u32(__builtin_amdgcn_readlane(incl, 63));
        if (U == 0u) continue;
        /* a dense union (many photons per cell, e.g. C5's caustic scene: 4x
         * C2's density) costs more to stage than its lanes read on their own:
         * above TILE_UMAX photons the group's lanes scan their own cells */
        if (U > umax) { direct = direct || mine; continue; }
        const uint32_t gofs = B - pre; /* photon index of concatenated position t in row u: t + gofs_u */
        /* this lane's rows as KR runs of the concatenation: rows (y0 .. y1, z)
         * are neighbours in the union, so each z-layer of the lane's box is
         * one contiguous run [s_k, e_k) */
        const uint32_t ny = mine ? R.y1 - R.y0 + 1u : 1u;
        const uint32_t nz = mine ? R.z1 - R.z0 + 1u : 0u;
        uint32_t sK[KR], eK[KR];
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            /* every lane shuffles: a bpermute from a lane that is inactive at
             * the shuffle reads 0 */
            const int u = mine && (uint32_t)k < nz ? (int)(((R.z0 + (uint32_t)k - Z0) << LY) + (R.y0 - Y0)) : 0;
            const uint32_t s0 = (uint32_t)__shfl((int)pre, u), e0 = (uint32_t)__shfl((int)incl, u + (int)ny - 1);
            sK[k] = (uint32_t)k < nz ? s0 : 0u;
            eK[k] = (uint32_t)k < nz ? e0 : 0u;
        }
        gp.mark(1);
        for (uint32_t T0 = 0; T0 < U; T0 += TILE_CAP) {
            const uint32_t n = min((uint32_t)TILE_CAP, U - T0);
            TILE_STAT(1, 1);
            TILE_STAT(7, n);
            /* 2. stage positions T0 + lane (and T0 + 64 + lane) */
            constexpr int H = TILE_CAP / 64;
            static_assert(H == 1 || H == 2, "TILE_CAP is 64 or 128");
#pragma unroll
            for (int h = 0; h < H; ++h) T.mark[lane + 64 * h] = -1;
            wave_lds_sync();
            if (len > 0u) {
                if (pre >= T0 && pre < T0 + TILE_CAP) T.mark[pre - T0] = lane;
                else if (pre < T0 && pre + len > T0) T.mark[0] = lane; /* row running into the window */
            }
            wave_lds_sync();
            const float *phb = reinterpret_cast<const float *>(P.ph_b);
            static_assert(H == 2, "paired staging: two positions per lane");
            {
                /* lane l stages positions 2 l and 2 l + 1, a whole pair: one
                 * 16-B and one 8-B LDS write instead of three scattered words
                 * per position (bank conflicts) */
                const int2 m2 = *reinterpret_cast<const int2 *>(&T.mark[2 * lane]);
                const int incl = wave_incl_max_i32(max(m2.x, m2.y));
                const int prev = __shfl(incl, (lane + 63) & 63);
                const int u0 = max(lane == 0 ? -1 : prev, m2.x), u1 = incl;
                const uint32_t q0 = 2u * (uint32_t)lane;
                const uint32_t gi0 = T0 + q0 + (uint32_t)__shfl((int)gofs, u0);
                const uint32_t gi1 = T0 + q0 + 1u + (uint32_t)__shfl((int)gofs, u1);
                /* positions at or beyond n re-read position 0's photon (n >= 1) and are never read */
                const uint32_t g0 = (uint32_t)__builtin_amdgcn_readlane((int)gi0, 0);
                const uint32_t j0 = q0 < n ? gi0 : g0, j1 = q0 + 1u < n ? gi1 : g0;
                const float4 pa0 = P.ph_a[j0], pa1 = P.ph_a[j1];
                const float4 qa0 = P.ph_b[2 * (size_t)j0], qa1 = P.ph_b[2 * (size_t)j1];
                const float ca0 = phb[8 * (size_t)j0 + 4], ca1 = phb[8 * (size_t)j1 + 4];
                T.pr[2 * lane] = make_float4(pa0.x, pa1.x, pa0.y, pa1.y);
                *reinterpret_cast<f2 *>(&T.pr[2 * lane + 1]) = f2{pa0.z, pa1.z};
                *reinterpret_cast<f2 *>(&T.w[q0]) = f2{pa0.w, pa1.w};
                T.b[q0] = qa0; T.b[q0 + 1] = qa1;
                *reinterpret_cast<f2 *>(&T.c[q0]) = f2{ca0, ca1};
            }
            wave_lds_sync();
            gp.mark(2);
            /* 3. each run of this lane within the window: LDS positions [base,
             * base + m). Tested two photons per packed instruction, 32
             * positions at a time, into hit masks; the hits of all runs are
             * then summed in one loop with every lane busy (max over lanes of
             * its hits per chunk, not one masked pass per photon any lane hits). */
            /* the pairs from even position a + v0: cnt (<= 32) positions, bits 2j / 2j + 1 of pair j;
             * positions outside [lo_bit, hi_bit) of this chunk are another run's or the window's */
            auto test32p = [&](uint32_t a, uint32_t v0, uint32_t cnt, uint32_t lo_bit, uint32_t hi_bit) {
                const float4 *pp = &T.pr[a + v0]; /* pair (a + v0) / 2: two float4 each */
                uint32_t bits = 0u;
                const uint32_t np = (cnt + 1u) >> 1;
#ifndef PM_TEST_UNROLL
#define PM_TEST_UNROLL 2 /* 96 VGPRs, 5 waves/SIMD (4: 110 VGPRs, 4 waves): C2 gather 48.9-49.7 -> 47.5-48.4 us, C5 0.217 -> 0.206 ms, C3 0.545 -> 0.563 ms */
#endif
#pragma unroll PM_TEST_UNROLL
                for (uint32_t j = 0; j < np; ++j) {
                    const float4 xy = pp[2 * j];
                    const f2 zz = *reinterpret_cast<const f2 *>(&pp[2 * j + 1]);
                    const f2 ddx = px2 - f2{xy.x, xy.y}, ddy = py2 - f2{xy.z, xy.w}, ddz = pz2 - zz;
                    const f2 d2 = (ddx * ddx + ddy * ddy) + ddz * ddz;
                    /* d2 < r^2 is the sign of min(d2, FLT_MAX) - r^2: exact
                     * for finite d2 (a difference of unequal floats is never
                     * 0, d2 >= +0), and a NaN d2 (non-finite photon or record
                     * coordinates; its sign bit is arbitrary — the packed
                     * subtract negates an operand) becomes FLT_MAX, false as
                     * the comparison is; shifted in with one alignbit per
                     * photon; the first pair ends in the top bits: reversed
                     * below */
                    const f2 df = f2{fminf(d2.x, 0x1.fffffep127f), fminf(d2.y, 0x1.fffffep127f)} - r2v;
                    bits = __builtin_amdgcn_alignbit(bits, __float_as_uint(df.x), 31u);
                    bits = __builtin_amdgcn_alignbit(bits, __float_as_uint(df.y), 31u);
                }
                bits = __builtin_bitreverse32(bits) >> (32u - 2u * np);
                const uint32_t hi_m = hi_bit >= 32u ? 0xffffffffu : (1u << hi_bit) - 1u;
                return bits & hi_m & ~((1u << lo_bit) - 1u);
            };
            auto hit = [&](uint32_t t) {
                const float4 qb4 = T.b[t];
                const v3 wi = mk(T.w[t], qb4.w, T.c[t]);
                if (NN) {
                    /* fvs = fv * 2^S: the power-of-two scale commutes with the
                     * rounding, so this is rint(c * 2^S) for c of processPhoton */
                    const v3 c = fabsf(dot(R.ns, wi)) * fvs * xyz(qb4);
                    dx += (double)rintf(c.x); dy += (double)rintf(c.y); dz += (double)rintf(c.z);
                } else {
                    add_hit(Lf, R.ns, R.fv, make_float4(0.f, 0.f, 0.f, wi.x), qb4, wi.z, sc);
                }
            };
            uint32_t mK[KR], baseK[KR], vK[KR];
            uint32_t vmax = 0u;
#pragma unroll
            for (int k = 0; k < KR; ++k) {
                const uint32_t lo = max(sK[k], T0), hi = min(eK[k], T0 + n);
                mK[k] = hi > lo ? hi - lo : 0u;
                baseK[k] = mK[k] ? lo - T0 : 0u; /* < TILE_CAP */
                /* from the even position below the run: one more position when it starts odd */
                mK[k] += mK[k] ? (baseK[k] & 1u) : 0u;
                baseK[k] &= ~1u;
                vK[k] = wave_max_u32(mK[k]);
                vmax = max(vmax, vK[k]);
            }
            for (uint32_t vb = 0; vb < vmax; vb += 32) {
                TILE_STAT(5, 1);
                uint32_t bK[KR], any = 0u;
                int nh = 0;
#pragma unroll
                for (int k = 0; k < KR; ++k) {
                    TILE_STAT(2, (min(32u, vK[k] > vb ? vK[k] - vb : 0u) + 1) / 2);
                    /* the run's first position is odd: bit 0 of its first chunk is not its own */
                    const uint32_t lob = vb == 0u && mK[k] ? (uint32_t)(max(sK[k], T0) - T0 - baseK[k]) : 0u;
                    const uint32_t hib = mK[k] > vb ? mK[k] - vb : 0u;
                    bK[k] = vK[k] > vb ? test32p(baseK[k], vb, min(32u, vK[k] - vb), lob, hib) : 0u;
                    nh += __builtin_popcount(bK[k]);
                    any |= bK[k];
                }
                M += nh;
                gp.mark(3);
                TILE_STAT(3, wave_max_u32(nh));
                while (any) {
                    /* the first run with a hit left: its lowest position */
                    uint32_t t = 0u;
                    bool took = false;
                    any = 0u;
#pragma unroll
                    for (int k = 0; k < KR; ++k) {
                        if (!took && bK[k]) {
                            t = baseK[k] + vb + (uint32_t)__builtin_ctz(bK[k]);
                            bK[k] &= bK[k] - 1u;
                            took = true;
                        }
                        any |= bK[k];
                    }
                    hit(t);
                }
                gp.mark(4);
            }
            wave_lds_sync(); /* the window is read before the next one overwrites it */
        }
    }
    /* lanes whose radius exceeds the grid's design radius, and the lanes
     * of incoherent tiles, scan their own cells from global memory */
    TILE_STAT(4, __builtin_popcountll(__ballot(direct)));
    if (NN) {
        if (dx < 0x1p53 && dy < 0x1p53 && dz < 0x1p53) { /* NaN / inf fail: int64 path */
            Lf.x = d2ll(dx); Lf.y = d2ll(dy); Lf.z = d2ll(dz);
        } else if (small) { /* inexact (or NaN): this record again in int64 */
            M = 0;
            direct = true;
        }
    }
    gp.mark(4);
    /* Direct lanes with a small box whose cells hold few photons in all (an
     * incoherent tile's lanes no group took, C3: ~12 per wave, ~20 photons
     * each): the whole wave scans each one's cells in turn, 64 photons per
     * load. Many photons (a dense union's group, C5; a tile of unrelated
     * surfaces at a depth edge): each lane its own, side by side — the
     * cooperative scan's time grows with the sum over the lanes, the
     * per-lane scans' with the largest lane. */
    if (__ballot(direct)) {
        const bool cand = direct && small;
        uint32_t own = 0u;
        if (cand) { /* every row of the lane's box (up to KR x KR with finer cells) */
            for (uint32_t cz = R.z0; cz <= R.z1; ++cz)
                for (uint32_t cy = R.y0; cy <= R.y1; ++cy) {
                    const uint32_t row = (cz * (uint32_t)g.dy + cy) * (uint32_t)g.dx;
                    own += P.cell_start[row + R.x1 + 1u] - P.cell_start[row + R.x0];
                }
        }
        const uint32_t tot = uniform_u32(__builtin_amdgcn_readlane(wave_incl_sum_u32(own), 63));
#ifdef PM_COOP_STATS
        const uint32_t nc = (uint32_t)__builtin_popcountll(__ballot(cand)), nd = (uint32_t)__builtin_popcountll(__ballot(direct));
        if (lane == 0 && P.counters) {
            atomicAdd(&P.counters[8], 1ull); atomicAdd(&P.counters[9], (unsigned long long)nc);
            atomicAdd(&P.counters[10], (unsigned long long)tot); atomicMax(&P.counters[11], (unsigned long long)tot);
            atomicAdd(&P.counters[12], (unsigned long long)nd);
            if (nc > 16) { atomicAdd(&P.counters[13], 1ull); atomicAdd(&P.counters[14], (unsigned long long)tot); }
            atomicMax(&P.counters[15], (unsigned long long)nc);
        }
#endif
        if (tot <= (uint32_t)P.coop_steps * 64u) {
            bool sel = cand;
            coop_batch(P, T, lane, R, sel, M, Lf);
            direct = direct && !cand;
        }
    }
    if (direct) lane_scan<0, 1>(P, R.p, R.r2, R.ns, R.fv, R.x0, R.x1, R.y0, R.y1, R.z0, R.z1, M, Lf, nv, nr);
    gp.mark(5);
    R.store<PARTIAL>(P, r, M, Lf);
    if (!PARTIAL && P.r2hist) r2_histogram(P, R.live, R.st.w);
    if (COST && lane == 0)
        P.tile_cost[w] = (uint16_t)min(__builtin_amdgcn_s_memrealtime() - tc0, 65535ull);
    gp.mark(6);
    gp.flush(P.counters);
#ifdef PM_TILE_TIMES
    if (P.tile_times && lane == 0) {
        uint32_t xcc, hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        unsigned long long *o = P.tile_times + 8 * (size_t)blockIdx.x;
        o[0] = tt0; o[1] = __builtin_amdgcn_s_memrealtime(); o[2] = xcc; o[3] = hw;
        /* groups | windows << 32, test pairs | hit iterations << 32, direct lanes | chunks << 32, staged | record << 32 */
        o[4] = tstat[0] | ((unsigned long long)tstat[1] << 32);
        o[5] = tstat[2] | ((unsigned long long)tstat[3] << 32);
        o[6] = tstat[4] | ((unsigned long long)tstat[5] << 32);
        o[7] = tstat[7] | ((unsigned long long)(r - lane) << 32);
    }
#endif
}

/* kd-tree range query in the reference layout (gathering.cu:25-96):
 * same visiting order, same accumulation order -> bit-exact with it. */
template <int PARTIAL, int COUNT>
__global__ __launch_bounds__(GATHER_BLOCK) void k_gather_kd(GatherParams P) {
    __shared__ uint32_t stk[KD_STACK * GATHER_BLOCK];
    uint32_t *stack = stk + threadIdx.x;
    const int64_t r = P.rec_begin + (int64_t)blockIdx.x * GATHER_BLOCK + threadIdx.x;
    unsigned long long vis = 0, hits = 0, rows = 0, act = 0;
    if (r < P.rec_end) {
        float4 pos = P.R.pos[r];
        uint32_t flags = (uint32_t)__float_as_int(pos.w);
        if (flags & (PM_REC_MISS | PM_REC_EXCEPTION | PM_REC_INVALID)) {
            if (PARTIAL) write_partial(P, partial_index(P, r), 0, Fx3{0, 0, 0});
        } else {
            float4 st = P.fresh ? make_float4(0.f, 0.f, 0.f, P.r2init) : P.R.state[r];
            float4 nrm = P.R.nrm[r];
            const float maxDist2 = st.w;
            float4 m = P.materials[__float_as_int(nrm.w)];
            v3 fv = __float_as_int(m.w) == PM_MATTE ? xyz(m) * INV_PI : mk(0.f, 0.f, 0.f);
            const v3 p = xyz(pos), ns = xyz(nrm);
            int M = 0;
            v3 L = mk(0.f, 0.f, 0.f);
            if (P.kd_count > 0) {
                int sp = 0;
                uint32_t nodeNum = 0;
                stack[0] = 0; sp = 1;
                int64_t guard = 0; /* each node is visited at most once */
                const int stack_max = P.kd_stack < KD_STACK ? P.kd_stack : KD_STACK;
                bool overflow = false;
                do {
                    if (++guard > P.kd_count || nodeNum >= (uint64_t)P.kd_count) { /* not a pbrt kd-tree */
                        atomicOr(P.error, PM_GATHER_ERR_TREE);
                        break;
                    }
                    const float2 *q = reinterpret_cast<const float2 *>(P.kd_nodes + nodeNum);
                    float2 q0 = q[0], q1 = q[1];
                    uint32_t bits = (uint32_t)__float_as_int(q0.x);
                    uint32_t axis = (bits >> 1) & 3u, hasLeft = bits & 1u, right = bits >> 3;
                    v3 np = mk(q0.y, q1.x, q1.y);
                    v3 diff = p - np;
                    float dist2 = diff.x * diff.x + diff.y * diff.y + diff.z * diff.z;
                    if (COUNT) vis++;
                    if (dist2 < maxDist2) {
                        M++;
                        float2 q2 = q[2], q3 = q[3], q4 = q[4];
                        v3 al = mk(q2.x, q2.y, q3.x), wi = mk(q3.y, q4.x, q4.y);
                        L = L + fabsf(dot(ns, wi)) * fv * al;
                    }
                    if (axis < 3) {
                        float pa = comp(p, (int)axis), na = comp(np, (int)axis);
                        float d2 = (pa - na) * (pa - na);
                        if (pa <= na) {
                            if (d2 < maxDist2 && right < PM_PHOTON_MAX_RIGHT_CHILD) {
                                if (sp < stack_max) { stack[sp * GATHER_BLOCK] = right; ++sp; } else overflow = true;
                            }
                            if (hasLeft) nodeNum = nodeNum + 1; else { --sp; nodeNum = stack[sp * GATHER_BLOCK]; }
                        } else {
                            if (d2 < maxDist2 && hasLeft) {
                                if (sp < stack_max) { stack[sp * GATHER_BLOCK] = nodeNum + 1; ++sp; } else overflow = true;
                            }
                            if (right < PM_PHOTON_MAX_RIGHT_CHILD) nodeNum = right;
                            else { --sp; nodeNum = stack[sp * GATHER_BLOCK]; }
                        }
                    } else {
                        --sp;
                        nodeNum = stack[sp * GATHER_BLOCK];
                    }
                } while (nodeNum);
                /* a dropped subtree would silently lose photons: the launch reports it */
                if (overflow) atomicOr(P.error, PM_GATHER_ERR_STACK);
            }
            if (COUNT) { hits += (unsigned long long)M; act++; }
            if (PARTIAL) {
                const float sc = P.fx_scale;
                write_partial(P, partial_index(P, r), M, Fx3{to_fx(L.x, sc), to_fx(L.y, sc), to_fx(L.z, sc)});
            } else {
                float N = P.fresh ? 0.f : P.R.n[r];
                ppm_apply(st, N, M, L, P.ppm_alpha);
                if (M > 0 || P.fresh) { P.R.state[r] = st; P.R.n[r] = N; }
            }
        }
    }
    if (COUNT) count4(P.counters, vis, hits, rows, act);
}

template <int PARTIAL, int NN, bool COST>
static void launch_tile_nn(const GatherParams &p, unsigned g, hipStream_t s) {
    switch (p.span) { /* cells per axis of a lane box at the grid's design radius */
    case 2: pm_launch((k_gather_tile<PARTIAL, NN, 2, COST>), dim3(g), dim3(TILE_BLOCK), 0, s, p); break;
    case 3: pm_launch((k_gather_tile<PARTIAL, NN, 3, COST>), dim3(g), dim3(TILE_BLOCK), 0, s, p); break;
    case 4: pm_launch((k_gather_tile<PARTIAL, NN, 4, COST>), dim3(g), dim3(TILE_BLOCK), 0, s, p); break;
    default: pm_launch((k_gather_tile<PARTIAL, NN, 5, COST>), dim3(g), dim3(TILE_BLOCK), 0, s, p); break;
    }
}
template <int PARTIAL>
static void launch_tile(const GatherParams &p, unsigned g, hipStream_t s) {
    /* only a list launch measures tile costs (they index the list) */
    const bool cost = p.tile_cost != nullptr && p.tiles != nullptr;
    if (p.fx_nonneg) cost ? launch_tile_nn<PARTIAL, 1, true>(p, g, s) : launch_tile_nn<PARTIAL, 1, false>(p, g, s);
    else cost ? launch_tile_nn<PARTIAL, 0, true>(p, g, s) : launch_tile_nn<PARTIAL, 0, false>(p, g, s);
}

template <int STRUCT, int PARTIAL, int COUNT>
static void launch_g(const GatherParams &p, hipStream_t s) {
    unsigned grid = (unsigned)((p.rec_end - p.rec_begin + GATHER_BLOCK - 1) / GATHER_BLOCK);
    if (STRUCT == PM_GATHER_GRID && !COUNT && p.kernel == PM_GK_TILE && p.tiles) {
        /* the tile list: only tiles with an active record */
        const int64_t waves = p.n_tiles;
        const unsigned g = (unsigned)((waves + TILE_BLOCK / 64 - 1) / (TILE_BLOCK / 64));
        if (g == 0) return;
        launch_tile<PARTIAL>(p, g, s);
        return;
    }
    /* a counting launch always runs the per-lane kernel: its census (rows and
     * photons per RECORD) is the algorithm's unit count bench.py prices; the
     * tile and wave kernels find exactly the same photons (bit-identical records) */
    if (STRUCT == PM_GATHER_GRID && !COUNT && p.kernel == PM_GK_TILE)
        launch_tile<PARTIAL>(p, (unsigned)((p.rec_end - p.rec_begin + TILE_BLOCK - 1) / TILE_BLOCK), s);
    else if (STRUCT == PM_GATHER_GRID)
        pm_launch((k_gather_grid<PARTIAL, COUNT>), dim3(grid), dim3(GATHER_BLOCK), 0, s, p);
    else
        pm_launch((k_gather_kd<PARTIAL, COUNT>), dim3(grid), dim3(GATHER_BLOCK), 0, s, p);
}

hipError_t launch_gather(const GatherParams &p, int structure, int partial, int count, hipStream_t s) {
    if (p.rec_end <= p.rec_begin) return hipSuccess;
    int key = (structure ? 4 : 0) | (partial ? 2 : 0) | (count ? 1 : 0);
    switch (key) {
    case 0: launch_g<0, 0, 0>(p, s); break;
    case 1: launch_g<0, 0, 1>(p, s); break;
    case 2: launch_g<0, 1, 0>(p, s); break;
    case 3: launch_g<0, 1, 1>(p, s); break;
    case 4: launch_g<1, 0, 0>(p, s); break;
    case 5: launch_g<1, 0, 1>(p, s); break;
    case 6: launch_g<1, 1, 0>(p, s); break;
    default: launch_g<1, 1, 1>(p, s); break;
    }
    return hipGetLastError();
}

} // namespace pm
