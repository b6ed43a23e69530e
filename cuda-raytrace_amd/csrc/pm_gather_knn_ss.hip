/*
 * pm_gather_knn_ss.hip — the scalar-stream kNN gather (the default kNN path):
 * k_gather_knn_ss with its photon-pair packing (k_knn_pack), and
 * launch_knn_ss. It computes the estimate of pm_gather_knn.hip's kernels bit
 * for bit and hands the tiles it does not handle back to k_gather_knn_tile.
 *
 * wave64; 8x8 pixel tiles map onto one wave (see pm_gather.hip).
 */
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pm_kernels.h"
#include "pm_knn_dev.h"

#pragma clang fp contract(off)

namespace pm {
/* wave-uniform float minimum / maximum on pm_gather_dev.h's DPP scan (every
 * lane active): k_gather_knn_ss's pass bounds */
PMD float wave_min_f(float v) {
    const int m = wave_scan_dpp(__float_as_int(v), __float_as_int(INFINITY),
                                [](int a, int b) { return __float_as_int(fminf(__int_as_float(a), __int_as_float(b))); });
    return __int_as_float(__builtin_amdgcn_readlane(m, 63));
}
PMD float wave_max_f(float v) {
    const int m = wave_scan_dpp(__float_as_int(v), __float_as_int(-INFINITY),
                                [](int a, int b) { return __float_as_int(fmaxf(__int_as_float(a), __int_as_float(b))); });
    return __int_as_float(__builtin_amdgcn_readlane(m, 63));
}

/* wave-uniform vector loads through the scalar cache (k_gather_knn_ss) */
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef const f32x16 __attribute__((address_space(4), aligned(4))) sv16;
typedef const f32x8 __attribute__((address_space(4), aligned(4))) sv8;

/* ---------------------------------------------------------------------- */
/* kNN scalar-stream kernel (the default kNN path): the estimate of
 * k_gather_knn_tile / k_gather_knn bit for bit, with the photons streamed
 * through the scalar cache instead of staged into LDS.
 *  - A wave (one 8x8 tile) forms the same groups as k_gather_knn_tile. Per
 *    pass it walks the rows of the union box of its lanes' bounds; a row is a
 *    contiguous run of the cell-sorted photons, read as photon PAIRS
 *    (k_knn_pack: x0 x1 | y0 y1 | z0 z1 | wx0 wx1 ...) with s_load, so one
 *    SGPR pair is the wave-uniform operand of a packed v_pk_* instruction and
 *    every lane tests both photons of the pair against its own record. No
 *    staging, no index mapping, no LDS traffic for the photons at all.
 *  - r_k^2 by radix-style histograms on the d^2 BIT PATTERNS (a non-negative
 *    float orders like its bits): bin = min(sat(bits - A) >> sh, 32), 32 bins
 *    + a sink per lane in LDS (one ds_add per photon, no conversions, exact
 *    bin edges). Level 0 covers the two octaves below maxD^2 at 1/16 octave
 *    (bin 0 also takes everything nearer); the bin holding the K-th value is
 *    COLLECTed into a per-lane list (<= 12) and ranked, or, when it holds
 *    more, histogrammed again at 32x the resolution (or, for a dense lane
 *    whose K-th is in bin 0, over all of [0, hi) in 4-octave bins).
 *  - SUM: every lane adds, for each pair, the pbrt kernel terms of the
 *    photons below its r_k^2 that face it, in the record's fixed point
 *    (rint, exact double sums: order-free), masked per lane; a pair no lane
 *    hits costs only its distance test.
 *  - Passes are phase-serialised per wave (HIST before COLLECT before SUM),
 *    so each pass runs one specialised loop.
 * A tile this kernel does not handle — a lane group whose union box exceeds
 * the 128-row map, r_k^2 = 0 (pbrt's 0/0 and its lowest-slot ties) — is
 * appended to P.knn_ovf and re-run by k_gather_knn_tile. */
/* waves per SIMD (VGPR budget; the 4.25 KB histogram allows 9): C2 kNN gather
 * 5 (81 VGPRs) 0.746-0.757 ms, 6 (73) 0.735, 7 (72) 0.747 (same box) */
#define KS_OCC __attribute__((amdgpu_waves_per_eu(6, 6)))
constexpr int KS_NB = 32;   /* bins per histogram level (+1 sink), 16-bit counters: two lanes per word */
constexpr int KS_HW = KS_NB / 2 + 1; /* LDS words per lane: (KS_NB + 1) 16-bit counters, or KS_LIST + 1 list rows + a sink row */
constexpr int KS_LIST = 12; /* values a COLLECT keeps per lane (rows 0..KS_LIST of the histogram, +1 scratch) */
/* (y, z) rows of a group's union box: two per lane. With 64, a tile across a
 * corner of the room (lanes on two walls, the union deeper than 8 x 8 rows)
 * split into leader groups, each running its own passes over nearly the same
 * photons: those tiles took up to 19 passes against 3.65 on average and set
 * the launch's length (tools/tile_times.py knn) */
constexpr int KS_ROWS = 128;
enum { KS_HIST = 0, KS_COLLECT = 1, KS_SUM = 2, KS_DONE = 3 };
static_assert(KS_LIST + 1 < KS_HW, "the COLLECT list aliases histogram rows (not the sink's)");

/* photon pairs of the bucket order for the scalar stream: pair k = photons
 * 2k, 2k + 1, P block (x x y y z z wx wx), Q block (r r g g b b wy wy wz wz
 * . .); photons past the map are zero (the stream masks them). Block 0
 * 0 also clears the KNN_OVF_HDR overflow-tile counters of this gather. */
__global__ __launch_bounds__(256) void k_knn_pack(const uint32_t *cell_start, uint32_t ncells, const float4 *ph_a,
                                                  const float4 *ph_b, float4 *pk_p, float4 *pk_q, int64_t npairs,
                                                  uint32_t *ovf_n) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < KNN_OVF_HDR && ovf_n) ovf_n[k] = 0u;
    if (k >= npairs) return;
    const int64_t n = cell_start[ncells], j = 2 * k;
    if (j >= n + 16) return; /* a few zero pairs past the map: never read unmasked */
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, b0 = a0, b1 = a0;
    float c0 = 0.f, c1 = 0.f;
    if (j < n) { a0 = ph_a[j]; b0 = ph_b[2 * j]; c0 = ph_b[2 * j + 1].x; }
    if (j + 1 < n) { a1 = ph_a[j + 1]; b1 = ph_b[2 * j + 2]; c1 = ph_b[2 * j + 3].x; }
    pk_p[2 * k] = make_float4(a0.x, a1.x, a0.y, a1.y);
    pk_p[2 * k + 1] = make_float4(a0.z, a1.z, a0.w, a1.w);
    pk_q[3 * k] = make_float4(b0.x, b1.x, b0.y, b1.y);
    pk_q[3 * k + 1] = make_float4(b0.z, b1.z, b0.w, b1.w);
    pk_q[3 * k + 2] = make_float4(c0, c1, 0.f, 0.f);
}

/* gap (cell units) between [lo, hi] and cell c of an axis of dim cells —
 * the border cells extend to infinity (cell_axis clamps) — less a 1e-3
 * margin for the rounding of the cell-unit coordinates */
PMD float box_gap(float lo, float hi, uint32_t c, int dim) {
    const float a = c == 0 ? -INFINITY : (float)c, b = (int)c + 1 == dim ? INFINITY : (float)(c + 1);
    return fmaxf(fmaxf(a - hi, lo - b) - 1e-3f, 0.f);
}
/* cell of a cell-unit coordinate, clamped like cell_axis */
PMD uint32_t cell_u(float u, int dim) {
    const int c = (int)floorf(u);
    return (uint32_t)(c < 0 ? 0 : (c >= dim ? dim - 1 : c));
}
__global__ __launch_bounds__(64) KS_OCC void k_gather_knn_ss(GatherParams P) {
#ifdef PM_TILE_TIMES
    uint32_t tstat[8] = {0, 0, 0, 0, 0, 0, 0, 0}; /* TILE_STAT's sink (unused here) */
    (void)tstat;
#endif
    /* 4.25 KB: HIST counts 16-bit halves (bin h of lane l: half l & 1 of
     * word 32 h + l / 2, bins 0..32); COLLECT lists 32-bit words (entry a of
     * lane l: word 64 a + l, rows 0..KS_LIST, the sink row KS_HW - 1) */
    __shared__ uint32_t H[KS_HW * 64];
    const int lane = threadIdx.x & 63;
    if (P.tiles && P.n_tiles_dev && (int64_t)blockIdx.x >= (int64_t)*P.n_tiles_dev) return;
#ifdef PM_TILE_TIMES
    const unsigned long long tc0 = __builtin_amdgcn_s_memrealtime();
#else
    const unsigned long long tc0 = P.tile_cost ? __builtin_amdgcn_s_memrealtime() : 0ull;
#endif
    /* the wave's lifetime for the cost-ordered tile list (k_tile_sort) */
    auto record_cost = [&]() {
        if (P.tile_cost && lane == 0)
            P.tile_cost[blockIdx.x] = (uint16_t)min(__builtin_amdgcn_s_memrealtime() - tc0, 65535ull);
    };
    const uint32_t tile = P.tiles ? P.tiles[blockIdx.x] : blockIdx.x;
    const int64_t r = P.rec_begin + (int64_t)tile * 64 + lane;
    const int K = P.knn_k;
    const float maxd2 = P.knn_r2;
#pragma unroll
    for (int b = 0; b < KS_HW; ++b) H[b * 64 + lane] = 0u;
    bool active = false, live = false, back = false;
    float4 pos = make_float4(0.f, 0.f, 0.f, 0.f), nrm = pos;
    if (r < P.rec_end) {
        pos = P.R.pos[r];
        const uint32_t flags = (uint32_t)__float_as_int(pos.w);
        active = !(flags & (PM_REC_MISS | PM_REC_EXCEPTION | PM_REC_INVALID));
        back = (flags & PM_REC_BACKFACE) != 0;
        if (active) {
            nrm = P.R.nrm[r];
            live = __float_as_int(P.materials[__float_as_int(nrm.w)].w) == PM_MATTE; /* non-specular BSDF only */
        }
    }
    const v3 p = xyz(pos);
    /* Faceforward folded into the normal: Dot(-n, w) = -Dot(n, w) exactly */
    const float nsx = back ? -nrm.x : nrm.x, nsy = back ? -nrm.y : nrm.y, nsz = back ? -nrm.z : nrm.z;
    const GridDesc g = P.grid;
    TILE_STAT(0, 1);
    GProf gp; /* PM_GATHER_PROFILE: record + groups, pass setup, HIST, COLLECT, SUM, pass end, store */
    gp.begin();
    uint32_t x0 = 0, x1 = 0, y0 = 0, y1 = 0, z0 = 0, z1 = 0;
    if (live) knn_cells(g, p, maxd2, x0, x1, y0, y1, z0, z1); /* KnnGrid::init's cells */
    /* selection state: HIST level (A, sh) counts the values below
     * A + (32 << sh) (bin 0 includes everything below A + (1 << sh)) */
    const uint32_t Bm = __float_as_uint(maxd2);
    uint32_t sh = 19u;
    while (sh > 0u && (32u << sh) > Bm) --sh;
    uint32_t A = Bm - (32u << sh);
    /* lowopen: bin 0 also holds everything below A (level 0, before any
     * refinement); otherwise the K-th is known to be >= A and `base` values
     * lie below A (bin 0 counts them too: every histogram counts global ranks) */
    uint32_t base = 0u;
    int phase = live ? KS_HIST : KS_DONE;
    bool lvl0 = true, full = true, defer = false, lowopen = true;
    uint32_t klo = 0u, kw = 0u, cc = 0u;
    int need = 0, less = 0, cnt = 0;
    float md2 = maxd2, inv = 0.f, sc = 1.f;
    Kx3 acc{0, 0, 0};

    const const_f32_ptr pkp = (const_f32_ptr)P.knn_pk_p;
    const const_f32_ptr pkq = (const_f32_ptr)P.knn_pk_q;
    const f2 px2 = {p.x, p.x}, py2 = {p.y, p.y}, pz2 = {p.z, p.z};
    bool pend = live;
    while (!defer) {
        const unsigned long long pm = __ballot(pend);
        if (pm == 0ull) break;
        /* the group: every pending lane if their union box fits the row map
         * (two rows per lane), else the first pending lane's neighbourhood */
        uint32_t X0, X1, Y0, Y1, Z0, Z1;
        bool mine = pend;
        union_box6(g, mine, x0, x1, y0, y1, z0, z1, X0, X1, Y0, Y1, Z0, Z1);
        uint32_t LY = rowmap_bits(Y0, Y1);
        if (LY > 7u || ((uint64_t)(Z1 - Z0 + 1u) << LY) > (uint64_t)KS_ROWS) {
            /* the first pending lane's neighbourhood: the lanes whose box
             * starts within GRk cells of the leader's, for the widest GRk whose
             * union still fits the row map (a surface seen at a grazing angle
             * spreads its tile over several cells: wider groups, fewer of them,
             * each with its own passes) */
            const int leader = __builtin_ctzll(pm);
            const uint32_t lx = __builtin_amdgcn_readlane(x0, leader), ly = __builtin_amdgcn_readlane(y0, leader),
                           lz = __builtin_amdgcn_readlane(z0, leader);
            bool fits = false;
            for (uint32_t GRk = 4u; !fits && GRk >= KT_GROUP_R; GRk >>= 1) {
                mine = pend && x0 + GRk - lx <= 2u * GRk && y0 + GRk - ly <= 2u * GRk && z0 + GRk - lz <= 2u * GRk;
                union_box6(g, mine, x0, x1, y0, y1, z0, z1, X0, X1, Y0, Y1, Z0, Z1);
                LY = rowmap_bits(Y0, Y1);
                fits = LY <= 7u && ((uint64_t)(Z1 - Z0 + 1u) << LY) <= (uint64_t)KS_ROWS;
            }
            if (!fits) { defer = true; break; } /* grid too coarse */
        }
        pend = pend && !mine;
        /* passes until every lane of the group has its estimate (a level
         * descends 5 bits or slides to [0, hi): far fewer than 64 passes;
         * the bound only guarantees that every wave ends) */
        for (int npass = 0;; ++npass) {
            if (npass == 64) { defer = true; break; }
            const bool in = mine && phase != KS_DONE;
            const unsigned long long mh = __ballot(in && phase == KS_HIST), mc = __ballot(in && phase == KS_COLLECT),
                                     ms = __ballot(in && phase == KS_SUM);
            if ((mh | mc | ms) == 0ull) break;
            const int pt = mh ? KS_HIST : (mc ? KS_COLLECT : KS_SUM);
            const bool act = in && phase == pt;
            TILE_STAT(1, 1);
            TILE_STAT(2, pt == KS_HIST);
            gp.mark(0);
            /* this lane's bound (every value the pass needs is below it) */
            float bnd = 0.f;
            if (act) {
                if (pt == KS_HIST) { /* the level's upper edge A + (32 << sh), at most maxD^2 */
                    const uint64_t ub = (uint64_t)A + ((uint64_t)32u << sh);
                    bnd = ub >= (uint64_t)Bm ? maxd2 : __uint_as_float((uint32_t)ub);
                }
                else if (pt == KS_COLLECT) bnd = __uint_as_float(klo + kw);
                else bnd = full ? next_up(md2) : md2;
            }
            /* the pass's union: cells of [p - r', p + r'], r'^2 = bnd: a
             * sub-box of the group's (bnd <= maxD^2), so it fits the row map */
            uint32_t a0 = 0, a1 = 0, b0 = 0, b1 = 0, c0 = 0, c1 = 0;
            if (act) knn_cells(g, p, bnd, a0, a1, b0, b1, c0, c1);
            uint32_t PX0, PX1, PY0, PY1, PZ0, PZ1;
            union_box6(g, act, a0, a1, b0, b1, c0, c1, PX0, PX1, PY0, PY1, PZ0, PZ1);
            const uint32_t PLY = rowmap_bits(PY0, PY1);
            /* rows pruned to the union of the pass's spheres: with the act
             * lanes' positions in the box [Pmin, Pmax] and R the largest
             * bound (cell units), a photon within R_l of lane l lies in a row
             * whose (y, z) gap to the box is <= R and, in that row, within
             * sqrt(R^2 - gap^2) of [Pmin.x, Pmax.x] (KnnGrid::scan's pruning
             * for the whole pass at once; cell_gap's 1e-3 margins) */
            const float ux = (p.x - g.gx) * g.inv_cs, uy = (p.y - g.gy) * g.inv_cs, uz = (p.z - g.gz) * g.inv_cs;
            const float Rq = wave_max_f(act ? (sqrtf(bnd) * 1.0001f + 1e-4f) * g.inv_cs : 0.f);
            const float mnx = wave_min_f(act ? ux : INFINITY), mxx = wave_max_f(act ? ux : -INFINITY);
            const float mny = wave_min_f(act ? uy : INFINITY), mxy = wave_max_f(act ? uy : -INFINITY);
            const float mnz = wave_min_f(act ? uz : INFINITY), mxz = wave_max_f(act ? uz : -INFINITY);
            /* union rows u = lane and lane + 64: photons [Bu, Bu + Lu) of cells
             * xa..xb of its (y, z) */
            uint32_t Bu[2] = {0u, 0u}, Lu[2] = {0u, 0u};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t u = (uint32_t)lane + 64u * (uint32_t)h;
                const uint32_t cy = PY0 + (u & ((1u << PLY) - 1u)), cz = PZ0 + (u >> PLY);
                if (cy <= PY1 && cz <= PZ1) {
                    const float gy = box_gap(mny, mxy, cy, g.dy), gz = box_gap(mnz, mxz, cz, g.dz);
                    const float rem = Rq * Rq - (gy * gy + gz * gz);
                    if (rem >= 0.f) {
                        const float sx = sqrtf(rem) * 1.0001f + 1e-3f;
                        const uint32_t xa = max(PX0, cell_u(mnx - sx, g.dx)), xb = min(PX1, cell_u(mxx + sx, g.dx));
                        if (xa <= xb) {
                            const uint32_t row = (cz * (uint32_t)g.dy + cy) * (uint32_t)g.dx;
                            Bu[h] = P.cell_start[row + xa];
                            Lu[h] = P.cell_start[row + xb + 1u] - Bu[h];
                        }
                    }
                }
            }
            const unsigned long long rows = __ballot(Lu[0] > 0u), rows_hi = __ballot(Lu[1] > 0u);
            /* 16-bit bin counters: a union of >= 2^16 photons goes to k_gather_knn_tile */
            if (uniform_u32(__builtin_amdgcn_readlane(wave_incl_sum_u32(Lu[0] + Lu[1]), 63)) >= 65536u) { defer = true; break; }
            /* per-lane constants of the pass (lanes outside it never hit) */
            const uint32_t hA = act ? A : 0u, hsh = act ? sh : 0u;
            const uint32_t clo = act ? klo : 0u, cw = act ? kw : 0u;
            const float smd = act ? md2 : -1.f, sinv = inv, ssc = sc;
            /* 1/r_k^2 times the power-of-two scale: exact, one multiply per term */
            const float sis = sinv * ssc;
            const f2 inv2 = {sinv, sinv}, is2 = {sis, sis}, one2 = {1.f, 1.f}, c3 = {3.f * INV_PI, 3.f * INV_PI};
            const f2 nx2 = {nsx, nsx}, ny2 = {nsy, nsy}, nz2 = {nsz, nsz};
            uint32_t *hcol = H + lane;
            /* HIST counters: bin h of lane l is the (l & 1) half of word
             * h * 32 + l / 2 (lanes l, l ^ 1 share a word column), so a count
             * is one address op and a per-lane constant increment */
            uint32_t *hpair = H + (lane >> 1);
            /* lanes outside the pass add 0 (their half of each word stays 0) */
            const uint32_t hinc = act ? 1u << ((lane & 1) * 16) : 0u;
            /* COLLECT: the lane's list rows (lanes outside the pass write the sink row) */
            uint32_t *lcol = hcol + (act ? 0 : (KS_HW - 1) * 64);
            uint32_t ccl = 0u;
            /* one specialised loop per pass type over the rows' photon pairs,
             * NP pairs per batch: the batch's s_loads are issued together and
             * waited on once (the scalar cache returns out of order, so a wave
             * cannot wait for an older load while a younger one is in flight) */
            auto stream = [&](auto PT_) PM_INLINE {
                constexpr int PT = decltype(PT_)::value;
                constexpr int NP = PT == KS_SUM ? 2 : 4;
                unsigned long long rm = rows, rm_hi = rows_hi;
                while (rm | rm_hi) {
                    /* rows 0..63 (Bu[0] of lane u), then 64..127 (Bu[1]) */
                    const bool hi = rm == 0ull;
                    const unsigned long long cur = hi ? rm_hi : rm;
                    const int u = __builtin_ctzll(cur);
                    if (hi) rm_hi &= rm_hi - 1ull;
                    else rm &= rm - 1ull;
                    const uint32_t b = uniform_u32(__builtin_amdgcn_readlane(hi ? Bu[1] : Bu[0], u));
                    const uint32_t e = b + uniform_u32(__builtin_amdgcn_readlane(hi ? Lu[1] : Lu[0], u));
                    const uint32_t k1 = (e + 1u) >> 1;
                    TILE_STAT(3, 1);
                    TILE_STAT(PT == KS_HIST ? 4 : PT == KS_COLLECT ? 5 : 6, k1 - (b >> 1));
                    for (uint32_t k0 = b >> 1; k0 < k1; k0 += NP) {
                        /* the batch (reads past the run stay inside the packed
                         * buffer's zero pairs; their photons are never counted) */
                        /* whole-vector loads: one s_load_dwordx16 per 64 B, none of
                         * them sunk into the per-pair branches below */
                        float pv[NP][8], qv[PT == KS_SUM ? NP : 1][12];
                        const sv16 *q = (const sv16 *)(pkp + 8 * (size_t)k0);
                        if constexpr (PT == KS_SUM) {
                            static_assert(NP == 2, "one P vector + 24 Q floats per batch");
                            f32x16 v = q[0], a = ((const sv16 *)(pkq + 12 * (size_t)k0))[0];
                            f32x8 c8 = ((const sv8 *)(pkq + 12 * (size_t)k0 + 16))[0];
                            asm volatile("" : "+s"(v), "+s"(a), "+s"(c8)); /* the whole batch, one wait */
#pragma unroll
                            for (int c = 0; c < 16; ++c) pv[c / 8][c % 8] = v[c];
#pragma unroll
                            for (int c = 0; c < 12; ++c) qv[0][c] = a[c];
#pragma unroll
                            for (int c = 0; c < 4; ++c) qv[1][c] = a[12 + c];
#pragma unroll
                            for (int c = 0; c < 8; ++c) qv[1][4 + c] = c8[c];
                        } else {
                            static_assert(NP == 4, "two P vectors per batch");
                            f32x16 v0 = q[0], v1 = q[1];
                            asm volatile("" : "+s"(v0), "+s"(v1)); /* the whole batch, one wait */
#pragma unroll
                            for (int c = 0; c < 16; ++c) { pv[c / 8][c % 8] = v0[c]; pv[2 + c / 8][c % 8] = v1[c]; }
                        }
#pragma unroll
                        for (int i = 0; i < NP; ++i) {
                            const uint32_t k = k0 + (uint32_t)i;
                            if (i > 0 && k >= k1) break;
                            f2 X = {pv[i][0], pv[i][1]};
                            const f2 Y = {pv[i][2], pv[i][3]}, Z = {pv[i][4], pv[i][5]};
                            /* the run's ends: a half pair outside [b, e) is pushed to infinity */
                            if (2u * k < b) X.x = INFINITY;
                            if (2u * k + 1u >= e) X.y = INFINITY;
                            const f2 dx = px2 - X, dy = py2 - Y, dz = pz2 - Z;
                            const f2 d2 = (dx * dx + dy * dy) + dz * dz; /* in_radius / KnnGrid::scan's order */
                            const uint32_t u0 = __float_as_uint(d2.x), u1 = __float_as_uint(d2.y);
                            if constexpr (PT == KS_HIST) {
                                const uint32_t h0 = min(__builtin_elementwise_sub_sat(u0, hA) >> hsh, (uint32_t)KS_NB);
                                const uint32_t h1 = min(__builtin_elementwise_sub_sat(u1, hA) >> hsh, (uint32_t)KS_NB);
                                atomicAdd(hpair + h0 * 32u, hinc);
                                atomicAdd(hpair + h1 * 32u, hinc);
                            } else if constexpr (PT == KS_COLLECT) {
                                lcol[ccl * 64u] = u0;
                                ccl += (u0 - clo) < cw ? 1u : 0u;
                                lcol[ccl * 64u] = u1;
                                ccl += (u1 - clo) < cw ? 1u : 0u;
                            } else {
                                const f2 WX = {pv[i][6], pv[i][7]}, R = {qv[i][0], qv[i][1]}, G = {qv[i][2], qv[i][3]};
                                const f2 Bl = {qv[i][4], qv[i][5]}, WY = {qv[i][6], qv[i][7]}, WZ = {qv[i][8], qv[i][9]};
                                const bool h0 = d2.x < smd, h1 = d2.y < smd;
                                less += (int)h0 + (int)h1;
                                if (__ballot(h0 || h1)) {
                                    TILE_STAT(7, 1);
                                    const f2 dn = (nx2 * WX + ny2 * WY) + nz2 * WZ; /* knn_facing */
                                    /* knn_add: s = 1 - d^2 / r_k^2, kernel 3/pi s^2, times 1/r_k^2 and alpha;
                                     * a photon that does not count gets ki = 0, so every term of it is rint(0) = 0 */
                                    const f2 sv = one2 - d2 * inv2;
                                    f2 ki = ((c3 * sv) * sv) * is2;
                                    if (!(h0 && dn.x > 0.f)) ki.x = 0.f;
                                    if (!(h1 && dn.y > 0.f)) ki.y = 0.f;
                                    const f2 cr = ki * R, cg = ki * G, cb = ki * Bl;
                                    acc.x += knn_rnd(cr.x) + knn_rnd(cr.y); /* knn_add's rounding */
                                    acc.y += knn_rnd(cg.x) + knn_rnd(cg.y);
                                    acc.z += knn_rnd(cb.x) + knn_rnd(cb.y);
                                }
                            }
                        }
                    }
                }
            };
            gp.mark(1);
            if (pt == KS_HIST) stream(std::integral_constant<int, KS_HIST>{});
            else if (pt == KS_COLLECT) stream(std::integral_constant<int, KS_COLLECT>{});
            else stream(std::integral_constant<int, KS_SUM>{});
            gp.mark(pt == KS_HIST ? 2 : pt == KS_COLLECT ? 3 : 4);
            if (!act) continue;
            if (pt == KS_HIST) {
                /* the bin holding the K-th value; the column is left zeroed */
                uint32_t cum = 0u, below = 0u, cntb = 0u;
                int bs = -1;
                /* both lanes of a word read it before either clears it (one
                 * instruction each); a neighbour outside the pass counted only
                 * into the sink, so its halves of bins 0..31 are zero anyway */
                const uint32_t hs = (uint32_t)(lane & 1) * 16u;
#pragma unroll 4
                for (int b = 0; b < KS_NB; ++b) {
                    const uint32_t c = (hpair[b * 32] >> hs) & 0xffffu;
                    hpair[b * 32] = 0u;
                    if (bs < 0 && cum + c >= (uint32_t)K) { bs = b; below = cum; cntb = c; }
                    cum += c;
                }
                hpair[KS_NB * 32] = 0u;
                if (lvl0 && cum < (uint32_t)K) { /* fewer than K inside maxD: r_k^2 = maxD^2 */
                    full = false;
                    md2 = maxd2;
                    phase = KS_SUM;
                } else {
                    lvl0 = false;
                    /* the K-th value's bin [lo, hi): bin 0 of an open level
                     * starts at 0; bin 0 of a refined level holds the base
                     * values below A as well, which are not in [A, hi) */
                    const bool open0 = bs == 0 && lowopen && A != 0u;
                    const uint32_t lo = open0 ? 0u : A + ((uint32_t)bs << sh), hi = A + ((uint32_t)(bs + 1) << sh);
                    if (bs == 0 && !open0) { cntb -= base; below = base; }
                    if (sh == 0u && !open0) { /* a bin of one bit pattern */
                        md2 = __uint_as_float(lo);
                        phase = KS_SUM;
                    } else if (cntb <= (uint32_t)KS_LIST) {
                        phase = KS_COLLECT;
                        klo = lo; kw = hi - lo; need = K - (int)below; cc = 0u;
                    } else if (!open0) { /* 32x finer over the bin */
                        A = lo;
                        base = below;
                        sh = sh >= 5u ? sh - 5u : 0u;
                    } else { /* the K-th is below A + 2^sh (a dense lane): the 32 bins
                               * slide down to end at hi, 4x wider (8 octaves at 1/4 octave) */
                        const uint32_t sh2 = min(sh + 2u, 26u);
                        A = hi > (32u << sh2) ? hi - (32u << sh2) : 0u;
                        base = 0u;
                        sh = sh2;
                    }
                    lowopen = open0 && A != 0u && cntb > (uint32_t)KS_LIST;
                }
            } else if (pt == KS_COLLECT) {
                cc = ccl;
                /* rank the kept values (cc of them): the need-th smallest */
                uint32_t v[KS_LIST];
#pragma unroll
                for (int a = 0; a < KS_LIST; ++a) v[a] = (uint32_t)a < cc ? hcol[a * 64] : 0xffffffffu;
                const uint32_t *lcand = hcol;
                uint32_t ans = v[0];
                for (uint32_t a = 0; a < cc; ++a) { /* candidate a (re-read from LDS: a rolled loop) */
                    const uint32_t va = lcand[a * 64];
                    int lt = 0, le = 0;
#pragma unroll
                    for (int bb = 0; bb < KS_LIST; ++bb) { lt += v[bb] < va; le += v[bb] <= va; }
                    if (lt < need && need <= le) ans = va;
                }
#pragma unroll
                for (int a = 0; a <= KS_LIST; ++a) hcol[a * 64] = 0u;
                md2 = __uint_as_float(ans);
                phase = KS_SUM;
                if (md2 == 0.f) defer = true; /* pbrt's 0/0: k_gather_knn_tile's tie rules */
            }
            if (phase == KS_SUM && pt != KS_SUM) { /* begin_sum */
                sc = knn_scale(P.knn_fx, md2);
                inv = 1.f / md2;
                acc = Kx3{0, 0, 0};
                less = 0;
            } else if (pt == KS_SUM) {
                cnt = full ? K : less;
                phase = KS_DONE;
            }
        }
        if (__ballot(defer)) defer = true;
        gp.mark(5);
    }
    if (__ballot(defer)) { /* re-run by k_gather_knn_tile */
        if (lane == 0) P.knn_ovf[atomicAdd(P.knn_ovf_n, 1u)] = tile;
        record_cost();
        return;
    }
    if (active) {
        if (!live) md2 = maxd2; /* specular: nothing found, cnt 0 */
        const float4 st = P.fresh ? make_float4(0.f, 0.f, 0.f, P.r2init) : P.R.state[r];
        const double isc = 1.0 / (double)sc;
        const v3 Lr = mk((float)((double)acc.x * isc), (float)((double)acc.y * isc), (float)((double)acc.z * isc));
        const v3 flux = xyz(st) + Lr;
        P.R.state[r] = make_float4(flux.x, flux.y, flux.z, md2);
        P.R.n[r] = (float)cnt;
    }
    record_cost();
    gp.mark(6);
    gp.flush(P.counters);
#ifdef PM_TILE_TIMES
    if (P.tile_times && lane == 0) {
        uint32_t xcc, hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        unsigned long long *o = P.tile_times + 8 * (size_t)blockIdx.x;
        o[0] = tc0; o[1] = __builtin_amdgcn_s_memrealtime(); o[2] = xcc; o[3] = hw;
        o[4] = tstat[1] | ((unsigned long long)tstat[2] << 32);   /* passes | HIST passes */
        o[5] = tstat[4] | ((unsigned long long)tstat[5] << 32);   /* HIST pairs | COLLECT pairs */
        o[6] = tstat[6] | ((unsigned long long)tstat[3] << 32);   /* SUM pairs | rows */
        o[7] = tstat[7] | ((unsigned long long)(r - lane) << 32); /* hit batches | record */
    }
#endif
}

hipError_t launch_knn_ss(const GatherParams &p, unsigned grid, hipStream_t s) {
    /* the pairs once per photon map (band gathers reuse them); the overflow
     * counters of every gather */
    const int64_t np = p.knn_pk_pairs;
    if (p.knn_pack)
        pm_launch(k_knn_pack, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, p.cell_start, p.grid.ncells, p.ph_a,
                  p.ph_b, p.knn_pk_p, p.knn_pk_q, np, p.knn_ovf_n);
    else {
        const hipError_t e = hipMemsetAsync(p.knn_ovf_n, 0, KNN_OVF_HDR * sizeof(uint32_t), s);
        if (e != hipSuccess) return e;
    }
    pm_launch(k_gather_knn_ss, dim3(grid), dim3(64), 0, s, p);
    return hipSuccess; /* launch errors: the caller's hipGetLastError, after its own launch */
}

} // namespace pm
