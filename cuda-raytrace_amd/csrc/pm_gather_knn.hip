/*
 * pm_gather_knn.hip — the kNN estimator (pbrt-v2 PhotonIntegrator::LPhoton)
 * over the photon buckets: the per-lane heap kernel (k_gather_knn, census
 * launches), the LDS tile kernel (k_gather_knn_tile), the scalar-stream
 * kernel (k_gather_knn_ss) with its photon-pair packing (k_knn_pack), and
 * launch_gather_knn. All three kernels compute the same estimate bit for bit.
 *
 * wave64; 8x8 pixel tiles map onto one wave (see pm_gather.hip).
 */
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pm_gather_dev.h"
#include "pm_kernels.h"

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

/* ---------------------------------------------------------------------- */
/* kNN estimator: pbrt-v2 PhotonIntegrator::LPhoton (integrators/photonmap.cpp,
 * diffuse branch) with PhotonProcess / KdTree::Lookup semantics, over the
 * photon buckets. Per record (one lane), the found set is the K photons with
 * the smallest keys (d^2, slot) among those with d^2 < maxD2 — the set pbrt's
 * lookup finds, up to the order among photons at exactly equal d^2, where
 * the lower slot wins here and the first visited in pbrt. r_k^2 = the K-th
 * smallest d^2 once K were found (pbrt's shrunk maxDistSquared), else maxD2.
 *     S = sum over found photons with Dot(Nf, wi) > 0 of
 *         (3/pi (1 - d^2/r_k^2)^2 / r_k^2) * alpha        (kernel(), photonmap.cpp)
 * with Nf = Faceforward(ns, wo) (PM_REC_BACKFACE).
 * Two passes over the buckets: (1) a max-heap of d^2 values alone (4 B per
 * entry, LDS columns [K][64]) finds r_k^2; (2) a rescan bounded by r_k^2 sums
 * the photons with d^2 < r_k^2 and, of those at exactly r_k^2, the lowest
 * slots (slot ids ride in ph_b; a third scan runs only when more ties than
 * places exist). The sum is exact and order-free: integer-valued terms
 * in the record's fixed point (scale: the power of two below knn_fx * r_k^2,
 * every term <= 2^22) added in int32 (Kx3). Fused record update: flux += S, radius2 = r_k^2,
 * photon_count = found; the final pass applies 1/paths and rho/pi = Kd/pi
 * (k_final, pm_records.hip). Both passes visit rows in rings around the query's row,
 * nearest first, and skip rows / cells beyond the current bound. */
PMD float sq(float x) { return x * x; }
/* kNN sums: each term round(c * sc) is an integer <= 2^22
 * (knn_fx), at most PM_KNN_MAX = 2^6 of them per record, so their int32 sum
 * is exact (< 2^28): order-free like the PPM gather's int64 fixed point, at
 * one rounding, one conversion and one integer add per channel (round 4
 * summed terms <= 2^47 in double: two double-rate operations per term; the
 * scalar-stream SUM pass is 41 % of the kNN gather) */
struct Kx3 { int x, y, z; };
/* a kNN term to the nearest integer, floor(x + 0.5) in one instruction
 * (v_cvt_rpi_i32_f32): an error of at most half a unit of the record's fixed
 * point per term, without the one-sided bias of truncation (round 6) */
PMD int knn_rnd(float x) {
    int r;
    asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
/* Dot(Faceforward(ns, wo), wi) > 0 for the photon's wi = (wx, b.w, wz) */
PMD bool knn_facing(v3 ns, bool back, const float4 &b, float wx, float wz) {
    float dn = dot(ns, mk(wx, b.w, wz));
    if (back) dn = -dn;
    return dn > 0.f;
}
/* pbrt kernel() 3/pi (1 - d^2/r_k^2)^2 / r_k^2 times alpha, inv = 1/r_k^2,
 * in the record's fixed point sc */
PMD void knn_add(Kx3 &a, float d2, float inv, float sc, const float4 &b) {
    const float s = 1.f - d2 * inv;
    const float kk = 3.f * INV_PI * s * s;
    /* sc is a power of two: k * (inv * sc) * alpha rounds like (k * inv * alpha) * sc;
     * terms are rounded to the nearest integer (knn_rnd: <= 1/2 unit each) */
    const float ks = kk * (inv * sc);
    a.x += knn_rnd(ks * b.x); a.y += knn_rnd(ks * b.y); a.z += knn_rnd(ks * b.z);
}
/* distance, in cell units, from coordinate u (cell units) to cell c of an
 * axis with dim cells — the border cells extend to infinity (cell_axis
 * clamps) — less a 1e-3 margin that covers the float rounding of u and of the
 * photons' own d^2, so pruning with it never drops a photon that counts */
PMD float cell_gap(float u, uint32_t c, int dim) {
    const float lo = c == 0 ? -INFINITY : (float)c, hi = (int)c + 1 == dim ? INFINITY : (float)(c + 1);
    return fmaxf(fmaxf(lo - u, u - hi) - 1e-3f, 0.f);
}
/* max-heap of d^2 bits in LDS columns: entry k of this lane at h[k * KNN_BLOCK] */
PMD void heap_push(uint32_t *h, int n, uint32_t d) {
    int i = n;
    while (i > 0) {
        const int pa = (i - 1) >> 1;
        const uint32_t pd = h[pa * KNN_BLOCK];
        if (pd >= d) break;
        h[i * KNN_BLOCK] = pd;
        i = pa;
    }
    h[i * KNN_BLOCK] = d;
}
PMD void heap_replace_top(uint32_t *h, int n, uint32_t d) {
    int i = 0;
    while (true) {
        int c = 2 * i + 1;
        if (c >= n) break;
        uint32_t cd = h[c * KNN_BLOCK];
        if (c + 1 < n) {
            const uint32_t rd = h[(c + 1) * KNN_BLOCK];
            if (rd > cd) { c = c + 1; cd = rd; }
        }
        if (d >= cd) break;
        h[i * KNN_BLOCK] = cd;
        i = c;
    }
    h[i * KNN_BLOCK] = d;
}

/* the bucket rows around p within sqrt(maxd2), nearest rings first; bound()
 * (in world units^2) is re-read per row; visit(j, d2) per photon of the kept
 * cells. Returns nothing; COUNT census through vis / rows. */
struct KnnGrid {
    GridDesc g; /* a copy: a pointer into the kernel arguments would force them into scratch */
    uint32_t x0, x1, y0, y1, z0, z1;
    int cyc, czc, rings;
    float ux, uy, uz, inv2;
    PMD void init(const GridDesc &G, v3 p, float maxd2) {
        g = G;
        const float rq = sqrtf(maxd2) * 1.0001f + 1e-4f;
        x0 = cell_axis(p.x - rq, G.gx, G.inv_cs, G.dx); x1 = cell_axis(p.x + rq, G.gx, G.inv_cs, G.dx);
        y0 = cell_axis(p.y - rq, G.gy, G.inv_cs, G.dy); y1 = cell_axis(p.y + rq, G.gy, G.inv_cs, G.dy);
        z0 = cell_axis(p.z - rq, G.gz, G.inv_cs, G.dz); z1 = cell_axis(p.z + rq, G.gz, G.inv_cs, G.dz);
        cyc = (int)cell_axis(p.y, G.gy, G.inv_cs, G.dy); czc = (int)cell_axis(p.z, G.gz, G.inv_cs, G.dz);
        /* the query point in cell units (cell_axis before the floor) */
        ux = (p.x - G.gx) * G.inv_cs; uy = (p.y - G.gy) * G.inv_cs; uz = (p.z - G.gz) * G.inv_cs;
        inv2 = G.inv_cs * G.inv_cs;
        rings = max((int)(y1 - y0), (int)(z1 - z0));
    }
    template <class B, class V>
    PMD void scan(const uint32_t *cell_start, const float4 *ph_a, v3 p, B bound, V visit, unsigned long long &vis,
                  unsigned long long &rows) const {
        for (int ring = 0; ring <= rings; ++ring)
            for (uint32_t cz = z0; cz <= z1; ++cz)
                for (uint32_t cy = y0; cy <= y1; ++cy) {
                    if (max(abs((int)cy - cyc), abs((int)cz - czc)) != ring) continue;
                    const float gy = cell_gap(uy, cy, g.dy), gz = cell_gap(uz, cz, g.dz);
                    const float lim = bound() * inv2 - (gy * gy + gz * gz);
                    if (lim < 0.f) continue;
                    uint32_t xa = x0, xb = x1;
                    while (xa <= xb && sq(cell_gap(ux, xa, g.dx)) > lim) ++xa;
                    while (xb > xa && sq(cell_gap(ux, xb, g.dx)) > lim) --xb;
                    if (xa > xb) continue;
                    const uint32_t row = (cz * (uint32_t)g.dy + cy) * (uint32_t)g.dx;
                    const uint32_t b = cell_start[row + xa], e = cell_start[row + xb + 1];
                    vis += e - b; rows++;
                    for (uint32_t j = b; j < e; ++j) {
                        const float4 a = ph_a[j];
                        const v3 diff = p - xyz(a);
                        visit(j, a, diff.x * diff.x + diff.y * diff.y + diff.z * diff.z);
                    }
                }
    }
};

template <int COUNT>
__global__ __launch_bounds__(KNN_BLOCK) void k_gather_knn(GatherParams P) {
    extern __shared__ uint32_t kheap[]; /* [K][KNN_BLOCK] d^2 bits */
    const int K = P.knn_k;
    uint32_t *h = kheap + threadIdx.x;
    const int64_t r = P.rec_begin + (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
    unsigned long long vis = 0, hits = 0, rows = 0, act = 0;
    if (r < P.rec_end) {
        const float4 pos = P.R.pos[r];
        const uint32_t flags = (uint32_t)__float_as_int(pos.w);
        if (!(flags & (PM_REC_MISS | PM_REC_EXCEPTION | PM_REC_INVALID))) {
            float4 st = P.fresh ? make_float4(0.f, 0.f, 0.f, P.r2init) : P.R.state[r];
            const float4 nrm = P.R.nrm[r];
            const float4 m = P.materials[__float_as_int(nrm.w)];
            const float maxd2 = P.knn_r2;
            const v3 p = xyz(pos), ns = xyz(nrm);
            int cnt = 0;
            float md2 = maxd2;
            Kx3 acc{0, 0, 0};
            float sc = 1.f;
            bool nan = false;
            if (__float_as_int(m.w) == PM_MATTE) { /* non-specular BSDF components only */
                KnnGrid G;
                G.init(P.grid, p, maxd2);
                /* pass 1: r_k^2 */
                uint32_t topd = 0xffffffffu;
                G.scan(P.cell_start, P.ph_a, p, [&]() { return cnt == K ? __uint_as_float(topd) : maxd2; },
                       [&](uint32_t, const float4 &, float d2) {
                           if (!(d2 < maxd2)) return;
                           const uint32_t db = __float_as_uint(d2); /* d2 >= 0: bits order = value order */
                           if (cnt < K) {
                               heap_push(h, cnt, db);
                               if (++cnt == K) topd = h[0];
                           } else if (db < topd) {
                               heap_replace_top(h, K, db);
                               topd = h[0];
                           }
                       }, vis, rows);
                const bool full = cnt == K;
                if (full) md2 = __uint_as_float(topd);
                sc = md2 == 0.f ? 1.f : __uint_as_float(__float_as_uint(P.knn_fx * md2) & 0xff800000u); /* 2^n: exact */
                const bool back = (flags & PM_REC_BACKFACE) != 0;
                const float *phb = reinterpret_cast<const float *>(P.ph_b);
                /* contribution of photon j (LPhoton term) into a */
                const float inv = 1.f / md2;
                auto add = [&](Kx3 &a, uint32_t j, const float4 &pa, float d2) {
                    const float4 b0 = P.ph_b[2 * (size_t)j];
                    if (!knn_facing(ns, back, b0, pa.w, phb[8 * (size_t)j + 4])) return;
                    if (md2 == 0.f) { nan = true; return; } /* K photons at distance 0: kernel() is 0/0 */
                    knn_add(a, d2, inv, sc, b0);
                };
                /* pass 2: every photon below r_k^2 (all below maxD2 when not full);
                 * ties at r_k^2 aside */
                int less = 0, ties = 0;
                Kx3 acc_eq{0, 0, 0};
                G.scan(P.cell_start, P.ph_a, p, [&]() { return md2; },
                       [&](uint32_t j, const float4 &pa, float d2) {
                           if (d2 < md2) { less++; add(acc, j, pa, d2); }
                           else if (full && d2 == md2) { ties++; add(acc_eq, j, pa, d2); }
                       }, vis, rows);
                const int need = full ? K - less : 0;
                if (ties == need) {
                    acc.x += acc_eq.x; acc.y += acc_eq.y; acc.z += acc_eq.z;
                } else {
                    /* more photons at exactly r_k^2 than places: the lowest slots (rare) */
                    uint32_t last = 0u;
                    bool first = true;
                    for (int t = 0; t < need; ++t) {
                        uint32_t best = 0xffffffffu, bj = 0u;
                        float4 ba = make_float4(0.f, 0.f, 0.f, 0.f);
                        G.scan(P.cell_start, P.ph_a, p, [&]() { return md2; },
                               [&](uint32_t j, const float4 &pa, float d2) {
                                   if (d2 != md2) return;
                                   const uint32_t sl = __float_as_uint(phb[8 * (size_t)j + 5]);
                                   if ((first || sl > last) && sl <= best) { best = sl; bj = j; ba = pa; }
                               }, vis, rows);
                        add(acc, bj, ba, md2);
                        last = best;
                        first = false;
                    }
                }
                cnt = full ? K : less;
            }
            if (COUNT) { hits += (unsigned long long)cnt; act++; }
            const double isc = 1.0 / (double)sc;
            v3 L = mk((float)((double)acc.x * isc), (float)((double)acc.y * isc), (float)((double)acc.z * isc));
            if (nan) L = mk(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
            const v3 flux = xyz(st) + L;
            P.R.state[r] = make_float4(flux.x, flux.y, flux.z, md2);
            P.R.n[r] = (float)cnt;
        }
    }
    if (COUNT) count4(P.counters, vis, hits, rows, act);
}

/* ---------------------------------------------------------------------- */
/* kNN tile kernel (default kNN path): k_gather_knn's estimate, bit for bit
 * (same found set, r_k^2, per-record scale and exact sums), for the 64
 * records of an 8x8 tile at once.
 *  - Photon source: the wave stages the union of its lanes' bucket rows (each
 *    lane's box [p - maxD, p + maxD]) into LDS windows of KT_CAP photons with
 *    coalesced loads, as k_gather_tile does; every lane tests every staged
 *    photon against its own d^2 interval. The union is a superset of each
 *    lane's cells and anything at d^2 >= maxD^2 is dropped, so the found set
 *    is unchanged, and the scan loop is wave-uniform instead of 64 lanes
 *    walking their own rows with a divergent heap.
 *  - r_k^2 without a heap: the K-th smallest d^2 is selected exactly by
 *    passes over the same photons. HIST counts each lane's photons of its
 *    interval into 32 bins of a monotone bin function (float subtract,
 *    multiply, clamp, truncate: every step is monotone, so a bin is an
 *    interval of d^2 values) with one LDS add per photon; a prefix walk finds
 *    the bin holding the K-th. COLLECT then keeps that bin's values (<= 12,
 *    in LDS) with their min and max: <= 12 values are ranked directly, equal
 *    values are the answer, otherwise [min, max] is re-binned (the extremes
 *    land in bins 0 and 31, so every level shrinks the set). A deep or
 *    overflowing (>= 2^16 photons) search extracts minima one by one instead.
 *    A record with < K photons inside maxD (r_k^2 = maxD^2) goes from level
 *    0's HIST straight to its SUM pass.
 *  - HIST counts inline in the test loop (no per-hit loop); COLLECT, MIN and
 *    SUM lanes take their hits one per lane per iteration, COLLECT over the
 *    chosen bin's d^2 range only (conservative float bounds, exact bin test).
 *  - Incoherent tiles: k_gather_tile's groups (leader neighbourhoods); lanes
 *    left over in groups of < KT_GROUP_MIN run the same passes over their own
 *    rows from global memory. */
#ifndef PM_KT_CAP
#define PM_KT_CAP 64
#endif
/* C2 kNN: 12 -> 1.07 ms, 4 -> 0.99, 1 -> 0.95: every lane gets an LDS group
 * (its own if need be); per-lane passes remain for grids too coarse for the
 * row map */
#ifndef PM_KT_GROUP_MIN
#define PM_KT_GROUP_MIN 1
#endif
constexpr int KT_CAP = PM_KT_CAP;  /* photons per LDS window (one per lane) */
/* bins / kept values (C2 kNN, ms): 64/8 1.25, 48/8 1.12, 32/16 1.10, 24/12
 * 1.08, 32/10 1.07, 32/12 1.03 — 32/12 keeps the LDS at ~9.8 KB per wave
 * (4 waves/SIMD, the VGPR limit) with few re-binning passes */
#ifndef PM_KT_BINS
#define PM_KT_BINS 32
#endif
constexpr int KT_BINS = PM_KT_BINS; /* histogram bins per pass */
#ifndef PM_KT_LIST
#define PM_KT_LIST 12
#endif
constexpr int KT_LIST = PM_KT_LIST; /* values a COLLECT pass keeps per lane */
constexpr int KT_LEVELS = 4;       /* re-binning levels before minimum extraction */
constexpr uint32_t KT_GROUP_R = 1; /* lane boxes span <= 5 cells: a group's union <= 7 per axis */
constexpr int KT_GROUP_MIN = PM_KT_GROUP_MIN;
struct KnnLds {
    float x[KT_CAP + 4], y[KT_CAP + 4], z[KT_CAP + 4]; /* +4: the pair test reads one past the window */
    float4 b[KT_CAP];                                   /* alpha.rgb, wi.y */
    float w[KT_CAP], c[KT_CAP];                         /* wi.x, wi.z */
    int mark[KT_CAP];
    uint32_t hist[KT_BINS / 2][64]; /* two 16-bit counters per word, a column per lane */
    uint32_t list[KT_LIST][64];
};
#define PM_INLINE __attribute__((always_inline))
enum { KP_DONE = 0, KP_HIST = 1, KP_COLLECT = 2, KP_MIN = 3, KP_SUM = 4 };
PMD float next_up(float x) { return __uint_as_float(__float_as_uint(x) + 1u); } /* x >= 0, finite */
/* wave-uniform vector loads through the scalar cache (k_gather_knn_ss) */
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef const f32x16 __attribute__((address_space(4), aligned(4))) sv16;
typedef const f32x8 __attribute__((address_space(4), aligned(4))) sv8;
/* per-record fixed-point scale: the power of two below knn_fx * r_k^2 */
PMD float knn_scale(float fx, float md2) {
    return md2 == 0.f ? 1.f : __uint_as_float(__float_as_uint(fx * md2) & 0xff800000u);
}
/* one lane's selection state */
struct KnnSel {
    int phase = KP_DONE, level = 0, need = 0, kbin = 0;
    float blo = INFINITY, bhi = 0.f; /* this pass's hit interval [blo, bhi) */
    float lo = 0.f, s = 0.f;         /* bin function of HIST / COLLECT */
    uint32_t cntf = 0, cc = 0, tcnt = 0;
    float mn = INFINITY, mx = 0.f, tmin = INFINITY;
    float md2 = 0.f, sc = 1.f;
    int less = 0, ties = 0, cnt = 0;
    bool full = true, tiefix = false, nan = false, nan_eq = false;
    float inv = 0.f; /* 1 / r_k^2 */
    Kx3 acc{0, 0, 0};
    PMD int bin(float d2) const { return (int)fminf((d2 - lo) * s, (float)(KT_BINS - 1)); }
};

__global__ __launch_bounds__(KNN_BLOCK) void k_gather_knn_tile(GatherParams P) {
#ifdef PM_TILE_TIMES
    uint32_t tstat[8] = {0, 0, 0, 0, 0, 0, 0, 0}; /* TILE_STAT's sink (unused here) */
    (void)tstat;
#endif
    __shared__ KnnLds L;
    const int lane = threadIdx.x & 63;
    if (P.tiles && P.n_tiles_dev && (int64_t)blockIdx.x >= (int64_t)*P.n_tiles_dev) return; /* one wave per block */
    const int64_t r = P.rec_begin + (P.tiles ? (int64_t)P.tiles[blockIdx.x] * 64 + lane
                                             : (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x);
    const GridDesc &g = P.grid;
    GProf gp; /* PM_GATHER_PROFILE: record, pass setup, stage, test, hits, pass end, direct + store */
    gp.begin();
    const int K = P.knn_k;
    const float maxd2 = P.knn_r2;
#pragma unroll
    for (int w = 0; w < KT_BINS / 2; ++w) L.hist[w][lane] = 0u;
    /* record */
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
    const v3 p = xyz(pos), ns = xyz(nrm);
    uint32_t x0 = 0, x1 = 0, y0 = 0, y1 = 0, z0 = 0, z1 = 0;
    if (live) { /* KnnGrid::init's cells */
        const float rq = sqrtf(maxd2) * 1.0001f + 1e-4f;
        x0 = cell_axis(p.x - rq, g.gx, g.inv_cs, g.dx); x1 = cell_axis(p.x + rq, g.gx, g.inv_cs, g.dx);
        y0 = cell_axis(p.y - rq, g.gy, g.inv_cs, g.dy); y1 = cell_axis(p.y + rq, g.gy, g.inv_cs, g.dy);
        z0 = cell_axis(p.z - rq, g.gz, g.inv_cs, g.dz); z1 = cell_axis(p.z + rq, g.gz, g.inv_cs, g.dz);
    }
    KnnSel S;
    if (live) { S.phase = KP_HIST; S.need = K; S.blo = 0.f; S.bhi = maxd2; S.s = (float)KT_BINS / maxd2; }
    if (live && !(S.s <= 3.402823466e38f)) S.s = 3.402823466e38f;

    /* contribution of a found photon (pbrt kernel(), LPhoton diffuse term) into
     * a; returns true when it is pbrt's 0/0 (K photons at distance 0) */
    auto contrib = [&](Kx3 &a, float d2, const float4 &b, float wx, float wz) PM_INLINE {
        if (!knn_facing(ns, back, b, wx, wz)) return false;
        if (S.md2 == 0.f) return true;
        knn_add(a, d2, S.inv, S.sc, b);
        return false;
    };
    /* a photon inside this pass's interval; fl() -> its (b, wi.x, wi.z) */
    auto on_hit = [&](float d2, auto fl) PM_INLINE {
        switch (S.phase) {
        case KP_HIST: { /* per-lane passes only: the tile passes count inline */
            const int b = S.bin(d2);
            atomicAdd(&L.hist[b >> 1][lane], 1u << ((b & 1) * 16));
            S.cntf++;
            break;
        }
        case KP_COLLECT:
            if (S.bin(d2) == S.kbin) {
                if (S.cc < (uint32_t)KT_LIST) L.list[S.cc][lane] = __float_as_uint(d2);
                S.cc++;
                S.mn = fminf(S.mn, d2);
                S.mx = fmaxf(S.mx, d2);
            }
            break;
        case KP_MIN:
            if (d2 < S.tmin) { S.tmin = d2; S.tcnt = 1u; }
            else if (d2 == S.tmin) S.tcnt++;
            break;
        case KP_SUM: {
            float4 fb; float wx, wz;
            fl(fb, wx, wz);
            if (d2 < S.md2) { S.less++; S.nan |= contrib(S.acc, d2, fb, wx, wz); }
            else { /* d2 == r_k^2 (full lookups): the kernel is 0 there; only pbrt's 0/0 matters */
                S.ties++;
                if (S.md2 == 0.f) S.nan_eq |= knn_facing(ns, back, fb, wx, wz);
            }
            break;
        }
        default: break;
        }
    };
    auto begin_sum = [&]() PM_INLINE {
        S.sc = knn_scale(P.knn_fx, S.md2);
        S.inv = 1.f / S.md2;
        S.acc = Kx3{0, 0, 0};
        S.less = S.ties = 0;
        S.nan = S.nan_eq = false;
        S.blo = 0.f; S.bhi = S.full ? next_up(S.md2) : S.md2; /* not full: every d^2 < maxD^2 */
        S.phase = KP_SUM;
    };
    auto begin_min = [&](float lo_incl, float hi_excl) PM_INLINE {
        S.blo = lo_incl; S.bhi = hi_excl;
        S.tmin = INFINITY; S.tcnt = 0u;
        S.phase = KP_MIN;
    };
    /* end of a pass: the next phase */
    auto finish = [&]() PM_INLINE {
        switch (S.phase) {
        case KP_HIST: {
            if (S.level == 0) {
                if (S.cntf < (uint32_t)K) { /* fewer than K inside maxD: r_k^2 = maxD^2 */
                    S.full = false;
                    S.md2 = maxd2;
                    begin_sum();
                    break;
                }
                if (S.cntf >= 65536u) { begin_min(0.f, maxd2); break; } /* 16-bit bins may have wrapped */
            }
            uint32_t cum = 0u;
            bool found = false;
#pragma unroll
            for (int w = 0; w < KT_BINS / 2; ++w) {
                const uint32_t hw = L.hist[w][lane];
                L.hist[w][lane] = 0u;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const uint32_t c = (hw >> (16 * h)) & 0xffffu;
                    if (!found && cum + c >= (uint32_t)S.need) { found = true; S.kbin = 2 * w + h; }
                    else if (!found) cum += c;
                }
            }
            S.need -= (int)cum;
            S.cc = 0u; S.mn = INFINITY; S.mx = 0.f;
            /* the bin's d^2 range, widened: (d2 - lo) * s is within 2^-23
             * relative of exact, so bin k lies in lo + [k - 0.01, k + 1.01) / s,
             * and two ulps cover the rounding of that bound */
            if (S.kbin > 0) {
                const float cl = S.lo + ((float)S.kbin - 0.01f) / S.s;
                S.blo = fmaxf(S.blo, __uint_as_float(max((int)__float_as_uint(cl) - 2, 0)));
            }
            if (S.kbin < KT_BINS - 1) {
                const float ch = S.lo + ((float)S.kbin + 1.01f) / S.s;
                if (ch < 3.0e38f) S.bhi = fminf(S.bhi, next_up(next_up(ch)));
            }
            S.phase = KP_COLLECT; /* same bin function, exact bin test per hit */
            break;
        }
        case KP_COLLECT:
            if (S.cc <= (uint32_t)KT_LIST) { /* rank the kept values: the need-th smallest */
                uint32_t v[KT_LIST];
#pragma unroll
                for (int a = 0; a < KT_LIST; ++a) v[a] = (uint32_t)a < S.cc ? L.list[a][lane] : 0xffffffffu;
                uint32_t ans = v[0];
#pragma unroll
                for (int a = 0; a < KT_LIST; ++a) {
                    int lt = 0, le = 0;
#pragma unroll
                    for (int b = 0; b < KT_LIST; ++b) { lt += v[b] < v[a]; le += v[b] <= v[a]; }
                    if ((uint32_t)a < S.cc && lt < S.need && S.need <= le) ans = v[a];
                }
                S.md2 = __uint_as_float(ans);
                begin_sum();
            } else if (S.mn == S.mx) {
                S.md2 = S.mn;
                begin_sum();
            } else if (S.level >= KT_LEVELS) {
                begin_min(S.mn, next_up(S.mx));
            } else { /* re-bin [mn, mx] */
                S.level++;
                S.lo = S.mn;
                S.s = (float)KT_BINS / (S.mx - S.mn);
                if (!(S.s <= 3.402823466e38f)) S.s = 3.402823466e38f;
                S.blo = S.mn; S.bhi = next_up(S.mx);
                S.cntf = 0u;
                S.phase = KP_HIST;
            }
            break;
        case KP_MIN:
            if (S.tcnt == 0u || S.tcnt >= (uint32_t)S.need) { S.md2 = S.tcnt ? S.tmin : maxd2; begin_sum(); }
            else { S.need -= (int)S.tcnt; begin_min(next_up(S.tmin), S.bhi); }
            break;
        case KP_SUM:
            if (S.full) {
                /* K found: those below r_k^2 and K - less of the ties; the ties
                 * add 0 unless r_k^2 = 0, where the selected ones decide the NaN */
                if (S.ties == K - S.less) S.nan |= S.nan_eq;
                else if (S.md2 == 0.f) S.tiefix = true;
                S.cnt = K;
            } else {
                S.cnt = S.less;
            }
            S.phase = KP_DONE;
            break;
        default: break;
        }
    };

    const f2 px2 = {p.x, p.x}, py2 = {p.y, p.y}, pz2 = {p.z, p.z};
    bool pend = live, direct = false;
    gp.mark(0);
    while (true) {
        const unsigned long long pm = __ballot(pend);
        if (pm == 0ull) break;
        /* the group: every pending lane if the union box fits the 64-lane row
         * map, else the leader's neighbourhood (k_gather_tile) */
        uint32_t X0, X1, Y0, Y1, Z0, Z1;
        bool mine = pend;
        union_box6(g, mine, x0, x1, y0, y1, z0, z1, X0, X1, Y0, Y1, Z0, Z1);
        uint32_t LY = Y1 > Y0 ? 32u - (uint32_t)__builtin_clz(Y1 - Y0) : 0u;
        if (LY > 6u || ((uint64_t)(Z1 - Z0 + 1u) << LY) > 64u) {
            const int leader = __builtin_ctzll(pm);
            const uint32_t lx = __builtin_amdgcn_readlane(x0, leader), ly = __builtin_amdgcn_readlane(y0, leader),
                           lz = __builtin_amdgcn_readlane(z0, leader);
            mine = pend && x0 + KT_GROUP_R - lx <= 2u * KT_GROUP_R && y0 + KT_GROUP_R - ly <= 2u * KT_GROUP_R &&
                   z0 + KT_GROUP_R - lz <= 2u * KT_GROUP_R;
            if (__builtin_popcountll(__ballot(mine)) < KT_GROUP_MIN) {
                direct = direct || pend;
                break;
            }
            union_box6(g, mine, x0, x1, y0, y1, z0, z1, X0, X1, Y0, Y1, Z0, Z1);
            LY = Y1 > Y0 ? 32u - (uint32_t)__builtin_clz(Y1 - Y0) : 0u;
            if (LY > 6u || ((uint64_t)(Z1 - Z0 + 1u) << LY) > 64u) { /* a grid too coarse for the bound: per lane */
                direct = direct || pend;
                break;
            }
        }
        pend = pend && !mine;
        TILE_STAT(0, 1);
        /* passes until every lane of the group has its estimate */
        while (__ballot(mine && S.phase != KP_DONE)) {
            const bool act = mine && S.phase != KP_DONE;
            TILE_STAT(1, 1);
            /* this pass's union: the cells of [p - r', p + r'] for r'^2 = the
             * pass's upper bound (after level 0 mostly r_k^2, not maxD^2) —
             * a sub-box of the group's, so it fits the row map as well */
            uint32_t PX0 = X0, PX1 = X1, PY0 = Y0, PY1 = Y1, PZ0 = Z0, PZ1 = Z1, PLY = LY;
            {
                uint32_t a0 = 0, a1 = 0, b0 = 0, b1 = 0, c0 = 0, c1 = 0;
                if (act) {
                    const float rq = sqrtf(S.bhi) * 1.0001f + 1e-4f;
                    a0 = cell_axis(p.x - rq, g.gx, g.inv_cs, g.dx); a1 = cell_axis(p.x + rq, g.gx, g.inv_cs, g.dx);
                    b0 = cell_axis(p.y - rq, g.gy, g.inv_cs, g.dy); b1 = cell_axis(p.y + rq, g.gy, g.inv_cs, g.dy);
                    c0 = cell_axis(p.z - rq, g.gz, g.inv_cs, g.dz); c1 = cell_axis(p.z + rq, g.gz, g.inv_cs, g.dz);
                }
                uint32_t QX0, QX1, QY0, QY1, QZ0, QZ1;
                union_box6(g, act, a0, a1, b0, b1, c0, c1, QX0, QX1, QY0, QY1, QZ0, QZ1);
                const uint32_t QLY = QY1 > QY0 ? 32u - (uint32_t)__builtin_clz(QY1 - QY0) : 0u;
                if (QLY <= 6u && ((uint64_t)(QZ1 - QZ0 + 1u) << QLY) <= 64u) {
                    PX0 = QX0; PX1 = QX1; PY0 = QY0; PY1 = QY1; PZ0 = QZ0; PZ1 = QZ1; PLY = QLY;
                }
            }
            /* union row u = lane: photons [B, B + len) of cells PX0..PX1 */
            uint32_t B = 0u, len = 0u;
            const uint32_t cy = PY0 + ((uint32_t)lane & ((1u << PLY) - 1u)), cz = PZ0 + ((uint32_t)lane >> PLY);
            if (cy <= PY1 && cz <= PZ1) {
                const uint32_t row = (cz * (uint32_t)g.dy + cy) * (uint32_t)g.dx;
                B = P.cell_start[row + PX0];
                len = P.cell_start[row + PX1 + 1u] - B;
            }
            const uint32_t incl = wave_incl_sum_u32(len), pre = incl - len;
            const uint32_t U = uniform_u32(__builtin_amdgcn_readlane(incl, 63));
            const uint32_t gofs = B - pre;
            TILE_STAT(6, __builtin_popcountll(__ballot(act && S.phase == KP_MIN)));
            TILE_STAT(7, __builtin_popcountll(__ballot(act && S.phase == KP_HIST && S.level > 0)));
            const float blo = act ? S.blo : INFINITY, bhi = act ? S.bhi : 0.f;
            const bool hl = act && S.phase == KP_HIST; /* counts inline */
            const bool hist_any = __ballot(hl) != 0ull;
            const bool other_any = __ballot(act && !hl) != 0ull;
            /* the sums need the photons' flux and direction */
            const bool flux = __ballot(act && S.phase == KP_SUM) != 0ull;
            const f2 lo2 = {S.lo, S.lo}, s2 = {S.s, S.s};
            uint32_t cntf = 0u;
            auto window = [&](uint32_t n, auto DO_HIST, auto DO_OTHER) PM_INLINE {
                /* every lane tests every staged photon, two per packed step,
                 * 32 at a time: HIST lanes count them into their histogram on
                 * the spot, the others collect a hit mask and then take the
                 * hits one per lane per iteration */
                for (uint32_t vb = 0; vb < n; vb += 32) {
                    const uint32_t cnt = min(32u, n - vb);
                    uint32_t bits = 0u;
#pragma unroll 4
                    for (uint32_t j = 0; j < cnt; j += 2) {
                        const f2 ddx = px2 - f2{L.x[vb + j], L.x[vb + j + 1]}, ddy = py2 - f2{L.y[vb + j], L.y[vb + j + 1]},
                                 ddz = pz2 - f2{L.z[vb + j], L.z[vb + j + 1]};
                        const f2 d2 = (ddx * ddx + ddy * ddy) + ddz * ddz;
                        const bool hx = d2.x >= blo && d2.x < bhi && j < cnt, hy = d2.y >= blo && d2.y < bhi && j + 1 < cnt;
                        if (decltype(DO_HIST)::value) {
                            if (hl) {
                                /* S.bin of both, packed: the same IEEE operations.
                                 * Branch-free: a miss adds 0 to bin 0 */
                                const f2 bb = (d2 - lo2) * s2;
                                const int b0 = hx ? (int)fminf(bb.x, (float)(KT_BINS - 1)) : 0;
                                const int b1 = hy ? (int)fminf(bb.y, (float)(KT_BINS - 1)) : 0;
                                atomicAdd(&L.hist[b0 >> 1][lane], (uint32_t)hx << ((b0 & 1) * 16));
                                atomicAdd(&L.hist[b1 >> 1][lane], (uint32_t)hy << ((b1 & 1) * 16));
                                cntf += (uint32_t)hx + (uint32_t)hy;
                            }
                        }
                        if (decltype(DO_OTHER)::value) {
                            if (hx) bits |= 1u << j;
                            if (hy) bits |= 2u << j;
                        }
                    }
                    gp.mark(3);
                    if (decltype(DO_OTHER)::value) {
                        if (hl) bits = 0u;
                        TILE_STAT(4, wave_max_u32(__builtin_popcount(bits)));
                        while (bits) {
                            const uint32_t t = vb + (uint32_t)__builtin_ctz(bits);
                            bits &= bits - 1u;
                            const v3 diff = p - mk(L.x[t], L.y[t], L.z[t]);
                            const float d2 = diff.x * diff.x + diff.y * diff.y + diff.z * diff.z;
                            on_hit(d2, [&](float4 &fb, float &wx, float &wz) PM_INLINE { fb = L.b[t]; wx = L.w[t]; wz = L.c[t]; });
                        }
                    }
                }
            };
            gp.mark(1);
            /* software-pipelined staging (one photon per lane per window):
             * the next window's positions are requested before this window
             * is written to LDS and tested, so a window's load round trip
             * overlaps the previous window's tests; the flux words (SUM
             * passes only) are requested at the start of their own window.
             * Staging each window in turn: C2 kNN 0.954-0.975 ms against
             * 0.940-0.942 ms (docs/HISTORY.md, kNN tile kernel, round 3). */
            static_assert(KT_CAP == 64, "pipelined staging: one photon per lane per window");
            const float *phb = reinterpret_cast<const float *>(P.ph_b);
            /* photon index of this lane's position in window T0: its row from
             * a max scan over the row-start marks; past the union -> the
             * window's first photon (never read) */
            auto window_index = [&](uint32_t T0) PM_INLINE {
                L.mark[lane] = -1;
                wave_lds_sync();
                if (len > 0u) {
                    if (pre >= T0 && pre < T0 + KT_CAP) L.mark[pre - T0] = lane;
                    else if (pre < T0 && pre + len > T0) L.mark[0] = lane;
                }
                wave_lds_sync();
                const int u = wave_incl_max_i32(L.mark[lane]);
                const uint32_t gi = T0 + (uint32_t)lane + (uint32_t)__shfl((int)gofs, u);
                const uint32_t g0 = (uint32_t)__builtin_amdgcn_readlane((int)gi, 0);
                return (uint32_t)lane < min((uint32_t)KT_CAP, U - T0) ? gi : g0;
            };
            uint32_t jn = U > 0u ? window_index(0u) : 0u;
            float4 pan = U > 0u ? P.ph_a[jn] : make_float4(0.f, 0.f, 0.f, 0.f);
            for (uint32_t T0 = 0; T0 < U; T0 += KT_CAP) {
                const uint32_t n = min((uint32_t)KT_CAP, U - T0);
                TILE_STAT(2, 1);
                TILE_STAT(3, n);
                const uint32_t j = jn;
                const float4 pa = pan;
                float4 qa = make_float4(0.f, 0.f, 0.f, 0.f);
                float ca = 0.f;
                if (flux) { qa = P.ph_b[2 * (size_t)j]; ca = phb[8 * (size_t)j + 4]; }
                if (T0 + KT_CAP < U) {
                    jn = window_index(T0 + KT_CAP);
                    pan = P.ph_a[jn];
                }
                L.x[lane] = pa.x; L.y[lane] = pa.y; L.z[lane] = pa.z;
                if (flux) { L.w[lane] = pa.w; L.b[lane] = qa; L.c[lane] = ca; }
                wave_lds_sync();
                gp.mark(2);
                using T_ = std::true_type;
                using F_ = std::false_type;
                if (hist_any && other_any) window(n, T_{}, T_{});
                else if (hist_any) window(n, T_{}, F_{});
                else window(n, F_{}, T_{});
                gp.mark(4);
                wave_lds_sync(); /* the window is read before the next one overwrites it */
            }
            if (hl) S.cntf += cntf;
            if (act) finish();
            gp.mark(5);
        }
    }
    /* lanes of incoherent tiles: the same passes over their own rows */
    TILE_STAT(5, __builtin_popcountll(__ballot(direct)));
    KnnGrid G;
    unsigned long long nv = 0, nr = 0;
    if (__ballot(direct)) {
        if (direct) G.init(P.grid, p, maxd2);
        const float *phb = reinterpret_cast<const float *>(P.ph_b);
        while (__ballot(direct && S.phase != KP_DONE)) {
            if (direct && S.phase != KP_DONE) {
                G.scan(P.cell_start, P.ph_a, p, [&]() { return S.bhi; },
                       [&](uint32_t j, const float4 &a, float d2) {
                           if (!(d2 >= S.blo && d2 < S.bhi)) return;
                           on_hit(d2, [&](float4 &fb, float &wx, float &wz) PM_INLINE {
                               fb = P.ph_b[2 * (size_t)j]; wx = a.w; wz = phb[8 * (size_t)j + 4];
                           });
                       }, nv, nr);
                finish();
            }
        }
    }
    /* r_k^2 = 0 with more photons at the query point than places: the lowest
     * slots are the found ones (k_gather_knn's third scan) */
    if (__ballot(S.tiefix)) {
        if (S.tiefix) {
            if (!direct) G.init(P.grid, p, maxd2);
            const float *phb = reinterpret_cast<const float *>(P.ph_b);
            const int need = K - S.less;
            uint32_t last = 0u;
            bool first = true, nan = false;
            for (int t = 0; t < need; ++t) {
                uint32_t best = 0xffffffffu, bj = 0u;
                float4 ba = make_float4(0.f, 0.f, 0.f, 0.f);
                G.scan(P.cell_start, P.ph_a, p, [&]() { return S.md2; },
                       [&](uint32_t j, const float4 &a, float d2) {
                           if (d2 != S.md2) return;
                           const uint32_t sl = __float_as_uint(phb[8 * (size_t)j + 5]);
                           if ((first || sl > last) && sl <= best) { best = sl; bj = j; ba = a; }
                       }, nv, nr);
                nan |= knn_facing(ns, back, P.ph_b[2 * (size_t)bj], ba.w, phb[8 * (size_t)bj + 4]); /* r_k^2 = 0: 0/0 */
                last = best;
                first = false;
            }
            S.nan |= nan;
        }
    }
    if (active) {
        if (!live) S.md2 = maxd2; /* specular: nothing found, cnt 0 */
        const float4 st = P.fresh ? make_float4(0.f, 0.f, 0.f, P.r2init) : P.R.state[r];
        const double isc = 1.0 / (double)S.sc;
        v3 Lr = mk((float)((double)S.acc.x * isc), (float)((double)S.acc.y * isc), (float)((double)S.acc.z * isc));
        if (S.nan) Lr = mk(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
        const v3 flux = xyz(st) + Lr;
        P.R.state[r] = make_float4(flux.x, flux.y, flux.z, S.md2);
        P.R.n[r] = (float)S.cnt;
    }
    gp.mark(6);
    gp.flush(P.counters);
}

/* ---------------------------------------------------------------------- */
/* kNN scalar-stream kernel (round 4, the default kNN path): the estimate of
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
 * the 64-row map, r_k^2 = 0 (pbrt's 0/0 and its lowest-slot ties) — is
 * appended to P.knn_ovf and re-run by k_gather_knn_tile. */
/* waves per SIMD (VGPR budget; the 4.25 KB histogram allows 9): C2 kNN gather
 * 5 (81 VGPRs) 0.746-0.757 ms, 6 (73) 0.735, 7 (72) 0.747 (same box) */
#ifndef PM_KS_WAVES
#define PM_KS_WAVES 6
#endif
#define KS_OCC __attribute__((amdgpu_waves_per_eu(PM_KS_WAVES, PM_KS_WAVES)))
constexpr int KS_NB = 32;   /* bins per histogram level (+1 sink), 16-bit counters: two lanes per word */
constexpr int KS_HW = KS_NB / 2 + 1; /* LDS words per lane: (KS_NB + 1) 16-bit counters, or KS_LIST + 1 list rows + a sink row */
#ifndef PM_KS_LIST
#define PM_KS_LIST 12
#endif
constexpr int KS_LIST = PM_KS_LIST; /* values a COLLECT keeps per lane (rows 0..KS_LIST of the histogram, +1 scratch) */
/* (y, z) rows of a group's union box: two per lane. With 64, a tile across a
 * corner of the room (lanes on two walls, the union deeper than 8 x 8 rows)
 * split into leader groups, each running its own passes over nearly the same
 * photons: those tiles took up to 19 passes against 3.65 on average and set
 * the launch's length (tools/tile_times.py knn) */
#ifndef PM_KS_ROWS
#define PM_KS_ROWS 128
#endif
constexpr int KS_ROWS = PM_KS_ROWS;
static_assert(KS_ROWS == 64 || KS_ROWS == 128, "one or two union rows per lane");
enum { KS_HIST = 0, KS_COLLECT = 1, KS_SUM = 2, KS_DONE = 3 };
static_assert(KS_LIST + 1 < KS_HW, "the COLLECT list aliases histogram rows (not the sink's)");

/* photon pairs of the bucket order for the scalar stream: pair k = photons
 * 2k, 2k + 1, P block (x x y y z z wx wx), Q block (r r g g b b wy wy wz wz
 * . .); photons past the map are zero (the stream masks them). Block 0
 * thread 0 also clears the overflow-tile counter of this gather. */
__global__ __launch_bounds__(256) void k_knn_pack(const uint32_t *cell_start, uint32_t ncells, const float4 *ph_a,
                                                  const float4 *ph_b, float4 *pk_p, float4 *pk_q, int64_t npairs,
                                                  uint32_t *ovf_n) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < 64 && ovf_n) ovf_n[k] = 0u;
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
    if (live) { /* KnnGrid::init's cells */
        const float rq = sqrtf(maxd2) * 1.0001f + 1e-4f;
        x0 = cell_axis(p.x - rq, g.gx, g.inv_cs, g.dx); x1 = cell_axis(p.x + rq, g.gx, g.inv_cs, g.dx);
        y0 = cell_axis(p.y - rq, g.gy, g.inv_cs, g.dy); y1 = cell_axis(p.y + rq, g.gy, g.inv_cs, g.dy);
        z0 = cell_axis(p.z - rq, g.gz, g.inv_cs, g.dz); z1 = cell_axis(p.z + rq, g.gz, g.inv_cs, g.dz);
    }
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
        /* the group: every pending lane if their union box fits the 64-lane
         * row map, else the first pending lane's neighbourhood */
        uint32_t X0, X1, Y0, Y1, Z0, Z1;
        bool mine = pend;
        union_box6(g, mine, x0, x1, y0, y1, z0, z1, X0, X1, Y0, Y1, Z0, Z1);
        uint32_t LY = Y1 > Y0 ? 32u - (uint32_t)__builtin_clz(Y1 - Y0) : 0u;
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
            for (uint32_t GRk = KS_ROWS > 64 ? 4u : KT_GROUP_R; !fits && GRk >= KT_GROUP_R; GRk >>= 1) {
                mine = pend && x0 + GRk - lx <= 2u * GRk && y0 + GRk - ly <= 2u * GRk && z0 + GRk - lz <= 2u * GRk;
                union_box6(g, mine, x0, x1, y0, y1, z0, z1, X0, X1, Y0, Y1, Z0, Z1);
                LY = Y1 > Y0 ? 32u - (uint32_t)__builtin_clz(Y1 - Y0) : 0u;
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
            if (act) {
                const float rq = sqrtf(bnd) * 1.0001f + 1e-4f;
                a0 = cell_axis(p.x - rq, g.gx, g.inv_cs, g.dx); a1 = cell_axis(p.x + rq, g.gx, g.inv_cs, g.dx);
                b0 = cell_axis(p.y - rq, g.gy, g.inv_cs, g.dy); b1 = cell_axis(p.y + rq, g.gy, g.inv_cs, g.dy);
                c0 = cell_axis(p.z - rq, g.gz, g.inv_cs, g.dz); c1 = cell_axis(p.z + rq, g.gz, g.inv_cs, g.dz);
            }
            uint32_t PX0, PX1, PY0, PY1, PZ0, PZ1;
            union_box6(g, act, a0, a1, b0, b1, c0, c1, PX0, PX1, PY0, PY1, PZ0, PZ1);
            const uint32_t PLY = PY1 > PY0 ? 32u - (uint32_t)__builtin_clz(PY1 - PY0) : 0u;
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
            for (int h = 0; h < KS_ROWS / 64; ++h) {
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
            const unsigned long long rows = __ballot(Lu[0] > 0u), rows_hi = KS_ROWS > 64 ? __ballot(Lu[1] > 0u) : 0ull;
            /* 16-bit bin counters: a union of >= 2^16 photons goes to k_gather_knn_tile */
            if (uniform_u32(__builtin_amdgcn_readlane(wave_incl_sum_u32(Lu[0] + Lu[1]), 63)) >= 65536u) { defer = true; break; }
#ifdef PM_KNN_SS_DBG
            const unsigned long long rows0 = rows | rows_hi;
#endif
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
            /* one specialised loop per pass type over the rows' photon pairs */
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
#ifdef PM_KNN_SS_DBG
                if (ans == 0xffffffffu) {
                    const uint32_t i = atomicAdd(P.knn_ovf_n + 1, 1u);
                    if (i < 60u) {
                        uint32_t *d = P.knn_ovf_n + 64 + 16 * i;
                        d[0] = tile; d[1] = lane; d[2] = cc; d[3] = (uint32_t)need; d[4] = klo; d[5] = kw; d[6] = A;
                        d[7] = sh; d[8] = __float_as_uint(p.x); d[9] = __float_as_uint(p.y); d[10] = __float_as_uint(p.z);
                        d[11] = PX0; d[12] = PX1; d[13] = PY0 | (PY1 << 16); d[14] = PZ0 | (PZ1 << 16); d[15] = (uint32_t)__popcll(rows0);
                    }
                }
#endif
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
#ifdef PM_KNN_SS_DBG
    if (active && md2 != md2) atomicAdd(P.knn_ovf_n + 2, 1u);
#endif
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

hipError_t launch_gather_knn(const GatherParams &p, int count, hipStream_t s) {
    if (p.rec_end <= p.rec_begin) return hipSuccess;
    if (p.knn_k < 1 || p.knn_k > PM_KNN_MAX) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((p.rec_end - p.rec_begin + KNN_BLOCK - 1) / KNN_BLOCK);
    /* census launches run the per-lane kernel (its photons-tested count is the
     * per-record unit bench.py prices); the tile kernels find the same set */
    if (!count && p.kernel == PM_GK_TILE) {
        const unsigned g = p.tiles ? (unsigned)p.n_tiles : grid;
        if (!g) return hipSuccess;
        if (p.knn_pk_p && p.knn_r2 > 1e-30f) { /* the level-0 bins need bits(maxD^2) >= 32 << sh */
            /* scalar stream, then k_gather_knn_tile over the tiles it handed back */
            /* the pairs once per photon map (band gathers reuse them); the
             * overflow counters of every gather */
            const int64_t np = p.knn_pk_pairs;
            if (p.knn_pack)
                pm_launch(k_knn_pack, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, p.cell_start, p.grid.ncells,
                          p.ph_a, p.ph_b, p.knn_pk_p, p.knn_pk_q, np, p.knn_ovf_n);
            else {
                const hipError_t e = hipMemsetAsync(p.knn_ovf_n, 0, 64 * sizeof(uint32_t), s);
                if (e != hipSuccess) return e;
            }
            pm_launch(k_gather_knn_ss, dim3(g), dim3(64), 0, s, p);
            GatherParams q = p;
            q.tiles = p.knn_ovf;
            q.n_tiles_dev = p.knn_ovf_n;
            q.rec_begin = p.rec_begin;
            pm_launch(k_gather_knn_tile, dim3(g), dim3(KNN_BLOCK), 0, s, q);
            return hipGetLastError();
        }
        pm_launch(k_gather_knn_tile, dim3(g), dim3(KNN_BLOCK), 0, s, p);
        return hipGetLastError();
    }
    const uint32_t lds = (uint32_t)(p.knn_k * KNN_BLOCK * sizeof(uint32_t));
    if (count) pm_launch(k_gather_knn<1>, dim3(grid), dim3(KNN_BLOCK), lds, s, p);
    else pm_launch(k_gather_knn<0>, dim3(grid), dim3(KNN_BLOCK), lds, s, p);
    return hipGetLastError();
}

} // namespace pm
