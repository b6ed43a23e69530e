/*
 * pm_gather_knn.hip — the kNN estimator (pbrt-v2 PhotonIntegrator::LPhoton)
 * over the photon buckets: the per-lane heap kernel (k_gather_knn, census
 * launches), the LDS tile kernel (k_gather_knn_tile: the fallback of the
 * default path, the scalar-stream kernel of pm_gather_knn_ss.hip) and
 * launch_gather_knn. All three kernels compute the same estimate bit for bit.
 *
 * wave64; 8x8 pixel tiles map onto one wave (see pm_gather.hip).
 */
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pm_kernels.h"
#include "pm_knn_dev.h"

#pragma clang fp contract(off)

namespace pm {
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
/* kNN tile kernel (the scalar stream's fallback): k_gather_knn's estimate, bit for bit
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
 *  - Incoherent tiles: k_gather_tile's groups (leader neighbourhoods), as
 *    small as the leader alone (KT_GROUP_MIN); on a grid too coarse for the
 *    row map the lanes run the same passes over their own rows from global
 *    memory. */
constexpr int KT_CAP = 64; /* photons per LDS window (one per lane: the pipelined staging) */
/* C2 kNN: 12 -> 1.07 ms, 4 -> 0.99, 1 -> 0.95: every lane gets an LDS group
 * (its own if need be); per-lane passes remain for grids too coarse for the
 * row map */
constexpr int KT_GROUP_MIN = 1; /* lanes a leader group needs: the leader is one, so no group is too small */
/* bins / kept values (C2 kNN, ms): 64/8 1.25, 48/8 1.12, 32/16 1.10, 24/12
 * 1.08, 32/10 1.07, 32/12 1.03 — 32/12 keeps the LDS at ~9.8 KB per wave
 * (4 waves/SIMD, the VGPR limit) with few re-binning passes */
constexpr int KT_BINS = 32;  /* histogram bins per pass */
constexpr int KT_LIST = 12;  /* values a COLLECT pass keeps per lane */
constexpr int KT_LEVELS = 4; /* re-binning levels before minimum extraction */
struct KnnLds {
    float x[KT_CAP + 4], y[KT_CAP + 4], z[KT_CAP + 4]; /* +4: the pair test reads one past the window */
    float4 b[KT_CAP];                                   /* alpha.rgb, wi.y */
    float w[KT_CAP], c[KT_CAP];                         /* wi.x, wi.z */
    int mark[KT_CAP];
    uint32_t hist[KT_BINS / 2][64]; /* two 16-bit counters per word, a column per lane */
    uint32_t list[KT_LIST][64];
};
enum { KP_DONE = 0, KP_HIST = 1, KP_COLLECT = 2, KP_MIN = 3, KP_SUM = 4 };
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
    if (live) { /* knn_cells, written out here and below: the call changes this kernel's code */
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
        uint32_t LY = rowmap_bits(Y0, Y1);
        if (LY > 6u || ((uint64_t)(Z1 - Z0 + 1u) << LY) > 64u) {
            const int leader = __builtin_ctzll(pm);
            const uint32_t lx = __builtin_amdgcn_readlane(x0, leader), ly = __builtin_amdgcn_readlane(y0, leader),
                           lz = __builtin_amdgcn_readlane(z0, leader);
            mine = pend && x0 + KT_GROUP_R - lx <= 2u * KT_GROUP_R && y0 + KT_GROUP_R - ly <= 2u * KT_GROUP_R &&
                   z0 + KT_GROUP_R - lz <= 2u * KT_GROUP_R;
            /* never taken (the leader is in its own group), which the compiler
             * does not see: without it the kernel's code changes */
            if (__builtin_popcountll(__ballot(mine)) < KT_GROUP_MIN) {
                direct = direct || pend;
                break;
            }
            union_box6(g, mine, x0, x1, y0, y1, z0, z1, X0, X1, Y0, Y1, Z0, Z1);
            LY = rowmap_bits(Y0, Y1);
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
                const uint32_t QLY = rowmap_bits(QY0, QY1);
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
            const hipError_t e = launch_knn_ss(p, g, s);
            if (e != hipSuccess) return e;
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
