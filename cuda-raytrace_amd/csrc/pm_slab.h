/*
 * pm_slab.h — what tests a box: the slab test and its two error terms, the
 * per-ray pad (RaySlab, ray_oinv_hi), and the quantized 4-wide and 8-wide
 * nodes' tests (QSlab, node4_test, node8_test). Included by pm_traverse.h.
 */
#pragma once
#include "pm_device.h"

#pragma clang fp contract(off)

namespace pm {

/* a missed box's entry distance */
constexpr float INF = __builtin_inff();

/* Slab test of one child box; returns tnear (INF = miss). */
/* t = (plane - o) / d as one FMA, plane * inv - o * inv (oinv precomputed per ray). The slab test only culls, and it
 * must never cull a box holding a hit the triangle test accepts. Its error has two parts: a few ulps of the plane
 * coordinate, which the commit pad of every primitive box (1e-4 max(1, |coordinate|), thousands of ulps of it)
 * covers, and a few ulps of o * inv, i.e. of the ray's *origin*, which that pad does not scale with: from an origin
 * 1e4 away an ulp of o is 1e-3, ten times the pad of a unit-sized scene. The second part is covered per ray:
 * ray_slab() / ray_oinv_hi() widen every box by pad = 2^-20 max|o| (16 ulps of the origin; the FMA, the product o *
 * inv and the <= 1 ulp reciprocal together stay below 4) through the two offsets oinv = (o + pad) * inv for the low
 * planes and oinvH = (o - pad) * inv for the high ones, at no cost per box. Tested for |o| <= 2^20, the bound
 * pm_set_eye_rays and pm_set_pinhole hold eye rays to. */
/* oinvH offsets the high planes: an instance tree widens every box by a pad of its own the same way (blas_isect) */
struct RaySlab { v3 inv, oinv; }; /* what a walk keeps of its ray: inv = 1 / d, oinv the low planes' offset */
PMD float box_near(float lx, float ly, float lz, float hx, float hy, float hz, const RaySlab &r, v3 oinvH, float tmin,
                   float tmax) {
    const v3 inv = r.inv, oinv = r.oinv;
    float t0x = __builtin_fmaf(lx, inv.x, -oinv.x), t1x = __builtin_fmaf(hx, inv.x, -oinvH.x);
    float t0y = __builtin_fmaf(ly, inv.y, -oinv.y), t1y = __builtin_fmaf(hy, inv.y, -oinvH.y);
    float t0z = __builtin_fmaf(lz, inv.z, -oinv.z), t1z = __builtin_fmaf(hz, inv.z, -oinvH.z);
    float tn = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fmaxf(fminf(t0z, t1z), tmin));
    float tf = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fminf(fmaxf(t0z, t1z), tmax));
    return tn <= tf ? tn : INF;
}

PMD v3 safe_inv(v3 d) {
    const float tiny = 1e-20f;
    float x = fabsf(d.x) < tiny ? copysignf(tiny, d.x) : d.x;
    float y = fabsf(d.y) < tiny ? copysignf(tiny, d.y) : d.y;
    float z = fabsf(d.z) < tiny ? copysignf(tiny, d.z) : d.z;
    /* hardware reciprocal (<= 1 ulp): the slab test only culls; an ulp in 1/d moves t = (plane - o) / d by an ulp of
     * the plane and of the origin, which the commit pad and the per-ray pad (ray_pad2) cover, so it never drops a box
     * holding the closest hit (which is order-independent) */
    return mk(__builtin_amdgcn_rcpf(x), __builtin_amdgcn_rcpf(y), __builtin_amdgcn_rcpf(z));
}
/* the per-ray box pad (box_near's comment): 2 * 2^-20 max|o| */
PMD float ray_pad2(v3 o) { return 0x1p-19f * fmaxf(fabsf(o.x), fmaxf(fabsf(o.y), fabsf(o.z))); }
/* the per-ray setup of every walk: oinv = (o + pad) * inv */
PMD RaySlab ray_slab(const Ray &ray) {
    RaySlab r;
    r.inv = safe_inv(ray.d);
    const float pad = 0.5f * ray_pad2(ray.o);
    r.oinv = mk((ray.o.x + pad) * r.inv.x, (ray.o.y + pad) * r.inv.y, (ray.o.z + pad) * r.inv.z);
    return r;
}
/* oinvH = (o - pad) * inv = oinv - 2 pad inv, the high planes' offset. Built anew at every node visit (a v_max3, a
 * multiply and these three FMAs) and not kept: three more live registers across the walk cost k_eye a wave of
 * occupancy and the pooled trace kernel scratch; the empty asm keeps the compiler from hoisting it out of the walk's
 * loop again. What it protects (gfx950, `make resource-usage`): k_trace_pool<0,0> / <0,1> 96 VGPRs with 28 / 104 B of
 * scratch, k_trace_pool8<0,0> 102 VGPRs, k_eye<MODE_GLOBAL> 113 VGPRs at 4 waves (kept hoisted, when this was
 * measured: k_eye at 3 waves, k_trace_pool<0,0> 52 B of scratch). If a compiler changes these, re-measure before
 * keeping it. */
PMD v3 ray_oinv_hi(const RaySlab &r, v3 o) {
    float pad2 = ray_pad2(o);
    asm volatile("" : "+v"(pad2));
    return mk(__builtin_fmaf(-pad2, r.inv.x, r.oinv.x), __builtin_fmaf(-pad2, r.inv.y, r.oinv.y),
              __builtin_fmaf(-pad2, r.inv.z, r.oinv.z));
}

/* a quantized node's box origin and steps (its first 16 B: o.xyz, then the exponent bytes) folded with the ray, for
 * both wide formats: the plane o + q 2^e and the slab (plane - O) / d folded: t = q a + b with a = 2^e / d, b = o / d
 * - O / d per node, one FMA per plane instead of a decode FMA and a slab FMA. Not the decoded plane's t bit for bit,
 * but within a few ulps of the plane coordinate (inside the commit pad of every primitive box) and of the ray's
 * origin (inside the per-ray pad carried by oinv / oinvH, see box_near): culling stays conservative; closest hits do
 * not depend on it. (Decoding each plane first and then box_near, the encoder's decode bit for bit, measured slower:
 * C3 trace 3.88 vs 3.93-3.96 ms, profiles/r05/trace_c3 qslab.) */
struct QSlab { float ax, ay, az, bx, by, bz, bxH, byH, bzH; };
PMD QSlab qslab(const uint4 w0, const RaySlab &r, const v3 &oinvH) {
    const v3 &oinv = r.oinv, &inv = r.inv;
    const float ox = __uint_as_float(w0.x), oy = __uint_as_float(w0.y), oz = __uint_as_float(w0.z);
    /* step 2^e: exponent field e + 127 = stored byte - 1 */
    const float sx = __uint_as_float(((w0.w & 0xffu) - 1u) << 23);
    const float sy = __uint_as_float((((w0.w >> 8) & 0xffu) - 1u) << 23);
    const float sz = __uint_as_float((((w0.w >> 16) & 0xffu) - 1u) << 23);
    QSlab q;
    q.ax = sx * inv.x; q.ay = sy * inv.y; q.az = sz * inv.z;
    q.bx = __builtin_fmaf(ox, inv.x, -oinv.x); q.by = __builtin_fmaf(oy, inv.y, -oinv.y);
    q.bz = __builtin_fmaf(oz, inv.z, -oinv.z);
    q.bxH = __builtin_fmaf(ox, inv.x, -oinvH.x); q.byH = __builtin_fmaf(oy, inv.y, -oinvH.y);
    q.bzH = __builtin_fmaf(oz, inv.z, -oinvH.z);
    return q;
}
/* one child box from the low bytes of its six quantized planes: whether the ray enters it within [tmin, tmax], and
 * the entry distance in tn */
PMD bool qslab_hit(const QSlab &q, uint32_t lx, uint32_t ly, uint32_t lz, uint32_t hx, uint32_t hy, uint32_t hz,
                   float tmin, float tmax, float &tn) {
    const float t0x = __builtin_fmaf((float)(lx & 0xffu), q.ax, q.bx);
    const float t0y = __builtin_fmaf((float)(ly & 0xffu), q.ay, q.by);
    const float t0z = __builtin_fmaf((float)(lz & 0xffu), q.az, q.bz);
    const float t1x = __builtin_fmaf((float)(hx & 0xffu), q.ax, q.bxH);
    const float t1y = __builtin_fmaf((float)(hy & 0xffu), q.ay, q.byH);
    const float t1z = __builtin_fmaf((float)(hz & 0xffu), q.az, q.bzH);
    tn = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fmaxf(fminf(t0z, t1z), tmin));
    const float tf = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fminf(fmaxf(t0z, t1z), tmax));
    return tn <= tf;
}

/* entry distances of the four children of 4-wide node `cur` (INF: missed) and their codes / counts, from its 64
 * quantized bytes (pm_build.h quantize_bvh4: each bound decodes as o + q * 2^e, a box containing the float one). The
 * one 4-wide format: 128-B float nodes were dropped after C3 trace 5.16 -> 4.75 ms per 1M paths (same box) for the
 * quantized ones: half the bytes per visit, 24 byte conversions more per node. */
PMD void node4_test(const SceneDev &S, int cur, const RaySlab &r, const v3 &oinvH, float tmin, float tmax, float t[4],
                    int c[4], int n[4]) {
    const uint4 *nd = reinterpret_cast<const uint4 *>(S.wnodes) + 4 * cur;
    const uint4 w0 = nd[0], w1 = nd[1], w2 = nd[2], w3 = nd[3];
    const QSlab q = qslab(w0, r, oinvH);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t sh = 8u * (uint32_t)k;
        float tn;
        t[k] = qslab_hit(q, w1.x >> sh, w1.y >> sh, w1.z >> sh, w1.w >> sh, w2.x >> sh, w2.y >> sh, tmin, tmax, tn) ? tn : INF;
    }
    c[0] = (int)w3.x; c[1] = (int)w3.y; c[2] = (int)w3.z; c[3] = (int)w3.w;
    n[0] = (int)(int16_t)(w2.z & 0xffffu); n[1] = (int)(int16_t)(w2.z >> 16);
    n[2] = (int)(int16_t)(w2.w & 0xffffu); n[3] = (int)(int16_t)(w2.w >> 16);
}

/* S.wide == 3 (round 6, pm_build.h quantize_bvh8): 128-B quantized nodes of eight children; the child word is the
 * internal node index (>= 0), INT_MIN for an empty slot, or a leaf ~((s << 5) | (tris << 4) | n). One visit tests
 * eight boxes: a third fewer node visits per ray than the 4-wide tree on C3's soup (tools/bvh_width_sim.cpp: 30.1 ->
 * 20.1), each a dependent fetch. */
constexpr int BVH8_EMPTY = (int)0x80000000;
PMD void node8_test(const SceneDev &S, int cur, const RaySlab &r, const v3 &oinvH, float tmin, float tmax, float t[8],
                    int c[8]) {
    const uint4 *nd = reinterpret_cast<const uint4 *>(S.wnodes) + 8 * cur;
    const uint4 w0 = nd[0], w1 = nd[1], w2 = nd[2], w3 = nd[3], w4 = nd[4], w5 = nd[5];
    const QSlab q = qslab(w0, r, oinvH);
    /* byte planes: lo x (w1.x, w1.y), lo y (w1.z, w1.w), lo z (w2.x, w2.y), hi x (w2.z, w2.w), hi y (w3.x, w3.y), hi
     * z (w3.z, w3.w) */
    const uint32_t LX[2] = {w1.x, w1.y}, LY[2] = {w1.z, w1.w}, LZ[2] = {w2.x, w2.y};
    const uint32_t HX[2] = {w2.z, w2.w}, HY[2] = {w3.x, w3.y}, HZ[2] = {w3.z, w3.w};
    c[0] = (int)w4.x; c[1] = (int)w4.y; c[2] = (int)w4.z; c[3] = (int)w4.w;
    c[4] = (int)w5.x; c[5] = (int)w5.y; c[6] = (int)w5.z; c[7] = (int)w5.w;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int h = k >> 2;
        const uint32_t sh = 8u * (uint32_t)(k & 3);
        float tn;
        t[k] = qslab_hit(q, LX[h] >> sh, LY[h] >> sh, LZ[h] >> sh, HX[h] >> sh, HY[h] >> sh, HZ[h] >> sh, tmin, tmax, tn) &&
                       c[k] != BVH8_EMPTY
                   ? tn : INF;
    }
}

} // namespace pm
