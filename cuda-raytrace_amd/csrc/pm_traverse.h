/*
 * pm_traverse.h — closest-hit and any-hit ray queries: the slab test and the
 * per-ray pad, the census hooks, the brute-force pair test, the leaf test,
 * the binary walk (traverse), the quantized 4-wide walk (traverse4, the
 * instance walk blas_isect, and the resumable trav_step of the pooled trace
 * kernel) and the 8-wide walk. Included only by the units that trace rays:
 * pm_trace.hip and pm_eye.hip.
 */
#pragma once
#include "pm_isect.h"

#pragma clang fp contract(off)

namespace pm {

/* ---------------------------------------------------------- traversal */
/* Slab test of one child box; returns tnear (inf = miss). */
/* t = (plane - o) / d as one FMA, plane * inv - o * inv (oinv precomputed per
 * ray). The slab test only culls, and it must never cull a box holding a hit
 * the triangle test accepts. Its error has two parts: a few ulps of the plane
 * coordinate, which the commit pad of every primitive box (1e-4 max(1,
 * |coordinate|), thousands of ulps of it) covers, and a few ulps of o * inv,
 * i.e. of the ray's *origin*, which that pad does not scale with: from an
 * origin 1e4 away an ulp of o is 1e-3, ten times the pad of a unit-sized
 * scene. The second part is covered per ray: ray_oinv() / ray_oinv_hi() widen every box by
 * pad = 2^-20 max|o| (16 ulps of the origin; the FMA, the product o * inv and
 * the <= 1 ulp reciprocal together stay below 4) through the two offsets
 * oinv = (o + pad) * inv for the low planes and oinvH = (o - pad) * inv for
 * the high ones, at no cost per box. Tested for |o| <= 2^20, the bound
 * pm_set_eye_rays and pm_set_pinhole hold eye rays to. */
/* slab test; oinvH (default oinv) offsets the high planes: an instance tree
 * widens every box by a pad with oinv = (o' + pad) * inv, oinvH = (o' - pad)
 * * inv at no cost per box (blas_isect) */
PMD float box_near(float lx, float ly, float lz, float hx, float hy, float hz, v3 oinv, v3 inv, float tmin,
                   float tmax, v3 oinvH) {
    float t0x = __builtin_fmaf(lx, inv.x, -oinv.x), t1x = __builtin_fmaf(hx, inv.x, -oinvH.x);
    float t0y = __builtin_fmaf(ly, inv.y, -oinv.y), t1y = __builtin_fmaf(hy, inv.y, -oinvH.y);
    float t0z = __builtin_fmaf(lz, inv.z, -oinv.z), t1z = __builtin_fmaf(hz, inv.z, -oinvH.z);
    float tn = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fmaxf(fminf(t0z, t1z), tmin));
    float tf = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fminf(fmaxf(t0z, t1z), tmax));
    return tn <= tf ? tn : __int_as_float(0x7f800000);
}
PMD float box_near(float lx, float ly, float lz, float hx, float hy, float hz, v3 oinv, v3 inv, float tmin,
                   float tmax) {
    return box_near(lx, ly, lz, hx, hy, hz, oinv, inv, tmin, tmax, oinv);
}

PMD v3 safe_inv(v3 d) {
    const float tiny = 1e-20f;
    float x = fabsf(d.x) < tiny ? copysignf(tiny, d.x) : d.x;
    float y = fabsf(d.y) < tiny ? copysignf(tiny, d.y) : d.y;
    float z = fabsf(d.z) < tiny ? copysignf(tiny, d.z) : d.z;
    /* hardware reciprocal (<= 1 ulp): the slab test only culls; an ulp in 1/d
     * moves t = (plane - o) / d by an ulp of the plane and of the origin,
     * which the commit pad and the per-ray pad (ray_pad2) cover, so it never
     * drops a box holding the closest hit (which is order-independent) */
    return mk(__builtin_amdgcn_rcpf(x), __builtin_amdgcn_rcpf(y), __builtin_amdgcn_rcpf(z));
}
/* the per-ray box pad (box_near's comment): 2 * 2^-20 max|o| */
PMD float ray_pad2(v3 o) { return 0x1p-19f * fmaxf(fabsf(o.x), fmaxf(fabsf(o.y), fabsf(o.z))); }
/* oinv = (o + pad) * inv, the low planes' offset */
PMD v3 ray_oinv(v3 o, v3 inv, float pad2) {
    const float pad = 0.5f * pad2;
    return mk((o.x + pad) * inv.x, (o.y + pad) * inv.y, (o.z + pad) * inv.z);
}
/* oinvH = (o - pad) * inv = oinv - 2 pad inv, the high planes' offset. Built
 * anew at every node visit (a v_max3, a multiply and these three FMAs) and not
 * kept: three more live registers across the walk cost k_eye a wave of
 * occupancy and the pooled trace kernel scratch; the empty asm keeps the
 * compiler from hoisting it out of the walk's loop again. What it protects
 * (gfx950, `make resources`): k_trace_pool<0,0> / <0,1> 96 VGPRs with 28 /
 * 108 B of scratch, k_trace_pool8<0,0> 102 VGPRs, k_eye<MODE_GLOBAL> 125
 * VGPRs at 4 waves (kept hoisted: 129 at 3 waves; k_trace_pool<0,0> 52 B
 * of scratch). If a compiler changes these, re-measure before keeping it. */
PMD v3 ray_oinv_hi(v3 oinv, v3 inv, v3 o) {
    float pad2 = ray_pad2(o);
    asm volatile("" : "+v"(pad2));
    return mk(__builtin_fmaf(-pad2, inv.x, oinv.x), __builtin_fmaf(-pad2, inv.y, oinv.y), __builtin_fmaf(-pad2, inv.z, oinv.z));
}

/* per-lane traversal census (bench roofline / DESIGN.md): nodes entered and
 * primitive tests; NoCensus compiles to nothing */
struct NoCensus { PMD void node() {} PMD void prim() {} };
struct Census {
    uint32_t nodes = 0, prims = 0;
    PMD void node() { ++nodes; }
    PMD void prim() { ++prims; }
};

/* closest hit so far: smaller t wins, equal t -> lowest global primitive id
 * (callers pass only t <= best.t), so the result is independent of the order
 * primitives are tested in (BVH or brute force) */
PMD void consider(Hit &best, float t, float b, float g, uint32_t ref, uint32_t gid) {
    if (t < best.t || gid < best.gid) { best.t = t; best.beta = b; best.gamma = g; best.ref = ref; best.gid = gid; }
}

/* a query starts with no hit: t at the ray's far end, no primitive */
PMD void best_begin(Hit &best, float tmax) {
    best.t = tmax;
    best.gid = 0xffffffffu;
    best.ref = 0xffffffffu;
}

/* MODE_BRUTE: every primitive, wave-uniform loop (same primitive in every
 * lane: broadcast LDS reads, no divergence, no stack) */
/* 16 B through the scalar cache (wave-uniform address; const_f32_ptr: pm_math.h) */
PMD float4 ldc4(const_f32_ptr q) { return make_float4(q[0], q[1], q[2], q[3]); }

typedef float f2 __attribute__((ext_vector_type(2)));
PMD f2 bc2(float x) { return f2{x, x}; }

/* isect_tri_v for two triangles at once (packed v_pk_mul/add_f32): the same
 * per-component IEEE operations in the same order, so each lane of the pair is
 * bit-identical to the scalar test. */
/* two triangles' (p0, e0, e1, n) as packed pairs, wave-uniform */
struct TriPair { f2 p0x, p0y, p0z, e0x, e0y, e0z, e1x, e1y, e1z, nx, ny, nz; };
/* the ray's origin and direction as packed splats. The components pass
 * through an empty asm first: splatting a value loaded from the path state
 * otherwise became a <2 x float> load of the state, which kept the ray in
 * scratch memory (5 scratch loads per ray in k_trace_lane) */
struct RaySplat { f2 ox, oy, oz, dx, dy, dz; };
PMD RaySplat splat_ray(const Ray &r) {
    float ox = r.o.x, oy = r.o.y, oz = r.o.z, dx = r.d.x, dy = r.d.y, dz = r.d.z;
    asm("" : "+v"(ox), "+v"(oy), "+v"(oz), "+v"(dx), "+v"(dy), "+v"(dz));
    return RaySplat{bc2(ox), bc2(oy), bc2(oz), bc2(dx), bc2(dy), bc2(dz)};
}
PMD void isect_tri_pair(const TriPair &q, const RaySplat &ray, f2 &t, f2 &beta, f2 &gamma) {
    const f2 p0x = q.p0x, p0y = q.p0y, p0z = q.p0z, e0x = q.e0x, e0y = q.e0y, e0z = q.e0z;
    const f2 e1x = q.e1x, e1y = q.e1y, e1z = q.e1z, nx = q.nx, ny = q.ny, nz = q.nz;
    const f2 dx = ray.dx, dy = ray.dy, dz = ray.dz;
    const f2 den = (nx * dx + ny * dy) + nz * dz; /* dot(n, d) */
    /* rcp_exact of both, one range check for the pair (either outside
     * [2^-125, 2^125): both divide; a NaN passes the check and gives NaN
     * either way) and the Newton step as two packed FMAs */
    const f2 r0 = f2{__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
    f2 inv = __builtin_elementwise_fma(__builtin_elementwise_fma(-den, r0, bc2(1.0f)), r0, r0);
    const float alo = fminf(fabsf(den.x), fabsf(den.y)), ahi = fmaxf(fabsf(den.x), fabsf(den.y));
    if (__builtin_expect(!(alo >= 0x1p-125f) | !(ahi < 0x1p125f), 0)) { inv.x = 1.0f / den.x; inv.y = 1.0f / den.y; }
    const f2 e2x = inv * (p0x - ray.ox), e2y = inv * (p0y - ray.oy), e2z = inv * (p0z - ray.oz);
    const f2 ix = dy * e2z - dz * e2y, iy = dz * e2x - dx * e2z, iz = dx * e2y - dy * e2x; /* cross(d, e2) */
    beta = (ix * e1x + iy * e1y) + iz * e1z;
    gamma = (ix * e0x + iy * e0y) + iz * e0z;
    t = (nx * e2x + ny * e2y) + nz * e2z;
}

/* Brute-force scenes store their triangles in global-id order (pm_api.cpp
 * build_scene), and triangles, disks, spheres are tested in that order, which
 * is ascending global id: a strict t < best.t keeps the first of equal-t hits
 * = the lowest id, the same hit consider() picks in any order — no id loads
 * in the loop. best.gid is left unset (nothing after the query reads it). */
PMD void take(Hit &best, float t, float b, float g, uint32_t ref) {
    best.t = t; best.beta = b; best.gamma = g; best.ref = ref;
}
/* a pair of SceneDev::tri_pairs_g: component c of triangle h at q[2c + h] */
PMD TriPair load_pair_il(const_f32_ptr q) {
    TriPair t;
    t.p0x = f2{q[0], q[1]}; t.p0y = f2{q[2], q[3]}; t.p0z = f2{q[4], q[5]};
    t.e0x = f2{q[6], q[7]}; t.e0y = f2{q[8], q[9]}; t.e0z = f2{q[10], q[11]};
    t.e1x = f2{q[12], q[13]}; t.e1y = f2{q[14], q[15]}; t.e1z = f2{q[16], q[17]};
    t.nx = f2{q[18], q[19]}; t.ny = f2{q[20], q[21]}; t.nz = f2{q[22], q[23]};
    return t;
}
template <bool ANY, class C>
PMD bool brute_isect(const SceneDev &S, const Ray &ray, Hit &best, C &cen) {
    const const_f32_ptr tg = (const_f32_ptr)S.tri_geo_g; /* constant address space: s_load */
    const RaySplat rs = splat_ray(ray);
    int k = 0;
    /* (software-pipelining the next pair's scalar loads measured slower:
     * C2 trace 91 vs 86 us — more live SGPRs, no unroll; so did pipelined
     * vector loads of the pairs into VGPRs: 73.5 -> 99 us, 111 VGPRs) */
    /* the running best in locals (one register per field: with the Hit
     * reference the compiler kept best.t twice, one more move per hit) */
    float bt = best.t, bb = best.beta, bg = best.gamma;
    uint32_t bref = best.ref;
#pragma unroll 2
    for (; k + 1 < S.n_tris; k += 2) {
        cen.prim(); cen.prim();
        f2 t, b, g;
        isect_tri_pair(load_pair_il((const_f32_ptr)S.tri_pairs_g + 12 * k), rs, t, b, g); /* pair k / 2: 24 floats */
        /* closest hit: t < best.t <= ray.tmax (traverse starts best.t at
         * tmax) implies t < tmax, so only the any-hit query tests tmax */
        const bool ok0 = (!ANY || t.x < ray.tmax) & (t.x > ray.tmin) & (b.x >= 0.0f) & (g.x >= 0.0f) & (b.x + g.x <= 1);
        const bool ok1 = (!ANY || t.y < ray.tmax) & (t.y > ray.tmin) & (b.y >= 0.0f) & (g.y >= 0.0f) & (b.y + g.y <= 1);
        if (ANY) { if (ok0 | ok1) return true; continue; }
        if (ok0 && t.x < bt) { bt = t.x; bb = b.x; bg = g.x; bref = (PRIM_TRI << 30) | (uint32_t)k; }
        if (ok1 && t.y < bt) { bt = t.y; bb = b.y; bg = g.y; bref = (PRIM_TRI << 30) | (uint32_t)(k + 1); }
    }
    if (!ANY) { best.t = bt; best.beta = bb; best.gamma = bg; best.ref = bref; }
    if (k < S.n_tris) {
        cen.prim();
        float t, b, g;
        const const_f32_ptr q = tg + 12 * k;
        const float4 a = make_float4(q[0], q[1], q[2], q[3]), bb = make_float4(q[4], q[5], q[6], q[7]),
                     cc = make_float4(q[8], q[9], q[10], q[11]);
        const bool ok = isect_tri_v(a, bb, cc, ray, &t, &b, &g);
        if (ANY && ok) return true;
        if (!ANY && ok && t < best.t) take(best, t, b, g, (PRIM_TRI << 30) | (uint32_t)k);
    }
    for (int k = 0; k < S.n_disks; ++k) {
        cen.prim();
        float t;
        const bool ok = isect_disk(S.disks + 5 * k, ray, &t);
        if (ANY) { if (ok) return true; continue; }
        if (ok && t < best.t) take(best, t, 0.f, 0.f, (PRIM_DISK << 30) | (uint32_t)k);
    }
    for (int k = 0; k < S.n_spheres; ++k) {
        cen.prim();
        float t;
        const bool ok = isect_sphere(S.spheres + 4 * k, ray, &t);
        if (ANY) { if (ok) return true; continue; }
        if (ok && t < best.t) take(best, t, 0.f, 0.f, (PRIM_SPHERE << 30) | (uint32_t)k);
    }
    return false;
}

/* Tests the primitives of one leaf; for ANY=true returns at the first hit.
 * TRIRUN: the leaf comes from a quantized wide node, whose count may carry
 * pm_build.h's LEAF_TRIS flag (only quantize_bvh4 / quantize_bvh8 set it;
 * binary leaves are always decoded through their refs, whatever their size). */
template <bool ANY, class C>
PMD bool blas_isect(const SceneDev &S, uint32_t inst, const Ray &ray, Hit &best, int *stack, int stride, C &cen);
/* INST: the leaf's refs may be instances (MODE_INST), whose trees are walked
 * with the stack entries above the caller's (stack, stride) */
template <bool ANY, bool TRIRUN = false, class C, bool INST = false>
PMD bool leaf_isect(const SceneDev &S, uint32_t start, uint32_t count, const Ray &ray, Hit &best, C &cen,
                    int *istack = nullptr, int istride = 0) {
    if (TRIRUN && (count & 0x4000u)) { /* LEAF_TRIS: triangles at storage slots [start, start + n), no refs */
        for (uint32_t idx = start; idx < start + (count & 0x3fffu); ++idx) {
            cen.prim();
            float t, b, g;
            const bool ok = isect_tri(S.tri_geo + 3 * idx, ray, &t, &b, &g);
            if (ANY) { if (ok) return true; continue; }
            if (!ok || t > best.t) continue;
            const uint32_t gid = S.tri_id[idx];
            if (t < best.t || gid < best.gid) {
                best.t = t; best.beta = b; best.gamma = g; best.ref = (PRIM_TRI << 30) | idx; best.gid = gid;
            }
        }
        return false;
    }
    for (uint32_t k = start; k < start + count; ++k) {
        cen.prim();
        uint32_t ref = S.refs[k];
        uint32_t kind = ref >> 30, idx = ref & 0x3fffffffu;
        float t, b = 0.f, g = 0.f;
        bool ok;
        uint32_t gid;
        if (INST && kind == PRIM_INST) {
            if (blas_isect<ANY>(S, idx, ray, best, istack, istride, cen) && ANY) return true;
            continue;
        }
        if (kind == PRIM_TRI) {
            ok = isect_tri(S.tri_geo + 3 * idx, ray, &t, &b, &g);
            if (ANY) { if (ok) return true; continue; }
            if (!ok || t > best.t) continue;
            gid = S.tri_id[idx];
        } else if (kind == PRIM_DISK) {
            ok = isect_disk(S.disks + 5 * idx, ray, &t);
            if (ANY) { if (ok) return true; continue; }
            if (!ok || t > best.t) continue;
            gid = (uint32_t)fbits(S.disks[5 * idx + 4].w);
        } else {
            ok = isect_sphere(S.spheres + 4 * idx, ray, &t);
            if (ANY) { if (ok) return true; continue; }
            if (!ok || t > best.t) continue;
            gid = (uint32_t)fbits(S.spheres[4 * idx + 3].w);
        }
        if (t < best.t || gid < best.gid) { /* t <= best.t here: ties -> lowest id */
            best.t = t; best.beta = b; best.gamma = g; best.ref = ref; best.gid = gid;
        }
    }
    return false;
}

/* BVH traversal with a per-lane stack column in LDS (stack[depth*stride]).
 * Closest hit (ANY=false) or occlusion (ANY=true). Node = 4 float4:
 * (l.lo, l.hi.x) (l.hi.yz, r.lo.xy) (r.lo.z, r.hi) (left, right, lcount, rcount);
 * child >= 0 internal node, child < 0 leaf with refs start ~child. */
template <bool ANY, class C, bool INST = false>
PMD bool traverse4(const SceneDev &S, const Ray &ray, Hit &best, int *stack, int stride, C &cen);
template <bool ANY, class C>
PMD bool traverse8(const SceneDev &S, const Ray &ray, Hit &best, int *stack, int stride, C &cen);

template <bool ANY, int MODE, class C>
PMD bool traverse(const SceneDev &S, const Ray &ray, Hit &best, int *stack, int stride, C &cen) {
    best_begin(best, ray.tmax);
    const v3 inv = safe_inv(ray.d);
    const v3 oinv = ray_oinv(ray.o, inv, ray_pad2(ray.o));
    int sp = 0;
    int cur = 0; /* next node to enter; -1: none left */
    /* Leaves found while descending are postponed (at most the two children of
     * one node) and tested in a separate loop, so a wave runs the primitive
     * code once for all lanes that reached leaves instead of once per node
     * iteration for a few of them (Aila & Laine's "while-while"). Culling is
     * unchanged: a postponed leaf's box was hit within the current best t. */
    if constexpr (MODE == MODE_BRUTE) {
        cen.node();
        if (brute_isect<ANY>(S, ray, best, cen)) return true;
        return ANY ? false : best.ref != 0xffffffffu;
    }
    if constexpr (MODE == MODE_INST) {
        return traverse4<ANY, C, true>(S, ray, best, stack, stride, cen);
    } else if constexpr (MODE == MODE_GLOBAL) {
        if (S.wide == 3) return traverse8<ANY>(S, ray, best, stack, stride, cen);
        if (S.wide) return traverse4<ANY>(S, ray, best, stack, stride, cen);
    }
    uint32_t l0s = 0, l0n = 0, l1s = 0, l1n = 0; /* pending leaves: first ref, count (0 = none) */
    int guard = 0; /* every node is entered at most once per ray: a bound every lane reaches */
    while (true) {
        while (cur >= 0 && l0n == 0 && guard <= S.n_nodes) {
            ++guard;
            cen.node();
            const float4 *nd = S.nodes + 4 * cur;
            float4 a = nd[0], b = nd[1], c = nd[2];
            int4 ch = *reinterpret_cast<const int4 *>(nd + 3);
            const v3 oinvH = ray_oinv_hi(oinv, inv, ray.o);
            float tl = box_near(a.x, a.y, a.z, a.w, b.x, b.y, oinv, inv, ray.tmin, best.t, oinvH);
            float tr = box_near(b.z, b.w, c.x, c.y, c.z, c.w, oinv, inv, ray.tmin, best.t, oinvH);
            bool hl = tl != __int_as_float(0x7f800000) && ch.z >= 0;
            bool hr = tr != __int_as_float(0x7f800000) && ch.w >= 0;
            if (hl && ch.x < 0) { l0s = (uint32_t)~ch.x; l0n = (uint32_t)ch.z; hl = false; }
            if (hr && ch.y < 0) {
                if (l0n == 0) { l0s = (uint32_t)~ch.y; l0n = (uint32_t)ch.w; }
                else { l1s = (uint32_t)~ch.y; l1n = (uint32_t)ch.w; }
                hr = false;
            }
            if (hl && hr && sp < S.stack_depth) {
                int nearc = ch.x, farc = ch.y;
                if (tr < tl) { nearc = ch.y; farc = ch.x; }
                stack[sp * stride] = farc;
                ++sp;
                cur = nearc;
            } else if (hl) {
                cur = ch.x;
            } else if (hr) {
                cur = ch.y;
            } else if (sp > 0) {
                --sp;
                cur = stack[sp * stride];
            } else {
                cur = -1;
            }
        }
        while (l0n != 0) {
            if (leaf_isect<ANY>(S, l0s, l0n, ray, best, cen)) return true;
            l0s = l1s; l0n = l1n; l1n = 0;
        }
        if (cur < 0 || guard > S.n_nodes) break;
    }
    return ANY ? false : best.ref != 0xffffffffu;
}
/* a quantized node's box origin and steps (its first 16 B: o.xyz, then the
 * exponent bytes) folded with the ray, for both wide formats:
 * the plane o + q 2^e and the slab (plane - O) / d folded: t = q a + b
 * with a = 2^e / d, b = o / d - O / d per node, one FMA per plane
 * instead of a decode FMA and a slab FMA. Not the decoded plane's t
 * bit for bit, but within a few ulps of the plane coordinate (inside
 * the commit pad of every primitive box) and of the ray's origin
 * (inside the per-ray pad carried by oinv / oinvH, see box_near):
 * culling stays conservative; closest hits do not depend on it.
 * (Decoding each plane first and then box_near, the encoder's decode bit
 * for bit, measured slower: C3 trace 3.88 vs 3.93-3.96 ms,
 * profiles/r05/trace_c3 qslab.) */
struct QSlab { float ax, ay, az, bx, by, bz, bxH, byH, bzH; };
PMD QSlab qslab(const uint4 w0, const v3 &oinv, const v3 &inv, const v3 &oinvH) {
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
/* one child box from the low bytes of its six quantized planes: whether the
 * ray enters it within [tmin, tmax], and the entry distance in tn */
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

/* entry distances of the four children of 4-wide node `cur` (INF: missed)
 * and their codes / counts, from its 64 quantized bytes (pm_build.h
 * quantize_bvh4: each bound decodes as o + q * 2^e, a box containing the
 * float one). The one 4-wide format: 128-B float nodes were dropped after
 * C3 trace 5.16 -> 4.75 ms per 1M paths (same box) for the quantized ones:
 * half the bytes per visit, 24 byte conversions more per node. */
PMD void node4_test(const SceneDev &S, int cur, const v3 &oinv, const v3 &inv, float tmin, float tmax, float t[4],
                    int c[4], int n[4], const v3 &oinvH) {
    const uint4 *nd = reinterpret_cast<const uint4 *>(S.wnodes) + 4 * cur;
    const uint4 w0 = nd[0], w1 = nd[1], w2 = nd[2], w3 = nd[3];
    const QSlab q = qslab(w0, oinv, inv, oinvH);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t sh = 8u * (uint32_t)k;
        float tn;
        t[k] = qslab_hit(q, w1.x >> sh, w1.y >> sh, w1.z >> sh, w1.w >> sh, w2.x >> sh, w2.y >> sh, tmin, tmax, tn)
                   ? tn : __int_as_float(0x7f800000);
    }
    c[0] = (int)w3.x; c[1] = (int)w3.y; c[2] = (int)w3.z; c[3] = (int)w3.w;
    n[0] = (int)(int16_t)(w2.z & 0xffffu); n[1] = (int)(int16_t)(w2.z >> 16);
    n[2] = (int)(int16_t)(w2.w & 0xffffu); n[3] = (int)(int16_t)(w2.w >> 16);
}

/* 4-wide traversal (MODE_GLOBAL scenes with S.wide == 2): one 64-B node per
 * visit, its four boxes tested at once; hit internal children are ordered
 * near to far with a sorting network, the nearest entered next and the rest
 * pushed (the stack is sized by the builder's max_stack); hit leaves are
 * postponed and tested together as in traverse() (at most four per node). */
template <bool ANY, class C, bool INST>
PMD bool traverse4(const SceneDev &S, const Ray &ray, Hit &best, int *stack, int stride, C &cen) {
    best_begin(best, ray.tmax);
    const v3 inv = safe_inv(ray.d);
    const v3 oinv = ray_oinv(ray.o, inv, ray_pad2(ray.o));
    int sp = 0;
    int cur = 0;
    uint32_t l0s = 0, l0n = 0, l1s = 0, l1n = 0, l2s = 0, l2n = 0, l3s = 0, l3n = 0;
    int guard = 0;
    const float INF = __int_as_float(0x7f800000);
    while (true) {
        while (cur >= 0 && l0n == 0 && guard <= S.n_nodes) {
            ++guard;
            cen.node();
            float t[4];
            int c[4], n[4];
            node4_test(S, cur, oinv, inv, ray.tmin, best.t, t, c, n, ray_oinv_hi(oinv, inv, ray.o));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (t[k] != INF && n[k] > 0) { /* leaf: postpone */
                    const uint32_t s0 = (uint32_t)~c[k], n0 = (uint32_t)n[k];
                    if (l0n == 0) { l0s = s0; l0n = n0; }
                    else if (l1n == 0) { l1s = s0; l1n = n0; }
                    else if (l2n == 0) { l2s = s0; l2n = n0; }
                    else { l3s = s0; l3n = n0; }
                }
                if (n[k] != 0) t[k] = INF; /* only internal children stay */
            }
            /* near to far: (0,1) (2,3) (0,2) (1,3) (1,2) */
            auto cs = [&](int a, int b) {
                if (t[b] < t[a]) { const float tt = t[a]; t[a] = t[b]; t[b] = tt; const int cc = c[a]; c[a] = c[b]; c[b] = cc; }
            };
            cs(0, 1); cs(2, 3); cs(0, 2); cs(1, 3); cs(1, 2);
            if (t[3] != INF) { stack[sp * stride] = c[3]; ++sp; }
            if (t[2] != INF) { stack[sp * stride] = c[2]; ++sp; }
            if (t[1] != INF) { stack[sp * stride] = c[1]; ++sp; }
            if (t[0] != INF) cur = c[0];
            else if (sp > 0) { --sp; cur = stack[sp * stride]; }
            else cur = -1;
        }
        while (l0n != 0) {
            /* instance trees use the stack entries above the ones in use */
            if (leaf_isect<ANY, true, C, INST>(S, l0s, l0n, ray, best, cen, stack + sp * stride, stride))
                return true;
            l0s = l1s; l0n = l1n; l1s = l2s; l1n = l2n; l2s = l3s; l2n = l3n; l3n = 0;
        }
        if (cur < 0 || guard > S.n_nodes) break;
    }
    return ANY ? false : best.ref != 0xffffffffu;
}

/* ------------------------------------------------------ instance trees */
/* Closest hit (or any hit) among an instance's triangles. The object tree
 * is walked in object space: the ray taken through w2o (o' = w2o o, d' =
 * w2o d; the same t parameterises both, the transform being affine) and
 * every box widened by pad = 1e-5 (a (2 |o| + W) + k B), a = |w2o| (row
 * sums), W the instance's world extent, k = |o2w| |w2o|, B the object's
 * extent (both per instance, I[7]) — beyond the rounding of o', d' and of
 * the world vertices mapped back (~3 ulps of those magnitudes), so culling
 * is conservative: every triangle that can win is tested. Triangles are
 * rebuilt in world space (inst_tri) and tested with the world ray like a
 * flattened mesh's, so hits equal the flattened scene's bit for bit. The
 * stack entries above the caller's hold the walk (collapse_bvh4's bound). */
template <bool ANY, class C>
PMD bool blas_isect(const SceneDev &S, uint32_t inst, const Ray &ray, Hit &best, int *stack, int stride, C &cen) {
    const float4 *I = S.insts + 8 * inst;
    const float4 hd = I[6], pk = I[7];
    const uint32_t gid0 = (uint32_t)__float_as_int(hd.z);
    const float4 w0 = I[3], w1 = I[4], w2 = I[5];
    const v3 o = inst_point(I + 3, ray.o.x, ray.o.y, ray.o.z);
    const v3 d = mk((w0.x * ray.d.x + w0.y * ray.d.y) + w0.z * ray.d.z, (w1.x * ray.d.x + w1.y * ray.d.y) + w1.z * ray.d.z,
                    (w2.x * ray.d.x + w2.y * ray.d.y) + w2.z * ray.d.z);
    const float on = fmaxf(fabsf(ray.o.x), fmaxf(fabsf(ray.o.y), fabsf(ray.o.z)));
    const float pad = 1e-5f * (pk.y * (2.f * on) + pk.z);
    const v3 inv = safe_inv(d);
    const v3 oL = mk((o.x + pad) * inv.x, (o.y + pad) * inv.y, (o.z + pad) * inv.z);
    const v3 oH = mk((o.x - pad) * inv.x, (o.y - pad) * inv.y, (o.z - pad) * inv.z);
    const float INF = __int_as_float(0x7f800000);
    int sp = 0, cur = __float_as_int(hd.x), guard = 0;
    while (cur >= 0 && guard <= S.n_nodes) {
        ++guard;
        cen.node();
        float t[4];
        int c[4], n[4];
        node4_test(S, cur, oL, inv, ray.tmin, best.t, t, c, n, oH);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (t[k] == INF || n[k] <= 0) continue;
            /* a leaf: its triangles at object slots [~c, ~c + count) (LEAF_TRIS) */
            const uint32_t s0 = (uint32_t)~c[k], cnt = (uint32_t)n[k] & 0x3fffu;
            for (uint32_t q = s0; q < s0 + cnt; ++q) {
                cen.prim();
                v3 p0, p1, p2;
                float4 g[3];
                inst_tri(S, I, q, p0, p1, p2, g);
                float tt, bb, gg;
                const bool ok = isect_tri_v(g[0], g[1], g[2], ray, &tt, &bb, &gg);
                if (ANY) { if (ok) return true; continue; }
                if (!ok || tt > best.t) continue;
                const uint32_t gid = gid0 + (uint32_t)__float_as_int(S.obj_v[3 * q].w);
                if (tt < best.t || gid < best.gid) {
                    best.t = tt; best.beta = bb; best.gamma = gg; best.ref = (PRIM_INST << 30) | q; best.gid = gid;
                }
            }
            t[k] = INF;
        }
        /* internal children: nearest next, the others pushed */
        auto cs = [&](int a, int b) {
            if (t[b] < t[a]) { const float tt = t[a]; t[a] = t[b]; t[b] = tt; const int cc = c[a]; c[a] = c[b]; c[b] = cc; }
        };
        cs(0, 1); cs(2, 3); cs(0, 2); cs(1, 3); cs(1, 2);
        if (t[3] != INF) { stack[sp * stride] = c[3]; ++sp; }
        if (t[2] != INF) { stack[sp * stride] = c[2]; ++sp; }
        if (t[1] != INF) { stack[sp * stride] = c[1]; ++sp; }
        if (t[0] != INF) cur = c[0];
        else if (sp > 0) { --sp; cur = stack[sp * stride]; }
        else cur = -1;
    }
    return false;
}

/* Resumable closest-hit traversal of the 4-wide BVH for kernels that keep a
 * ray's traversal alive across iterations of an outer loop (k_trace_pool):
 * trav_step advances by one node visit or one leaf; the result equals
 * traverse4's (same culling, same leaf tests, same tie-break). */
struct TravState {
    v3 inv, oinv; /* oinv: the low planes' offset (ray_oinv); the high planes' is rebuilt per visit */
    Hit best;
    int cur, sp, guard;
    uint32_t l0s, l0n, l1s, l1n, l2s, l2n, l3s, l3n;
};
PMD void trav_begin(const Ray &ray, TravState &t) {
    best_begin(t.best, ray.tmax);
    t.best.beta = t.best.gamma = 0.f;
    t.inv = safe_inv(ray.d);
    t.oinv = ray_oinv(ray.o, t.inv, ray_pad2(ray.o));
    t.cur = 0; t.sp = 0; t.guard = 0;
    t.l0n = t.l1n = t.l2n = t.l3n = 0;
    t.l0s = t.l1s = t.l2s = t.l3s = 0;
}
/* a lane's traversal stack: entries below cap in its LDS column, deeper ones
 * (rare: the bound is exact, typical depths are far below it) in a global
 * spill area, entry i of thread gid at spill[(i - cap) * sstride + gid] —
 * so the LDS a block reserves can be sized for occupancy, not the worst ray */
struct SpillStack {
    int *lds;
    int stride, cap;
    int *spill;
    uint32_t sstride, gid;
    PMD void put(int i, int v) const {
        if (i < cap) lds[i * stride] = v;
        else spill[(size_t)(i - cap) * sstride + gid] = v;
    }
    PMD int get(int i) const { return i < cap ? lds[i * stride] : spill[(size_t)(i - cap) * sstride + gid]; }
};
/* false once the ray is done (best holds its closest hit, if any) */
template <class C>
PMD bool trav_step(const SceneDev &S, const Ray &ray, TravState &T, const SpillStack &stk, C &cen) {
    /* (requesting the node before the pending leaf's test, so a wave's leaf
     * and node loads overlap, measured slower: C3 trace 4.14 -> 4.22-4.27 ms,
     * 88 B of scratch at 5 waves/SIMD or 4.23-4.26 ms at 4; profiles/r05/trace_c3) */
    if (T.l0n != 0) {
        leaf_isect<false, true>(S, T.l0s, T.l0n, ray, T.best, cen);
        T.l0s = T.l1s; T.l0n = T.l1n; T.l1s = T.l2s; T.l1n = T.l2n; T.l2s = T.l3s; T.l2n = T.l3n; T.l3n = 0;
        /* the last pending leaf done: this step also visits the next node, so
         * a lane's leaf tests share steps with node visits (the wave runs
         * both codes whenever its lanes differ anyway). Against a step that
         * ends after every leaf, C3 trace per 1M paths 4.42-4.43 -> 4.07-4.10
         * ms (same box, round 3); also testing the first leaf a visit finds
         * in the same step: 4.44 (the second leaf code costs every step) */
        if (T.l0n != 0) return true;
    }
    if (T.cur < 0 || T.guard > S.n_nodes) return false;
    ++T.guard;
    cen.node();
    const float INF = __int_as_float(0x7f800000);
    float t[4];
    int c[4], n[4];
    node4_test(S, T.cur, T.oinv, T.inv, ray.tmin, T.best.t, t, c, n, ray_oinv_hi(T.oinv, T.inv, ray.o));
    /* the pending-leaf queue is empty here (a visit follows the last pending
     * leaf's test): the hit leaves, in child order, enter it by shifting from
     * the back — selects only, no branch per child. (traverse4's chain of
     * first-free-slot tests measured slower here: C3 trace 3.86-3.88 vs
     * 3.81-3.85 ms, profiles/r05/trace_c3 pool_tuning.) */
    {
        uint32_t a0s = 0, a0n = 0, a1s = 0, a1n = 0, a2s = 0, a2n = 0, a3s = 0, a3n = 0;
#pragma unroll
        for (int k = 3; k >= 0; --k) {
            if (t[k] != INF && n[k] > 0) {
                a3s = a2s; a3n = a2n; a2s = a1s; a2n = a1n; a1s = a0s; a1n = a0n;
                a0s = (uint32_t)~c[k]; a0n = (uint32_t)n[k];
            }
        }
        T.l0s = a0s; T.l0n = a0n; T.l1s = a1s; T.l1n = a1n; T.l2s = a2s; T.l2n = a2n; T.l3s = a3s; T.l3n = a3n;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (n[k] != 0) t[k] = INF;
    auto cs = [&](int a, int b) {
        if (t[b] < t[a]) { const float tt = t[a]; t[a] = t[b]; t[b] = tt; const int cc = c[a]; c[a] = c[b]; c[b] = cc; }
    };
    cs(0, 1); cs(2, 3); cs(0, 2); cs(1, 3); cs(1, 2);
    if (t[3] != INF) { stk.put(T.sp, c[3]); ++T.sp; }
    if (t[2] != INF) { stk.put(T.sp, c[2]); ++T.sp; }
    if (t[1] != INF) { stk.put(T.sp, c[1]); ++T.sp; }
    if (t[0] != INF) T.cur = c[0];
    else if (T.sp > 0) { --T.sp; T.cur = stk.get(T.sp); }
    else T.cur = -1;
    return T.l0n != 0 || T.cur >= 0;
}

/* ------------------------------------------------------- 8-wide trees */
/* S.wide == 3 (round 6, pm_build.h quantize_bvh8): 128-B quantized nodes of
 * eight children; the child word is the internal node index (>= 0), INT_MIN
 * for an empty slot, or a leaf ~((s << 5) | (tris << 4) | n). One visit tests
 * eight boxes: a third fewer node visits per ray than the 4-wide tree on
 * C3's soup (tools/bvh_width_sim.cpp: 30.1 -> 20.1), each a dependent fetch. */
constexpr int BVH8_EMPTY = (int)0x80000000;
PMD void node8_test(const SceneDev &S, int cur, const v3 &oinv, const v3 &inv, float tmin, float tmax, float t[8],
                    int c[8], const v3 &oinvH) {
    const uint4 *nd = reinterpret_cast<const uint4 *>(S.wnodes) + 8 * cur;
    const uint4 w0 = nd[0], w1 = nd[1], w2 = nd[2], w3 = nd[3], w4 = nd[4], w5 = nd[5];
    const QSlab q = qslab(w0, oinv, inv, oinvH);
    /* byte planes: lo x (w1.x, w1.y), lo y (w1.z, w1.w), lo z (w2.x, w2.y),
     * hi x (w2.z, w2.w), hi y (w3.x, w3.y), hi z (w3.z, w3.w) */
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
                   ? tn : __int_as_float(0x7f800000);
    }
}
/* a leaf child word's test (its refs, or LEAF_TRIS slots) */
template <bool ANY, class C>
PMD bool leaf8_isect(const SceneDev &S, int word, const Ray &ray, Hit &best, C &cen) {
    const uint32_t w = ~(uint32_t)word;
    return leaf_isect<ANY, true>(S, w >> 5, (w & 15u) | ((w & 16u) ? 0x4000u : 0u), ray, best, cen);
}
/* a node's hit internal children near to far: 32-bit keys (the entry t's
 * bits — non-negative floats order like their bits — with the low three
 * replaced by the child's slot; misses and leaves sort last as ~0) through
 * Batcher's odd-even merge network for 8 (19 min/max pairs). The order only
 * steers the walk; hits do not depend on it (lowest-id tie-break). */
PMD void sort8_keys(uint32_t k[8]) {
    auto cs = [&](int a, int b) { const uint32_t lo = min(k[a], k[b]), hi = max(k[a], k[b]); k[a] = lo; k[b] = hi; };
    cs(0, 1); cs(2, 3); cs(4, 5); cs(6, 7);
    cs(0, 2); cs(1, 3); cs(4, 6); cs(5, 7);
    cs(1, 2); cs(5, 6);
    cs(0, 4); cs(1, 5); cs(2, 6); cs(3, 7);
    cs(2, 4); cs(3, 5);
    cs(1, 2); cs(3, 4); cs(5, 6);
}
PMD int child8(const int c[8], uint32_t slot) { /* c[slot & 7] by selects (no dynamic register index) */
    const int a = (slot & 1u) ? c[1] : c[0], b = (slot & 1u) ? c[3] : c[2];
    const int d = (slot & 1u) ? c[5] : c[4], e = (slot & 1u) ? c[7] : c[6];
    const int f = (slot & 2u) ? b : a, g = (slot & 2u) ? e : d;
    return (slot & 4u) ? g : f;
}
/* one node visit of the 8-wide walk: the hit leaves tested at once (every
 * lane's, in one pass of the wave), the hit internal children sorted, the
 * nearest returned in `next` (-1: none) and the others pushed far to near */
template <bool ANY, class C, class Put>
PMD bool visit8(const SceneDev &S, int node, const Ray &ray, const v3 &oinv, const v3 &inv, const v3 &oinvH, Hit &best,
                C &cen, int &next, Put &&stack_put) {
    float t[8];
    int c[8];
    node8_test(S, node, oinv, inv, ray.tmin, best.t, t, c, oinvH);
    const float INF = __int_as_float(0x7f800000);
    uint32_t key[8], lm = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (t[k] != INF && c[k] < 0) lm |= 1u << k;
        key[k] = t[k] != INF && c[k] >= 0 ? (__float_as_uint(t[k]) & ~7u) | (uint32_t)k : 0xffffffffu;
    }
    /* the hit leaves, one per lane per round: as many rounds as the lane with
     * the most (unrolled per slot, the wave ran the leaf code for every slot
     * any lane hit) */
    while (lm != 0u) {
        const uint32_t k = (uint32_t)__builtin_ctz(lm);
        lm &= lm - 1u;
        if (leaf8_isect<ANY>(S, child8(c, k), ray, best, cen) && ANY) return true;
    }
    sort8_keys(key);
#pragma unroll
    for (int k = 7; k >= 1; --k)
        if (key[k] != 0xffffffffu) stack_put(child8(c, key[k]));
    next = key[0] != 0xffffffffu ? child8(c, key[0]) : -1;
    return false;
}
/* one-call closest / any hit on the 8-wide tree (eye pass, shadow rays,
 * per-lane kernels) */
template <bool ANY, class C>
PMD bool traverse8(const SceneDev &S, const Ray &ray, Hit &best, int *stack, int stride, C &cen) {
    best_begin(best, ray.tmax);
    const v3 inv = safe_inv(ray.d);
    const v3 oinv = ray_oinv(ray.o, inv, ray_pad2(ray.o));
    int sp = 0, cur = 0, guard = 0;
    while (cur >= 0 && guard <= S.n_nodes) {
        ++guard;
        cen.node();
        int next = -1;
        if (visit8<ANY>(S, cur, ray, oinv, inv, ray_oinv_hi(oinv, inv, ray.o), best, cen, next, [&](int v) { stack[sp * stride] = v; ++sp; }))
            return true;
        if (next >= 0) cur = next;
        else if (sp > 0) { --sp; cur = stack[sp * stride]; }
        else cur = -1;
    }
    return ANY ? false : best.ref != 0xffffffffu;
}
/* resumable 8-wide traversal for k_trace_pool (trav_step's contract): one
 * node visit per step, its hit leaves tested in the same step (no pending
 * queue: the registers of eight queued leaves spilled the pooled kernel) */
struct TravState8 {
    v3 inv, oinv;
    Hit best;
    int cur, sp, guard;
};
PMD void trav_begin(const Ray &ray, TravState8 &t) {
    best_begin(t.best, ray.tmax);
    t.best.beta = t.best.gamma = 0.f;
    t.inv = safe_inv(ray.d);
    t.oinv = ray_oinv(ray.o, t.inv, ray_pad2(ray.o));
    t.cur = 0; t.sp = 0; t.guard = 0;
}
template <class C>
PMD bool trav_step(const SceneDev &S, const Ray &ray, TravState8 &T, const SpillStack &stk, C &cen) {
    if (T.cur < 0 || T.guard > S.n_nodes) return false;
    ++T.guard;
    cen.node();
    int next = -1;
    visit8<false>(S, T.cur, ray, T.oinv, T.inv, ray_oinv_hi(T.oinv, T.inv, ray.o), T.best, cen, next,
                  [&](int v) { stk.put(T.sp, v); ++T.sp; });
    if (next >= 0) T.cur = next;
    else if (T.sp > 0) { --T.sp; T.cur = stk.get(T.sp); }
    else T.cur = -1;
    return T.cur >= 0;
}

template <bool ANY, int MODE>
PMD bool traverse(const SceneDev &S, const Ray &ray, Hit &best, int *stack, int stride) {
    NoCensus none;
    return traverse<ANY, MODE>(S, ray, best, stack, stride, none);
}

} // namespace pm
