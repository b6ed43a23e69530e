/*
 * pm_leaf.h — what tests primitives: the census hooks, the closest-hit rule
 * (consider, best_begin, found), the packed triangle-pair test with the
 * brute-force loop (brute_isect) and the leaf tests of the binary, 4-wide
 * (leaf_isect) and 8-wide (leaf8_isect) trees. Included by pm_traverse.h.
 */
#pragma once
#include "pm_isect.h"

#pragma clang fp contract(off)

namespace pm {

/* per-lane traversal census (bench roofline / DESIGN.md): nodes entered and primitive tests; NoCensus compiles to
 * nothing */
struct NoCensus { PMD void node() {} PMD void prim() {} };
struct Census {
    uint32_t nodes = 0, prims = 0;
    PMD void node() { ++nodes; }
    PMD void prim() { ++prims; }
};

/* closest hit so far: smaller t wins, equal t -> lowest global primitive id (callers pass only t <= best.t), so the
 * result is independent of the order primitives are tested in (BVH or brute force) */
PMD void consider(Hit &best, float t, float b, float g, uint32_t ref, uint32_t gid) {
    if (t < best.t || gid < best.gid) { best.t = t; best.beta = b; best.gamma = g; best.ref = ref; best.gid = gid; }
}

/* a query starts with no hit: t at the ray's far end, no primitive */
PMD void best_begin(Hit &best, float tmax) {
    best.t = tmax;
    best.gid = 0xffffffffu;
    best.ref = 0xffffffffu;
}
/* what a finished query returns: an any-hit query that got here found nothing */
template <bool ANY>
PMD bool found(const Hit &best) { return ANY ? false : best.ref != 0xffffffffu; }

/* MODE_BRUTE: every primitive, wave-uniform loop (same primitive in every lane: broadcast LDS reads, no divergence,
 * no stack) */
typedef float f2 __attribute__((ext_vector_type(2)));
PMD f2 bc2(float x) { return f2{x, x}; }

/* isect_tri_v for two triangles at once (packed v_pk_mul/add_f32): the same per-component IEEE operations in the same
 * order, so each lane of the pair is bit-identical to the scalar test. */
/* two triangles' (p0, e0, e1, n) as packed pairs, wave-uniform */
struct TriPair { f2 p0x, p0y, p0z, e0x, e0y, e0z, e1x, e1y, e1z, nx, ny, nz; };
/* the ray's origin and direction as packed splats. The components pass through an empty asm first: splatting a value
 * loaded from the path state otherwise became a <2 x float> load of the state, which kept the ray in scratch memory
 * (5 scratch loads per ray in k_trace_lane) */
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
    /* rcp_exact of both, one range check for the pair (either outside [2^-125, 2^125): both divide; a NaN passes the
     * check and gives NaN either way) and the Newton step as two packed FMAs */
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

/* Brute-force scenes store their triangles in global-id order (pm_api.cpp build_scene), and triangles, disks, spheres
 * are tested in that order, which is ascending global id: a strict t < best.t keeps the first of equal-t hits = the
 * lowest id, the same hit consider() picks in any order — no id loads in the loop. best.gid is left unset (nothing
 * after the query reads it). */
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
    /* (software-pipelining the next pair's scalar loads measured slower: C2 trace 91 vs 86 us — more live SGPRs, no
     * unroll; so did pipelined vector loads of the pairs into VGPRs: 73.5 -> 99 us, 111 VGPRs) */
    /* the running best in locals (one register per field: with the Hit reference the compiler kept best.t twice, one
     * more move per hit) */
    float bt = best.t, bb = best.beta, bg = best.gamma;
    uint32_t bref = best.ref;
#pragma unroll 2
    for (; k + 1 < S.n_tris; k += 2) {
        cen.prim(); cen.prim();
        f2 t, b, g;
        isect_tri_pair(load_pair_il((const_f32_ptr)S.tri_pairs_g + 12 * k), rs, t, b, g); /* pair k / 2: 24 floats */
        /* closest hit: t < best.t <= ray.tmax (traverse starts best.t at tmax) implies t < tmax, so only the any-hit
         * query tests tmax */
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

/* the instance walk (pm_traverse.h), which leaf_isect<INST> enters */
template <bool ANY, class C>
PMD bool blas_isect(const SceneDev &S, uint32_t inst, const Ray &ray, Hit &best, int *stack, int stride, C &cen);
/* Tests the primitives of one leaf; for ANY=true returns at the first hit. TRIRUN: the leaf comes from a quantized
 * wide node, whose count may carry pm_build.h's LEAF_TRIS flag (only quantize_bvh4 / quantize_bvh8 set it; binary
 * leaves are always decoded through their refs, whatever their size). INST: the leaf's refs may be instances
 * (MODE_INST), whose trees are walked with the stack entries above the caller's (stack, stride) */
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
            consider(best, t, b, g, (PRIM_TRI << 30) | idx, S.tri_id[idx]);
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
        consider(best, t, b, g, ref, gid); /* t <= best.t here: ties -> lowest id */
    }
    return false;
}
/* a leaf child word of the 8-wide tree (its refs, or LEAF_TRIS slots) */
template <bool ANY, class C>
PMD bool leaf8_isect(const SceneDev &S, int word, const Ray &ray, Hit &best, C &cen) {
    const uint32_t w = ~(uint32_t)word;
    return leaf_isect<ANY, true>(S, w >> 5, (w & 15u) | ((w & 16u) ? 0x4000u : 0u), ray, best, cen);
}

} // namespace pm
