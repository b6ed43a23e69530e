/*
 * pm_shade.h — what happens at a hit: its shading frame (Geo, shade), the
 * specular steps and the Lambert lobe (material_specular*, sample_f), the
 * light samplers and light_le, and, through the trailing pm_texture.h, the
 * texture lookup of a matte Kd. Included by the units that shade a hit:
 * pm_trace.hip and pm_eye.hip.
 */
#pragma once
#include "pm_isect.h"
#include "pm_sample.h"

#pragma clang fp contract(off)

namespace pm {

/* ------------------------------------------------------------- shading */
/* ng: the unit geometric normal of the hit primitive — for a triangle the
 * direction of cross(p1 - p0, p2 - p0), whatever its vertex normals say;
 * read by light_le for mesh lights only (dead code elsewhere) */
struct Geo { v3 ns, dpdu, ng; int material, light; };

/* the instance record holding global triangle id gid (records ascend by id) */
PMD uint32_t inst_of_gid(const SceneDev &S, uint32_t gid) {
    uint32_t lo = 0, hi = (uint32_t)S.n_inst - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if ((uint32_t)__float_as_int(S.insts[8 * mid + 6].z) <= gid) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

/* hit attributes (cudatrianglemesh.cu:20-78, cudadisk.cu:36-47,
 * cudasphere.cu:35-48), transformed and normalized as the closest-hit
 * programs do (raytracing.cu:110-117, cudamaterial.cu.h:84-85). */
/* INST: the scene may hold instances (MODE_INST kernels); the others compile
 * without that branch (its registers cost the pooled trace kernel scratch) */
template <bool INST = true>
PMD Geo shade(const SceneDev &S, const Ray &ray, const Hit &h) {
    Geo g;
    uint32_t kind = h.ref >> 30, idx = h.ref & 0x3fffffffu;
    v3 nsw, dpduw;
    if (INST && kind == PRIM_INST) { /* an instance's triangle: the flattened triangle's frame, rebuilt */
        const float4 *I = S.insts + 8 * inst_of_gid(S, h.gid);
        v3 p0, p1, p2;
        float4 gg[3];
        inst_tri(S, I, idx, p0, p1, p2, gg);
        const v3 n = mk(gg[2].y, gg[2].z, gg[2].w);
        const int4 vi = S.obj_info[idx];
        const int4 mi = S.obj_mesh[vi.w];
        g.material = mi.x; g.light = mi.y;
        /* tri_frame (pm_api.cpp): dp/du from the uvs (cudatrianglemesh.cu:49-58) */
        float uv0x = 0.f, uv0y = 0.f, uv1x = 1.f, uv1y = 0.f, uv2x = 0.f, uv2y = 1.f;
        if (mi.w) {
            const float4 a = S.obj_uv[vi.x], b = S.obj_uv[vi.y], c = S.obj_uv[vi.z];
            uv0x = a.x; uv0y = a.y; uv1x = b.x; uv1y = b.y; uv2x = c.x; uv2y = c.y;
        }
        const float du1 = uv0x - uv2x, du2 = uv1x - uv2x, dv1 = uv0y - uv2y, dv2 = uv1y - uv2y;
        const float det = du1 * dv2 - dv1 * du2;
        v3 d;
        if (det == 0.0f) {
            if (fabsf(n.x) > fabsf(n.y)) {
                const float il = rcp_exact(sqrtf(n.x * n.x + n.z * n.z));
                d = mk(-n.z * il, 0.f, n.x * il);
            } else {
                const float il = rcp_exact(sqrtf(n.y * n.y + n.z * n.z));
                d = mk(0.f, n.z * il, n.y * il);
            }
        } else {
            const float invdet = rcp_exact(det);
            const v3 dp1 = p0 - p2, dp2 = p1 - p2;
            d = mk((dv2 * dp1.x - dv1 * dp2.x) * invdet, (dv2 * dp1.y - dv1 * dp2.y) * invdet,
                   (dv2 * dp1.z - dv1 * dp2.z) * invdet);
        }
        g.dpdu = normalize(d);
        g.ng = normalize(n);
        if (!mi.z) { g.ns = g.ng; return g; }
        /* vertex normals through pbrt's Transform::operator()(Normal) (transpose
         * of mInv), then interpolated per hit as for a flattened mesh */
        const float4 *W = I + 3;
        const v3 n0 = xform_normal(W, xyz(S.obj_n[vi.x])), n1 = xform_normal(W, xyz(S.obj_n[vi.y])),
                 n2 = xform_normal(W, xyz(S.obj_n[vi.z]));
        g.ns = normalize(n1 * h.beta + n2 * h.gamma + n0 * (1.0f - h.beta - h.gamma));
        return g;
    }
    if (kind == PRIM_TRI) {
        /* per-triangle frame (cudatrianglemesh.cu:36-78 + normalize), see tri_shade */
        const float4 s0 = S.tri_shade[2 * idx], s1 = S.tri_shade[2 * idx + 1];
        const int mb = fbits(s0.w);
        g.material = mb & 0x7fffffff; g.light = fbits(s1.w);
        g.dpdu = xyz(s1);
        g.ng = xyz(s0);
        if (mb >= 0) { g.ns = xyz(s0); return g; }
        const int4 ti = S.tri_info[idx]; /* shading normals: interpolated per hit */
        v3 n0 = xyz(S.norms[ti.x]), n1 = xyz(S.norms[ti.y]), n2 = xyz(S.norms[ti.z]);
        g.ns = normalize(n1 * h.beta + n2 * h.gamma + n0 * (1.0f - h.beta - h.gamma));
        return g;
    } else if (kind == PRIM_DISK) {
        const float4 *dk = S.disks + 5 * idx;
        float4 a = dk[0], b = dk[1], c = dk[2], d = dk[3], e = dk[4];
        v3 x = xyz(b), y = xyz(c);
        v3 phit = ray.o + h.t * ray.d;
        v3 local = phit - xyz(a);
        float localx = dot(local, x) * d.w;
        float localy = dot(local, y) * e.x;
        nsw = xyz(d);
        dpduw = -localy * x + localx * y;
        g.material = fbits(e.y); g.light = fbits(e.z);
    } else {
        const float4 *s = S.spheres + 4 * idx;
        v3 o, d;
        xform_ray(s, ray, &o, &d);
        float rad = s[3].x;
        v3 phit = o + h.t * d;
        if (phit.x == 0.f && phit.y == 0.f) phit.x = 1e-5f * rad;
        v3 n = phit / rad;
        v3 dpdu = mk(-n.y, n.x, 0.f);
        nsw = xform_normal(s, n);
        dpduw = xform_normal(s, dpdu);
        g.material = fbits(s[3].y); g.light = fbits(s[3].z);
    }
    g.ns = normalize(nsw);
    g.ng = g.ns;
    g.dpdu = normalize(dpduw);
    return g;
}

PMD v3 world_to_local(v3 v, v3 nn, v3 sn, v3 tn) { return mk(dot(v, sn), dot(v, tn), dot(v, nn)); }
PMD v3 local_to_world(v3 v, v3 nn, v3 sn, v3 tn) {
    return mk(sn.x * v.x + tn.x * v.y + nn.x * v.z, sn.y * v.x + tn.y * v.y + nn.y * v.z,
              sn.z * v.x + tn.z * v.y + nn.z * v.z);
}
PMD bool is_specular(int type) { return type == PM_GLASS || type == PM_MIRROR; }

/* cudamaterial.cu.h:101-165; false on glass TIR */
PMD bool material_specular(int type, const Geo &g, v3 wow, v3 *wiw) {
    const v3 nn = g.ns, sn = g.dpdu, tn = cross(nn, sn);
    v3 wo = world_to_local(wow, nn, sn, tn);
    v3 wi;
    if (type == PM_MIRROR) {
        wi = mk(-wo.x, -wo.y, wo.z);
    } else {
        bool entering = wo.z > 0.f;
        float sini2 = fmaxf(0.f, 1.f - wo.z * wo.z);
        float eta = entering ? 1 / 1.5f : 1.5f;
        float sint2 = eta * eta * sini2;
        if (sint2 >= 1.0f) return false;
        float cost = sqrtf(fmaxf(0.f, 1.f - sint2));
        if (entering) cost = -cost;
        wi = mk(eta * -wo.x, eta * -wo.y, cost);
    }
    *wiw = local_to_world(wi, nn, sn, tn);
    return true;
}

/* The physical specular model of pm_add_material_specular (pm_api.h states
 * it): a mirror reflects with weight Kr and reads no u; glass is pbrt-v2's
 * FresnelDielectric(1, index) with a reflection lobe Kr and a transmission
 * lobe Kt, one of which u picks. a = (Kr, index), b = (Kt, flag) of
 * SceneDev::mat_spec. Returns false when both lobes are black (the path or
 * chain ends); else *wiw, the weight of the step and *eta2 = eta * eta for a
 * transmitted step (what an eye chain's radiance scales by), 1 otherwise. */
PMD bool material_specular_pbrt(int type, float4 a, float4 b, const Geo &g, v3 wow, float u, v3 *wiw, v3 *weight,
                                float *eta2) {
    const v3 nn = g.ns, sn = g.dpdu, tn = cross(nn, sn);
    const v3 wo = world_to_local(wow, nn, sn, tn);
    const v3 kr = xyz(a);
    v3 wi = mk(-wo.x, -wo.y, wo.z);
    *eta2 = 1.0f;
    if (type == PM_MIRROR) {
        if (is_black(kr)) return false;
        *weight = kr;
    } else {
        const v3 kt = xyz(b);
        const bool entering = wo.z > 0.f;
        const float ei = entering ? 1.0f : a.w, et = entering ? a.w : 1.0f;
        const float eta = ei / et;
        const float sini2 = fmaxf(0.f, 1.f - wo.z * wo.z);
        const float sint2 = eta * eta * sini2;
        float F = 1.0f, cost = 0.0f;
        if (!(sint2 >= 1.0f)) {
            cost = sqrtf(fmaxf(0.f, 1.f - sint2));
            const float ci = fabsf(wo.z);
            const float rpar = (et * ci - ei * cost) / (et * ci + ei * cost);
            const float rper = (ei * ci - et * cost) / (ei * ci + et * cost);
            F = 0.5f * (rpar * rpar + rper * rper);
        }
        const v3 wr = F * kr, wt = (1.0f - F) * kt;
        const bool rb = is_black(wr), tb = is_black(wt);
        if (rb && tb) return false;
        const float q = tb ? 1.0f : (rb ? 0.0f : F);
        const bool reflect = u < q;
        const bool both = q > 0.0f && q < 1.0f; /* the probability cancels: the lobe's colour itself */
        if (reflect) {
            *weight = both ? kr : wr;
        } else {
            *weight = both ? kt : wt;
            wi = mk(eta * -wo.x, eta * -wo.y, entering ? -cost : cost);
            *eta2 = eta * eta;
        }
    }
    *wiw = local_to_world(wi, nn, sn, tn);
    return true;
}

/* cudamaterial.cu.h:50-98 (Lambert lobe); returns f = Kd/pi */
PMD v3 sample_f(v3 kd, const Geo &g, v3 wow, float u1, float u2, v3 *wiw, float *pdf) {
    const v3 nn = g.ns, sn = g.dpdu, tn = cross(nn, sn);
    v3 wo = world_to_local(wow, nn, sn, tn);
    float x, y;
    concentric_sample_disk(u1, u2, &x, &y);
    v3 wi = mk(x, y, sqrtf(fmaxf(0.f, 1.f - x * x - y * y)));
    if (wo.z < 0.f) wi.z *= -1.f;
    *pdf = (wo.z * wi.z > 0.0f) ? fabsf(wi.z) * INV_PI : 0.f;
    *wiw = local_to_world(wi, nn, sn, tn);
    return kd * INV_PI;
}

/* ------------------------------------------------------------- lights */
/* A point of a mesh light (PM_LIGHT_AREA_MESH, ours: the reference emits from
 * disks only) for the 2-D sample (u1, u2), uniform over its area; *n = the
 * emitting side's unit normal there. u1 picks triangle k, the first with
 * cdf[k] > u1 (pm_add_light_mesh builds the table): a binary search whose
 * trip count depends on the light's triangle count alone, so the lanes of a
 * wave stay together and only their addresses differ; an empty bin (a
 * zero-area triangle) is never picked. u1 is held below 1 first (host rays
 * may carry a 2-D sample of exactly 1): the bin found is then never empty,
 * whatever the last triangles' areas, and the remap never divides 0 by 0.
 * u1 is then stretched over the bin, and pbrt's UniformSampleTriangle
 * (su = sqrt(u1), b0 = 1 - su, b1 = u2 su) places the point at
 * b0 p0 + b1 p1 + b2 p2, b2 = 1 - b0 - b1, evaluated as p0 + b1 e1 + b2 e2. */
PMD v3 sample_light_mesh(const LightDev &L, const LightTri *tris, float u1, float u2, v3 *n) {
    u1 = fminf(u1, 0x1.fffffep-1f);
    const LightTri *T = tris + fbits(L.o_type.x);
    int lo = 0, len = fbits(L.o_type.y);
    while (len > 1) {
        const int half = len >> 1;
        lo = T[lo + half - 1].p0_cdf.w > u1 ? lo : lo + half;
        len -= half;
    }
    const float4 a = T[lo].p0_cdf, e1 = T[lo].e1, e2 = T[lo].e2, nn = T[lo].n;
    const float cprev = lo > 0 ? T[lo - 1].p0_cdf.w : 0.f;
    const float su = sqrtf((u1 - cprev) / (a.w - cprev));
    const float b0 = 1.f - su, b1 = u2 * su;
    *n = xyz(nn);
    return xyz(a) + b1 * xyz(e1) + (1.f - b0 - b1) * xyz(e2);
}

/* cudalight.cu.h:18-64 */
PMD v3 sample_l_shading(const LightDev &L, const LightTri *tris, v3 point, float u1, float u2, v3 *uwi, float *pdf) {
    int type = fbits(L.o_type.w);
    if (type == PM_LIGHT_POINT) {
        *uwi = xyz(L.o_type) - point;
        float invlength2 = rcp_exact(dot(*uwi, *uwi));
        *pdf = 1.f;
        return xyz(L.le) * invlength2;
    }
    if (type == PM_LIGHT_DISTANT) { /* 2 R to_light: the shadow segment ends outside the world sphere */
        *uwi = -(xyz(L.n_area) * L.le.w);
        *pdf = 1.f;
        return xyz(L.le);
    }
    if (type == PM_LIGHT_AREA_MESH) { /* the disk's estimator below, with the sampled triangle's normal */
        v3 n;
        *uwi = sample_light_mesh(L, tris, u1, u2, &n) - point;
        v3 wi = normalize(*uwi);
        float distanceSquared = dot(*uwi, *uwi);
        float costha = -dot(n, wi);
        *pdf = distanceSquared / (costha * L.n_area.w);
        return costha > 0.0f ? xyz(L.le) : mk(0.f, 0.f, 0.f);
    }
    float x, y;
    concentric_sample_disk(u1, u2, &x, &y);
    *uwi = xyz(L.o_type) + x * xyz(L.p1_ns) + y * xyz(L.p2_r2d) - point;
    v3 wi = normalize(*uwi);
    float distanceSquared = dot(*uwi, *uwi);
    float costha = -dot(xyz(L.n_area), wi);
    *pdf = distanceSquared / (costha * L.n_area.w);
    return costha > 0.0f ? xyz(L.le) : mk(0.f, 0.f, 0.f);
}

/* cudalight.cu.h:78-124 — emission */
PMD v3 sample_le(const LightDev &L, const LightTri *tris, float lu1, float lu2, float u1, float u2, float eps,
                 Ray *ray, v3 *Ns, float *pdf) {
    int type = fbits(L.o_type.w);
    if (type == PM_LIGHT_POINT) {
        ray->o = xyz(L.o_type);
        ray->d = uniform_sample_sphere(lu1, lu2);
        ray->tmin = eps;
        *Ns = ray->d;
        *pdf = (float)(1.f / (4.f * M_PI));
        return xyz(L.le);
    }
    if (type == PM_LIGHT_DISTANT) { /* the disk's point below on the world sphere's disk, one direction */
        float x, y;
        concentric_sample_disk(lu1, lu2, &x, &y);
        ray->o = xyz(L.o_type) + x * xyz(L.p1_ns) + y * xyz(L.p2_r2d);
        ray->d = xyz(L.n_area);
        ray->tmin = eps;
        *Ns = ray->d;
        *pdf = 1.f; /* 1 / (pi R^2), with the area on Le as the disk carries it */
        return xyz(L.le) * L.n_area.w;
    }
    if (type == PM_LIGHT_AREA_MESH) { /* the disk's emission below from a point of the mesh */
        v3 org = sample_light_mesh(L, tris, lu1, lu2, Ns);
        v3 dir = uniform_sample_sphere(u1, u2);
        if (dot(dir, *Ns) < 0.f) dir = dir * -1.f;
        ray->o = org; ray->d = dir; ray->tmin = 1e-2f;
        *pdf = INV_TWOPI;
        return xyz(L.le) * L.n_area.w;
    }
    float x, y;
    concentric_sample_disk(lu1, lu2, &x, &y);
    v3 org = xyz(L.o_type) + x * xyz(L.p1_ns) + y * xyz(L.p2_r2d);
    v3 dir = uniform_sample_sphere(u1, u2);
    *Ns = xyz(L.n_area);
    if (dot(dir, *Ns) < 0.f) dir = dir * -1.f;
    ray->o = org; ray->d = dir; ray->tmin = 1e-2f;
    *pdf = INV_TWOPI;
    return xyz(L.le) * L.n_area.w;
}

/* cudalight.cu.h:128-138; ng: the geometric normal of the primitive that was
 * hit (Geo::ng). A mesh light has no normal of its own: it emits from the
 * side of the hit triangle's cross(p1 - p0, p2 - p0), the other side when
 * its reverse_orientation flag is set (the sign its light_tris normals carry) */
PMD v3 light_le(const LightDev &L, v3 wow, v3 ng) {
    if (fbits(L.o_type.w) == PM_LIGHT_AREA_MESH) {
        const float c = dot(ng, wow);
        return (fbits(L.o_type.z) ? -c : c) > 0.f ? xyz(L.le) : mk(0.f, 0.f, 0.f);
    }
    if (dot(xyz(L.n_area), wow) > 0.f) return xyz(L.le);
    return mk(0.f, 0.f, 0.f);
}

} // namespace pm

#include "pm_texture.h"
