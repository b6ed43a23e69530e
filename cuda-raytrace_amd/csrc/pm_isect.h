/*
 * pm_isect.h — the primitive intersectors (triangle, disk, sphere), the
 * sphere's ray and normal transforms, and the world-space triangle of an
 * instance's object slot (inst_point, inst_tri), which the instance walk
 * intersects and shade() rebuilds its frame from. Included by pm_leaf.h
 * (so by pm_traverse.h) and pm_shade.h.
 */
#pragma once
#include "pm_device.h"

#pragma clang fp contract(off)

namespace pm {

/* ------------------------------------------------------------ intersect */
/* OptiX 3 intersect_triangle (cudatrianglemesh.cu:24) on precomputed
 * e0 = p1-p0, e1 = p0-p2, n = e1 x e0 (identical float values). */
PMD bool isect_tri_v(const float4 a, const float4 b, const float4 c, const Ray &ray, float *t, float *beta,
                     float *gamma) {
    v3 p0 = mk(a.x, a.y, a.z), e0 = mk(a.w, b.x, b.y), e1 = mk(b.z, b.w, c.x), n = mk(c.y, c.z, c.w);
    const v3 e2 = rcp_exact(dot(n, ray.d)) * (p0 - ray.o);
    const v3 i = cross(ray.d, e2);
    *beta = dot(i, e1);
    *gamma = dot(i, e0);
    *t = dot(n, e2);
    return (*t < ray.tmax) & (*t > ray.tmin) & (*beta >= 0.0f) & (*gamma >= 0.0f) & (*beta + *gamma <= 1);
}
PMD bool isect_tri(const float4 *g, const Ray &ray, float *t, float *beta, float *gamma) {
    return isect_tri_v(g[0], g[1], g[2], ray, t, beta, gamma);
}

/* cudadisk.cu:18-50 */
PMD bool isect_disk(const float4 *dk, const Ray &ray, float *thit_out) {
    float4 a = dk[0], b = dk[1], c = dk[2], d = dk[3], e = dk[4];
    v3 o = xyz(a), x = xyz(b), y = xyz(c), z = xyz(d);
    float thit = (c.w - dot(z, ray.o)) / dot(z, ray.d);
    if (!(thit > ray.tmin && thit < ray.tmax)) return false;
    v3 phit = ray.o + thit * ray.d;
    v3 local = phit - o;
    float localx = dot(local, x) * d.w;
    float localy = dot(local, y) * e.x;
    float dist2 = localx * localx + localy * localy;
    if (dist2 > 1.f || dist2 < a.w * a.w) return false;
    /* phi <= (float)2pi always, so a full disk (phiMax >= (float)2pi) can
     * never reject here: skip the double-precision atan2 (same result) */
    if (b.w < 6.28318548202514648438f) {
        float phi = pmdm_atan2f(localy, localx);
        if (phi < 0) phi = (float)((double)phi + 2.f * M_PI);
        if (phi > b.w) return false;
    }
    *thit_out = thit;
    return true;
}

PMD void xform_ray(const float4 *m, const Ray &r, v3 *o, v3 *d) {
    float4 r0 = m[0], r1 = m[1], r2 = m[2];
    *o = mk(((r0.x * r.o.x + r0.y * r.o.y) + r0.z * r.o.z) + r0.w,
            ((r1.x * r.o.x + r1.y * r.o.y) + r1.z * r.o.z) + r1.w,
            ((r2.x * r.o.x + r2.y * r.o.y) + r2.z * r.o.z) + r2.w);
    *d = mk((r0.x * r.d.x + r0.y * r.d.y) + r0.z * r.d.z,
            (r1.x * r.d.x + r1.y * r.d.y) + r1.z * r.d.z,
            (r2.x * r.d.x + r2.y * r.d.y) + r2.z * r.d.z);
}
/* rtTransformNormal(RT_OBJECT_TO_WORLD, n) = transpose(W2O) n */
PMD v3 xform_normal(const float4 *m, v3 n) {
    float4 r0 = m[0], r1 = m[1], r2 = m[2];
    return mk((r0.x * n.x + r1.x * n.y) + r2.x * n.z,
              (r0.y * n.x + r1.y * n.y) + r2.y * n.z,
              (r0.z * n.x + r1.z * n.y) + r2.z * n.z);
}

/* cudasphere.cu:7-72 */
PMD bool isect_sphere(const float4 *s, const Ray &ray, float *thit) {
    v3 o, d;
    xform_ray(s, ray, &o, &d);
    float rad = s[3].x;
    float A = dot(d, d);
    float B = 2.f * dot(d, o);
    float C = dot(o, o) - rad * rad;
    float discrim = B * B - 4.f * A * C;
    if (discrim < 0.f) return false;
    float root = sqrtf(discrim);
    float q = (B < 0) ? -.5f * (B - root) : -.5f * (B + root);
    float t0 = q / A, t1 = C / q;
    if (t0 > t1) { float tmp = t0; t0 = t1; t1 = tmp; }
    if (t0 > ray.tmin && t0 < ray.tmax) { *thit = t0; return true; }
    if (t1 > ray.tmin && t1 < ray.tmax) { *thit = t1; return true; }
    return false;
}

/* pbrt Transform::operator()(Point) for an affine transform (its w row is
 * (0, 0, 0, 1), checked at pm_add_mesh_instance, so w == 1 and no divide):
 * the host's flattening evaluates m[0] * x + m[1] * y + m[2] * z + m[3]
 * left to right — the same IEEE operations, in the same order */
PMD v3 inst_point(const float4 *m, float x, float y, float z) {
    const float4 r0 = m[0], r1 = m[1], r2 = m[2];
    return mk(((r0.x * x + r0.y * y) + r0.z * z) + r0.w, ((r1.x * x + r1.y * y) + r1.z * z) + r1.w,
              ((r2.x * x + r2.y * y) + r2.z * z) + r2.w);
}
/* object slot k of instance record I as the world triangle pm_commit would
 * have stored for the flattened mesh (tri_record: p0, e0 = p1 - p0,
 * e1 = p0 - p2, n = e1 x e0) */
PMD void inst_tri(const SceneDev &S, const float4 *I, uint32_t k, v3 &p0, v3 &p1, v3 &p2, float4 g[3]) {
    const float4 a = S.obj_v[3 * k], b = S.obj_v[3 * k + 1], c = S.obj_v[3 * k + 2];
    p0 = inst_point(I, a.x, a.y, a.z);
    p1 = inst_point(I, b.x, b.y, b.z);
    p2 = inst_point(I, c.x, c.y, c.z);
    const v3 e0 = p1 - p0, e1 = p0 - p2;
    const v3 n = mk(e1.y * e0.z - e1.z * e0.y, e1.z * e0.x - e1.x * e0.z, e1.x * e0.y - e1.y * e0.x);
    g[0] = make_float4(p0.x, p0.y, p0.z, e0.x);
    g[1] = make_float4(e0.y, e0.z, e1.x, e1.y);
    g[2] = make_float4(e1.z, n.x, n.y, n.z);
}

} // namespace pm
