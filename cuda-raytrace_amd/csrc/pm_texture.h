/*
 * pm_texture.h — device-side texture lookup (included at the end of
 * pm_shade.h): the (u, v) of a triangle hit and tex_eval, which maps a texture
 * record (pm_scene_pod.h TexRec) and (u, v) to the rgb of a matte Kd. The
 * photon bounce, the eye pass and the simple renderer all call it.
 *
 * The image lookup is pbrt-v2's MIPMap::triangle(0, s, t), level 0 only: in
 * texel space x = s w - 0.5, y = t h - 0.5, the four texels around it fetched
 * through the wrap mode and blended as a + f (b - a), along x on both rows,
 * then along y. That form is part of the contract (pm_api.h): four equal
 * texels return that texel bit for bit.
 */
#pragma once

namespace pm {

/* texel (x, y) of an image operand through its wrap mode; every index that
 * reaches memory lies in [0, w) x [0, h) */
PMD v3 tex_texel(const float4 *texels, const TexOperand &o, int x, int y) {
    if (o.wrap == TEX_WRAP_REPEAT) { /* pbrt's Mod */
        x %= o.w; if (x < 0) x += o.w;
        y %= o.h; if (y < 0) y += o.h;
    } else if (o.wrap == TEX_WRAP_CLAMP) {
        x = x < 0 ? 0 : (x >= o.w ? o.w - 1 : x);
        y = y < 0 ? 0 : (y >= o.h ? o.h - 1 : y);
    } else if (x < 0 || x >= o.w || y < 0 || y >= o.h) {
        return mk(0.f, 0.f, 0.f);
    }
    return xyz(texels[(size_t)o.texel0 + (size_t)y * (size_t)o.w + (size_t)x]);
}

/* a texel-space coordinate held where its floor converts to int and + 1 does
 * not overflow (a NaN becomes the lower bound) */
PMD float tex_coord(float x) { return fminf(fmaxf(x, -1.0e9f), 1.0e9f); }

PMD v3 tex_operand(const float4 *texels, const TexOperand &o, float u, float v) {
    const v3 c = mk(o.rgb[0], o.rgb[1], o.rgb[2]);
    if (o.texel0 < 0) return c;
    const float s = o.map[0] * u + o.map[2], t = o.map[1] * v + o.map[3];
    const float x = tex_coord(s * (float)o.w - 0.5f), y = tex_coord(t * (float)o.h - 0.5f);
    const float x0 = floorf(x), y0 = floorf(y);
    const float fx = x - x0, fy = y - y0;
    const int ix = (int)x0, iy = (int)y0;
    const v3 a = tex_texel(texels, o, ix, iy), b = tex_texel(texels, o, ix + 1, iy);
    const v3 cc = tex_texel(texels, o, ix, iy + 1), d = tex_texel(texels, o, ix + 1, iy + 1);
    const v3 r0 = a + fx * (b - a), r1 = cc + fx * (d - cc);
    return (r0 + fy * (r1 - r0)) * c;
}

/* the rgb of texture record T at (u, v) */
PMD v3 tex_eval(const float4 *texels, const TexRec &T, float u, float v) {
    if (T.kind == TEX_CHECKER) { /* pbrt-v2 Checkerboard2DTexture, aamode "none" */
        const float s = tex_coord(T.map[0] * u + T.map[2]), t = tex_coord(T.map[1] * v + T.map[3]);
        const bool first = ((int)floorf(s) + (int)floorf(t)) % 2 == 0;
        return first ? tex_operand(texels, T.op[0], u, v) : tex_operand(texels, T.op[1], u, v);
    }
    const v3 a = tex_operand(texels, T.op[0], u, v);
    if (T.kind == TEX_SCALE) return a * tex_operand(texels, T.op[1], u, v);
    return a;
}

/* (u, v) of a triangle hit: b0 uv0 + b1 uv1 + b2 uv2 from the hit's
 * barycentrics (b1 = beta, b2 = gamma), summed left to right. A flattened
 * mesh reads its three corners from SceneDev::tri_uv (per storage slot, the
 * default corners (0,0) (1,0) (0,1) of tri_frame already filled in for a mesh
 * without uvs); an instance's triangle reads obj_uv as shade() does, so it
 * equals its flattened copy bit for bit.
 * A disk: pbrt-v2's u = phi / phiMax, v = 1 - (r - r_i) / (R - r_i), from the
 * hit point's coordinates in the disk's frame (normalised by the radius, as
 * isect_disk has them). A full sphere: pbrt-v2's u = phi / 2 pi, v = (theta -
 * thetaMin) / (thetaMax - thetaMin) with thetaMin = pi, thetaMax = 0, from
 * the hit point taken to object space; theta = acos(z / r) is evaluated as
 * atan2(sqrt(x^2 + y^2), z), the same angle through the deterministic atan2. */
template <bool INST>
PMD void hit_uv(const SceneDev &S, const Hit &h, v3 point, float *u, float *v) {
    const uint32_t kind = h.ref >> 30, idx = h.ref & 0x3fffffffu;
    float uv0x = 0.f, uv0y = 0.f, uv1x = 1.f, uv1y = 0.f, uv2x = 0.f, uv2y = 1.f;
    if (INST && kind == PRIM_INST) {
        const int4 vi = S.obj_info[idx];
        if (S.obj_mesh[vi.w].w) {
            const float4 a = S.obj_uv[vi.x], b = S.obj_uv[vi.y], c = S.obj_uv[vi.z];
            uv0x = a.x; uv0y = a.y; uv1x = b.x; uv1y = b.y; uv2x = c.x; uv2y = c.y;
        }
    } else if (kind == PRIM_TRI) {
        const float4 a = S.tri_uv[2 * idx], b = S.tri_uv[2 * idx + 1];
        uv0x = a.x; uv0y = a.y; uv1x = a.z; uv1y = a.w; uv2x = b.x; uv2y = b.y;
    }
    else if (kind == PRIM_DISK) {
        const float4 *dk = S.disks + 5 * idx;
        const float4 a = dk[0], b = dk[1], c = dk[2], d = dk[3], e = dk[4];
        const v3 local = point - xyz(a);
        const float lx = dot(local, xyz(b)) * d.w, ly = dot(local, xyz(c)) * e.x;
        float phi = pmdm_atan2f(ly, lx);
        if (phi < 0.f) phi = (float)((double)phi + 2.f * M_PI);
        const float r = sqrtf(lx * lx + ly * ly);
        *u = phi / b.w;
        *v = 1.0f - (r - a.w) / (1.0f - a.w);
        return;
    } else if (kind == PRIM_SPHERE) {
        const float4 *s = S.spheres + 4 * idx;
        const v3 po = inst_point(s, point.x, point.y, point.z); /* world to object: rows s[0..2] */
        float phi = pmdm_atan2f(po.y, po.x);
        if (phi < 0.f) phi = (float)((double)phi + 2.f * M_PI);
        const float theta = pmdm_atan2f(sqrtf(po.x * po.x + po.y * po.y), po.z);
        const float pi = 3.14159265358979323846f;
        *u = phi / (2.0f * pi);
        *v = (theta - pi) / (0.0f - pi);
        return;
    }
    const float b0 = 1.0f - h.beta - h.gamma;
    *u = (b0 * uv0x + h.beta * uv1x) + h.gamma * uv2x;
    *v = (b0 * uv0y + h.beta * uv1y) + h.gamma * uv2y;
}

/* Kd of a matte hit: the material's colour `kd`, or its texture at the hit */
template <bool INST>
PMD v3 hit_kd(const SceneDev &S, const Hit &h, v3 point, int material, v3 kd) {
    const int t = S.mat_tex[material];
    if (t < 0) return kd;
    float u, v;
    hit_uv<INST>(S, h, point, &u, &v);
    return tex_eval(S.texels, S.tex_recs[t], u, v);
}

} // namespace pm
