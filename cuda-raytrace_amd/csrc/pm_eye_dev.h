/*
 * pm_eye_dev.h — device-inline code shared by the units that trace from the
 * eye (pm_eye.hip: k_eye, k_eye_spec, k_eye_resample, k_simple, k_camera_rays;
 * pm_fgather.hip: k_fg_rays), which walk one specular chain and sum one direct
 * light bit for bit: the camera and primary rays (camera_ray, primary_ray),
 * the walk to a non-specular hit (specular_chain), the loop over lights and
 * their samples with a shadow ray each (direct_light) and the store of a
 * record that holds nothing (store_inactive). Only what more than one kernel
 * uses lives here.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "pm_kernels.h"
#include "pm_sample.h"
#include "pm_shade.h"
#include "pm_traverse.h"

#pragma clang fp contract(off)

namespace pm {

/* The camera ray of sample (ix, iy) of the WS x HS raster, in the order of
 * operations pm_api.h pins (its jitter and film position, camera_randoms and
 * camera_film_xy of pm_kernels.h, are the film kernel's too): shared by k_eye,
 * k_simple and k_camera_rays. pass: the eye pass of a resampled render
 * (pm_eye_resample), the constant 0 anywhere else. */
PMD void camera_ray(const CameraDev &C, float4 eye4, float4 fwd4, float4 right4, float4 up4, int WS, int HS, int ix,
                    int iy, uint32_t pass, v3 *o, v3 *d, float *fx, float *fy) {
    float ju, jv, lu, lv;
    camera_randoms(C, (int64_t)iy * WS + ix, pass, &ju, &jv, &lu, &lv);
    camera_film_xy(C, ix, iy, ju, jv, fx, fy);
    const v3 eye = xyz(eye4), fwd = xyz(fwd4), right = xyz(right4), up = xyz(up4);
    const float sx = (2.0f * ((float)ix + ju)) / (float)WS - 1.0f;
    const float sy = 1.0f - (2.0f * ((float)iy + jv)) / (float)HS;
    const v3 d0 = fwd + sx * right + sy * up;
    if (C.lens_radius > 0.0f) {
        float cx, cy;
        concentric_sample_disk(lu, lv, &cx, &cy);
        const v3 ol = eye + C.lens_radius * (cx * normalize(right) + cy * normalize(up));
        const float ft = C.focal / sqrtf(dot(fwd, fwd));
        const v3 pf = eye + d0 * ft;
        *o = ol;
        *d = normalize(pf - ol);
    } else {
        *o = eye;
        *d = normalize(d0);
    }
}

/* The ray of record r and the sample index that keys its light samples: the
 * raster sample's camera ray (CAM: camera_ray in eye pass `pass`, over the
 * sample raster P.W x P.H; uniform per launch, so the other instantiations
 * carry none of it), the pinhole ray through its centre, or host ray r. False
 * for a record of the 8x8-tile ordering outside the raster. */
template <bool CAM>
PMD bool primary_ray(const EyeParams &P, int64_t r, uint32_t pass, Ray *ray, int64_t *pixel) {
    if (CAM || P.pinhole) {
        int px, py;
        rec_to_pixel(r, P.W, &px, &py);
        if (px >= P.W || py >= P.H) return false;
        *pixel = (int64_t)py * P.W + px;
        if (CAM) {
            float fx, fy;
            camera_ray(P.cam, P.eye, P.fwd, P.right, P.up, P.W, P.H, px, py, pass, &ray->o, &ray->d, &fx, &fy);
        } else {
            float sx = (2.0f * ((float)px + 0.5f)) / (float)P.W - 1.0f;
            float sy = 1.0f - (2.0f * ((float)py + 0.5f)) / (float)P.H;
            v3 d = xyz(P.fwd) + sx * xyz(P.right) + sy * xyz(P.up);
            ray->o = xyz(P.eye);
            ray->d = normalize(d);
        }
    } else {
        *pixel = r;
        const float *q = P.rays + 6 * r;
        ray->o = mk(q[0], q[1], q[2]);
        ray->d = mk(q[3], q[4], q[5]);
    }
    ray->tmin = P.eps;
    ray->tmax = RT_DEFAULT_MAX;
    return true;
}

/* The walk from `ray` to its first non-specular hit (raytracing.cu:19-47).
 * Returns 0 with the hit in h and g, the hit point in ray.o and the incident
 * direction left in ray.d; PM_REC_MISS when a ray leaves the scene;
 * PM_REC_EXCEPTION after more than max_spec specular steps or a step without
 * a direction. SPEC: a material of the physical specular model follows one
 * branch per sample, picked with a Philox draw keyed by `pixel` (counter word
 * 2 = 2, word 3 = the depth) under `seed`, and multiplies the chain's rgb
 * throughput into *T; a material of the reference's model steps as it always
 * did. Without SPEC pixel, seed and T are not read. */
template <int MODE, bool SPEC>
PMD uint32_t specular_chain(const SceneDev &S, int *stack, Ray &ray, Hit &h, Geo &g, float eps, int max_spec,
                            int64_t pixel, uint32_t seed, v3 *T) {
    int depth = 0;
    while (true) {
        if (!traverse<false, MODE>(S, ray, h, stack, EYE_BLOCK)) return PM_REC_MISS;
        g = shade<MODE == MODE_INST>(S, ray, h);
        const v3 point = ray.o + ray.d * h.t;
        int mtype = fbits(S.materials[g.material].w);
        if (!is_specular(mtype)) {
            ray.o = point; /* keep the hit point; ray.d stays the incident direction */
            return 0u;
        }
        v3 wi;
        bool ok;
        float4 sa, sb;
        bool pbrt = false;
        if (SPEC) {
            sa = S.mat_spec[2 * g.material]; sb = S.mat_spec[2 * g.material + 1];
            pbrt = fbits(sb.w) != 0;
        }
        if (SPEC && pbrt) {
            float u = 0.f;
            if (mtype == PM_GLASS) {
                uint32_t o4[4];
                pmdm_philox4x32_10((uint32_t)((uint64_t)pixel & 0xffffffffu), (uint32_t)((uint64_t)pixel >> 32), 2u,
                                   (uint32_t)(depth + 1), seed, 0u, o4);
                u = pmdm_u01(o4[0]);
            }
            v3 w; float eta2;
            ok = material_specular_pbrt(mtype, sa, sb, g, -ray.d, u, &wi, &w, &eta2);
            if (ok) *T = (*T * w) * eta2; /* radiance: a transmitted step scales by (ei / et)^2 */
        } else {
            ok = material_specular(mtype, g, -ray.d, &wi);
        }
        depth++;
        if (depth > max_spec || !ok) return PM_REC_EXCEPTION;
        ray.o = point; ray.d = wi; ray.tmin = eps; ray.tmax = RT_DEFAULT_MAX;
    }
}

/* L plus the light every light sends to `point` (shading normal ns, f(wo, wi)
 * = fv): directLight's loop over the lights and their samples
 * (raytracing.cu:49-84), a shadow ray per sample, each term
 * (atten |ns . wi|) fv li / (pdf nS) added to L in light, then sample order.
 * sampler(slot, &u1, &u2) supplies the sample of light slot `slot`
 * (random2DStart + the sample's number) and is called for disk and mesh lights
 * alone; every other light takes (0, 0). FIRST_ONLY (the simple renderer,
 * simplerender.cu:40-72): sample 0 of every light, not divided by its pdf.
 * The emitted term of a hit on a light, and the guard that skips a hit whose
 * g.light is out of range, stay with the caller. */
template <int MODE, bool FIRST_ONLY = false, class Sampler>
PMD v3 direct_light(const SceneDev &S, int *stack, v3 point, v3 ns, v3 fv, v3 L, Sampler sampler) {
    for (int i = 0; i < S.n_lights; ++i) {
        const LightDev Lt = S.lights[i];
        const int ltype = fbits(Lt.o_type.w);
        /* sample s of the light, shadow-tested: (atten |ns . wi|) fv li and its pdf */
        auto term = [&](int s, float *pdf) {
            float u1 = 0.f, u2 = 0.f;
            if (ltype == PM_LIGHT_AREA_DISK || ltype == PM_LIGHT_AREA_MESH) sampler(fbits(Lt.p2_r2d.w) + s, &u1, &u2);
            v3 uwi;
            const v3 li = sample_l_shading(Lt, S.light_tris, point, u1, u2, &uwi, pdf);
            Ray sr;
            sr.o = point; sr.d = uwi; sr.tmin = 0.001f; sr.tmax = 1.0f - 0.001f;
            Hit sh;
            const float atten = traverse<true, MODE>(S, sr, sh, stack, EYE_BLOCK) ? 0.0f : 1.0f;
            const v3 wi = normalize(uwi);
            return (atten * fabsf(dot(ns, wi))) * fv * li;
        };
        float pdf;
        if (FIRST_ONLY) { /* no loop of one turn: as such k_simple<MODE_BRUTE> spilled two SGPRs it did not before */
            L = L + term(0, &pdf);
        } else {
            const int nS = fbits(Lt.p1_ns.w);
            for (int s = 0; s < nS; ++s) {
                const v3 c = term(s, &pdf);
                L = L + c / (pdf * nS);
            }
        }
    }
    return L;
}

/* a record that holds nothing: flags (PM_REC_MISS, _EXCEPTION or _INVALID) in
 * pos.w, every other word 0, its albedo factor (TEX) included */
template <bool TEX>
PMD void store_inactive(const RecordsDev &R, float4 *kd, int64_t i, uint32_t flags) {
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    R.pos[i] = make_float4(0.f, 0.f, 0.f, __int_as_float((int)flags));
    R.nrm[i] = zero4; R.state[i] = zero4; R.n[i] = 0.f; R.dl[i] = zero4;
    if (TEX) kd[i] = zero4;
}

} // namespace pm
