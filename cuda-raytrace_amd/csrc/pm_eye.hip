/*
 * pm_eye.hip — eye-side kernels (HIP/CDNA4).
 *
 *   k_eye          eye pass: camera ray -> specular chain -> gather record +
 *                  direct light with shadow rays   (raytracing.cu:19-147)
 *   k_eye_resample eye pass k > 0 of a resampled render (pm_eye_resample): the
 *                  records move under their statistics, dl accumulates
 *   k_simple       the simple renderer: direct light per eye sample
 *                  (simple_render/simplerender.cu)
 *   k_camera_rays  pm_camera_rays: the rays of pm_set_camera's samples
 * (photon pass: pm_trace.hip)
 */
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

/* ====================================================================== */
/* eye pass                                                               */
/* ====================================================================== */
/* CAM: the rays of pm_set_camera (camera_ray above) over the sample
 * raster P.W x P.H; uniform per launch, so the pinhole / host-ray
 * instantiations (CAM = false) carry none of it */
/* TEX: the committed scene has a textured material (SceneDev::tex_recs): the
 * direct light's f takes Kd from the texture at the hit, and the record's
 * albedo factor goes to P.kd (pm_kernels.h EyeParams::kd). The other
 * instantiations hold none of it. */
/* SPEC: the committed scene has a material of the physical specular model
 * (SceneDev::mat_spec; always with TEX): the chain follows one branch per
 * sample, picked with a Philox draw keyed like the light samples (word 2 = 2,
 * word 3 = the depth), and carries an rgb throughput T that multiplies what
 * the record contributes: dl = T L, P.kd = T x (the texel, or 1). A material
 * of the reference's model in such a scene steps as it always did. */
/* RESAMPLE (with CAM, without TEX and SPEC): eye pass P.pass > 0 of
 * pm_eye_resample. The record keeps its statistics (state, n) and moves under
 * them: the camera randoms and the light samples take P.pass as counter word
 * 3, pos / nrm are this sample's, and dl += this sample's direct light (0 for
 * a miss or an exception). Padding records are left as pass 0 wrote them. The
 * other instantiations hold none of it: their pass is the constant 0. */
template <int MODE, bool CAM, bool TEX, bool SPEC, bool RESAMPLE = false>
PMD void eye_body(const EyeParams &P) {
    extern __shared__ __attribute__((aligned(16))) int stk[]; /* [stack_depth x EYE_BLOCK][scene blob (LDS)] */
    int *stack = stk + threadIdx.x;
    const SceneDev S = scene_view<mode_lds(MODE)>(P.S, reinterpret_cast<uint4 *>(stk + P.S.stack_depth * EYE_BLOCK),
                                                       threadIdx.x, EYE_BLOCK);
    if (mode_lds(MODE)) __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * EYE_BLOCK + threadIdx.x;
    if (r >= P.R.count) return;

    Ray ray;
    int64_t pixel;
    float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const uint32_t pass = RESAMPLE ? P.pass : 0u;
    if (CAM) {
        int px, py;
        rec_to_pixel(r, P.W, &px, &py);
        if (px >= P.W || py >= P.H) {
            if (RESAMPLE) return;
            P.R.pos[r] = make_float4(0.f, 0.f, 0.f, __int_as_float(PM_REC_INVALID));
            P.R.nrm[r] = zero4; P.R.state[r] = zero4; P.R.n[r] = 0.f; P.R.dl[r] = zero4;
            if (TEX) P.kd[r] = zero4;
            return;
        }
        pixel = (int64_t)py * P.W + px; /* the sample index q: keys the light samples below */
        float fx, fy;
        camera_ray(P.cam, P.eye, P.fwd, P.right, P.up, P.W, P.H, px, py, pass, &ray.o, &ray.d, &fx, &fy);
    } else if (P.pinhole) {
        int px, py;
        rec_to_pixel(r, P.W, &px, &py);
        if (px >= P.W || py >= P.H) {
            P.R.pos[r] = make_float4(0.f, 0.f, 0.f, __int_as_float(PM_REC_INVALID));
            P.R.nrm[r] = zero4; P.R.state[r] = zero4; P.R.n[r] = 0.f; P.R.dl[r] = zero4;
            if (TEX) P.kd[r] = zero4;
            return;
        }
        pixel = (int64_t)py * P.W + px;
        float sx = (2.0f * ((float)px + 0.5f)) / (float)P.W - 1.0f;
        float sy = 1.0f - (2.0f * ((float)py + 0.5f)) / (float)P.H;
        v3 d = xyz(P.fwd) + sx * xyz(P.right) + sy * xyz(P.up);
        ray.o = xyz(P.eye);
        ray.d = normalize(d);
    } else {
        pixel = r;
        const float *q = P.rays + 6 * r;
        ray.o = mk(q[0], q[1], q[2]);
        ray.d = mk(q[3], q[4], q[5]);
    }
    ray.tmin = P.eps;
    ray.tmax = RT_DEFAULT_MAX;

    int depth = 0;
    Hit h;
    Geo g;
    uint32_t flags = 0;
    v3 T = mk(1.f, 1.f, 1.f); /* SPEC: the chain's throughput */
    while (true) {
        if (!traverse<false, MODE>(S, ray, h, stack, EYE_BLOCK)) { flags = PM_REC_MISS; break; }
        g = shade<MODE == MODE_INST>(S, ray, h);
        const v3 point = ray.o + ray.d * h.t;
        int mtype = fbits(S.materials[g.material].w);
        if (is_specular(mtype)) {
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
                                       (uint32_t)(depth + 1), P.light_seed, 0u, o4);
                    u = pmdm_u01(o4[0]);
                }
                v3 w; float eta2;
                ok = material_specular_pbrt(mtype, sa, sb, g, -ray.d, u, &wi, &w, &eta2);
                if (ok) T = (T * w) * eta2; /* radiance: a transmitted step scales by (ei / et)^2 */
            } else {
                ok = material_specular(mtype, g, -ray.d, &wi);
            }
            depth++;
            if (depth > P.max_spec || !ok) { flags = PM_REC_EXCEPTION; break; }
            ray.o = point; ray.d = wi; ray.tmin = P.eps; ray.tmax = RT_DEFAULT_MAX;
            continue;
        }
        ray.o = point; /* keep the hit point; ray.d stays the incident direction */
        break;
    }
    if (flags) {
        P.R.pos[r] = make_float4(0.f, 0.f, 0.f, __int_as_float((int)flags));
        if (RESAMPLE) { /* this sample adds no light (dl + 0 is dl: a sum from +0 is never -0); the statistics stay */
            P.R.nrm[r] = zero4;
            return;
        }
        P.R.nrm[r] = zero4; P.R.state[r] = zero4; P.R.n[r] = 0.f; P.R.dl[r] = zero4;
        if (TEX) P.kd[r] = zero4;
        return;
    }
    const v3 point = ray.o, ns = g.ns, dir = ray.d;
    /* the factor pm_final applies to the record's indirect term: the texel of
     * a textured matte (whose table Kd is 1), else 1 */
    v3 kdf = mk(1.f, 1.f, 1.f);
    bool textured = false;
    if (TEX) { /* looked up for every hit, whatever the light guard below decides */
        textured = fbits(S.materials[g.material].w) == PM_MATTE && S.mat_tex[g.material] >= 0;
        if (textured) kdf = hit_kd<MODE == MODE_INST>(S, h, point, g.material, kdf);
    }

    /* directLight (raytracing.cu:49-84) */
    v3 L = mk(0.f, 0.f, 0.f);
    const int total = S.n_lights;
    if (g.light < total) {
        if (g.light >= 0) L = L + light_le(S.lights[g.light], -dir, g.ng);
        float4 m = S.materials[g.material];
        v3 kd = xyz(m);
        if (TEX && textured) kd = kdf;
        v3 fv = fbits(m.w) == PM_MATTE ? kd * INV_PI : mk(0.f, 0.f, 0.f);
        for (int i = 0; i < total; ++i) {
            const LightDev Lt = S.lights[i];
            const int nS = fbits(Lt.p1_ns.w);
            const int ltype = fbits(Lt.o_type.w);
            for (int s = 0; s < nS; ++s) {
                float u1 = 0.f, u2 = 0.f;
                if (ltype == PM_LIGHT_AREA_DISK || ltype == PM_LIGHT_AREA_MESH) {
                    int slot = fbits(Lt.p2_r2d.w) + s;
                    if (P.pinhole) {
                        uint32_t o4[4];
                        pmdm_philox4x32_10((uint32_t)pixel, (uint32_t)slot, 0u, pass, P.light_seed, 0u, o4);
                        u1 = pmdm_u01(o4[0]); u2 = pmdm_u01(o4[1]);
                    } else {
                        const float *q = P.rand2d + ((size_t)pixel * P.n2d + slot) * 2;
                        u1 = q[0]; u2 = q[1];
                    }
                }
                v3 uwi; float pdf;
                v3 li = sample_l_shading(Lt, S.light_tris, point, u1, u2, &uwi, &pdf);
                Ray sr;
                sr.o = point; sr.d = uwi; sr.tmin = 0.001f; sr.tmax = 1.0f - 0.001f;
                Hit sh;
                float atten = traverse<true, MODE>(S, sr, sh, stack, EYE_BLOCK) ? 0.0f : 1.0f;
                v3 wi = normalize(uwi);
                L = L + (atten * fabsf(dot(ns, wi))) * fv * li / (pdf * nS);
            }
        }
    }
    /* Faceforward(nn, wo) side, for the kNN estimator (the reference keeps
     * record.direction itself, raytracing.cu:117) */
    const uint32_t side = dot(ns, -dir) < 0.f ? PM_REC_BACKFACE : 0u;
    P.R.pos[r] = make_float4(point.x, point.y, point.z, __uint_as_float(side));
    P.R.nrm[r] = make_float4(ns.x, ns.y, ns.z, __int_as_float(g.material));
    if (RESAMPLE) { /* one fp32 add per channel onto the earlier samples' sum */
        const float4 a = P.R.dl[r];
        P.R.dl[r] = make_float4(a.x + L.x, a.y + L.y, a.z + L.z, 0.f);
        return;
    }
    P.R.state[r] = make_float4(0.f, 0.f, 0.f, P.r2init);
    P.R.n[r] = 0.f;
    if (SPEC) { L = T * L; kdf = T * kdf; }
    P.R.dl[r] = make_float4(L.x, L.y, L.z, 0.f);
    if (TEX) P.kd[r] = make_float4(kdf.x, kdf.y, kdf.z, 0.f);
}

template <int MODE, bool CAM = false, bool TEX = false>
__global__ __launch_bounds__(EYE_BLOCK) void k_eye(EyeParams P) { eye_body<MODE, CAM, TEX, false>(P); }
template <int MODE, bool CAM>
__global__ __launch_bounds__(EYE_BLOCK) void k_eye_spec(EyeParams P) { eye_body<MODE, CAM, true, true>(P); }
template <int MODE>
__global__ __launch_bounds__(EYE_BLOCK) void k_eye_resample(EyeParams P) { eye_body<MODE, true, false, false, true>(P); }

template <bool CAM, bool TEX>
static void launch_eye_mode(const EyeParams &p, unsigned grid, size_t lds, hipStream_t s) {
    switch (scene_mode(p.S)) {
    case MODE_BRUTE: pm_launch((k_eye<MODE_BRUTE, CAM, TEX>), dim3(grid), dim3(EYE_BLOCK), lds, s, p); break;
    case MODE_LDS: pm_launch((k_eye<MODE_LDS, CAM, TEX>), dim3(grid), dim3(EYE_BLOCK), lds, s, p); break;
    case MODE_INST: pm_launch((k_eye<MODE_INST, CAM, TEX>), dim3(grid), dim3(EYE_BLOCK), lds, s, p); break;
    default: pm_launch((k_eye<MODE_GLOBAL, CAM, TEX>), dim3(grid), dim3(EYE_BLOCK), lds, s, p); break;
    }
}

template <bool CAM>
static void launch_eye_spec(const EyeParams &p, unsigned grid, size_t lds, hipStream_t s) {
    switch (scene_mode(p.S)) {
    case MODE_BRUTE: pm_launch((k_eye_spec<MODE_BRUTE, CAM>), dim3(grid), dim3(EYE_BLOCK), lds, s, p); break;
    case MODE_LDS: pm_launch((k_eye_spec<MODE_LDS, CAM>), dim3(grid), dim3(EYE_BLOCK), lds, s, p); break;
    case MODE_INST: pm_launch((k_eye_spec<MODE_INST, CAM>), dim3(grid), dim3(EYE_BLOCK), lds, s, p); break;
    default: pm_launch((k_eye_spec<MODE_GLOBAL, CAM>), dim3(grid), dim3(EYE_BLOCK), lds, s, p); break;
    }
}

hipError_t launch_eye(const EyeParams &p, hipStream_t s) {
    if (p.R.count <= 0) return hipSuccess;
    unsigned grid = (unsigned)((p.R.count + EYE_BLOCK - 1) / EYE_BLOCK);
    const size_t lds = (size_t)p.S.stack_depth * EYE_BLOCK * 4 + p.S.lds_bytes;
    if (p.S.mat_spec) { /* a material of the physical specular model: the SPEC instantiations */
        if (!p.kd || !p.S.mat_tex) return hipErrorInvalidValue;
        if (p.camera) launch_eye_spec<true>(p, grid, lds, s);
        else launch_eye_spec<false>(p, grid, lds, s);
    } else if (p.S.tex_recs) { /* a textured scene: the TEX instantiations, which write the records' albedo */
        if (!p.kd) return hipErrorInvalidValue;
        if (p.camera) launch_eye_mode<true, true>(p, grid, lds, s);
        else launch_eye_mode<false, true>(p, grid, lds, s);
    } else if (p.camera) launch_eye_mode<true, false>(p, grid, lds, s);
    else launch_eye_mode<false, false>(p, grid, lds, s);
    return hipGetLastError();
}

hipError_t launch_eye_resample(const EyeParams &p, hipStream_t s) {
    if (p.R.count <= 0) return hipSuccess;
    if (!p.camera || p.pass == 0u || p.S.mat_spec || p.S.tex_recs) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((p.R.count + EYE_BLOCK - 1) / EYE_BLOCK);
    const size_t lds = (size_t)p.S.stack_depth * EYE_BLOCK * 4 + p.S.lds_bytes;
    switch (scene_mode(p.S)) {
    case MODE_BRUTE: pm_launch((k_eye_resample<MODE_BRUTE>), dim3(grid), dim3(EYE_BLOCK), lds, s, p); break;
    case MODE_LDS: pm_launch((k_eye_resample<MODE_LDS>), dim3(grid), dim3(EYE_BLOCK), lds, s, p); break;
    case MODE_INST: pm_launch((k_eye_resample<MODE_INST>), dim3(grid), dim3(EYE_BLOCK), lds, s, p); break;
    default: pm_launch((k_eye_resample<MODE_GLOBAL>), dim3(grid), dim3(EYE_BLOCK), lds, s, p); break;
    }
    return hipGetLastError();
}

/* ====================================================================== */
/* simple renderer (direct light only, simple_render/simplerender.cu)     */
/* ====================================================================== */
/* One lane per eye sample: closest hit of the camera ray (no specular
 * chain), then for every light one shadow-tested sample (iSample 0, no pdf
 * division, no emitted term): L += att·|ns·wi|·f·li (simplerender.cu:40-72);
 * a miss is black (:75-79). The host's NaN / negative / infinite check
 * (simplerender.cpp:70-87) is fused into the store. Output: raster order
 * (pinhole) or sample order (host rays), float3 per sample. */
template <int MODE, bool CAM = false, bool TEX = false>
__global__ __launch_bounds__(EYE_BLOCK) void k_simple(EyeParams P, float *out) {
    extern __shared__ __attribute__((aligned(16))) int stk[];
    int *stack = stk + threadIdx.x;
    const SceneDev S = scene_view<mode_lds(MODE)>(P.S, reinterpret_cast<uint4 *>(stk + P.S.stack_depth * EYE_BLOCK),
                                                       threadIdx.x, EYE_BLOCK);
    if (mode_lds(MODE)) __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * EYE_BLOCK + threadIdx.x;
    if (r >= P.R.count) return;

    Ray ray;
    int64_t pixel;
    if (CAM) {
        int px, py;
        rec_to_pixel(r, P.W, &px, &py);
        if (px >= P.W || py >= P.H) return;
        pixel = (int64_t)py * P.W + px;
        float fx, fy;
        camera_ray(P.cam, P.eye, P.fwd, P.right, P.up, P.W, P.H, px, py, 0u, &ray.o, &ray.d, &fx, &fy);
    } else if (P.pinhole) {
        int px, py;
        rec_to_pixel(r, P.W, &px, &py);
        if (px >= P.W || py >= P.H) return;
        pixel = (int64_t)py * P.W + px;
        float sx = (2.0f * ((float)px + 0.5f)) / (float)P.W - 1.0f;
        float sy = 1.0f - (2.0f * ((float)py + 0.5f)) / (float)P.H;
        v3 d = xyz(P.fwd) + sx * xyz(P.right) + sy * xyz(P.up);
        ray.o = xyz(P.eye);
        ray.d = normalize(d);
    } else {
        pixel = r;
        const float *q = P.rays + 6 * r;
        ray.o = mk(q[0], q[1], q[2]);
        ray.d = mk(q[3], q[4], q[5]);
    }
    ray.tmin = P.eps;
    ray.tmax = RT_DEFAULT_MAX;

    v3 L = mk(0.f, 0.f, 0.f);
    Hit h;
    if (traverse<false, MODE>(S, ray, h, stack, EYE_BLOCK)) {
        const Geo g = shade<MODE == MODE_INST>(S, ray, h);
        const v3 point = ray.o + ray.d * h.t;
        const float4 m = S.materials[g.material];
        v3 kd = xyz(m);
        if (TEX && fbits(m.w) == PM_MATTE) kd = hit_kd<MODE == MODE_INST>(S, h, point, g.material, kd);
        const v3 fv = fbits(m.w) == PM_MATTE ? kd * INV_PI : mk(0.f, 0.f, 0.f); /* f(wo, wi) */
        for (int i = 0; i < S.n_lights; ++i) {
            const LightDev Lt = S.lights[i];
            float u1 = 0.f, u2 = 0.f;
            if (fbits(Lt.o_type.w) == PM_LIGHT_AREA_DISK || fbits(Lt.o_type.w) == PM_LIGHT_AREA_MESH) {
                const int slot = fbits(Lt.p2_r2d.w); /* random2DStart + iSample 0 */
                if (P.pinhole) {
                    uint32_t o4[4];
                    pmdm_philox4x32_10((uint32_t)pixel, (uint32_t)slot, 0u, 0u, P.light_seed, 0u, o4);
                    u1 = pmdm_u01(o4[0]); u2 = pmdm_u01(o4[1]);
                } else {
                    const float *q = P.rand2d + ((size_t)pixel * P.n2d + slot) * 2;
                    u1 = q[0]; u2 = q[1];
                }
            }
            v3 uwi; float pdf;
            const v3 li = sample_l_shading(Lt, S.light_tris, point, u1, u2, &uwi, &pdf);
            Ray sr;
            sr.o = point; sr.d = uwi; sr.tmin = 0.001f; sr.tmax = 1.0f - 0.001f;
            Hit sh;
            const float atten = traverse<true, MODE>(S, sr, sh, stack, EYE_BLOCK) ? 0.0f : 1.0f;
            const v3 wi = normalize(uwi);
            L = L + (atten * fabsf(dot(g.ns, wi))) * fv * li;
        }
    }
    const float y = 0.212671f * L.x + 0.715160f * L.y + 0.072169f * L.z; /* pbrt RGBSpectrum::y */
    if (isnan(L.x) || isnan(L.y) || isnan(L.z) || y < -1e-5f || isinf(y)) L = mk(0.f, 0.f, 0.f);
    out[3 * pixel + 0] = L.x;
    out[3 * pixel + 1] = L.y;
    out[3 * pixel + 2] = L.z;
}

template <bool CAM, bool TEX>
static void launch_simple_mode(const EyeParams &p, float *out, unsigned grid, size_t lds, hipStream_t s) {
    switch (scene_mode(p.S)) {
    case MODE_BRUTE: pm_launch((k_simple<MODE_BRUTE, CAM, TEX>), dim3(grid), dim3(EYE_BLOCK), lds, s, p, out); break;
    case MODE_LDS: pm_launch((k_simple<MODE_LDS, CAM, TEX>), dim3(grid), dim3(EYE_BLOCK), lds, s, p, out); break;
    case MODE_INST: pm_launch((k_simple<MODE_INST, CAM, TEX>), dim3(grid), dim3(EYE_BLOCK), lds, s, p, out); break;
    default: pm_launch((k_simple<MODE_GLOBAL, CAM, TEX>), dim3(grid), dim3(EYE_BLOCK), lds, s, p, out); break;
    }
}

hipError_t launch_simple(const EyeParams &p, float *out, hipStream_t s) {
    if (p.R.count <= 0) return hipSuccess;
    unsigned grid = (unsigned)((p.R.count + EYE_BLOCK - 1) / EYE_BLOCK);
    const size_t lds = (size_t)p.S.stack_depth * EYE_BLOCK * 4 + p.S.lds_bytes;
    if (p.S.tex_recs) {
        if (p.camera) launch_simple_mode<true, true>(p, out, grid, lds, s);
        else launch_simple_mode<false, true>(p, out, grid, lds, s);
    } else if (p.camera) launch_simple_mode<true, false>(p, out, grid, lds, s);
    else launch_simple_mode<false, false>(p, out, grid, lds, s);
    return hipGetLastError();
}

/* pm_camera_rays_pass: the rays and film positions of samples [first, first +
 * count) in raster order for eye pass P.pass, through camera_ray as the eye
 * pass calls it */
__global__ __launch_bounds__(256) void k_camera_rays(EyeParams P, int64_t first, int64_t count, float *rays6,
                                                     float *film_xy) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t q = first + i;
    const int ix = (int)(q % P.W), iy = (int)(q / P.W);
    v3 o, d;
    float fx, fy;
    camera_ray(P.cam, P.eye, P.fwd, P.right, P.up, P.W, P.H, ix, iy, P.pass, &o, &d, &fx, &fy);
    if (rays6) {
        float *r = rays6 + 6 * i;
        r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z;
    }
    if (film_xy) { film_xy[2 * i] = fx; film_xy[2 * i + 1] = fy; }
}

hipError_t launch_camera_rays(const EyeParams &p, int64_t first, int64_t count, float *rays6, float *film_xy,
                              hipStream_t s) {
    if (count <= 0) return hipSuccess;
    pm_launch(k_camera_rays, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, p, first, count, rays6, film_xy);
    return hipGetLastError();
}

} // namespace pm
