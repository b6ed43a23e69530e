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
 *
 * The rays, the specular chain and the direct-light loop are pm_eye_dev.h's,
 * which final gathering (pm_fgather.hip) shares.
 */
#include <hip/hip_runtime.h>

#include "pm_eye_dev.h"

#pragma clang fp contract(off)

namespace pm {

/* the light samples of the eye pass and the simple renderer for sample index
 * `pixel`: a Philox draw keyed (pixel, slot) with the eye pass as counter word
 * 3 (pinhole and camera rays), else the host's rand2d table (host rays) */
struct EyeLightSampler {
    const EyeParams &P;
    int64_t pixel;
    uint32_t pass;
    PMD void operator()(int slot, float *u1, float *u2) const {
        if (P.pinhole) {
            uint32_t o4[4];
            pmdm_philox4x32_10((uint32_t)pixel, (uint32_t)slot, 0u, pass, P.light_seed, 0u, o4);
            *u1 = pmdm_u01(o4[0]); *u2 = pmdm_u01(o4[1]);
        } else {
            const float *q = P.rand2d + ((size_t)pixel * P.n2d + slot) * 2;
            *u1 = q[0]; *u2 = q[1];
        }
    }
};

/* ====================================================================== */
/* eye pass                                                               */
/* ====================================================================== */
/* CAM: the rays of pm_set_camera (primary_ray<true>) */
/* TEX: the committed scene has a textured material (SceneDev::tex_recs): the
 * direct light's f takes Kd from the texture at the hit, and the record's
 * albedo factor goes to P.kd (pm_kernels.h EyeParams::kd). The other
 * instantiations hold none of it. */
/* SPEC: the committed scene has a material of the physical specular model
 * (SceneDev::mat_spec; always with TEX): specular_chain<MODE, true> carries an
 * rgb throughput T that multiplies what the record contributes: dl = T L,
 * P.kd = T x (the texel, or 1). */
/* RESAMPLE (with CAM, without TEX and SPEC): eye pass P.pass > 0 of
 * pm_eye_resample. The record keeps its statistics (state, n) and moves under
 * them: the camera randoms and the light samples take P.pass as counter word
 * 3, pos / nrm are this sample's, and dl += this sample's direct light (0 for
 * a miss or an exception). Padding records are left as pass 0 wrote them. The
 * other instantiations hold none of it: their pass is the constant 0. */
template <int MODE, bool CAM, bool TEX, bool SPEC, bool RESAMPLE = false>
PMD void eye_body(const EyeParams &P) {
    static_assert(!RESAMPLE || CAM, "the resampled eye pass moves its records along pm_set_camera's rays");
    extern __shared__ __attribute__((aligned(16))) int stk[]; /* [stack_depth x EYE_BLOCK][scene blob (LDS)] */
    int *stack = stk + threadIdx.x;
    const SceneDev S = scene_view<mode_lds(MODE)>(P.S, reinterpret_cast<uint4 *>(stk + P.S.stack_depth * EYE_BLOCK),
                                                       threadIdx.x, EYE_BLOCK);
    if (mode_lds(MODE)) __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * EYE_BLOCK + threadIdx.x;
    if (r >= P.R.count) return;

    Ray ray;
    int64_t pixel; /* the sample index q: keys the light samples below */
    const uint32_t pass = RESAMPLE ? P.pass : 0u;
    if (!primary_ray<CAM>(P, r, pass, &ray, &pixel)) {
        if (!RESAMPLE) store_inactive<TEX>(P.R, P.kd, r, PM_REC_INVALID);
        return;
    }
    Hit h;
    Geo g;
    v3 T = mk(1.f, 1.f, 1.f); /* SPEC: the chain's throughput */
    const uint32_t flags = specular_chain<MODE, SPEC>(S, stack, ray, h, g, P.eps, P.max_spec, pixel, P.light_seed, &T);
    if (flags) {
        if (RESAMPLE) { /* this sample adds no light (dl + 0 is dl: a sum from +0 is never -0); the statistics stay */
            P.R.pos[r] = make_float4(0.f, 0.f, 0.f, __int_as_float((int)flags));
            P.R.nrm[r] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else store_inactive<TEX>(P.R, P.kd, r, flags);
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
    if (g.light < S.n_lights) {
        if (g.light >= 0) L = L + light_le(S.lights[g.light], -dir, g.ng);
        float4 m = S.materials[g.material];
        v3 kd = xyz(m);
        if (TEX && textured) kd = kdf;
        v3 fv = fbits(m.w) == PM_MATTE ? kd * INV_PI : mk(0.f, 0.f, 0.f);
        L = direct_light<MODE>(S, stack, point, ns, fv, L, EyeLightSampler{P, pixel, pass});
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

hipError_t launch_eye(const EyeParams &p, hipStream_t s) {
    if (p.R.count <= 0) return hipSuccess;
    /* a material of the physical specular model selects the SPEC instantiations, else a textured one the TEX
     * instantiations; both write the records' albedo */
    if ((p.S.mat_spec && !p.S.mat_tex) || ((p.S.mat_spec || p.S.tex_recs) && !p.kd)) return hipErrorInvalidValue;
    unsigned grid;
    size_t lds;
    eye_launch_geometry(p.S, p.R.count, &grid, &lds);
    dispatch_mode(scene_mode(p.S), [&](auto M) {
        constexpr int MODE = decltype(M)::value;
        void (*k)(EyeParams);
        if (p.S.mat_spec) k = p.camera ? k_eye_spec<MODE, true> : k_eye_spec<MODE, false>;
        else if (p.S.tex_recs) k = p.camera ? k_eye<MODE, true, true> : k_eye<MODE, false, true>;
        else k = p.camera ? k_eye<MODE, true, false> : k_eye<MODE, false, false>;
        pm_launch(k, dim3(grid), dim3(EYE_BLOCK), lds, s, p);
    });
    return hipGetLastError();
}

hipError_t launch_eye_resample(const EyeParams &p, hipStream_t s) {
    if (p.R.count <= 0) return hipSuccess;
    if (!p.camera || p.pass == 0u || p.S.mat_spec || p.S.tex_recs) return hipErrorInvalidValue;
    unsigned grid;
    size_t lds;
    eye_launch_geometry(p.S, p.R.count, &grid, &lds);
    dispatch_mode(scene_mode(p.S), [&](auto M) {
        pm_launch((k_eye_resample<decltype(M)::value>), dim3(grid), dim3(EYE_BLOCK), lds, s, p);
    });
    return hipGetLastError();
}

/* ====================================================================== */
/* simple renderer (direct light only, simple_render/simplerender.cu)     */
/* ====================================================================== */
/* One lane per eye sample: closest hit of the camera ray (no specular
 * chain), then for every light one shadow-tested sample (iSample 0, no pdf
 * division, no emitted term): direct_light's FIRST_ONLY form; a miss is black
 * (:75-79). The host's NaN / negative / infinite check (simplerender.cpp:70-87)
 * is fused into the store. Output: raster order (pinhole) or sample order
 * (host rays), float3 per sample. */
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
    if (!primary_ray<CAM>(P, r, 0u, &ray, &pixel)) return;

    v3 L = mk(0.f, 0.f, 0.f);
    Hit h;
    if (traverse<false, MODE>(S, ray, h, stack, EYE_BLOCK)) {
        const Geo g = shade<MODE == MODE_INST>(S, ray, h);
        const v3 point = ray.o + ray.d * h.t;
        const float4 m = S.materials[g.material];
        v3 kd = xyz(m);
        if (TEX && fbits(m.w) == PM_MATTE) kd = hit_kd<MODE == MODE_INST>(S, h, point, g.material, kd);
        const v3 fv = fbits(m.w) == PM_MATTE ? kd * INV_PI : mk(0.f, 0.f, 0.f); /* f(wo, wi) */
        L = direct_light<MODE, true>(S, stack, point, g.ns, fv, L, EyeLightSampler{P, pixel, 0u});
    }
    store_rgb(out, pixel, sanitise_radiance(L));
}

hipError_t launch_simple(const EyeParams &p, float *out, hipStream_t s) {
    if (p.R.count <= 0) return hipSuccess;
    unsigned grid;
    size_t lds;
    eye_launch_geometry(p.S, p.R.count, &grid, &lds);
    dispatch_mode(scene_mode(p.S), [&](auto M) {
        constexpr int MODE = decltype(M)::value;
        void (*k)(EyeParams, float *);
        if (p.S.tex_recs) k = p.camera ? k_simple<MODE, true, true> : k_simple<MODE, false, true>;
        else k = p.camera ? k_simple<MODE, true, false> : k_simple<MODE, false, false>;
        pm_launch(k, dim3(grid), dim3(EYE_BLOCK), lds, s, p, out);
    });
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
