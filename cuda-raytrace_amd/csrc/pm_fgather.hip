/*
 * pm_fgather.hip — final gathering (HIP/CDNA4): pm_api.h pm_final_gather_pass
 * states the operation.
 *
 *   k_fg_rays       gather ray j of primary record r (a rotated Hammersley
 *                   point through pbrt's CosineSampleHemisphere about the
 *                   record's normal) -> specular chain -> secondary gather
 *                   record + direct light with shadow rays, no emitted term
 *   k_fg_ray_dump   pm_final_gather_rays: the same rays, nothing traced
 *   k_fg_accumulate A_r += Li_j over a primary record's rays, ascending j
 *
 * Between k_fg_rays and k_fg_accumulate the host runs the kNN gather
 * (pm_gather_knn*.hip) and k_final (pm_records.hip) over the secondary records
 * as they are. The resolve (k_fg_resolve) is pm_caustic.hip's, beside the
 * caustic radiance it may add. The specular chain and the direct-light loop
 * are pm_eye_dev.h's, which the eye pass (pm_eye.hip) shares.
 */
#include <hip/hip_runtime.h>

#include "pm_eye_dev.h"

#pragma clang fp contract(off)

namespace pm {

/* pbrt's CoordinateSystem(v1, &v2, &v3) in fp32 */
PMD void coordinate_system(v3 n, v3 *v1, v3 *v2) {
    if (fabsf(n.x) > fabsf(n.y)) {
        const float il = 1.0f / sqrtf(n.x * n.x + n.z * n.z);
        *v1 = mk(-n.z * il, 0.f, n.x * il);
    } else {
        const float il = 1.0f / sqrtf(n.y * n.y + n.z * n.z);
        *v1 = mk(0.f, n.z * il, -n.y * il);
    }
    *v2 = cross(n, *v1);
}

/* Gather ray j of primary record r, in the order of operations pm_api.h pins:
 * shared by k_fg_rays and k_fg_ray_dump. False (and *d = 0) for a ray that is
 * not traced: an inactive primary record, or z == 0. */
PMD bool fg_ray(const FgParams &P, int64_t r, int j, v3 *o, v3 *d) {
    const float4 pos = P.P.pos[r];
    const uint32_t flags = (uint32_t)__float_as_int(pos.w);
    *o = xyz(pos);
    *d = mk(0.f, 0.f, 0.f);
    if (flags & REC_INACTIVE) { *o = mk(0.f, 0.f, 0.f); return false; }
    uint32_t o4[4];
    pmdm_philox4x32_10((uint32_t)((uint64_t)r & 0xffffffffu), (uint32_t)((uint64_t)r >> 32), 3u, P.pass, P.light_seed, 0u,
                       o4);
    const float ru = pmdm_u01(o4[0]), rv = pmdm_u01(o4[1]);
    const float a = ((float)j + 0.5f) / (float)P.n_gather + ru;
    const float b = (float)__builtin_bitreverse32((uint32_t)j) * 0x1p-32f + rv;
    const float u1 = fminf(a - floorf(a), 0x1.fffffep-1f), u2 = fminf(b - floorf(b), 0x1.fffffep-1f);
    float dx, dy;
    concentric_sample_disk(u1, u2, &dx, &dy);
    const float z = sqrtf(fmaxf(0.f, 1.f - dx * dx - dy * dy));
    if (z == 0.0f) return false;
    v3 n = xyz(P.P.nrm[r]);
    if (flags & PM_REC_BACKFACE) n = -n;
    v3 v1, v2;
    coordinate_system(n, &v1, &v2);
    *d = normalize(dx * v1 + dy * v2 + z * n);
    return true;
}

/* the light samples of secondary record s: a Philox draw keyed by s, with the
 * slot in the seed's second word */
struct FgLightSampler {
    int64_t s;
    uint32_t pass, light_seed;
    PMD void operator()(int slot, float *u1, float *u2) const {
        uint32_t o4[4];
        pmdm_philox4x32_10((uint32_t)((uint64_t)s & 0xffffffffu), (uint32_t)((uint64_t)s >> 32), 0u, pass, light_seed,
                           (uint32_t)slot, o4);
        *u1 = pmdm_u01(o4[0]); *u2 = pmdm_u01(o4[1]);
    }
};

/* One lane per secondary record. From the ray on it calls what k_eye calls
 * (pm_eye.hip eye_body without TEX / SPEC, which pm_final_gather_pass
 * refuses): pm_eye_dev.h's specular_chain, store_inactive and direct_light.
 * Two things differ: the light samples are keyed by the secondary record's
 * index, and the emitted term of a hit on a light is left out. */
template <int MODE>
__global__ __launch_bounds__(EYE_BLOCK) void k_fg_rays(FgParams P) {
    extern __shared__ __attribute__((aligned(16))) int stk[]; /* [stack_depth x EYE_BLOCK][scene blob (LDS)] */
    int *stack = stk + threadIdx.x;
    const SceneDev S = scene_view<mode_lds(MODE)>(P.S, reinterpret_cast<uint4 *>(stk + P.S.stack_depth * EYE_BLOCK),
                                                       threadIdx.x, EYE_BLOCK);
    if (mode_lds(MODE)) __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * EYE_BLOCK + threadIdx.x;
    if (i >= P.R.count) return;
    const int64_t s = P.sec_begin + i;
    const int64_t r = s / P.n_gather;
    const int j = (int)(s - r * P.n_gather);

    Ray ray;
    uint32_t flags = 0;
    if (r >= P.P.count || !fg_ray(P, r, j, &ray.o, &ray.d)) flags = PM_REC_MISS; /* not traced: contributes 0 */
    ray.tmin = P.eps;
    ray.tmax = RT_DEFAULT_MAX;
    Hit h;
    Geo g;
    if (!flags) flags = specular_chain<MODE, false>(S, stack, ray, h, g, P.eps, P.max_spec, 0, 0u, nullptr);
    if (flags) {
        store_inactive<false>(P.R, nullptr, i, flags);
        return;
    }
    const v3 point = ray.o, ns = g.ns, dir = ray.d;

    /* directLight (raytracing.cu:49-84) without the emitted term */
    v3 L = mk(0.f, 0.f, 0.f);
    if (g.light < S.n_lights) {
        const float4 m = S.materials[g.material];
        const v3 fv = fbits(m.w) == PM_MATTE ? xyz(m) * INV_PI : mk(0.f, 0.f, 0.f);
        L = direct_light<MODE>(S, stack, point, ns, fv, L, FgLightSampler{s, P.pass, P.light_seed});
    }
    const uint32_t side = dot(ns, -dir) < 0.f ? PM_REC_BACKFACE : 0u;
    P.R.pos[i] = make_float4(point.x, point.y, point.z, __uint_as_float(side));
    P.R.nrm[i] = make_float4(ns.x, ns.y, ns.z, __int_as_float(g.material));
    P.R.state[i] = make_float4(0.f, 0.f, 0.f, P.r2init);
    P.R.n[i] = 0.f;
    P.R.dl[i] = make_float4(L.x, L.y, L.z, 0.f);
}

hipError_t launch_fg_rays(const FgParams &p, hipStream_t s) {
    if (p.R.count <= 0) return hipSuccess;
    if (p.n_gather < 1 || p.S.tex_recs || p.S.mat_spec) return hipErrorInvalidValue;
    unsigned grid;
    size_t lds;
    eye_launch_geometry(p.S, p.R.count, &grid, &lds);
    dispatch_mode(scene_mode(p.S), [&](auto M) {
        pm_launch((k_fg_rays<decltype(M)::value>), dim3(grid), dim3(EYE_BLOCK), lds, s, p);
    });
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_fg_ray_dump(FgParams P, int64_t first, int64_t count, float *rays6) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t s = first + i;
    const int64_t r = s / P.n_gather;
    v3 o, d;
    fg_ray(P, r, (int)(s - r * P.n_gather), &o, &d);
    float *q = rays6 + 6 * i;
    q[0] = o.x; q[1] = o.y; q[2] = o.z; q[3] = d.x; q[4] = d.y; q[5] = d.z;
}

hipError_t launch_fg_ray_dump(const FgParams &p, int64_t first, int64_t count, float *rays6, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    if (p.n_gather < 1 || first < 0 || first + count > p.P.count * p.n_gather) return hipErrorInvalidValue;
    pm_launch(k_fg_ray_dump, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, p, first, count, rays6);
    return hipGetLastError();
}

/* one lane per primary record of the chunk: its rays' radiances are n_gather
 * consecutive float3 of li */
__global__ __launch_bounds__(256) void k_fg_accumulate(FgSumParams P) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.rec_count) return;
    const int64_t r = P.rec_begin + i;
    float4 a = P.zero ? make_float4(0.f, 0.f, 0.f, 0.f) : P.sum[r];
    const uint32_t flags = (uint32_t)__float_as_int(P.P.pos[r].w);
    if (!(flags & REC_INACTIVE)) {
        const float *q = P.li + 3 * i * (int64_t)P.n_gather;
        for (int j = 0; j < P.n_gather; ++j) {
            a.x = a.x + q[3 * j];
            a.y = a.y + q[3 * j + 1];
            a.z = a.z + q[3 * j + 2];
        }
    }
    P.sum[r] = a;
}

hipError_t launch_fg_accumulate(const FgSumParams &p, hipStream_t s) {
    if (p.rec_count <= 0) return hipSuccess;
    pm_launch(k_fg_accumulate, dim3((unsigned)((p.rec_count + 255) / 256)), dim3(256), 0, s, p);
    return hipGetLastError();
}

} // namespace pm
