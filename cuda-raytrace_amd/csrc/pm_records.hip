/*
 * pm_records.hip — kernels over the gather-point records that gather
 * nothing: radius exchange I/O, the PPM update of reduced partials
 * (gathering.cu:104-126) in its whole, split and radius / flux forms, the
 * record view, final radiance + sanitisation (gathering.cu:129-146,
 * photonmappingrenderer.cpp:251-268), the tile list and its cost sort, and
 * the per-step record reset.
 */
#include <hip/hip_runtime.h>

#include "pm_gather_dev.h"
#include "pm_kernels.h"

#pragma clang fp contract(off)

namespace pm {
/* radius^2 of a record range to / from a contiguous float array: after the
 * owner's PPM update every rank needs the new radii for the next pass's
 * range queries (pmrender/dist.py, "reduce" exchange) */
__global__ __launch_bounds__(256) void k_radius2_io(RecordsDev R, float *buf, int64_t rec_begin, int64_t rec_count,
                                                    int to_records, const uint32_t *view) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rec_count) return;
    const int64_t r = view ? (int64_t)view[rec_begin + i] : rec_begin + i;
    if (to_records) R.state[r].w = buf[i];
    else buf[i] = R.state[r].w;
}

hipError_t launch_radius2_io(const RecordsDev &R, float *buf, int64_t rec_begin, int64_t rec_count, int to_records,
                             const uint32_t *view, hipStream_t s) {
    if (rec_count <= 0) return hipSuccess;
    pm_launch(k_radius2_io, dim3((unsigned)((rec_count + 255) / 256)), dim3(256), 0, s, R, buf, rec_begin,
                       rec_count, to_records, view);
    return hipGetLastError();
}

/* PPM update from summed partials (M, L in fixed point), record chunk */
__global__ __launch_bounds__(256) void k_ppm_update(RecordsDev R, const long long *partial, int64_t rec_begin,
                                                    int64_t rec_count, float alpha, double inv, const uint32_t *view) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rec_count) return;
    const int64_t r = view ? (int64_t)view[rec_begin + i] : rec_begin + i;
    uint32_t flags = (uint32_t)__float_as_int(R.pos[r].w);
    if (flags & REC_INACTIVE) return;
    const longlong2 *q = reinterpret_cast<const longlong2 *>(partial + 4 * i);
    const longlong2 a = q[0], b = q[1];
    const int M = (int)a.x;
    if (M <= 0) return;
    float4 st = R.state[r];
    float N = R.n[r];
    v3 L = mk((float)((double)a.y * inv), (float)((double)b.x * inv), (float)((double)b.y * inv));
    ppm_apply(st, N, M, L, alpha);
    R.state[r] = st;
    R.n[r] = N;
}

hipError_t launch_ppm_update(const GatherParams &p, const long long *partial, int64_t rec_begin, int64_t rec_count,
                             hipStream_t s) {
    if (rec_count <= 0) return hipSuccess;
    pm_launch(k_ppm_update, dim3((unsigned)((rec_count + 255) / 256)), dim3(256), 0, s, p.R, partial,
                       rec_begin, rec_count, p.ppm_alpha, p.fx_inv, p.view_list);
    return hipGetLastError();
}

/* PPM update of the split exchange: every rank holds the global photon
 * count M of every view record (all-reduced), so it updates every radius and
 * photon count itself — no radius exchange — while the summed flux arrives
 * only for its own chunk [v_begin, v_begin + v_count) (reduce-scattered).
 * fresh: the records are in a deferred reset — start from the initial state
 * and write every view record. */
__global__ __launch_bounds__(256) void k_ppm_update_split(RecordsDev R, const int *count, const long long *flux,
                                                          int64_t n_view, int64_t v_begin, int64_t v_count, float alpha,
                                                          double inv, const uint32_t *view, int fresh, float r2init) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_view) return;
    const int64_t r = view ? (int64_t)view[i] : i;
    const uint32_t flags = (uint32_t)__float_as_int(R.pos[r].w);
    if (flags & REC_INACTIVE) return;
    const int M = count[i];
    if (M <= 0 && !fresh) return;
    float4 st = fresh ? make_float4(0.f, 0.f, 0.f, r2init) : R.state[r];
    float N = fresh ? 0.f : R.n[r];
    v3 L = mk(0.f, 0.f, 0.f);
    const int64_t k = i - v_begin;
    if (k >= 0 && k < v_count) {
        const long long *f = flux + 3 * k;
        L = mk((float)((double)f[0] * inv), (float)((double)f[1] * inv), (float)((double)f[2] * inv));
    }
    ppm_apply(st, N, M, L, alpha);
    R.state[r] = st;
    R.n[r] = N;
}

/* pm_ppm_update_split in two halves (ppm_apply's operations, split at the
 * ratio): radius2 and N of every view record now, the ratio kept for the
 * owner's flux update after the flux reduce-scatter has landed */
__global__ __launch_bounds__(256) void k_ppm_update_radius(RecordsDev R, const int *count, float *ratio_out,
                                                           int64_t n_view, float alpha, const uint32_t *view,
                                                           int fresh, float r2init) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_view) return;
    const int64_t r = view ? (int64_t)view[i] : i;
    ratio_out[i] = -1.f;
    const uint32_t flags = (uint32_t)__float_as_int(R.pos[r].w);
    if (flags & REC_INACTIVE) return;
    const int M = count[i];
    if (M <= 0 && !fresh) return;
    float4 st = fresh ? make_float4(0.f, 0.f, 0.f, r2init) : R.state[r];
    float N = fresh ? 0.f : R.n[r];
    if (M > 0) { /* ppm_apply without the flux */
        int totalPhotons = N + alpha * M;
        float ratio = totalPhotons / (N + M);
        st.w = st.w * ratio;
        N = totalPhotons;
        ratio_out[i] = ratio;
    }
    R.state[r] = st;
    R.n[r] = N;
}
__global__ __launch_bounds__(256) void k_ppm_update_flux(RecordsDev R, const float *ratio, const long long *flux,
                                                         int64_t v_begin, int64_t v_count, double inv,
                                                         const uint32_t *view) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= v_count) return;
    const int64_t i = v_begin + k;
    const float q = ratio[i];
    if (!(q >= 0.f)) return;
    const int64_t r = view ? (int64_t)view[i] : i;
    const long long *f = flux + 3 * k;
    const v3 L = mk((float)((double)f[0] * inv), (float)((double)f[1] * inv), (float)((double)f[2] * inv));
    float4 st = R.state[r];
    const v3 fl = (xyz(st) + L) * q;
    st.x = fl.x; st.y = fl.y; st.z = fl.z;
    R.state[r] = st;
}
hipError_t launch_ppm_update_radius(const GatherParams &p, const int *count, float *ratio, int64_t n_view, int fresh,
                                    hipStream_t s) {
    if (n_view <= 0) return hipSuccess;
    pm_launch(k_ppm_update_radius, dim3((unsigned)((n_view + 255) / 256)), dim3(256), 0, s, p.R, count, ratio, n_view,
              p.ppm_alpha, p.view_list, fresh, p.r2init);
    return hipGetLastError();
}
hipError_t launch_ppm_update_flux(const GatherParams &p, const float *ratio, const long long *flux, int64_t v_begin,
                                  int64_t v_count, hipStream_t s) {
    if (v_count <= 0) return hipSuccess;
    pm_launch(k_ppm_update_flux, dim3((unsigned)((v_count + 255) / 256)), dim3(256), 0, s, p.R, ratio, flux, v_begin,
              v_count, p.fx_inv, p.view_list);
    return hipGetLastError();
}

hipError_t launch_ppm_update_split(const GatherParams &p, const int *count, const long long *flux, int64_t n_view,
                                   int64_t v_begin, int64_t v_count, int fresh, hipStream_t s) {
    if (n_view <= 0) return hipSuccess;
    pm_launch(k_ppm_update_split, dim3((unsigned)((n_view + 255) / 256)), dim3(256), 0, s, p.R, count, flux, n_view,
              v_begin, v_count, p.ppm_alpha, p.fx_inv, p.view_list, fresh, p.r2init);
    return hipGetLastError();
}

/* ====================================================================== */
/* record view (active records, compacted in record order)               */
/* ====================================================================== */
__global__ __launch_bounds__(256) void k_view_flags(RecordsDev R, uint32_t *flags) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > R.count) return;
    if (r == R.count) { flags[r] = 0u; return; } /* scanned tail -> total */
    const uint32_t f = (uint32_t)__float_as_int(R.pos[r].w);
    flags[r] = (f & REC_INACTIVE) ? 0u : 1u;
}

__global__ __launch_bounds__(256) void k_view_list(RecordsDev R, const uint32_t *flags, uint32_t *rank,
                                                   uint32_t *list) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R.count) return;
    if (flags[r]) list[rank[r]] = (uint32_t)r;
    else rank[r] = 0xffffffffu;
}

hipError_t launch_record_view(const RecordsDev &R, uint32_t *flags, uint32_t *rank, uint32_t *list, uint32_t *sums,
                              hipStream_t s) {
    const int64_t n = R.count;
    pm_launch(k_view_flags, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s, R, flags);
    hipError_t e = launch_exclusive_scan(flags, n + 1, rank, sums, s);
    if (e != hipSuccess) return e;
    pm_launch(k_view_list, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, R, flags, rank, list);
    return hipGetLastError();
}

/* ====================================================================== */
/* final gathering                                                        */
/* ====================================================================== */
__global__ __launch_bounds__(256) void k_final(FinalParams P) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.rec_count) return;
    const int64_t r = P.view ? (int64_t)P.view[P.rec_begin + i] : P.rec_begin + i;
    const uint32_t flags = (uint32_t)__float_as_int(P.R.pos[r].w);
    int64_t o;
    if (!out_index(r, i, P.raster, P.W, flags, &o)) return;
    v3 out = mk(0.f, 0.f, 0.f);
    if (!(flags & REC_INACTIVE)) {
        float4 dl = P.R.dl[r], st = P.R.state[r];
        float N = P.R.n[r];
        v3 IDL = mk(0.f, 0.f, 0.f);
        if (P.knn) { /* LPhoton: Lr * rho / pi with Lr's 1/nPaths = 1/emitted (passes averaged) */
            const float4 m = P.materials[__float_as_int(P.R.nrm[r].w)];
            const v3 fv = __float_as_int(m.w) == PM_MATTE ? xyz(m) * INV_PI : mk(0.f, 0.f, 0.f);
            if (P.kd) IDL = (xyz(st) / P.emitted) * (fv * xyz(P.kd[r])); /* the texel, factored out of the gather */
            else IDL = (xyz(st) / P.emitted) * fv;
        } else if (N != 0) {
            if (P.kd) IDL = (xyz(P.kd[r]) * xyz(st)) * INV_PI / (st.w * P.emitted);
            else IDL = xyz(st) * INV_PI / (st.w * P.emitted);
        }
        out = sanitise_radiance(xyz(dl) + IDL);
    }
    store_rgb(P.out, o, out);
}

/* k_final over the records of a resampled render (FinalParams::resampled,
 * pm_eye_resample: PPM, no albedo factors): dl holds the sum of n_eye samples,
 * and the current flags are only the last sample's, so a MISS or EXCEPTION
 * record is written like any other: dl / n_eye + flux (1 / pi) / (radius2
 * emitted), the indirect term 0 while the record has gathered nothing */
__global__ __launch_bounds__(256) void k_final_resampled(FinalParams P) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.rec_count) return;
    const int64_t r = P.view ? (int64_t)P.view[P.rec_begin + i] : P.rec_begin + i;
    const uint32_t flags = (uint32_t)__float_as_int(P.R.pos[r].w);
    int64_t o;
    if (!out_index(r, i, P.raster, P.W, flags, &o)) return;
    v3 out = mk(0.f, 0.f, 0.f);
    if (!(flags & PM_REC_INVALID)) {
        const float4 dl = P.R.dl[r], st = P.R.state[r];
        const float N = P.R.n[r];
        v3 IDL = mk(0.f, 0.f, 0.f);
        if (N != 0) IDL = xyz(st) * INV_PI / (st.w * P.emitted);
        const float ne = (float)P.n_eye; /* one IEEE division per channel (v3 / float would multiply by 1 / ne) */
        out = sanitise_radiance(mk(dl.x / ne, dl.y / ne, dl.z / ne) + IDL);
    }
    store_rgb(P.out, o, out);
}

__global__ __launch_bounds__(256) void k_tile_flags(RecordsDev R, uint8_t *flags) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool act = false;
    if (r < R.count) act = !((uint32_t)__float_as_int(R.pos[r].w) & REC_INACTIVE);
    const unsigned long long m = __ballot(act);
    if ((threadIdx.x & 63) == 0 && r < R.count) flags[r >> 6] = m != 0ull ? 1 : 0;
}
/* one block compacts the flags in order: 1024 tiles per step, ballot ranks
 * inside each wave, wave totals through LDS */
__global__ __launch_bounds__(1024) void k_tile_compact(const uint8_t *flags, int64_t nt, uint32_t *list,
                                                       uint32_t *count) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t base;
    if (threadIdx.x == 0) base = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (int64_t t0 = 0; t0 < nt; t0 += 1024) {
        const int64_t t = t0 + threadIdx.x;
        const bool f = t < nt && flags[t] != 0;
        const unsigned long long m = __ballot(f);
        if (lane == 0u) wsum[w] = (uint32_t)__builtin_popcountll(m);
        __syncthreads();
        uint32_t off = base;
        for (uint32_t k = 0; k < w; ++k) off += wsum[k];
        if (f) list[off + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = (uint32_t)t;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t tot = 0u;
            for (int k = 0; k < 16; ++k) tot += wsum[k];
            base += tot;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = base;
}
/* Cost-ordered tile list (one block): the tile gather's launch ends with
 * the waves dispatched last (each a tile's whole lifetime, 9.5 us on average
 * at C2, up to 35 us for the densest tiles), so the order of the list sets
 * the drain. The groups of 8 entries a wave's XCD takes together (xcd_tile)
 * are counting-sorted by the largest lifetime among them, heaviest first, in
 * 256 log-spaced buckets (3 % each); the order inside a bucket is the atomics'
 * (any order gives the same sums). */
__global__ __launch_bounds__(1024) void k_tile_sort(const uint32_t *list, const uint16_t *cost, const uint32_t *n_dev,
                                                    int64_t n_host, uint32_t *out) {
    __shared__ uint32_t hist[256];
    const int tid = threadIdx.x;
    const int64_t n = n_dev ? (int64_t)*n_dev : n_host, S = n / 8;
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    auto bucket = [&](int64_t g) {
        uint32_t c = 1u;
        for (int k = 0; k < 8; ++k) c = max(c, (uint32_t)cost[8 * g + k]);
        /* 24 buckets per octave from 16 ticks (0.16 us) up; heaviest -> 0 */
        const int b = (int)(24.f * (__log2f((float)c) - 4.f));
        return 255 - min(max(b, 0), 255);
    };
    for (int64_t g = tid; g < S; g += 1024) atomicAdd(&hist[bucket(g)], 1u);
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0u;
        for (int b = 0; b < 256; ++b) { const uint32_t c = hist[b]; hist[b] = run; run += c; }
    }
    __syncthreads();
    for (int64_t g = tid; g < S; g += 1024) {
        const uint32_t pos = atomicAdd(&hist[bucket(g)], 1u);
        const uint4 *src = reinterpret_cast<const uint4 *>(list + 8 * g);
        uint4 *dst = reinterpret_cast<uint4 *>(out + 8 * (int64_t)pos);
        dst[0] = src[0];
        dst[1] = src[1];
    }
    for (int64_t i = 8 * S + tid; i < n; i += 1024) out[i] = list[i]; /* the partial group stays last */
}
hipError_t launch_tile_sort(const uint32_t *list, const uint16_t *cost, const uint32_t *n_dev, int64_t n, uint32_t *out,
                            hipStream_t s) {
    pm_launch(k_tile_sort, dim3(1), dim3(1024), 0, s, list, cost, n_dev, n, out);
    return hipGetLastError();
}

hipError_t launch_tile_list(const RecordsDev &R, uint8_t *flags, uint32_t *list, uint32_t *count, hipStream_t s) {
    if (R.count <= 0) return hipSuccess;
    pm_launch(k_tile_flags, dim3((unsigned)((R.count + 255) / 256)), dim3(256), 0, s, R, flags);
    pm_launch(k_tile_compact, dim3(1), dim3(1024), 0, s, (const uint8_t *)flags, (R.count + 63) / 64, list, count);
    return hipGetLastError();
}

hipError_t launch_final(const FinalParams &p, hipStream_t s) {
    if (p.rec_count <= 0) return hipSuccess;
    if (p.resampled) {
        if (p.n_eye < 1 || p.knn || p.kd) return hipErrorInvalidValue;
        pm_launch(k_final_resampled, dim3((unsigned)((p.rec_count + 255) / 256)), dim3(256), 0, s, p);
    } else
        pm_launch(k_final, dim3((unsigned)((p.rec_count + 255) / 256)), dim3(256), 0, s, p);
    return hipGetLastError();
}

/* restore the eye pass's initial PPM state (flux 0, N 0, r^2 init;
 * raytracing.cu:121-123) so that every benchmark step gathers the same
 * workload as the reference's single pass */
__global__ __launch_bounds__(256) void k_reset_records(RecordsDev R, float r2init) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R.count) return;
    uint32_t flags = (uint32_t)__float_as_int(R.pos[r].w);
    if (flags & REC_INACTIVE) return;
    R.state[r] = make_float4(0.f, 0.f, 0.f, r2init);
    R.n[r] = 0.f;
}

hipError_t launch_reset_records(const RecordsDev &R, float r2init, hipStream_t s) {
    if (R.count <= 0) return hipSuccess;
    pm_launch(k_reset_records, dim3((unsigned)((R.count + 255) / 256)), dim3(256), 0, s, R, r2init);
    return hipGetLastError();
}

} // namespace pm
