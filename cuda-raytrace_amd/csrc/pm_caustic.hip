/*
 * pm_caustic.hip — the caustic map of final gathering (HIP/CDNA4): pm_api.h
 * pm_set_caustic_map states the definition and the operations.
 *
 *   k_caustic_count        pm_bucket.hip's k_bucket_count over the slots with
 *                          bit 1 of pm_photon::bits set (a caustic photon,
 *                          marked by the MARK trace kernels): cell key on the
 *                          map's grid, rank = returning atomicAdd on the
 *                          cell's counter; every other slot gets the invalid key
 *   (scan)                 pm_bucket.hip's k_scan_reduce / k_scan_down through
 *                          launch_exclusive_scan_clear
 *   k_caustic_fill         k_bucket_fill: slot -> cell_start[key] + rank in the
 *                          map's own ph_a / ph_b, ph_b keeping the slot index
 *                          in the slot buffer (the kNN tie-break reads it)
 *   k_caustic_radiance     Lc_r of the primary records after pm_caustic_gather
 *   k_fg_resolve<CAUSTIC>  final gathering's resolve (the accumulation is
 *                          pm_fgather.hip's): out_r = dl_r + Kd_r x A_r / (N P),
 *                          sanitised as k_final does; CAUSTIC: with Lc_r,
 *                          (dl + Lc) + Kd x (A / (N P))
 *
 * The kNN gather over the map is pm_gather_knn*.hip's, as it is.
 */
#include <hip/hip_runtime.h>

#include "pm_kernels.h"

#pragma clang fp contract(off)

namespace pm {

constexpr uint32_t PHOTON_VALID = 1u, PHOTON_CAUSTIC = 2u;

__global__ __launch_bounds__(256) void k_caustic_count(const pm_photon *slots, int64_t n, GridDesc g, uint32_t *count,
                                                       uint32_t *key_out, uint32_t *rank_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float2 *q = reinterpret_cast<const float2 *>(slots + i);
    const float2 a = q[0], b = q[1];
    uint32_t key = 0xffffffffu, rank = 0u;
    if (((uint32_t)__float_as_int(a.x) & (PHOTON_VALID | PHOTON_CAUSTIC)) == (PHOTON_VALID | PHOTON_CAUSTIC)) {
        const uint32_t cx = cell_axis(a.y, g.gx, g.inv_cs, g.dx);
        const uint32_t cy = cell_axis(b.x, g.gy, g.inv_cs, g.dy);
        const uint32_t cz = cell_axis(b.y, g.gz, g.inv_cs, g.dz);
        key = (cz * (uint32_t)g.dy + cy) * (uint32_t)g.dx + cx; /* < ncells: every axis is clamped */
        rank = atomicAdd(&count[key], 1u);
    }
    key_out[i] = key;
    rank_out[i] = rank;
}

__global__ __launch_bounds__(256) void k_caustic_fill(const pm_photon *slots, int64_t n, const uint32_t *key,
                                                      const uint32_t *rank, const uint32_t *cell_start, float4 *ph_a,
                                                      float4 *ph_b) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = key[i];
    if (k == 0xffffffffu) return;
    const uint32_t dst = cell_start[k] + rank[i]; /* < cell_start[ncells] <= n */
    const float2 *q = reinterpret_cast<const float2 *>(slots + i);
    const float2 a = q[0], b = q[1], c = q[2], d = q[3], e = q[4];
    /* k_bucket_fill's layout: a = (bits, p.x) b = (p.y, p.z) c = (alpha.x, alpha.y) d = (alpha.z, wi.x) e = (wi.y, wi.z) */
    ph_a[dst] = make_float4(a.y, b.x, b.y, d.y);
    ph_b[2 * (size_t)dst] = make_float4(c.x, c.y, d.x, e.x);
    ph_b[2 * (size_t)dst + 1] = make_float4(e.y, __uint_as_float((uint32_t)i), 0.f, 0.f);
}

size_t caustic_scratch_words(int64_t n_slots, uint32_t ncells) { return 2 * (size_t)n_slots + scan_scratch_words((int64_t)ncells + 1); }

hipError_t launch_caustic_build(const pm_photon *slots, int64_t n, GridDesc g, uint32_t *count, uint32_t *cell_start,
                                uint32_t *scratch, float4 *ph_a, float4 *ph_b, hipStream_t s) {
    const int64_t nc = (int64_t)g.ncells + 1; /* the last counter stays 0: cell_start[ncells] = caustic photons */
    uint32_t *key = scratch, *rank = scratch + n, *sums = scratch + 2 * n;
    if (n > 0) pm_launch(k_caustic_count, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, slots, n, g, count, key, rank);
    const hipError_t e = launch_exclusive_scan_clear(count, nc, cell_start, sums, s);
    if (e != hipSuccess) return e;
    if (n > 0)
        pm_launch(k_caustic_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, slots, n, key, rank, cell_start, ph_a, ph_b);
    return hipGetLastError();
}

/* k_final's kNN term of record r, the direct light left out: (flux / emitted) * (Kd / pi), 0 unless PM_MATTE */
PMD v3 caustic_radiance(const RecordsDev &R, const float4 *materials, float emitted, int64_t r) {
    const float4 st = R.state[r];
    const float4 m = materials[__float_as_int(R.nrm[r].w)];
    const v3 fv = __float_as_int(m.w) == PM_MATTE ? xyz(m) * INV_PI : mk(0.f, 0.f, 0.f);
    return (xyz(st) / emitted) * fv;
}

__global__ __launch_bounds__(256) void k_caustic_radiance(FgResolveParams P, float emitted) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.rec_count) return;
    const int64_t r = P.rec_begin + i;
    const uint32_t flags = (uint32_t)__float_as_int(P.P.pos[r].w);
    v3 lc = mk(0.f, 0.f, 0.f);
    if (!(flags & REC_INACTIVE)) lc = caustic_radiance(P.P, P.materials, emitted, r);
    store_rgb(P.out, i, lc);
}

hipError_t launch_caustic_radiance(const FgResolveParams &p, float emitted, hipStream_t s) {
    if (p.rec_count <= 0) return hipSuccess;
    pm_launch(k_caustic_radiance, dim3((unsigned)((p.rec_count + 255) / 256)), dim3(256), 0, s, p, emitted);
    return hipGetLastError();
}

/* pm_final_gather_resolve: k_final's layout and sanitising with the
 * final-gathered indirect term, out = dl + Kd x (A / denom); CAUSTIC: with the
 * caustic radiance beside the direct light, (dl + Lc) + Kd x (A / denom)
 * (`emitted` is read by that instantiation alone) */
template <bool CAUSTIC>
__global__ __launch_bounds__(256) void k_fg_resolve(FgResolveParams P, float emitted) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.rec_count) return;
    const int64_t r = P.rec_begin + i;
    const uint32_t flags = (uint32_t)__float_as_int(P.P.pos[r].w);
    int64_t o;
    if (!out_index(r, i, P.raster, P.W, flags, &o)) return;
    v3 out = mk(0.f, 0.f, 0.f);
    if (!(flags & REC_INACTIVE)) {
        const float4 dl = P.P.dl[r], a = P.sum[r];
        const float4 m = P.materials[__float_as_int(P.P.nrm[r].w)];
        const v3 kd = __float_as_int(m.w) == PM_MATTE ? xyz(m) : mk(0.f, 0.f, 0.f);
        v3 direct = xyz(dl);
        if (CAUSTIC) direct = direct + caustic_radiance(P.P, P.materials, emitted, r);
        out = sanitise_radiance(direct + kd * mk(a.x / P.denom, a.y / P.denom, a.z / P.denom)); /* one IEEE division per channel */
    }
    store_rgb(P.out, o, out);
}

hipError_t launch_fg_resolve(const FgResolveParams &p, hipStream_t s) {
    if (p.rec_count <= 0) return hipSuccess;
    pm_launch(k_fg_resolve<false>, dim3((unsigned)((p.rec_count + 255) / 256)), dim3(256), 0, s, p, 0.f);
    return hipGetLastError();
}

hipError_t launch_fg_resolve_caustic(const FgResolveParams &p, float emitted, hipStream_t s) {
    if (p.rec_count <= 0) return hipSuccess;
    pm_launch(k_fg_resolve<true>, dim3((unsigned)((p.rec_count + 255) / 256)), dim3(256), 0, s, p, emitted);
    return hipGetLastError();
}

} // namespace pm
