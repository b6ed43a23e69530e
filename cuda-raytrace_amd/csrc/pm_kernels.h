/*
 * pm_kernels.h — kernel parameter blocks and launcher declarations shared by
 * the host orchestration (pm_api*.cpp around pm_ctx.h) and the HIP kernels (pm_trace.hip, pm_eye.hip, pm_bucket.hip,
 * pm_gather.hip, pm_gather_knn.hip, pm_records.hip, pm_bvh_gpu.hip, pm_film.hip, pm_fgather.hip, pm_caustic.hip),
 * with the few device and host helpers several of them use (REC_INACTIVE, the
 * output tail, dispatch_mode, dispatch_flag, eye_launch_geometry).
 */
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "pm_device.h"
#include "pm_plan_pod.h"

namespace pm {

enum TraceFamily : int; /* pm_plan.h (host only): the trace launch's plan */
struct TracePlan;

/* Stage timing without marker packets: the API (pm_api.cpp timer_begin /
 * timer_end) points g_stage at an event pair around one stage, and every
 * launch in the stage goes through pm_launch, which binds the start event to
 * the stage's first dispatch and the stop event to each dispatch (the last
 * one wins) — the timestamps come from the kernel dispatches themselves, so
 * timing adds no idle gap between kernels. */
struct StageEvents { hipEvent_t start = nullptr, stop = nullptr; int launched = 0; };
extern thread_local StageEvents *g_stage;

template <typename F, typename... Args>
inline void pm_launch(F kernel, dim3 grid, dim3 block, uint32_t shmem, hipStream_t s, Args... args) {
    hipEvent_t a = nullptr, b = nullptr;
    if (StageEvents *st = g_stage) {
        a = st->launched ? nullptr : st->start;
        b = st->stop;
        st->launched++;
    }
    hipExtLaunchKernelGGL(kernel, grid, block, shmem, s, a, b, 0u, args...);
}

constexpr int EYE_BLOCK = 128;     /* traversal kernels: LDS stack column per lane */
/* TRACE_BLOCK: pm_plan_pod.h */
constexpr int GATHER_BLOCK = 256;
/* k_gather_tile: waves per block. Its waves never synchronise with each
 * other, and a block's LDS is held until its last wave ends, so with several
 * waves per block a tile that runs long keeps its neighbours' LDS allocated
 * (LDS co-limits the kernel at 5 waves/SIMD). One wave per block: C2
 * gather 47.6 -> 46.5-47.1 us, C3 0.54-0.56 -> 0.53 ms, C5 0.30 -> 0.27 ms
 * (same box, against 256) */
#ifndef PM_TILE_BLOCK
#define PM_TILE_BLOCK 64
#endif
constexpr int TILE_BLOCK = PM_TILE_BLOCK;
enum { PM_GK_TILE = 0, PM_GK_LANE = 1 };
/* error word of a kd-tree gather: a record's traversal stack overflowed (a
 * subtree would have been dropped), or the node links are not a pbrt tree */
enum { PM_GATHER_ERR_STACK = 1u, PM_GATHER_ERR_TREE = 2u };
constexpr int KD_STACK = 32;       /* >= pbrt median kd-tree depth for < 2^31 photons */
constexpr int KNN_BLOCK = 64;      /* k_gather_knn: one wave per block, LDS heaps [K][64] */

/* a record that gathers nothing and shows black: its ray missed the scene, its
 * specular chain failed, or it lies outside the raster */
constexpr uint32_t REC_INACTIVE = PM_REC_MISS | PM_REC_EXCEPTION | PM_REC_INVALID;

/* device SoA record arrays */
struct RecordsDev {
    float4 *pos;    /* pos.xyz, flags (bits) */
    float4 *nrm;    /* ns.xyz, material (bits) */
    float4 *state;  /* flux.xyz, radius2 */
    float *n;       /* photon_count */
    float4 *dl;     /* direct light */
    int64_t count;
};

/* pm_set_camera's sampling state (pm_api.h pm_camera): the sample raster is
 * EyeParams::W x H (= image * strata) */
struct CameraDev {
    int xs, ys, jitter;
    float lens_radius, focal;
    uint32_t seed;
};

struct EyeParams {
    SceneDev S;
    RecordsDev R;
    int pinhole, W, H, n2d;
    float4 eye, fwd, right, up;
    const float *rays;
    const float *rand2d;
    float eps, r2init;
    int max_spec;
    uint32_t light_seed;
    /* camera != 0 (pm_set_camera): the CAM instantiations of k_eye / k_simple;
     * pinhole is 1 and W x H the sample raster, so everything but the ray
     * itself is the pinhole's */
    int camera;
    CameraDev cam;
    /* the resampled eye pass (pm_eye_resample, k_eye_resample) and
     * pm_camera_rays_pass: the pass number, Philox counter word 3 of the camera
     * randoms and of the light samples. 0 on every other path, whose kernels do
     * not read it (it fills what was padding in front of kd) */
    uint32_t pass;
    /* scenes with a textured material (S.tex_recs != null) or one of the
     * physical specular model (S.mat_spec != null) only: per record the
     * factor pm_final applies to its indirect term (float4, SoA like R's
     * arrays): the texel of a textured matte hit, (1, 1, 1) on any other
     * surface, times the throughput of the record's specular chain; 0 for
     * an inactive record. Null otherwise, and never read then */
    float4 *kd;
};

/* the jitter and lens randoms of sample q in eye pass `pass` (pm_api.h
 * pm_set_camera, pm_eye_resample); every caller but the resampled eye pass
 * and pm_camera_rays_pass passes the constant 0 */
PMD void camera_randoms(const CameraDev &C, int64_t q, uint32_t pass, float *ju, float *jv, float *lu, float *lv) {
    /* uniform per launch: stratum centres through a pinhole use none of the four */
    if (!C.jitter && !(C.lens_radius > 0.0f)) { *ju = *jv = 0.5f; *lu = *lv = 0.0f; return; }
    uint32_t o4[4];
    pmdm_philox4x32_10((uint32_t)((uint64_t)q & 0xffffffffu), (uint32_t)((uint64_t)q >> 32), 1u, pass, C.seed, 0u, o4);
    *ju = C.jitter ? pmdm_u01(o4[0]) : 0.5f;
    *jv = C.jitter ? pmdm_u01(o4[1]) : 0.5f;
    *lu = pmdm_u01(o4[2]);
    *lv = pmdm_u01(o4[3]);
}
/* film position of sample (ix, iy) with jitter (ju, jv), in pixels */
PMD void camera_film_xy(const CameraDev &C, int ix, int iy, float ju, float jv, float *fx, float *fy) {
    *fx = ((float)ix + ju) / (float)C.xs;
    *fy = ((float)iy + jv) / (float)C.ys;
}

/* the film (pm_film.hip k_film): one workgroup per FILM_TILE x FILM_TILE
 * output pixels, the tile's sample footprint staged through LDS in bands of
 * whole sample rows */
constexpr int FILM_TILE = 16;
constexpr int FILM_LDS_SAMPLES = 3072; /* band capacity: 5 planes x 4 B x 3072 = 60 KB, + 1 KB table */
struct FilmParams {
    const float *samples; /* float3 x WS * HS, raster order */
    float *image;         /* float3 x W * H */
    const float *table;   /* PM_FILM_TABLE^2 weights (pm_film_filter_table) */
    int W, H, WS, HS;
    CameraDev cam;
    float xw, yw, inv_xw, inv_yw;
    int hx, hy;           /* footprint halo in pixels per side (conservative) */
    int row_w, band_rows; /* staged row width (samples) and rows per band */
};

/* GridDesc, R2_BINS, R2_COPIES, R2_PER_OCTAVE: pm_plan_pod.h */

/* bucket coordinate along one axis, clamped (points outside the scene box
 * map to the border cells on both the build and the query side) */
PMD uint32_t cell_axis(float v, float g0, float inv_cs, int dim) {
    int c = (int)floorf((v - g0) * inv_cs);
    c = c < 0 ? 0 : (c >= dim ? dim - 1 : c);
    return (uint32_t)c;
}

struct TraceParams {
    SceneDev S;
    pm_photon *slots;
    uint32_t perm[28];
    uint32_t perm_bits[3]; /* the base 3, 5, 7 tables of perm, 3 bits per digit (permuted_halton4) */
    int64_t path_begin, path_count, slot_path_base;
    int64_t pool_paths; /* > 0: pooled kernel (k_trace_pool, 4-wide BVH scenes), paths per wave; else one path per lane */
    int pass, mpc, max_spec, light_index;
    float eps;
    uint32_t seed;
    unsigned long long *counters; /* census [rays, nodes, prim tests, deposits] */
    unsigned long long *prof;     /* phase cycles (PM_TRACE_PROFILE builds), 8 words */
    /* fused bucket counting (bucket != 0): per slot cell key (0xffffffff =
     * invalid) and rank = atomicAdd(count[key]) of the build's counting pass */
    int bucket;
    GridDesc grid;
    uint32_t *count, *key, *rank;
    /* per-lane / pooled kernels: a path's deposits held in registers and
     * written once per path (pm_trace.hip Held; used when mpc == 4 and the
     * slot buffer is 16-B aligned) */
    int hold;
    /* pooled kernel: LDS stack entries per lane (0: S.stack_depth); deeper
     * entries go to spill (entry i of thread g at spill[(i - pool_stack) *
     * spill_stride + g]) */
    int pool_stack;
    int *spill;
    uint32_t spill_stride;
    /* fused counting: keys / ranks plane-major (deposit k of path i at k * key_np + i) when > 0, else at the slot index */
    int64_t key_np;
    /* fused counting only: 1 = leave a path's unused slots as they are (their
     * keys say invalid; pm_api zeroes them with launch_zero_invalid_slots
     * before anything else reads the slot buffer) */
    int lazy_zero;
    /* light_index == PM_ALL_LIGHTS: the light selection table, S.n_lights
     * floats (pm_light_selection_cdf) in a buffer of its own in HBM like
     * SceneDev::light_tris: no part of the scene blob, so it changes no
     * scene's traversal mode and costs no LDS. Selects the ALL instantiations
     * of the trace kernels (launch_trace); the fixed-light ones never read it */
    const float *light_cdf;
    /* pm_set_caustic_map: != 0 selects the MARK instantiations (launch_trace),
     * which set bit 1 of pm_photon::bits on a deposit whose earlier hits were
     * all specular; never with held deposits, a textured material or one of
     * the physical specular model. The other kernels never read it */
    int mark;
};

struct GatherParams {
    RecordsDev R;
    int64_t rec_begin, rec_end; /* records gathered by this launch */
    const float4 *materials;
    float ppm_alpha;
    /* grid */
    GridDesc grid;
    const uint32_t *cell_start; /* ncells + 1 */
    const float4 *ph_a;         /* x, y, z, wi.x */
    const float4 *ph_b;         /* 2 per photon: (alpha.rgb, wi.y), (wi.z, 0, 0, 0) */
    /* kd-tree (reference layout) */
    const pm_photon *kd_nodes;
    int64_t kd_count;
    int kd_stack;         /* traversal stack entries (<= KD_STACK; smaller only to test the overflow report) */
    unsigned int *error;  /* PM_GATHER_ERR_* of the launch (device word, OR-ed) */
    /* fixed-point flux: contribution c -> rint(c * fx_scale), fx_inv = 1/fx_scale (2^-S) */
    float fx_scale;
    double fx_inv;
    /* every contribution is >= 0 (scene emission and albedos and the photon
     * fluxes are non-negative): the tile kernel may sum in double (exact) */
    int fx_nonneg;
    /* partial mode: per record int64 (M, L.x, L.y, L.z) in fixed point, or
     * (count != null) split: int32 M in count[k], three int64 in flux[3k..] */
    long long *partial;
    int *count;
    long long *flux;
    /* fresh: records are in a deferred reset (pm_reset_records): read the
     * initial PPM state (flux 0, N 0, r2init) instead of memory, write it back */
    int fresh;
    float r2init;
    /* record view: view_rank[r] = position of record r in the view (partials),
     * view_list[i] = record of view position i (update); null = all records */
    const uint32_t *view_rank;
    const uint32_t *view_list;
    /* grid gather kernel (PM_GK_*): tile (k_gather_tile, LDS-staged, default),
     * lane (k_gather_grid, per lane from global memory); census launches
     * always run k_gather_grid */
    int kernel;
    int span; /* tile kernel: cells per axis of a lane box at the grid's design radius (2..5) */
    /* tile kernel: a wave's direct lanes with small boxes are scanned by the
     * whole wave together (coop_batch) when their cells hold at most
     * 64 * coop_steps photons, else each lane scans its own */
    uint32_t coop_steps;
    /* non-null: k_gather_tile bins every updated radius, R2_COPIES x R2_BINS
     * counters, bin = floor(-log2(r^2 * r2hist_inv) * R2_PER_OCTAVE) clamped */
    uint32_t *r2hist;
    float r2hist_inv;
    /* kNN estimator (k_gather_knn): knn_k nearest photons with d^2 < knn_r2;
     * per-record fixed-point scale = power of two below knn_fx * r_k^2;
     * slots = the slot buffer the buckets were built from (ph_b carries the
     * slot index) */
    int knn_k;
    float knn_r2, knn_fx;
    const pm_photon *slots;
    unsigned long long *counters; /* [0] visited, [1] in radius */
    /* tile list (non-null: full-range gathers): the launch covers only the
     * n_tiles tiles of 64 records (tile t = records [64 t, 64 t + 64)) that
     * hold an active record, in record order */
    const uint32_t *tiles;
    int64_t n_tiles;
    /* non-null: the list's length is this device word (the host has not read
     * it back yet); n_tiles then bounds the grid (every tile) */
    const uint32_t *n_tiles_dev;
    /* non-null: each tile wave stores its lifetime (s_memrealtime ticks,
     * saturated to 16 bits) at tile_cost[list entry], for the cost-ordered
     * list of the next gathers (launch_tile_sort) */
    uint16_t *tile_cost;
    /* PM_TILE_TIMES diagnostic builds: per launched wave (start, end)
     * s_memrealtime and (XCC_ID, HW_ID), 4 u64 at tile_times[4 * block] */
    unsigned long long *tile_times;
    /* kNN scalar-stream kernel (k_gather_knn_ss): photon pairs (k_knn_pack,
     * knn_pk_pairs of them: 2 float4 + 3 float4 per pair) and the list of
     * tiles it hands back to k_gather_knn_tile (knn_ovf, length *knn_ovf_n) */
    float4 *knn_pk_p, *knn_pk_q;
    int64_t knn_pk_pairs;
    int knn_pack; /* 1: (re)write the pairs (the map changed since the last pack); else only clear the counters */
    uint32_t *knn_ovf, *knn_ovf_n;
};
/* knn_ovf_n[0] = handed-back tiles, in a header of 64 counters that
 * k_knn_pack / launch_knn_ss's memset clear; the list follows */
constexpr int KNN_OVF_HDR = 64;

struct FinalParams {
    RecordsDev R;
    int knn;                     /* records hold kNN sums: out = DL + flux / emitted * Kd/pi */
    const float4 *materials;
    float emitted;
    int64_t rec_begin, rec_count;
    float *out;     /* float3 */
    int raster;     /* 1: out indexed by pixel (pinhole), 0: by record - rec_begin */
    int W;
    const uint32_t *view; /* non-null: [rec_begin, rec_begin + rec_count) index the active-record view */
    /* non-null (a textured scene): the records' albedo factors (EyeParams::kd).
     * A textured matte's Kd is 1 in the materials table, so every gather sums
     * with f = 1 / pi, and the texel multiplies the indirect term here */
    const float4 *kd;
    /* resampled != 0 (pm_eye_resample's records, k_final_resampled; never with
     * knn or kd): dl is the sum of n_eye eye samples' direct light and is
     * divided by (float)n_eye, and a record whose last sample is MISS or
     * EXCEPTION still shows what its earlier samples gathered. Both 0 on every
     * other path, whose kernel (k_final) reads neither */
    int n_eye, resampled;
};

/* final gathering (pm_fgather.hip; pm_api.h pm_final_gather_pass states the
 * operation). Secondary record s = r * n_gather + j is gather ray j of primary
 * record r; a launch covers the secondary records [sec_begin, sec_begin +
 * R.count) of whole primary tiles, stored at R[s - sec_begin]. */
struct FgParams {
    SceneDev S;
    RecordsDev P;  /* the primary records (pm_eye_pass); read only */
    RecordsDev R;  /* the chunk's secondary records; R.count of them */
    int64_t sec_begin;
    int n_gather;
    uint32_t pass, light_seed;
    float eps, r2init;
    int max_spec;
};
struct FgSumParams {
    RecordsDev P;
    const float *li;   /* k_final's output over the chunk's secondary records, float3 in record order */
    float4 *sum;       /* A, one float4 per primary record */
    int64_t rec_begin, rec_count; /* the chunk's primary records */
    int n_gather;
    int zero;          /* pass 0: A starts from 0 */
};
struct FgResolveParams {
    RecordsDev P;
    const float4 *sum;
    const float4 *materials;
    float denom;       /* (float)(n_gather * passes) */
    int64_t rec_begin, rec_count;
    float *out;        /* float3 */
    int raster, W;     /* as FinalParams */
};

/* the output tail of the kernels that write radiance (k_final, k_final_resampled,
 * k_simple, k_fg_resolve): the host's check of photonmappingrenderer.cpp:251-268
 * and simplerender.cpp:70-87 (a NaN, or a negative or infinite luminance, pbrt
 * RGBSpectrum::y, shows black), the float3 store, and the place of record r,
 * number i of its launch, in `out`: i, or with `raster` its pixel (false for a
 * record outside the raster, which has none) */
PMD v3 sanitise_radiance(v3 v) {
    const float y = 0.212671f * v.x + 0.715160f * v.y + 0.072169f * v.z;
    if (isnan(v.x) || isnan(v.y) || isnan(v.z) || y < -1e-5f || isinf(y)) v = mk(0.f, 0.f, 0.f);
    return v;
}
PMD void store_rgb(float *out, int64_t o, v3 v) {
    out[3 * o + 0] = v.x;
    out[3 * o + 1] = v.y;
    out[3 * o + 2] = v.z;
}
PMD bool out_index(int64_t r, int64_t i, int raster, int W, uint32_t flags, int64_t *o) {
    *o = i;
    if (raster) {
        int px, py;
        rec_to_pixel(r, W, &px, &py);
        if (flags & PM_REC_INVALID) return false;
        *o = (int64_t)py * W + px;
    }
    return true;
}

/* traversal mode of a scene: LDS-resident blob (brute force when tiny) or HBM */
inline int scene_mode(const SceneDev &S) {
    return S.n_inst > 0 ? MODE_INST : S.lds_bytes ? (S.brute ? MODE_BRUTE : MODE_LDS) : MODE_GLOBAL;
}
/* f(std::integral_constant<int, MODE>) for the traversal mode `mode`: the one
 * switch from a scene's mode to the kernels instantiated per mode */
template <class F>
inline void dispatch_mode(int mode, F &&f) {
    switch (mode) {
    case MODE_BRUTE: f(std::integral_constant<int, MODE_BRUTE>{}); break;
    case MODE_LDS: f(std::integral_constant<int, MODE_LDS>{}); break;
    case MODE_INST: f(std::integral_constant<int, MODE_INST>{}); break;
    default: f(std::integral_constant<int, MODE_GLOBAL>{}); break;
    }
}
/* f(std::integral_constant<int, 1>) or <int, 0>: a launch's yes / no property
 * to the template argument of the kernels instantiated for both (pm_trace.hip
 * adds dispatch_mat for its four material classes) */
template <class F>
inline void dispatch_flag(bool flag, F &&f) {
    if (flag) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 0>{});
}
/* a launch of the eye-side traversal kernels over `count` lanes: blocks of
 * EYE_BLOCK, and as dynamic LDS a stack column per lane, then the scene blob
 * of the LDS modes */
inline void eye_launch_geometry(const SceneDev &S, int64_t count, unsigned *grid, size_t *lds) {
    *grid = (unsigned)((count + EYE_BLOCK - 1) / EYE_BLOCK);
    *lds = (size_t)S.stack_depth * EYE_BLOCK * 4 + S.lds_bytes;
}

hipError_t launch_eye(const EyeParams &p, hipStream_t s);
/* eye pass p.pass > 0 of pm_eye_resample over the records of an earlier eye
 * pass: pm_set_camera's rays, no textured or physically specular material */
hipError_t launch_eye_resample(const EyeParams &p, hipStream_t s);
/* simple renderer (simplerender.cu): direct light per eye sample into out
 * (float3, raster / sample order); only p.R.count of the records is read */
hipError_t launch_simple(const EyeParams &p, float *out, hipStream_t s);
/* pm_camera_rays_pass: rays6 (o.xyz, d.xyz) and film_xy (fx, fy) of samples
 * [first, first + count) of p's camera in eye pass p.pass (device buffers;
 * either may be null) */
hipError_t launch_camera_rays(const EyeParams &p, int64_t first, int64_t count, float *rays6, float *film_xy,
                              hipStream_t s);
/* the film (pm_film.hip): fills hx / hy / row_w / band_rows of p itself */
hipError_t launch_film(FilmParams p, hipStream_t s);
/* writes every slot of its paths (deposits, then zeros); count: census */
/* pm_plan.h's WavesPerCu from the occupancy API: resident waves per CU of a trace kernel family */
int trace_waves_per_cu(TraceFamily family, bool hold, size_t lds);
size_t scan_scratch_words(int64_t n);
/* adaptive-grid histogram: sum the R2_COPIES copies into host-mapped
 * out[R2_BINS] with plain stores (no copy engine) and zero the copies */
hipError_t launch_r2hist_reduce(uint32_t *hist, uint32_t *out_mapped, hipStream_t s);
/* kernel, grid and LDS bytes from pl, the plan p was filled from */
hipError_t launch_trace(const TraceParams &p, const TracePlan &pl, int count, hipStream_t s);
/* photon-bucket build (pm_bucket.hip): count + rank, scan, fill.
 * count and cell_start have ncells + 1 entries; cell_start[ncells] = valid
 * photons; scratch holds bucket_scratch_words() uint32: key[n], rank[n], ...
 * counted: key/rank/count were produced by the trace kernel (TraceParams::bucket);
 * otherwise count must arrive zeroed. count leaves zeroed (cleared by the scan). */
size_t bucket_scratch_words(int64_t n_slots, uint32_t ncells);
hipError_t launch_bucket_build(const pm_photon *slots, int64_t n, GridDesc g, uint32_t *count, uint32_t *cell_start,
                               uint32_t *scratch, float4 *ph_a, float4 *ph_b, bool counted, hipStream_t s,
                               int64_t key_np = 0, int mpc = 1);
/* the caustic bucket map (pm_caustic.hip): launch_bucket_build over the slots
 * with bit 1 of pm_photon::bits set alone, into a count / cell_start / ph_a /
 * ph_b set of its own on grid g (ph_b keeps the slot index). count arrives
 * zeroed and leaves zeroed; scratch holds caustic_scratch_words() uint32 */
size_t caustic_scratch_words(int64_t n_slots, uint32_t ncells);
hipError_t launch_caustic_build(const pm_photon *slots, int64_t n, GridDesc g, uint32_t *count, uint32_t *cell_start,
                                uint32_t *scratch, float4 *ph_a, float4 *ph_b, hipStream_t s);
/* launch_exclusive_scan that zeroes `in` as it reads it (the bucket build's scan) */
hipError_t launch_exclusive_scan_clear(uint32_t *in, int64_t n, uint32_t *out, uint32_t *sums, hipStream_t s);
/* the caustic radiance Lc of records [rec_begin, rec_begin + rec_count) (pm_api.h pm_caustic_gather), float3 in
 * record order; and pm_final_gather_resolve with it: out = (dl + Lc) + Kd x (A / denom) */
hipError_t launch_caustic_radiance(const FgResolveParams &p, float emitted, hipStream_t s);
hipError_t launch_fg_resolve_caustic(const FgResolveParams &p, float emitted, hipStream_t s);
/* gather: structure 0 grid, 1 kd; mode 0 fused PPM, 1 partial */
hipError_t launch_gather(const GatherParams &p, int structure, int partial, int count, hipStream_t s);
/* kNN estimator (pbrt LPhoton) over the photon buckets, fused record update */
hipError_t launch_gather_knn(const GatherParams &p, int count, hipStream_t s);
/* its scalar-stream step (pm_gather_knn_ss.hip): the photon pairs when
 * p.knn_pack (else only the handed-back counters cleared), then
 * k_gather_knn_ss over grid tiles; the tiles it does not handle are left in
 * p.knn_ovf[0 .. *p.knn_ovf_n) for k_gather_knn_tile. Returns the memset's
 * error; a launch error stays for the hipGetLastError after the tile launch */
hipError_t launch_knn_ss(const GatherParams &p, unsigned grid, hipStream_t s);
hipError_t launch_ppm_update(const GatherParams &p, const long long *partial, int64_t rec_begin, int64_t rec_count,
                             hipStream_t s);
hipError_t launch_ppm_update_split(const GatherParams &p, const int *count, const long long *flux, int64_t n_view,
                                   int64_t v_begin, int64_t v_count, int fresh, hipStream_t s);
hipError_t launch_ppm_update_radius(const GatherParams &p, const int *count, float *ratio, int64_t n_view, int fresh,
                                    hipStream_t s);
hipError_t launch_ppm_update_flux(const GatherParams &p, const float *ratio, const long long *flux, int64_t v_begin,
                                  int64_t v_count, hipStream_t s);
hipError_t launch_final(const FinalParams &p, hipStream_t s);
/* final gathering (pm_fgather.hip): the chunk's gather rays traced and shaded
 * into its secondary records; rays6 non-null: only the rays (o.xyz, d.xyz;
 * d = 0 for a ray that is not traced) of secondary records [first, first +
 * count), nothing traced (p.R unused) */
hipError_t launch_fg_rays(const FgParams &p, hipStream_t s);
hipError_t launch_fg_ray_dump(const FgParams &p, int64_t first, int64_t count, float *rays6, hipStream_t s);
hipError_t launch_fg_accumulate(const FgSumParams &p, hipStream_t s);
hipError_t launch_fg_resolve(const FgResolveParams &p, hipStream_t s);
/* list[0 .. *count) = the tiles (records [64 t, 64 t + 64)) holding an
 * active record, ascending, built on the device (flags: one byte per tile) */
/* the slots of [0, n) whose fused-count key is invalid (0xffffffff) set to
 * zero: the deferred zero fill of a lazy_zero trace (key index as the
 * trace wrote it: plane-major k * key_np + path when key_np > 0) */
hipError_t launch_zero_invalid_slots(pm_photon *slots, const uint32_t *key, int64_t n, int64_t key_np, int mpc,
                                     hipStream_t s);
hipError_t launch_tile_list(const RecordsDev &R, uint8_t *flags, uint32_t *list, uint32_t *count, hipStream_t s);
/* the tile list reordered by measured cost: groups of 8 consecutive entries
 * (a wave's XCD group, xcd_tile) in descending order of their largest
 * tile_cost, the last partial group kept last; n = *n_dev when non-null */
hipError_t launch_tile_sort(const uint32_t *list, const uint16_t *cost, const uint32_t *n_dev, int64_t n, uint32_t *out,
                            hipStream_t s);
hipError_t launch_radius2_io(const RecordsDev &R, float *buf, int64_t rec_begin, int64_t rec_count, int to_records,
                             const uint32_t *view, hipStream_t s);
/* exclusive scan of n uint32 (pm_bucket.hip); in/out 16-B aligned; sums: scan_scratch_words(n) */
size_t scan_scratch_words(int64_t n);
hipError_t launch_exclusive_scan(const uint32_t *in, int64_t n, uint32_t *out, uint32_t *sums, hipStream_t s);
/* active-record view: flags/rank n+1 words, list n words; rank[n] = active count */
hipError_t launch_record_view(const RecordsDev &R, uint32_t *flags, uint32_t *rank, uint32_t *list, uint32_t *sums,
                              hipStream_t s);
hipError_t launch_reset_records(const RecordsDev &R, float r2init, hipStream_t s);

/* scene BVH on the device (pm_bvh_gpu.hip): PLOC over the primitive boxes
 * (box: 2 float4 per primitive, (lo.xyz, ref bits) (hi.xyz, 0); Morton frame
 * of pm_build.h ploc_morton_frame), collapsed into quantized 4-wide nodes —
 * the tree pm_build.h build_ploc + ploc_to_bvh + collapse_bvh4 +
 * bvh4_bfs_order + quantize_bvh4 produce on the host, bit for bit. Outputs:
 * wnodes (<= max_nodes nodes of 4 uint4, breadth-first), refs (n, Morton
 * order; triangles as PRIM_TRI << 30 | storage slot) and tri_order (storage
 * slot -> triangle id, triangles in Morton order). Blocks on the stream. */
struct GpuBvhIn {
    const float4 *box;
    int n;
    float frame_lo[3], frame_scale[3];
    int radius;
};
struct GpuBvhOut {
    uint4 *wnodes;
    uint32_t *refs, *tri_order;
    int64_t max_nodes;
    int64_t nodes = 0, n_tris = 0;
    int depth = 0, max_stack = 0, rounds = 0;
};
hipError_t gpu_bvh_build(const GpuBvhIn &in, GpuBvhOut &out, hipStream_t s);
/* triangle records computed in triangle-id order -> storage order */
hipError_t launch_tri_permute(const uint32_t *tri_order, int64_t nst, const float4 *src_geo, const float4 *src_shade,
                              const int4 *src_info, float4 *geo, float4 *shade, uint32_t *tid, int4 *info,
                              hipStream_t s);

} // namespace pm
