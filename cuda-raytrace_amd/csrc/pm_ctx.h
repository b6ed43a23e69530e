/*
 * pm_ctx.h — what the units of the C-ABI (pm_api.cpp, pm_api_scene.cpp, the
 * stage units pm_api_records.cpp, pm_api_photons.cpp, pm_api_gather.cpp and
 * pm_api_fgather.cpp, pm_api_render.cpp) share and nothing else includes: the
 * context (DevBuf, RecordBufs, BucketMap, TileList, Ctx, Group), the error and
 * context macros (FAIL / HIPCHK / GETCTX / GROUP_FWD) and the few helpers more
 * than one unit calls. Everything here is hidden: the library exports the
 * pm_* entry points of include/pm_api.h alone.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "pm_build.h"
#include "pm_kernels.h"
#include "pm_plan.h"
#include "pm_scene.h"

#pragma clang fp contract(off)

using namespace pm;

#pragma GCC visibility push(hidden)

extern std::string g_last_error; /* pm_api.cpp */

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t n) {
        if (n <= bytes && p) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        if (n == 0) n = 16;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    /* ensure() with 50 % headroom: buffers sized by the photon grid or the
     * valid photons of a pass, which change from pass to pass of a
     * progressive render (the radius shrinks, the grid gains cells): a
     * reallocation's hipFree waits for the device and left a ~250 us bubble
     * in every C5 pass (profiles/r06/c5_realloc) */
    hipError_t ensure_slack(size_t n) { return n <= bytes && p ? hipSuccess : ensure(n + n / 2); }
    bool external = false; /* caller-owned memory: never freed or grown here */
    void release() { if (p && !external) (void)hipFree(p); p = nullptr; bytes = 0; external = false; }
    template <class T> T *as() const { return (T *)p; }
};

/* One record set (RecordsDev) in device memory: Ctx::rec holds the primary
 * records, Ctx::fg_rec the secondary records of a final-gather chunk. */
struct RecordBufs {
    DevBuf pos, nrm, state, n, dl;
    hipError_t ensure(int64_t cnt) {
        hipError_t e = hipSuccess;
        for (DevBuf *b : {&pos, &nrm, &state, &n, &dl})
            if ((e = b->ensure((size_t)cnt * (b == &n ? sizeof(float) : sizeof(float4)))) != hipSuccess) break;
        return e;
    }
    RecordsDev dev(int64_t cnt) const {
        return {pos.as<float4>(), nrm.as<float4>(), state.as<float4>(), n.as<float>(), dl.as<float4>(), cnt};
    }
    void release() { for (DevBuf *b : {&pos, &nrm, &state, &n, &dl}) b->release(); }
    /* blocking copies of the first cnt records to / from the C-ABI's layout (pm_api_records.cpp) */
    hipError_t download(pm_record *out, int64_t cnt) const;
    hipError_t upload(const pm_record *in, int64_t cnt);
};

/* One bucket map: the cell-sorted photons of a build on `grid`, and the kNN
 * scalar stream's buffers over them. Ctx::map is pm_build_photon_map's (its
 * count and scratch are also what a fused trace writes and materialize_slots
 * reads), Ctx::cmap pm_build_caustic_map's. */
struct BucketMap {
    DevBuf count, cell_start, scratch, ph_a, ph_b;
    DevBuf knn_pk, knn_ovf;    /* kNN scalar stream: photon pairs, handed-back tiles (+ count) */
    GridDesc grid{};
    int64_t slots = 0;         /* the slots of the last build */
    uint64_t gen = 0;          /* bumped by every build */
    uint64_t pack_gen = ~0ull; /* the build knn_pk's pairs were packed from */
    void *pack_ptr = nullptr;  /* ... and the pair buffer they were written to */

    void attach(GatherParams &G) const {
        G.grid = grid;
        G.cell_start = cell_start.as<uint32_t>();
        G.ph_a = ph_a.as<float4>(); G.ph_b = ph_b.as<float4>();
    }
    /* the valid photons of the last build, cell_start[ncells]: copied on s,
     * which the caller waits for, or (no s) by a blocking copy */
    hipError_t valid_photons(uint32_t *nv, hipStream_t s = nullptr) const {
        const uint32_t *last = cell_start.as<uint32_t>() + grid.ncells;
        return s ? hipMemcpyAsync(nv, last, 4, hipMemcpyDeviceToHost, s) : hipMemcpy(nv, last, 4, hipMemcpyDeviceToHost);
    }
    void release() { for (DevBuf *b : {&count, &cell_start, &scratch, &ph_a, &ph_b, &knn_pk, &knn_ovf}) b->release(); }
};

/* The tiles (64 records) that hold an active record, in record order:
 * full-range tile gathers launch over these only (records are fixed after
 * the eye pass). Built on the device without a host wait: flags + an
 * in-order compaction, its length copied to pinned memory behind an event.
 * Until that copy has landed (hipEventQuery, never waited on) the gather
 * kernels read the length from device memory and the grid covers every
 * tile. The list is reordered once by the measured cost of its tiles (the
 * first full-range tile gather on it records them, launch_tile_sort). */
struct TileList {
    DevBuf d_list, d_flags, d_count, d_cost, d_sorted;
    bool sort = true;         /* env PM_TILE_SORT=0 keeps record order */
    bool valid = false;       /* the list on the device matches the records */
    bool sorted = false;
    bool count_known = false; /* its length has landed in n */
    int64_t n = 0;
    uint32_t *h_count = nullptr;
    hipEvent_t event = nullptr;

    void invalidate() { valid = false; }
    hipError_t ensure(const RecordsDev &R, hipStream_t s) {
        hipError_t e = hipSuccess;
        auto ok = [&e](hipError_t r) { return (e = r) == hipSuccess; };
        if (!valid) {
            const int64_t nt = (R.count + 63) / 64;
            if (!ok(d_flags.ensure(std::max<int64_t>(nt, 16))) || !ok(d_list.ensure(std::max<int64_t>(nt * 4, 16))) ||
                !ok(d_count.ensure(16)))
                return e;
            if (!h_count && !ok(hipHostMalloc((void **)&h_count, 4, hipHostMallocDefault))) return e;
            if (!event) {
                if (!ok(hipEventCreateWithFlags(&event, hipEventDisableTiming))) return e;
            } else if (!count_known && !ok(hipEventSynchronize(event))) {
                /* a previous list's length still in flight (records replaced before
                 * any gather read it): that copy lands before the pinned word is reused */
                return e;
            }
            if (!ok(launch_tile_list(R, d_flags.as<uint8_t>(), d_list.as<uint32_t>(), d_count.as<uint32_t>(), s)) ||
                !ok(hipMemcpyAsync(h_count, d_count.p, 4, hipMemcpyDeviceToHost, s)) || !ok(hipEventRecord(event, s)))
                return e;
            valid = true;
            sorted = false;
            count_known = false;
        }
        if (!count_known && hipEventQuery(event) == hipSuccess) {
            n = (int64_t)*h_count;
            count_known = true;
        }
        return hipSuccess;
    }
    /* launch_tile_sort wrote the reordered list into d_sorted */
    void swap_sorted() { std::swap(d_list, d_sorted); sorted = true; }
    void release() {
        for (DevBuf *b : {&d_list, &d_flags, &d_count, &d_cost, &d_sorted}) b->release();
        if (event) (void)hipEventDestroy(event);
        if (h_count) (void)hipHostFree(h_count);
    }
};

struct Timer { hipEvent_t a = nullptr, b = nullptr; };
struct TimerPool { std::vector<Timer> ev; size_t used = 0; };

struct Group;
struct Ctx {
    Group *group = nullptr; /* non-null: a multi-device context (pm_config::n_devices), Group below */
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    HostScene hs; /* the host scene (pm_scene.h): the pm_add_* calls fill it, pm_commit assembles it */
    int rand2d_total = 0;
    float world_sphere[4] = {0, 0, 0, 0}; /* PM_SCENE_WORLD_SPHERE, of the last commit */
    int pinhole = 0, W = 0, H = 0;
    /* pm_set_camera: pinhole = 1 and W x H the sample raster (image * strata),
     * so records, views and bands are the pinhole's; cam keeps the image size,
     * the sampling state and the filter, film_table its weights */
    int camera = 0;
    pm_camera cam{};
    DevBuf d_film_table, d_img;
    float eye[3] = {0}, fwd[3] = {0}, right[3] = {0}, up[3] = {0};
    std::vector<float> rays, rand2d;
    int64_t nrays = 0;
    int n2d = 0;
    bool committed = false;
    /* device scene */
    DevBuf d_scene, d_rays, d_rand2d; /* d_scene: the scene blob (SceneDev) */
    DevBuf d_light_tris;              /* SceneDev::light_tris (kept out of the blob: never LDS-resident) */
    /* the committed scene's layout, and its light summary: emission / albedo
     * bounds for the fixed-point flux scale (flux_bound chooses the
     * emission bound per call) and the PM_ALL_LIGHTS selection table, whose
     * device copy is d_light_cdf (TraceParams::light_cdf: a buffer of its own
     * like d_light_tris) */
    SceneLayout L;
    LightSummary lsum;
    DevBuf d_light_cdf;
    DevBuf d_tripairs;                /* brute-force scenes: triangle pairs interleaved (SceneDev::tri_pairs_g) */
    /* textured scenes only (SceneDev::tex_recs, texels, mat_tex, tri_uv), and
     * the records' albedo factors (EyeParams::kd), sized like the records */
    DevBuf d_tex_recs, d_texels, d_mat_tex, d_tri_uv, d_rkd;
    bool textured = false;            /* the committed scene has a textured material */
    /* the physical specular model (SceneDev::mat_spec): the table, and whether
     * the committed scene has such a material. Such a scene also gets d_mat_tex
     * (all -1 without textures) and the albedo factors d_rkd */
    DevBuf d_mat_spec;
    bool specular = false;
    bool albedo() const { return textured || specular; } /* the records carry albedo factors (d_rkd) */
    SceneDev S{};
    float bbox_lo[3] = {0, 0, 0}, bbox_hi[3] = {0, 0, 0};
    bool slots_nonneg = true;  /* the slot buffer holds no negative flux (uploaded slots are checked) */
    int bvh_depth = 0;
    /* records */
    RecordBufs rec;
    int64_t nrec = 0;
    /* eye samples summed in the records' dl: 0 none yet (pm_set_camera,
     * pm_set_pinhole, pm_set_eye_rays), 1 after pm_eye_pass, +1 per
     * pm_eye_resample(pass > 0); above 1 pm_final / pm_final_view divide dl by
     * it and keep MISS / EXCEPTION records (FinalParams::n_eye, resampled) */
    int eye_samples = 0;
    /* slots */
    DevBuf d_slots;
    int64_t slots_used = 0;
    /* lazy zero fill (TraceParams::lazy_zero): slots [0, slots_dirty) may hold
     * stale data where their fused-count key (map.scratch, dirty_key_np /
     * dirty_mpc) is invalid; materialize_slots zeroes them before any reader
     * but the bucket fill (env PM_LAZY_ZERO=1; by default the trace zeroes them
     * itself: same-box A/B in profiles/r05/trace_writes) */
    int64_t slots_dirty = 0, dirty_key_np = 0;
    int dirty_mpc = 0;
    hipEvent_t dirty_event = nullptr;
    bool lazy_zero = false, slots_exposed = false;
    /* photon buckets (pm_build_photon_map); map.slots also counts a kd-tree build's slots */
    BucketMap map;
    DevBuf d_tile_times;      /* PM_TILE_TIMES diagnostic builds */
    bool knn_ss = true;       /* kNN: k_gather_knn_ss first (PM_KNN_SS=0: k_gather_knn_tile alone) */
    bool fuse_ok = true;      /* trace may fuse the bucket counting (off for the sub-contexts of a multi-device group) */
    struct { bool valid = false; int64_t n = 0; GridDesc grid{}; float r2 = 0.f; int64_t key_np = 0; int mpc = 1; } fused; /* counts made by the last trace (keys plane-major when key_np > 0) */
    float grid_r2 = 0.f; /* radius^2 the photon map's grid (map.grid) is designed for */
    int64_t bvh4_nodes = 0; /* 4-wide BVH of an HBM scene (0: binary traversal) */
    int bvh4_depth = 0;
    int map_kind = -1;
    /* kd-tree */
    DevBuf d_kd;
    int64_t kd_count = 0;
    /* misc */
    DevBuf d_out, d_counters;
    bool counting = false;
    /* record view (pm_set_record_view): active records compacted in record order */
    bool view_active = false;
    int64_t n_view = 0;
    DevBuf d_vflags, d_vrank, d_vlist, d_vsums;
    TileList tiles;
    /* pm_reset_records is deferred: records read as (flux 0, N 0, r2 = rec_fresh_r2) */
    bool rec_fresh = false;
    float rec_fresh_r2 = 0.f;
    /* estimator of the last gather: what the records' flux / radius2 /
     * photon_count mean for the final pass (PPM state or kNN sums) */
    int rec_estimator = PM_ESTIMATOR_PPM;
    /* final gathering (pm_final_gather_pass): the secondary records of one
     * chunk and k_final's radiances over them, the sums A (a float4 per
     * primary record, valid for fg_nrec records of fg_n rays over fg_passes
     * passes; any new primary records drop them) and the chunk cap in
     * secondary records (env PM_FG_CHUNK, tests only) */
    RecordBufs fg_rec;
    DevBuf d_fg_li, d_fg_sum;
    int64_t fg_nrec = 0, fg_chunk = (int64_t)1 << 22;
    int fg_n = 0, fg_passes = 0;
    int64_t fg_chunks = 0; /* chunks (launches per stage timer) of the last pass */
    /* the caustic map (pm_set_caustic_map): the bucket map pm_build_caustic_map
     * fills from the marked slots on the full map's grid (built: cg_built) and
     * the passes pm_caustic_gather has summed into the cg_nrec primary records */
    bool caustic_map = false;
    BucketMap cmap;
    bool cg_built = false;
    int cg_passes = 0;
    int64_t cg_nrec = 0;
    double cg_emitted = 0; /* paths_per_pass of the gathers, times cg_passes: the emitted paths of Lc */
    int kd_stack = KD_STACK;       /* kd gather stack entries (env PM_KD_STACK, tests only) */
    bool trace_pool = true;         /* 4-wide scenes: the pooled trace kernel (env PM_TRACE_POOL=0: one path per lane) */
    bool trace_hold = true;         /* deposits written once per path where it costs no waves (env PM_TRACE_HOLD=0: per deposit) */
    int pool_stack = 31;            /* pooled kernel: LDS stack entries per lane (env PM_POOL_STACK; 0 = the exact bound): 31 lets five blocks share a CU's LDS */
    int trace_cus = 0;              /* > 0: the compute units plan_trace sizes a wave's pool for, in place of the device's
                                     * (env PM_TRACE_CUS: tests and diagnosis; small traces then refill their lanes) */
    DevBuf d_spill;                 /* pooled kernel: stack entries beyond pool_stack */
    int gather_kernel = PM_GK_TILE; /* bucket gather kernel (env PM_GATHER_KERNEL=tile|lane) */
    int cell_span = 2;              /* PPM grid: cells per axis of a query box (env PM_CELL_SPAN 2..5) */
    /* adaptive grid radius: the state machine (pm_plan.h R2Plan) and the HIP
     * objects it speaks of — the device bins (R2_COPIES x R2_BINS), the
     * host-mapped R2_BINS words a reduce writes (and their device address),
     * the event behind the reduce */
    R2Plan grid_plan;
    DevBuf d_hist;
    uint32_t *h_hist = nullptr, *h_hist_dev = nullptr;
    hipEvent_t hist_event = nullptr;
    /* leading words of map.count known to be zero (the bucket scan clears the
     * counters it reads); valid while map.count.p == count_zero_ptr */
    size_t count_zero_words = 0;
    void *count_zero_ptr = nullptr;
    /* stages that get event pairs: "all", "" (none) or a comma list
     * (pm_set_stage_timing; env PM_STAGE_TIMERS=0 starts with none) */
    std::string timed_stages = "all";
    bool stage_active = false;
    StageEvents stage;             /* the stage being timed (g_stage points here) */
    bool stage_marker = false;
    std::map<std::string, TimerPool> timers;
    /* new or moved primary records: the final-gather and caustic sums are another
     * record set's, and so are the tile list and the radii the grid plan binned */
    void records_replaced() { fg_passes = 0; cg_passes = 0; tiles.invalidate(); grid_plan.invalidate(); }
};

#define FAIL(c, code, ...)                                                     \
    do {                                                                       \
        char _b[512];                                                          \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                                 \
        if (c) (c)->err = _b;                                                  \
        g_last_error = _b;                                                     \
        pm::g_stage = nullptr; /* an error inside a timed stage ends it */    \
        return code;                                                           \
    } while (0)

#define HIPCHK(c, expr)                                                                   \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess) FAIL(c, PM_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

#define GETCTX(ptr)                                                                                      \
    Ctx *c = (Ctx *)(ptr);                                                                               \
    if (!c) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "null context");                                        \
    if (c->group)                                                                                        \
        FAIL(c, PM_ERR_INVALID, "%s: a multi-device context takes the scene calls, pm_render and "       \
                                "pm_render_simple (the stage API needs one context per device)", __func__); \
    (void)hipSetDevice(c->device)

inline hipStream_t pick(Ctx *c, void *s) { return s ? (hipStream_t)s : c->stream; }

/* Single-process multi-device context (north_star: tiles and
 * photon batches over the GPUs of one node, RCCL all-gather of the photon
 * slots before the gather): one sub-context per device holds the whole
 * scene and record set; pm_render shards the paths by global id, all-gathers
 * the 40-B slots into every device's buffer (ncclAllGather over xGMI when the
 * devices are distinct, peer copies otherwise), builds the same map on every
 * device and gathers interleaved 8-row bands per device (pmrender/dist.py
 * _bands: runs of bands dealt round-robin, about four per device). */
struct Group {
    std::vector<Ctx *> subs;
    std::vector<int> devs;
    std::vector<ncclComm_t> comms; /* empty: peer-copy exchange */
    std::vector<hipEvent_t> ev;    /* per sub: end of its trace (peer-copy exchange) */
};
inline Group *group_of(void *ptr) { return ptr ? ((Ctx *)ptr)->group : nullptr; }
inline int group_fail(void *ptr, Ctx *sub, int rc) {
    Ctx *c = (Ctx *)ptr;
    c->err = "device " + std::to_string(sub->device) + ": " + sub->err;
    g_last_error = c->err;
    return rc;
}
/* scene calls go to every device's context */
#define GROUP_FWD(ptr, CALL)                                                                                  \
    if (Group *g_ = group_of(ptr)) {                                                                          \
        for (Ctx *sub : g_->subs) {                                                                           \
            const int rc_ = (CALL);                                                                           \
            if (rc_) return group_fail(ptr, sub, rc_);                                                        \
        }                                                                                                     \
        return PM_OK;                                                                                         \
    }

inline int64_t num_records(const Ctx *c) {
    if (c->pinhole) return (int64_t)((c->W + 7) / 8) * ((c->H + 7) / 8) * 64;
    return c->nrays;
}

inline bool real_filter(const pm_filter &f) { return f.type != PM_FILTER_NONE; }

inline bool has_film(const Ctx *c) { return c->camera && real_filter(c->cam.filter); }

inline RecordsDev recs(const Ctx *c) { return c->rec.dev(c->nrec); }

/* number of records the range-based record calls address, and their list */
inline int64_t view_size(const Ctx *c) { return c->view_active ? c->n_view : c->nrec; }
inline const uint32_t *view_list(const Ctx *c) { return c->view_active ? c->d_vlist.as<uint32_t>() : nullptr; }

inline bool same_grid(const GridDesc &a, const GridDesc &b) { return std::memcmp(&a, &b, sizeof(GridDesc)) == 0; }

/* the helpers more than one unit calls, by the unit that defines them.
 * pm_api.cpp: the stage timers (an event pair per launch of a stage) and the Halton table of a pass */
int timer_begin(Ctx *c, const char *name, hipStream_t s, bool marker = false);
void timer_end(Ctx *c, const char *name, hipStream_t s);
double timer_ms(Ctx *c, const char *name, size_t k = 1);
void halton_perm(uint32_t seed, uint32_t out[28]);
/* pm_api_scene.cpp */
void eye_camera(const Ctx *c, EyeParams &E);
/* pm_api_records.cpp */
int check_params(Ctx *c, const pm_render_params *p);
FinalParams final_params(Ctx *c, double emitted, int64_t begin, int64_t count, float *out);
int materialize_reset(Ctx *c, hipStream_t s);
int download_rgb(Ctx *c, const DevBuf &d, float *out_rgb, int64_t n);
/* pm_api_photons.cpp */
int materialize_slots(Ctx *c, hipStream_t s);
/* pm_api_gather.cpp */
GatherParams gather_params(Ctx *c, const pm_render_params *p);
int gather_knn_setup(Ctx *c, const pm_render_params *p, GatherParams &G, BucketMap &m);

#pragma GCC visibility pop
