/*
 * pm_api.cpp — the C-ABI of libpmhip.so (declared in include/pm_api.h):
 * context, scene calls, commit (the device BVH build, or the host assembly
 * of pm_scene.cpp, and the upload), stage orchestration (the grid each pass
 * gets is planned by pm_plan.cpp) and the whole-render entry point. Host code only; the kernels live in the .hip files
 * (launchers in pm_kernels.h). No CPU fallback: every compute entry point
 * launches HIP kernels and fails with PM_ERR_HIP when the device is unusable.
 */
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

namespace {

std::string g_last_error;

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
     * bounds for the fixed-point flux scale (emission_bound chooses the
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
    DevBuf d_pos, d_nrm, d_state, d_n, d_dl;
    int64_t nrec = 0;
    /* slots */
    DevBuf d_slots;
    int64_t slots_used = 0;
    /* lazy zero fill (TraceParams::lazy_zero): slots [0, slots_dirty) may hold
     * stale data where their fused-count key (d_scratch, dirty_key_np /
     * dirty_mpc) is invalid; materialize_slots zeroes them before any reader
     * but the bucket fill (env PM_LAZY_ZERO=1; by default the trace zeroes them
     * itself: same-box A/B in profiles/r05/trace_writes) */
    int64_t slots_dirty = 0, dirty_key_np = 0;
    int dirty_mpc = 0;
    hipEvent_t dirty_event = nullptr;
    bool lazy_zero = false, slots_exposed = false;
    /* photon buckets */
    DevBuf d_count, d_cell_start, d_scratch, d_pha, d_phb;
    DevBuf d_knnpk, d_knnovf; /* kNN scalar stream: photon pairs, handed-back tiles (+ count) */
    DevBuf d_tile_times;      /* PM_TILE_TIMES diagnostic builds */
    uint64_t map_gen = 0;      /* bumped by every bucket build */
    uint64_t knn_pack_gen = ~0ull; /* the map d_knnpk's pairs were packed from */
    void *knn_pack_ptr = nullptr;  /* ... and the pair buffer they were written to */
    bool knn_ss = true;       /* kNN: k_gather_knn_ss first (PM_KNN_SS=0: k_gather_knn_tile alone) */
    bool fuse_ok = true;      /* trace may fuse the bucket counting (off for the sub-contexts of a multi-device group) */
    struct { bool valid = false; int64_t n = 0; GridDesc grid{}; float r2 = 0.f; int64_t key_np = 0; int mpc = 1; } fused; /* counts made by the last trace (keys plane-major when key_np > 0) */
    GridDesc grid{};
    float grid_r2 = 0.f; /* radius^2 the photon map's grid is designed for */
    int64_t bvh4_nodes = 0; /* 4-wide BVH of an HBM scene (0: binary traversal) */
    int bvh4_depth = 0;
    int map_kind = -1;
    int64_t map_slots = 0;
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
    int kd_stack = KD_STACK;        /* kd gather stack entries (env PM_KD_STACK, tests only) */
    bool trace_pool = true;         /* 4-wide scenes: the pooled trace kernel (env PM_TRACE_POOL=0: one path per lane) */
    bool trace_hold = true;         /* deposits written once per path where it costs no waves (env PM_TRACE_HOLD=0: per deposit) */
    int pool_stack = 31;            /* pooled kernel: LDS stack entries per lane (env PM_POOL_STACK; 0 = the exact bound): 31 lets five blocks share a CU's LDS */
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
    /* leading words of d_count known to be zero (the bucket scan clears the
     * counters it reads); valid while d_count.p == count_zero_ptr */
    size_t count_zero_words = 0;
    void *count_zero_ptr = nullptr;
    /* stages that get event pairs: "all", "" (none) or a comma list
     * (pm_set_stage_timing; env PM_STAGE_TIMERS=0 starts with none) */
    std::string timed_stages = "all";
    bool stage_active = false;
    StageEvents stage;             /* the stage being timed (g_stage points here) */
    bool stage_marker = false;
    std::map<std::string, TimerPool> timers;
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

hipStream_t pick(Ctx *c, void *s) { return s ? (hipStream_t)s : c->stream; }

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
Group *group_of(void *ptr) { return ptr ? ((Ctx *)ptr)->group : nullptr; }
int group_fail(void *ptr, Ctx *sub, int rc) {
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

} // namespace
thread_local pm::StageEvents *pm::g_stage = nullptr;
namespace {

/* Every stage launch takes a fresh event pair from a per-stage pool. Kernel
 * stages bind the pair to their own dispatches (pm_launch, pm_kernels.h):
 * no marker packets, so timing leaves no idle gap between kernels. A stage
 * of host work / copies (marker = true) records the pair as markers.
 * Nothing synchronizes until a reader asks. */
bool stage_timed(const Ctx *c, const char *name) {
    const std::string &t = c->timed_stages;
    if (t == "all") return true;
    const size_t n = strlen(name);
    for (size_t i = 0; i < t.size();) {
        size_t j = t.find(',', i);
        if (j == std::string::npos) j = t.size();
        if (j - i == n && t.compare(i, n, name) == 0) return true;
        i = j + 1;
    }
    return false;
}
int timer_begin(Ctx *c, const char *name, hipStream_t s, bool marker = false) {
    c->stage_active = stage_timed(c, name);
    if (!c->stage_active) return 0;
    TimerPool &tp = c->timers[name];
    if (tp.used == tp.ev.size()) {
        Timer t;
        /* timing-only events: no system-scope fence (cache write-back +
         * invalidate) when recorded */
        (void)hipEventCreateWithFlags(&t.a, hipEventDisableSystemFence);
        (void)hipEventCreateWithFlags(&t.b, hipEventDisableSystemFence);
        tp.ev.push_back(t);
    }
    const Timer &t = tp.ev[tp.used];
    c->stage = StageEvents{t.a, t.b, 0};
    c->stage_marker = marker;
    if (marker) {
        (void)hipEventRecord(t.a, s);
        c->stage.launched = 1; /* start taken: kernels only move the stop */
    }
    g_stage = &c->stage;
    return 0;
}
void timer_end(Ctx *c, const char *name, hipStream_t s) {
    if (!c->stage_active) return;
    c->stage_active = false;
    g_stage = nullptr;
    TimerPool &tp = c->timers[name];
    const Timer &t = tp.ev[tp.used];
    if (c->stage.launched == 0) (void)hipEventRecord(t.a, s); /* nothing launched: an empty interval */
    if (c->stage_marker || c->stage.launched == 0) (void)hipEventRecord(t.b, s);
    tp.used++;
}
double pair_ms(const Timer &t) {
    (void)hipEventSynchronize(t.b);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, t.a, t.b) != hipSuccess) return -1.0;
    return ms;
}
/* duration of the most recent launch of a stage (k > 1: the sum of the last k) */
double timer_ms(Ctx *c, const char *name, size_t k = 1) {
    auto it = c->timers.find(name);
    if (it == c->timers.end() || it->second.used == 0) return -1.0;
    double ms = 0;
    for (size_t i = it->second.used - std::min(k, it->second.used); i < it->second.used; ++i) ms += pair_ms(it->second.ev[i]);
    return ms;
}

int64_t num_records(const Ctx *c) {
    if (c->pinhole) return (int64_t)((c->W + 7) / 8) * ((c->H + 7) / 8) * 64;
    return c->nrays;
}

/* pbrt-v2 PermutedHalton(5, RNG(seed)) table (montecarlo.h GeneratePermutation
 * + Shuffle over MT19937 == std::mt19937; photonmappingrenderer.cpp:216). */
void halton_perm(uint32_t seed, uint32_t out[28]) {
    std::mt19937 rng(seed);
    const uint32_t primes[5] = {2, 3, 5, 7, 11};
    uint32_t *p = out;
    for (int d = 0; d < 5; ++d) {
        uint32_t b = primes[d];
        for (uint32_t i = 0; i < b; ++i) p[i] = i;
        for (uint32_t i = 0; i < b; ++i) {
            uint32_t other = i + ((uint32_t)rng() % (b - i));
            std::swap(p[i], p[other]);
        }
        p += b;
    }
}

/* the deferred zero fill of a lazy_zero trace, on stream s after the trace
 * (s == nullptr: on the trace's own stream, waited for) */
static int materialize_slots(Ctx *c, hipStream_t s) {
    if (c->slots_dirty <= 0) return PM_OK;
    const bool wait = s == nullptr;
    if (wait) s = c->stream;
    HIPCHK(c, hipStreamWaitEvent(s, c->dirty_event, 0));
    HIPCHK(c, launch_zero_invalid_slots(c->d_slots.as<pm_photon>(), c->d_scratch.as<uint32_t>(), c->slots_dirty,
                                        c->dirty_key_np, c->dirty_mpc, s));
    c->slots_dirty = 0;
    if (wait) HIPCHK(c, hipStreamSynchronize(s));
    return PM_OK;
}

/* the bound of a path's emitted weight for this call's light_source_index (LightSummary) */
double emission_bound(const Ctx *c, const pm_render_params *p) {
    return p->light_source_index == PM_ALL_LIGHTS ? c->lsum.emit_max_all : c->lsum.emit_max;
}

template <class T>
int upload(Ctx *c, DevBuf &b, const std::vector<T> &v) {
    HIPCHK(c, b.ensure(std::max<size_t>(v.size() * sizeof(T), 16)));
    if (!v.empty()) HIPCHK(c, hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return PM_OK;
}

int ensure_records(Ctx *c) {
    int64_t n = num_records(c);
    if (n <= 0) FAIL(c, PM_ERR_INVALID, "no eye samples (call pm_set_pinhole or pm_set_eye_rays)");
    HIPCHK(c, c->d_pos.ensure(n * sizeof(float4)));
    HIPCHK(c, c->d_nrm.ensure(n * sizeof(float4)));
    HIPCHK(c, c->d_state.ensure(n * sizeof(float4)));
    HIPCHK(c, c->d_n.ensure(n * sizeof(float)));
    HIPCHK(c, c->d_dl.ensure(n * sizeof(float4)));
    /* the albedo factors, only for a textured or physically specular scene; a new buffer starts as
     * all ones (records uploaded without an eye pass keep their flux as it is) */
    if (c->albedo() && !(c->d_rkd.p && (size_t)n * sizeof(float4) <= c->d_rkd.bytes)) {
        HIPCHK(c, c->d_rkd.ensure(n * sizeof(float4)));
        const std::vector<float4> ones((size_t)n, f4(1.f, 1.f, 1.f, 0.f));
        HIPCHK(c, hipMemcpy(c->d_rkd.p, ones.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice));
    }
    c->nrec = n;
    c->tiles.invalidate();
    c->grid_plan.invalidate();
    return PM_OK;
}

RecordsDev recs(Ctx *c) {
    RecordsDev R;
    R.pos = c->d_pos.as<float4>(); R.nrm = c->d_nrm.as<float4>(); R.state = c->d_state.as<float4>();
    R.n = c->d_n.as<float>(); R.dl = c->d_dl.as<float4>(); R.count = c->nrec;
    return R;
}

/* cells per axis of a box of width 2 r' (r' of radius2) on grid g: the tile
 * kernel's run count (GatherParams::span), clamped to its instances 2..5
 * (larger boxes scan per lane) */
int grid_span(const GridDesc &g, float radius2) {
    const double rq = sqrt((double)radius2) * 1.0001 + 1e-4;
    const double w = 2.0 * rq * (double)g.inv_cs * (1.0 + 1e-6);
    return std::max(2, std::min(5, (int)std::floor(w) + 2));
}

/* the largest alpha a deposit can carry: the emission, max_photon_count
 * Lambert weights and max_specular_depth lobe colours of the physical specular
 * model (spec_max is 1, and the factor exactly 1, without such a material) */
double flux_bound(Ctx *c, const pm_render_params *p) {
    return emission_bound(c, p) * std::pow(c->lsum.kd_max, (double)p->max_photon_count) *
           std::pow(c->lsum.spec_max, (double)std::max(p->max_specular_depth, 0));
}

GatherParams gather_params(Ctx *c, const pm_render_params *p) {
    GatherParams G{};
    G.R = recs(c);
    G.materials = c->S.materials;
    G.ppm_alpha = p->ppm_alpha;
    G.grid = c->grid;
    G.cell_start = c->d_cell_start.as<uint32_t>();
    G.ph_a = c->d_pha.as<float4>(); G.ph_b = c->d_phb.as<float4>();
    G.kd_nodes = c->d_kd.as<pm_photon>(); G.kd_count = c->kd_count;
    G.counters = c->d_counters.as<unsigned long long>();
    G.kernel = c->gather_kernel;
    G.kd_stack = c->kd_stack;
    G.error = reinterpret_cast<unsigned int *>(c->d_counters.as<unsigned long long>() + 16);
    G.fx_nonneg = c->lsum.scene_nonneg && c->slots_nonneg ? 1 : 0;
    G.span = grid_span(c->grid, c->grid_r2 > 0.f ? c->grid_r2 : p->initial_radius2);
    /* The cooperative scan of a tile's direct lanes costs the sum of their
     * photons / 64 steps, the per-lane scans the largest lane's photons but
     * one scattered line per lane and load. Scenes traversed from HBM (many
     * small primitives: C3's 1M-triangle soup) give incoherent tiles whose
     * lanes share no cells — the cooperative scan takes them all (same box:
     * C3 gather 0.458 -> 0.216 ms); LDS-sized scenes (the Cornell family)
     * give coherent direct lanes (a dense union's group, C5), which the
     * per-lane scans serve from L1, so only light waves (<= 8 steps) go
     * cooperative (C5: all 0.214 ms vs 0.170 bounded). */
    G.coop_steps = scene_mode(c->S) == MODE_GLOBAL ? 0xffffffu : 8u;
    if (c->view_active) { G.view_rank = c->d_vrank.as<uint32_t>(); G.view_list = c->d_vlist.as<uint32_t>(); }
    /* fixed-point scale 2^S: a single contribution is bounded by
     * alpha_max * Kd_max / pi with alpha_max = emission * Kd_max^mpc (Lambert
     * weight ~Kd, specular weight 1); x4 headroom; 2^40 per contribution
     * leaves 2^23 contributions per record before int64 overflow */
    double cmax = flux_bound(c, p) * (c->lsum.kd_max / M_PI) * 4.0;
    int S = (int)std::floor(std::log2(std::ldexp(1.0, 40) / std::max(cmax, 1e-30)));
    S = std::max(-60, std::min(60, S));
    G.fx_scale = (float)std::ldexp(1.0, S);
    G.fx_inv = std::ldexp(1.0, -S);
    return G;
}

/* the final pass over records [begin, begin + count) into out, one radiance
 * per record in record order (callers set raster / view for another layout) */
FinalParams final_params(Ctx *c, double emitted, int64_t begin, int64_t count, float *out) {
    FinalParams F{};
    F.R = recs(c);
    F.knn = c->rec_estimator == PM_ESTIMATOR_KNN; F.materials = c->S.materials;
    F.emitted = (float)emitted; /* gContext["emittingPhotons"]->setFloat((float)totalPhotons) */
    F.rec_begin = begin; F.rec_count = count; F.out = out; F.raster = 0; F.W = c->W;
    F.kd = c->albedo() ? c->d_rkd.as<float4>() : nullptr;
    return F;
}

/* (re)builds the active-record view from the current records; synchronizes to read its size */
int build_view(Ctx *c, hipStream_t s) {
    const int64_t n = c->nrec;
    HIPCHK(c, c->d_vflags.ensure((size_t)(n + 1) * 4));
    HIPCHK(c, c->d_vrank.ensure((size_t)(n + 1) * 4));
    HIPCHK(c, c->d_vlist.ensure((size_t)std::max<int64_t>(n, 1) * 4));
    HIPCHK(c, c->d_vsums.ensure(scan_scratch_words(n + 1) * 4));
    HIPCHK(c, launch_record_view(recs(c), c->d_vflags.as<uint32_t>(), c->d_vrank.as<uint32_t>(),
                                 c->d_vlist.as<uint32_t>(), c->d_vsums.as<uint32_t>(), s));
    uint32_t total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, c->d_vrank.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    c->n_view = total;
    return PM_OK;
}

/* number of records the range-based record calls address */
int64_t view_size(const Ctx *c) { return c->view_active ? c->n_view : c->nrec; }
const uint32_t *view_list(Ctx *c) { return c->view_active ? c->d_vlist.as<uint32_t>() : nullptr; }

/* applies a deferred pm_reset_records before a reader that is not a fused full gather */
int materialize_reset(Ctx *c, hipStream_t s) {
    if (!c->rec_fresh) return PM_OK;
    timer_begin(c, "reset", s);
    HIPCHK(c, launch_reset_records(recs(c), c->rec_fresh_r2, s));
    timer_end(c, "reset", s);
    c->rec_fresh = false;
    return PM_OK;
}

int check_params(Ctx *c, const pm_render_params *p) {
    if (!p) FAIL(c, PM_ERR_INVALID, "null params");
    if (!c->committed) FAIL(c, PM_ERR_INVALID, "scene not committed (call pm_commit)");
    if (p->max_photon_count < 1 || p->max_photon_count > 64) FAIL(c, PM_ERR_INVALID, "max_photon_count out of range");
    if (p->light_source_index == PM_ALL_LIGHTS) {
        if (!c->lsum.cdf_ok)
            FAIL(c, PM_ERR_INVALID, "PM_ALL_LIGHTS: the total selection weight of the scene's %zu lights is 0 or not "
                                    "finite (no light to pick)", c->hs.lights.size());
    } else if (p->light_source_index < 0 || p->light_source_index >= (int)c->hs.lights.size())
        FAIL(c, PM_ERR_INVALID, "light_source_index %d out of range (%zu lights; PM_ALL_LIGHTS = -1 for every light)",
             p->light_source_index, c->hs.lights.size());
    if (!(p->initial_radius2 > 0.f)) FAIL(c, PM_ERR_INVALID, "initial_radius2 must be > 0");
    if (p->estimator != PM_ESTIMATOR_PPM && p->estimator != PM_ESTIMATOR_KNN)
        FAIL(c, PM_ERR_INVALID, "unknown estimator %d", p->estimator);
    if (p->estimator == PM_ESTIMATOR_KNN) {
        if (p->knn_lookup < 1 || p->knn_lookup > PM_KNN_MAX)
            FAIL(c, PM_ERR_INVALID, "knn_lookup must be in [1, %d]", PM_KNN_MAX);
        if (p->gather_structure != PM_GATHER_GRID)
            FAIL(c, PM_ERR_INVALID, "the kNN estimator runs on the photon buckets (PM_GATHER_GRID)");
    }
    return PM_OK;
}

struct TmpBuf : DevBuf {
    ~TmpBuf() { release(); }
};

/* the scene blob with the BVH built on the device: boxes from the host's
 * parallel pass uploaded, gpu_bvh_build writes the 4-wide nodes and refs in
 * place, the triangle records (computed on the host in triangle-id order
 * while the device builds) are uploaded and permuted into storage order.
 * built = false: the caller runs the host build (the device tree exceeded a
 * limit the traversal has, or the build failed — reported on stderr) */
int commit_gpu_bvh(Ctx *c, const std::vector<BuildPrim> &prims, const BuildOptions &opt, SceneLayout &L, bool &built) {
    built = false;
    const HostScene &hs = c->hs;
    const int64_t nt = (int64_t)hs.tris.size();
    const auto t0 = std::chrono::steady_clock::now();
    auto ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    const int n = (int)prims.size();
    GpuBvhIn in{};
    in.n = n;
    in.radius = opt.ploc_radius;
    ploc_morton_frame(prims, in.frame_lo, in.frame_scale);
    std::vector<float> geo(TRI_GEO_FLOATS * (size_t)nt), shade(TRI_SHADE_FLOATS * (size_t)nt);
    std::vector<int> info(TRI_INFO_INTS * (size_t)nt);
    struct Joiner {
        std::thread t;
        ~Joiner() { if (t.joinable()) t.join(); }
    } records;
    records.t = std::thread([&] {
        parallel_for(nt, [&](int64_t k0, int64_t k1) {
            for (int64_t k = k0; k < k1; ++k) tri_record(hs, (uint32_t)k, &geo[TRI_GEO_FLOATS * k], &shade[TRI_SHADE_FLOATS * k], &info[TRI_INFO_INTS * k]);
        });
    });
    std::vector<float4> hb(2 * (size_t)n);
    parallel_for(n, [&](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            const BuildPrim &p = prims[i];
            hb[2 * i] = f4(p.lo[0], p.lo[1], p.lo[2], bits_f(p.ref));
            hb[2 * i + 1] = f4(p.hi[0], p.hi[1], p.hi[2], 0.f);
        }
    });
    TmpBuf d_box, d_tord, d_src;
    HIPCHK(c, d_box.ensure(hb.size() * sizeof(float4)));
    HIPCHK(c, hipMemcpy(d_box.p, hb.data(), hb.size() * sizeof(float4), hipMemcpyHostToDevice));
    in.box = d_box.as<float4>();
    /* the host assembly's layout; no binary tree (a placeholder), room
     * for the n - 1 nodes a 4-wide tree over n leaves can have. Never
     * LDS-resident: the LDS modes traverse the binary tree this path does not build */
    const std::vector<float4> norms = vertex_normals(hs);
    L = SceneLayout();
    count_sections(L, hs, n, nt);
    L.size[SEC_NODES] = NODE_PLACEHOLDER_BYTES;
    L.size[SEC_WNODES] = BVH4Q_NODE_BYTES * (size_t)(n - 1);
    plan_layout(L, true);
    HIPCHK(c, c->d_scene.ensure(L.bytes));
    char *base = c->d_scene.as<char>();
    HIPCHK(c, hipMemsetAsync(base + L.off[SEC_NODES], 0, L.size[SEC_NODES], c->stream));
    auto put = [&](SceneSection sec, const void *src) {
        return L.size[sec] ? hipMemcpyAsync(base + L.off[sec], src, L.size[sec], hipMemcpyHostToDevice, c->stream) : hipSuccess;
    };
    HIPCHK(c, put(SEC_NORMS, norms.data()));
    HIPCHK(c, put(SEC_DISKS, hs.disks.data()));
    HIPCHK(c, put(SEC_SPHERES, hs.spheres.data()));
    HIPCHK(c, put(SEC_MATS, hs.materials.data()));
    HIPCHK(c, put(SEC_LIGHTS, hs.lights.data()));
    HIPCHK(c, d_tord.ensure(sizeof(uint32_t) * (size_t)std::max<int64_t>(nt, 1)));
    GpuBvhOut out;
    out.wnodes = reinterpret_cast<uint4 *>(base + L.off[SEC_WNODES]);
    out.refs = reinterpret_cast<uint32_t *>(base + L.off[SEC_REFS]);
    out.tri_order = d_tord.as<uint32_t>();
    out.max_nodes = n - 1;
    const double t_up = ms();
    const hipError_t e = gpu_bvh_build(in, out, c->stream);
    const double t_build = ms();
    if (e != hipSuccess) {
        (void)hipGetLastError();
        fprintf(stderr, "pm_commit: device BVH build failed (%s); host build\n", hipGetErrorString(e));
        return PM_OK;
    }
    if (out.max_stack > BVH_STACK || out.n_tris != nt) {
        fprintf(stderr, "pm_commit: device BVH stack bound %d (limit %d), %lld triangles; host build\n", out.max_stack,
                BVH_STACK, (long long)out.n_tris);
        return PM_OK;
    }
    records.t.join();
    const double t_rec = ms();
    HIPCHK(c, d_src.ensure((TRI_GEO_BYTES + TRI_SHADE_BYTES + TRI_INFO_BYTES) * (size_t)std::max<int64_t>(nt, 1)));
    float4 *src_geo = d_src.as<float4>(), *src_shade = reinterpret_cast<float4 *>(d_src.as<char>() + TRI_GEO_BYTES * (size_t)nt);
    int4 *src_info = reinterpret_cast<int4 *>(d_src.as<char>() + (TRI_GEO_BYTES + TRI_SHADE_BYTES) * (size_t)nt);
    HIPCHK(c, hipMemcpyAsync(src_geo, geo.data(), geo.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(src_shade, shade.data(), shade.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(src_info, info.data(), info.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_tri_permute(d_tord.as<uint32_t>(), nt, src_geo, src_shade, src_info,
                                 reinterpret_cast<float4 *>(base + L.off[SEC_GEO]),
                                 reinterpret_cast<float4 *>(base + L.off[SEC_SHADE]),
                                 reinterpret_cast<uint32_t *>(base + L.off[SEC_TID]),
                                 reinterpret_cast<int4 *>(base + L.off[SEC_INFO]),
                                 c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (opt.times)
        fprintf(stderr, "pm_commit: device build: boxes up %.1f ms, PLOC + collapse %.1f ms (%d rounds, %lld nodes, depth %d, "
                        "stack %d), records %.1f ms, permute %.1f ms\n", t_up, t_build - t_up, out.rounds,
                (long long)out.nodes, out.depth, out.max_stack, t_rec, ms());
    c->bvh_depth = out.depth;
    c->bvh4_nodes = out.nodes;
    c->bvh4_depth = out.depth;
    L.n_nodes = out.nodes;
    L.size[SEC_WNODES] = BVH4Q_NODE_BYTES * (size_t)out.nodes; /* the nodes in use */
    L.wide = 2;
    L.wide_stack = out.max_stack;
    built = true;
    return PM_OK;
}

} // namespace

extern "C" {

const char *pm_version(void) { return "pmhip 0.1 (gfx950)"; }

void pm_default_params(pm_render_params *p) {
    std::memset(p, 0, sizeof(*p));
    p->scene_epsilon = 0.1f;
    p->initial_radius2 = 4.0f;
    p->ppm_alpha = 0.7f;
    p->max_photon_count = 4;
    p->paths_per_pass = 512 * 512;
    p->passes = 1;
    p->light_source_index = 0;
    p->max_specular_depth = 10;
    p->rng_seed = 777u;
    p->light_rng_seed = 2047u;
    p->gather_structure = PM_GATHER_GRID;
    p->estimator = PM_ESTIMATOR_PPM;
    p->knn_lookup = 50; /* pbrt-v2 PhotonIntegrator "nused" */
}

int pm_create(void **out, const pm_config *cfg) {
    if (!out) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "null output pointer");
    *out = nullptr;
    if (cfg && cfg->n_devices > 0) { /* multi-device context (Group) */
        if (!cfg->devices || cfg->n_devices > 64) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "bad device list");
        Ctx *gc = new Ctx();
        gc->group = new Group();
        Group &G = *gc->group;
        bool distinct = true;
        for (int i = 0; i < cfg->n_devices; ++i) {
            pm_config one{};
            one.device = cfg->devices[i];
            void *sub = nullptr;
            if (pm_create(&sub, &one) != PM_OK) {
                const std::string e = g_last_error;
                pm_destroy(gc);
                FAIL((Ctx *)nullptr, PM_ERR_HIP, "device %d: %s", cfg->devices[i], e.c_str());
            }
            for (int d : G.devs) distinct = distinct && d != one.device;
            /* a device's trace covers one shard of the all-gathered slots, so
             * counts fused into it would never match the build: not made */
            if (cfg->n_devices > 1) ((Ctx *)sub)->fuse_ok = false;
            G.subs.push_back((Ctx *)sub);
            G.devs.push_back(one.device);
            hipEvent_t ev = nullptr;
            (void)hipSetDevice(one.device);
            if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
                pm_destroy(gc);
                FAIL((Ctx *)nullptr, PM_ERR_HIP, "hipEventCreate on device %d", one.device);
            }
            G.ev.push_back(ev);
        }
        gc->device = G.devs[0];
        const char *re = getenv("PM_GROUP_RCCL"); /* 0: peer copies even on distinct devices */
        if (distinct && !(re && atoi(re) == 0)) {
            G.comms.resize(G.devs.size());
            const ncclResult_t r = ncclCommInitAll(G.comms.data(), (int)G.devs.size(), G.devs.data());
            if (r != ncclSuccess) {
                G.comms.clear();
                pm_destroy(gc);
                FAIL((Ctx *)nullptr, PM_ERR_HIP, "ncclCommInitAll over %d devices: %s", cfg->n_devices, ncclGetErrorString(r));
            }
        } else if (distinct) {
            for (int a : G.devs)
                for (int b : G.devs)
                    if (a != b) { (void)hipSetDevice(a); (void)hipDeviceEnablePeerAccess(b, 0); }
            (void)hipGetLastError(); /* already-enabled peers are not errors here */
        }
        *out = gc;
        return PM_OK;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        FAIL((Ctx *)nullptr, PM_ERR_HIP, "no HIP device available (%s)", hipGetErrorString(e));
    int dev = cfg ? cfg->device : 0;
    if (dev < 0 || dev >= ndev) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "device %d out of range (%d devices)", dev, ndev);
    Ctx *c = new Ctx();
    c->device = dev;
    if (const char *e = getenv("PM_GATHER_KERNEL"))
        c->gather_kernel = !strcmp(e, "lane") ? PM_GK_LANE : PM_GK_TILE;
    if (const char *e = getenv("PM_KNN_SS")) c->knn_ss = atoi(e) != 0;
    if (const char *e = getenv("PM_CELL_SPAN")) c->cell_span = std::max(2, std::min(5, atoi(e)));
    if (const char *e = getenv("PM_TILE_SORT")) c->tiles.sort = atoi(e) != 0;
    if (const char *e = getenv("PM_LAZY_ZERO")) c->lazy_zero = atoi(e) != 0;
    if (const char *e = getenv("PM_GRID_QUANTILE")) c->grid_plan.quantile = atof(e);
    if (const char *e = getenv("PM_TRACE_HOLD")) c->trace_hold = atoi(e) != 0;
    if (const char *e = getenv("PM_TRACE_POOL")) c->trace_pool = atoi(e) != 0;
    if (const char *e = getenv("PM_POOL_STACK")) c->pool_stack = std::max(0, atoi(e));
    if (const char *e = getenv("PM_KD_STACK")) c->kd_stack = std::max(1, std::min(KD_STACK, atoi(e)));
    if (const char *e = getenv("PM_STAGE_TIMERS")) if (atoi(e) == 0) c->timed_stages.clear();
    (void)hipSetDevice(dev);
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        FAIL((Ctx *)nullptr, PM_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    e = c->d_counters.ensure(17 * sizeof(unsigned long long)); /* [gather x4][trace x4][trace profile x8][gather error] */
    if (e != hipSuccess) {
        delete c;
        FAIL((Ctx *)nullptr, PM_ERR_HIP, "hipMalloc: %s", hipGetErrorString(e));
    }
    *out = c;
    return PM_OK;
}

void pm_destroy(void *ptr) {
    Ctx *c = (Ctx *)ptr;
    if (!c) return;
    if (Group *g = c->group) {
        for (ncclComm_t cm : g->comms) (void)ncclCommDestroy(cm);
        for (size_t i = 0; i < g->ev.size(); ++i) { (void)hipSetDevice(g->devs[i]); (void)hipEventDestroy(g->ev[i]); }
        for (Ctx *sub : g->subs) pm_destroy(sub);
        delete g;
        delete c;
        return;
    }
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto &kv : c->timers)
        for (Timer &t : kv.second.ev) {
            (void)hipEventDestroy(t.a);
            (void)hipEventDestroy(t.b);
        }
    DevBuf *bufs[] = {&c->d_scene, &c->d_rays, &c->d_rand2d, &c->d_pos, &c->d_nrm, &c->d_state, &c->d_n,
                      &c->d_dl, &c->d_slots, &c->d_count, &c->d_scratch, &c->d_vflags, &c->d_vrank, &c->d_vlist, &c->d_vsums,
                      &c->d_cell_start, &c->d_pha, &c->d_phb, &c->d_knnpk, &c->d_knnovf, &c->d_tile_times,
                      &c->d_kd, &c->d_out, &c->d_counters, &c->d_hist, &c->d_spill, &c->d_light_tris, &c->d_light_cdf, &c->d_film_table, &c->d_img,
                      &c->d_tex_recs, &c->d_texels, &c->d_mat_tex, &c->d_tri_uv, &c->d_rkd, &c->d_mat_spec};
    for (DevBuf *b : bufs) b->release();
    c->tiles.release();
    if (c->hist_event) (void)hipEventDestroy(c->hist_event);
    if (c->dirty_event) (void)hipEventDestroy(c->dirty_event);
    if (c->h_hist) (void)hipHostFree(c->h_hist);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *pm_last_error(void *ptr) {
    Ctx *c = (Ctx *)ptr;
    return c ? c->err.c_str() : g_last_error.c_str();
}

int64_t pm_kdtree_build_host(const pm_photon *slots, int64_t nslots, pm_photon *nodes_out) {
    if (!slots || !nodes_out || nslots < 0) return -1;
    std::vector<pm_photon> nodes;
    int64_t m = build_kdtree_pbrt(slots, nslots, nodes);
    if (m > 0) std::memcpy(nodes_out, nodes.data(), (size_t)m * sizeof(pm_photon));
    return m;
}

int pm_halton_permutation(uint32_t seed, uint32_t out[28]) {
    if (!out) return PM_ERR_INVALID;
    halton_perm(seed, out);
    return PM_OK;
}

int pm_light_selection_cdf(const int *types, const float *le_rgb, const float *areas, int n, float *cdf_out) {
    std::string err;
    const int rc = light_selection_cdf(types, le_rgb, areas, n, cdf_out, err);
    if (rc) FAIL((Ctx *)nullptr, rc, "%s", err.c_str());
    return PM_OK;
}

/* ------------------------------------------------------------------ scene */
int pm_add_material(void *ptr, int type, const float rgb[3], int *out_id) {
    GROUP_FWD(ptr, pm_add_material(sub, type, rgb, out_id));
    GETCTX(ptr);
    if (type != PM_MATTE && type != PM_MIRROR && type != PM_GLASS) FAIL(c, PM_ERR_INVALID, "bad material type %d", type);
    float r = rgb ? rgb[0] : 0.f, g = rgb ? rgb[1] : 0.f, b = rgb ? rgb[2] : 0.f;
    c->hs.materials.push_back(f4(r, g, b, ibits(type)));
    if (out_id) *out_id = (int)c->hs.materials.size() - 1;
    c->committed = false;
    return PM_OK;
}

/* textures: the arguments are checked, and the records built, in the
 * host-only unit (pm_scene.cpp); what needs no context is checked before the
 * context is looked at */
int pm_add_texture_image(void *ptr, const float *rgb, int w, int h, int wrap, const float mapping[4], const float scale[3],
                         int *out_tex) {
    std::string err;
    if (!out_tex) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "pm_add_texture_image: null pointer");
    if (int rc = check_texture_image(rgb, w, h, wrap, mapping, scale, err)) FAIL((Ctx *)nullptr, rc, "%s", err.c_str());
    GROUP_FWD(ptr, pm_add_texture_image(sub, rgb, w, h, wrap, mapping, scale, out_tex));
    GETCTX(ptr);
    if (int rc = add_texture_image(c->hs, rgb, w, h, wrap, mapping, scale, out_tex, err)) FAIL(c, rc, "%s", err.c_str());
    c->committed = false;
    return PM_OK;
}

int pm_add_texture_checker(void *ptr, const float mapping[4], int tex1, const float rgb1[3], int tex2, const float rgb2[3],
                           int *out_tex) {
    std::string err;
    if (!out_tex) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "pm_add_texture_checker: null pointer");
    if (int rc = check_texture_operands("pm_add_texture_checker", mapping, true, tex1, rgb1, tex2, rgb2, err))
        FAIL((Ctx *)nullptr, rc, "%s", err.c_str());
    GROUP_FWD(ptr, pm_add_texture_checker(sub, mapping, tex1, rgb1, tex2, rgb2, out_tex));
    GETCTX(ptr);
    if (int rc = add_texture_checker(c->hs, mapping, tex1, rgb1, tex2, rgb2, out_tex, err)) FAIL(c, rc, "%s", err.c_str());
    c->committed = false;
    return PM_OK;
}

int pm_add_texture_scale(void *ptr, int tex1, const float rgb1[3], int tex2, const float rgb2[3], int *out_tex) {
    std::string err;
    if (!out_tex) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "pm_add_texture_scale: null pointer");
    if (int rc = check_texture_operands("pm_add_texture_scale", nullptr, false, tex1, rgb1, tex2, rgb2, err))
        FAIL((Ctx *)nullptr, rc, "%s", err.c_str());
    GROUP_FWD(ptr, pm_add_texture_scale(sub, tex1, rgb1, tex2, rgb2, out_tex));
    GETCTX(ptr);
    if (int rc = add_texture_scale(c->hs, tex1, rgb1, tex2, rgb2, out_tex, err)) FAIL(c, rc, "%s", err.c_str());
    c->committed = false;
    return PM_OK;
}

int pm_add_material_textured(void *ptr, int type, int kd_tex, int *out_id) {
    std::string err;
    if (int rc = check_material_textured(type, err)) FAIL((Ctx *)nullptr, rc, "%s", err.c_str());
    if (!out_id) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "pm_add_material_textured: null pointer");
    GROUP_FWD(ptr, pm_add_material_textured(sub, type, kd_tex, out_id));
    GETCTX(ptr);
    if (int rc = add_material_textured(c->hs, type, kd_tex, out_id, err)) FAIL(c, rc, "%s", err.c_str());
    c->committed = false;
    return PM_OK;
}

int pm_add_material_specular(void *ptr, int type, const float kr[3], const float kt[3], float index, int *out_id) {
    std::string err;
    if (int rc = check_material_specular(type, kr, kt, index, err)) FAIL((Ctx *)nullptr, rc, "%s", err.c_str());
    if (!out_id) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "pm_add_material_specular: null pointer");
    GROUP_FWD(ptr, pm_add_material_specular(sub, type, kr, kt, index, out_id));
    GETCTX(ptr);
    if (int rc = add_material_specular(c->hs, type, kr, kt, index, out_id, err)) FAIL(c, rc, "%s", err.c_str());
    c->committed = false;
    return PM_OK;
}

int pm_add_trimesh(void *ptr, const float *P, int nverts, const int *idx, int ntris, const float *N, const float *uv,
                   int material, int light) {
    GROUP_FWD(ptr, pm_add_trimesh(sub, P, nverts, idx, ntris, N, uv, material, light));
    GETCTX(ptr);
    if (!P || !idx || nverts <= 0 || ntris <= 0) FAIL(c, PM_ERR_INVALID, "empty or null mesh");
    if (material < 0 || material >= (int)c->hs.materials.size()) FAIL(c, PM_ERR_INVALID, "bad material id %d", material);
    for (int64_t i = 0; i < 3 * (int64_t)ntris; ++i)
        if (idx[i] < 0 || idx[i] >= nverts) FAIL(c, PM_ERR_INVALID, "vertex index %d out of range", idx[i]);
    if (c->hs.next_tri_id + ntris >= ((int64_t)1 << 31)) FAIL(c, PM_ERR_INVALID, "too many triangles (global ids reach 2^31)");
    int64_t base = (int64_t)c->hs.P.size() / 3;
    c->hs.P.insert(c->hs.P.end(), P, P + 3 * (size_t)nverts);
    if (N) c->hs.N.insert(c->hs.N.end(), N, N + 3 * (size_t)nverts);
    else c->hs.N.insert(c->hs.N.end(), 3 * (size_t)nverts, 0.f);
    if (uv) c->hs.UV.insert(c->hs.UV.end(), uv, uv + 2 * (size_t)nverts);
    else c->hs.UV.insert(c->hs.UV.end(), 2 * (size_t)nverts, 0.f);
    int mid = (int)c->hs.meshes.size();
    c->hs.meshes.push_back(HMesh{material, light, N != nullptr, uv != nullptr});
    for (int t = 0; t < ntris; ++t)
        c->hs.tris.push_back(HTri{{(int)(base + idx[3 * t]), (int)(base + idx[3 * t + 1]), (int)(base + idx[3 * t + 2])}, mid,
                               (uint32_t)c->hs.next_tri_id++});
    c->committed = false;
    return PM_OK;
}

int pm_add_object_mesh(void *ptr, const float *P, int nverts, const int *idx, int ntris, const float *N,
                       const float *uv, int material, int light, int *out_object) {
    GROUP_FWD(ptr, pm_add_object_mesh(sub, P, nverts, idx, ntris, N, uv, material, light, out_object));
    GETCTX(ptr);
    if (!P || !idx || nverts <= 0 || ntris <= 0) FAIL(c, PM_ERR_INVALID, "empty or null object mesh");
    if (material < 0 || material >= (int)c->hs.materials.size()) FAIL(c, PM_ERR_INVALID, "bad material id %d", material);
    for (int64_t i = 0; i < 3 * (int64_t)ntris; ++i)
        if (idx[i] < 0 || idx[i] >= nverts) FAIL(c, PM_ERR_INVALID, "vertex index %d out of range", idx[i]);
    HObj o;
    o.P.assign(P, P + 3 * (size_t)nverts);
    if (N) o.N.assign(N, N + 3 * (size_t)nverts);
    if (uv) o.UV.assign(uv, uv + 2 * (size_t)nverts);
    o.idx.assign(idx, idx + 3 * (size_t)ntris);
    o.material = material; o.light = light; o.has_n = N != nullptr; o.has_uv = uv != nullptr;
    c->hs.objs.push_back(std::move(o));
    if (out_object) *out_object = (int)c->hs.objs.size() - 1;
    c->committed = false;
    return PM_OK;
}

int pm_add_mesh_instance(void *ptr, int object, const float o2w[16], const float w2o[16]) {
    GROUP_FWD(ptr, pm_add_mesh_instance(sub, object, o2w, w2o));
    GETCTX(ptr);
    if (object < 0 || object >= (int)c->hs.objs.size()) FAIL(c, PM_ERR_INVALID, "bad object id %d", object);
    if (!o2w || !w2o) FAIL(c, PM_ERR_INVALID, "null instance transform");
    if (o2w[12] != 0.f || o2w[13] != 0.f || o2w[14] != 0.f || o2w[15] != 1.f)
        FAIL(c, PM_ERR_INVALID, "instance transform is not affine (flatten it with pm_add_trimesh)");
    /* every instance takes global ids for all of its triangles (as the
     * flattened scene would): heavy instancing must not wrap them */
    const int64_t n_obj_tris = (int64_t)(c->hs.objs[object].idx.size() / 3);
    if (c->hs.next_tri_id + n_obj_tris >= ((int64_t)1 << 31))
        FAIL(c, PM_ERR_INVALID, "too many instanced triangles (global ids reach 2^31)");
    HInst in;
    in.obj = object;
    std::memcpy(in.m, o2w, sizeof in.m);
    std::memcpy(in.minv, w2o, sizeof in.minv);
    in.gid_base = (uint32_t)c->hs.next_tri_id;
    c->hs.next_tri_id += n_obj_tris;
    c->hs.insts.push_back(in);
    c->committed = false;
    return PM_OK;
}

int pm_add_sphere(void *ptr, float radius, const float o2w[16], const float w2o[16], int material, int light) {
    GROUP_FWD(ptr, pm_add_sphere(sub, radius, o2w, w2o, material, light));
    GETCTX(ptr);
    if (!o2w || !w2o || !(radius > 0.f)) FAIL(c, PM_ERR_INVALID, "bad sphere");
    if (material < 0 || material >= (int)c->hs.materials.size()) FAIL(c, PM_ERR_INVALID, "bad material id %d", material);
    c->hs.spheres.push_back(f4(w2o[0], w2o[1], w2o[2], w2o[3]));
    c->hs.spheres.push_back(f4(w2o[4], w2o[5], w2o[6], w2o[7]));
    c->hs.spheres.push_back(f4(w2o[8], w2o[9], w2o[10], w2o[11]));
    c->hs.spheres.push_back(f4(radius, ibits(material), ibits(light), ibits(0)));
    c->hs.sphere_o2w.insert(c->hs.sphere_o2w.end(), o2w, o2w + 16);
    c->committed = false;
    return PM_OK;
}

/* derived uniforms as cudadisk.cpp:24-43 computes them */
int pm_add_disk(void *ptr, const float o[3], const float x[3], const float y[3], const float z[3], float inner,
                float phimax, int material, int light) {
    GROUP_FWD(ptr, pm_add_disk(sub, o, x, y, z, inner, phimax, material, light));
    GETCTX(ptr);
    if (!o || !x || !y || !z) FAIL(c, PM_ERR_INVALID, "null disk vector");
    if (material < 0 || material >= (int)c->hs.materials.size()) FAIL(c, PM_ERR_INVALID, "bad material id %d", material);
    float inv_rx2 = 1.f / (x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    float inv_ry2 = 1.f / (y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
    float moffset = o[0] * z[0] + o[1] * z[1] + o[2] * z[2];
    c->hs.disks.push_back(f4(o[0], o[1], o[2], inner));
    c->hs.disks.push_back(f4(x[0], x[1], x[2], phimax));
    c->hs.disks.push_back(f4(y[0], y[1], y[2], moffset));
    c->hs.disks.push_back(f4(z[0], z[1], z[2], inv_rx2));
    c->hs.disks.push_back(f4(inv_ry2, ibits(material), ibits(light), ibits(0)));
    c->committed = false;
    return PM_OK;
}

int pm_add_light_point(void *ptr, const float pos[3], const float I[3]) {
    GROUP_FWD(ptr, pm_add_light_point(sub, pos, I));
    GETCTX(ptr);
    if (!pos || !I) FAIL(c, PM_ERR_INVALID, "null point light");
    LightDev L{};
    L.o_type = f4(pos[0], pos[1], pos[2], ibits(PM_LIGHT_POINT));
    L.p1_ns = f4(0, 0, 0, ibits(1)); /* nSample = 1, cudalight.cpp:22 */
    L.p2_r2d = f4(0, 0, 0, ibits(0));
    L.n_area = f4(0, 0, 0, 0);
    L.le = f4(I[0], I[1], I[2], 0);
    c->hs.lights.push_back(L);
    c->committed = false;
    return PM_OK;
}

int pm_add_light_disk(void *ptr, const float o[3], const float p1[3], const float p2[3], const float n[3],
                      const float Le[3], float area, int nsamples) {
    GROUP_FWD(ptr, pm_add_light_disk(sub, o, p1, p2, n, Le, area, nsamples));
    GETCTX(ptr);
    if (!o || !p1 || !p2 || !n || !Le) FAIL(c, PM_ERR_INVALID, "null disk light vector");
    int ns = std::max(1, nsamples);
    LightDev L{};
    L.o_type = f4(o[0], o[1], o[2], ibits(PM_LIGHT_AREA_DISK));
    L.p1_ns = f4(p1[0], p1[1], p1[2], ibits(ns));
    L.p2_r2d = f4(p2[0], p2[1], p2[2], ibits(c->rand2d_total)); /* CudaSample::Add2D offset */
    L.n_area = f4(n[0], n[1], n[2], area);
    L.le = f4(Le[0], Le[1], Le[2], 0);
    c->rand2d_total += ns;
    c->hs.lights.push_back(L);
    c->committed = false;
    return PM_OK;
}

/* the emission table of a mesh light, as pm_api.h states it (tests restate it) */
int pm_add_light_mesh(void *ptr, const float *P, int nverts, const int *idx, int ntris, int reverse,
                      const float Le[3], int nsamples, int *out_light) {
    GROUP_FWD(ptr, pm_add_light_mesh(sub, P, nverts, idx, ntris, reverse, Le, nsamples, out_light));
    GETCTX(ptr);
    if (!P || !idx || !Le || !out_light) FAIL(c, PM_ERR_INVALID, "null mesh light argument");
    if (nverts <= 0 || ntris <= 0) FAIL(c, PM_ERR_INVALID, "empty mesh light");
    for (int64_t i = 0; i < 3 * (int64_t)ntris; ++i)
        if (idx[i] < 0 || idx[i] >= nverts) FAIL(c, PM_ERR_INVALID, "vertex index %d out of range", idx[i]);
    if (c->hs.light_tris.size() + (size_t)ntris >= ((size_t)1 << 31)) FAIL(c, PM_ERR_INVALID, "too many emitting triangles");
    std::vector<LightTri> tris((size_t)ntris);
    std::vector<double> sum((size_t)ntris);
    double total = 0.0;
    for (int t = 0; t < ntris; ++t) {
        const float *p0 = P + 3 * (size_t)idx[3 * t], *p1 = P + 3 * (size_t)idx[3 * t + 1], *p2 = P + 3 * (size_t)idx[3 * t + 2];
        const double a[3] = {(double)p1[0] - p0[0], (double)p1[1] - p0[1], (double)p1[2] - p0[2]};
        const double b[3] = {(double)p2[0] - p0[0], (double)p2[1] - p0[1], (double)p2[2] - p0[2]};
        const double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        total += 0.5 * len;
        sum[t] = total;
        /* a zero-area triangle is never sampled: its normal is left zero */
        const double inv = len > 0.0 ? (reverse ? -1.0 : 1.0) / len : 0.0;
        LightTri &T = tris[t];
        T.p0_cdf = f4(p0[0], p0[1], p0[2], 0.f);
        T.e1 = f4(p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2], 0.f);
        T.e2 = f4(p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2], 0.f);
        T.n = f4((float)(n[0] * inv), (float)(n[1] * inv), (float)(n[2] * inv), 0.f);
    }
    if (!(total > 0.0) || !std::isfinite(total) || !std::isfinite((float)total))
        FAIL(c, PM_ERR_INVALID, "mesh light area %g is zero or not finite", total);
    for (int t = 0; t < ntris; ++t) tris[t].p0_cdf.w = (float)(sum[t] / total);
    tris[ntris - 1].p0_cdf.w = 1.0f;
    const int ns = std::max(1, nsamples);
    LightDev L{};
    L.o_type = f4(ibits((int)c->hs.light_tris.size()), ibits(ntris), ibits(reverse ? 1 : 0), ibits(PM_LIGHT_AREA_MESH));
    L.p1_ns = f4(0, 0, 0, ibits(ns));
    L.p2_r2d = f4(0, 0, 0, ibits(c->rand2d_total)); /* CudaSample::Add2D offset, as the disk light */
    L.n_area = f4(0, 0, 0, (float)total);
    L.le = f4(Le[0], Le[1], Le[2], 0);
    c->rand2d_total += ns;
    c->hs.light_tris.insert(c->hs.light_tris.end(), tris.begin(), tris.end());
    c->hs.lights.push_back(L);
    *out_light = (int)c->hs.lights.size() - 1;
    c->committed = false;
    return PM_OK;
}

/* the record is made, and the parameters checked, in the host-only unit
 * (pm_scene.cpp), before the context is looked at */
int pm_add_light_distant(void *ptr, const float to_light[3], const float Lrgb[3], int *out_light) {
    LightDev L{};
    std::string err;
    if (!out_light) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "pm_add_light_distant: null pointer");
    if (int rc = make_distant_light(to_light, Lrgb, L, err)) FAIL((Ctx *)nullptr, rc, "%s", err.c_str());
    GROUP_FWD(ptr, pm_add_light_distant(sub, to_light, Lrgb, out_light));
    GETCTX(ptr);
    c->hs.lights.push_back(L);
    *out_light = (int)c->hs.lights.size() - 1;
    c->committed = false;
    return PM_OK;
}

int pm_set_pinhole(void *ptr, const float eye[3], const float fwd[3], const float right[3], const float up[3], int W,
                   int H) {
    GROUP_FWD(ptr, pm_set_pinhole(sub, eye, fwd, right, up, W, H));
    GETCTX(ptr);
    if (W <= 0 || H <= 0 || !eye || !fwd || !right || !up) FAIL(c, PM_ERR_INVALID, "bad pinhole camera");
    for (int a = 0; a < 3; ++a)
        if (!(fabsf(eye[a]) <= PM_MAX_RAY_ORIGIN) || !std::isfinite(fwd[a]) || !std::isfinite(right[a]) || !std::isfinite(up[a]))
            FAIL(c, PM_ERR_INVALID, "pinhole camera: eye beyond 2^20 or a non-finite vector");
    c->pinhole = 1; c->W = W; c->H = H; c->camera = 0;
    std::memcpy(c->eye, eye, 12); std::memcpy(c->fwd, fwd, 12);
    std::memcpy(c->right, right, 12); std::memcpy(c->up, up, 12);
    return PM_OK;
}

int pm_set_eye_rays(void *ptr, const float *rays, int64_t nrays, const float *rand2d, int n2d) {
    GROUP_FWD(ptr, pm_set_eye_rays(sub, rays, nrays, rand2d, n2d));
    GETCTX(ptr);
    if (!rays || nrays <= 0) FAIL(c, PM_ERR_INVALID, "no rays");
    /* the traversal modes agree bit for bit for finite rays with |o| <= 2^20 (pm_device.h box_near) */
    for (int64_t i = 0; i < nrays; ++i)
        for (int a = 0; a < 3; ++a)
            if (!(fabsf(rays[6 * i + a]) <= PM_MAX_RAY_ORIGIN) || !std::isfinite(rays[6 * i + 3 + a]))
                FAIL(c, PM_ERR_INVALID, "ray %lld: origin beyond 2^20 or a non-finite component", (long long)i);
    c->pinhole = 0; c->camera = 0;
    c->nrays = nrays;
    c->rays.assign(rays, rays + 6 * nrays);
    c->n2d = (rand2d && n2d > 0) ? n2d : 0;
    if (c->n2d) c->rand2d.assign(rand2d, rand2d + (size_t)2 * n2d * nrays);
    else c->rand2d.clear();
    HIPCHK(c, c->d_rays.ensure(c->rays.size() * sizeof(float)));
    HIPCHK(c, hipMemcpy(c->d_rays.p, c->rays.data(), c->rays.size() * sizeof(float), hipMemcpyHostToDevice));
    if (c->n2d) {
        HIPCHK(c, c->d_rand2d.ensure(c->rand2d.size() * sizeof(float)));
        HIPCHK(c, hipMemcpy(c->d_rand2d.p, c->rand2d.data(), c->rand2d.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return PM_OK;
}

/* ---- camera + film (pm_api.h pm_set_camera) ------------------------------ */
static bool real_filter(const pm_filter &f) { return f.type != PM_FILTER_NONE; }

int pm_film_filter_table(const pm_filter *f, float out[PM_FILM_TABLE * PM_FILM_TABLE]) {
    if (!f || !out) { g_last_error = "pm_film_filter_table: null pointer"; return PM_ERR_INVALID; }
    if (f->type < PM_FILTER_BOX || f->type > PM_FILTER_MITCHELL || !(f->xwidth > 0.f && f->xwidth <= 4.f) ||
        !(f->ywidth > 0.f && f->ywidth <= 4.f)) {
        g_last_error = "pm_film_filter_table: unknown filter type or a width outside (0, 4]";
        return PM_ERR_INVALID;
    }
    const double xw = f->xwidth, yw = f->ywidth, a = f->a, b = f->b;
    auto gauss = [&](double t, double w) { return std::max(0.0, std::exp(-a * t * t) - std::exp(-a * w * w)); };
    auto mitchell = [&](double x) { /* pbrt-v2 MitchellFilter::Mitchell1D, B = a, C = b */
        const double t = std::fabs(2.0 * x);
        if (t > 1.0)
            return ((-a - 6 * b) * t * t * t + (6 * a + 30 * b) * t * t + (-12 * a - 48 * b) * t + (8 * a + 24 * b)) / 6.0;
        return ((12 - 9 * a - 6 * b) * t * t * t + (-18 + 12 * a + 6 * b) * t * t + (6 - 2 * a)) / 6.0;
    };
    for (int j = 0; j < PM_FILM_TABLE; ++j)
        for (int i = 0; i < PM_FILM_TABLE; ++i) {
            const double x = (i + 0.5) / PM_FILM_TABLE * xw, y = (j + 0.5) / PM_FILM_TABLE * yw;
            double v = 1.0;
            switch (f->type) {
            case PM_FILTER_TRIANGLE: v = std::max(0.0, xw - std::fabs(x)) * std::max(0.0, yw - std::fabs(y)); break;
            case PM_FILTER_GAUSSIAN: v = gauss(x, xw) * gauss(y, yw); break;
            case PM_FILTER_MITCHELL: v = mitchell(x / xw) * mitchell(y / yw); break;
            default: break;
            }
            out[j * PM_FILM_TABLE + i] = (float)v;
        }
    return PM_OK;
}

int pm_set_camera(void *ptr, const pm_camera *cam) {
    GROUP_FWD(ptr, pm_set_camera(sub, cam));
    GETCTX(ptr);
    if (!cam) FAIL(c, PM_ERR_INVALID, "null camera");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(cam->eye[a]) || !std::isfinite(cam->fwd[a]) || !std::isfinite(cam->right[a]) ||
            !std::isfinite(cam->up[a]))
            FAIL(c, PM_ERR_INVALID, "camera: a non-finite vector");
    if (cam->width <= 0 || cam->height <= 0) FAIL(c, PM_ERR_INVALID, "camera: bad image size");
    if (cam->xsamples < 1 || cam->xsamples > 8 || cam->ysamples < 1 || cam->ysamples > 8)
        FAIL(c, PM_ERR_INVALID, "camera: %d x %d samples per pixel (1..8 each)", cam->xsamples, cam->ysamples);
    const int64_t WS = (int64_t)cam->width * cam->xsamples, HS = (int64_t)cam->height * cam->ysamples;
    if (WS >= (1ll << 31) || HS >= (1ll << 31) || WS * HS >= (1ll << 31))
        FAIL(c, PM_ERR_INVALID, "camera: %lld x %lld samples (2^31 or more)", (long long)WS, (long long)HS);
    if (!(cam->lens_radius >= 0.f) || !std::isfinite(cam->lens_radius))
        FAIL(c, PM_ERR_INVALID, "camera: lens_radius must be >= 0");
    if (cam->lens_radius > 0.f && !(cam->focal_distance > 0.f && std::isfinite(cam->focal_distance)))
        FAIL(c, PM_ERR_INVALID, "camera: a lens needs a focal_distance > 0");
    for (int a = 0; a < 3; ++a)
        if (!(fabsf(cam->eye[a]) + cam->lens_radius <= PM_MAX_RAY_ORIGIN))
            FAIL(c, PM_ERR_INVALID, "camera: eye + lens_radius beyond 2^20");
    const pm_filter &f = cam->filter;
    if (f.type < PM_FILTER_NONE || f.type > PM_FILTER_MITCHELL) FAIL(c, PM_ERR_INVALID, "camera: unknown filter type %d", f.type);
    float table[PM_FILM_TABLE * PM_FILM_TABLE];
    if (real_filter(f)) {
        /* film positions are fp32 pixel coordinates: beyond 2^20 samples per
         * axis they no longer resolve a stratum (and k_film's halo margin,
         * pm_film.hip film_halo, is sized for this bound) */
        if (WS > (1 << 20) || HS > (1 << 20))
            FAIL(c, PM_ERR_INVALID, "camera: a filmed raster of %lld x %lld samples (2^20 per axis at most)", (long long)WS, (long long)HS);
        if (!(f.xwidth > 0.f && f.xwidth <= 4.f) || !(f.ywidth > 0.f && f.ywidth <= 4.f))
            FAIL(c, PM_ERR_INVALID, "camera: filter width (%g, %g) outside (0, 4]", f.xwidth, f.ywidth);
        if (pm_film_filter_table(&f, table)) FAIL(c, PM_ERR_INVALID, "camera: bad filter");
        HIPCHK(c, c->d_film_table.ensure(sizeof(table)));
        HIPCHK(c, hipMemcpy(c->d_film_table.p, table, sizeof(table), hipMemcpyHostToDevice));
    }
    c->cam = *cam;
    c->camera = 1; c->pinhole = 1; c->W = (int)WS; c->H = (int)HS;
    std::memcpy(c->eye, cam->eye, 12); std::memcpy(c->fwd, cam->fwd, 12);
    std::memcpy(c->right, cam->right, 12); std::memcpy(c->up, cam->up, 12);
    return PM_OK;
}

/* the eye kernels' camera block (all of it the pinhole's when no camera is set) */
static void eye_camera(const Ctx *c, EyeParams &E) {
    E.pinhole = c->pinhole; E.W = c->W; E.H = c->H; E.n2d = c->n2d;
    E.eye = make_float4(c->eye[0], c->eye[1], c->eye[2], 0); E.fwd = make_float4(c->fwd[0], c->fwd[1], c->fwd[2], 0);
    E.right = make_float4(c->right[0], c->right[1], c->right[2], 0); E.up = make_float4(c->up[0], c->up[1], c->up[2], 0);
    E.camera = c->camera;
    if (c->camera) {
        E.cam.xs = c->cam.xsamples; E.cam.ys = c->cam.ysamples; E.cam.jitter = c->cam.jitter != 0;
        E.cam.lens_radius = c->cam.lens_radius; E.cam.focal = c->cam.focal_distance; E.cam.seed = c->cam.sample_seed;
    }
}

static bool has_film(const Ctx *c) { return c->camera && real_filter(c->cam.filter); }

int pm_film(void *ptr, const void *d_samples, void *d_image, void *stream) {
    if (Group *g_ = group_of(ptr)) { /* the assembled raster is filmed on the first device */
        (void)hipSetDevice(g_->subs[0]->device);
        const int rc_ = pm_film(g_->subs[0], d_samples, d_image, stream);
        return rc_ ? group_fail(ptr, g_->subs[0], rc_) : PM_OK;
    }
    GETCTX(ptr);
    if (!has_film(c)) FAIL(c, PM_ERR_INVALID, "pm_film: no camera with a filter (pm_set_camera)");
    if (!d_samples || !d_image) FAIL(c, PM_ERR_INVALID, "pm_film: null buffer");
    hipStream_t s = pick(c, stream);
    EyeParams E{};
    eye_camera(c, E);
    FilmParams F{};
    F.samples = (const float *)d_samples; F.image = (float *)d_image; F.table = c->d_film_table.as<float>();
    F.W = c->cam.width; F.H = c->cam.height; F.WS = c->W; F.HS = c->H;
    F.cam = E.cam;
    F.xw = c->cam.filter.xwidth; F.yw = c->cam.filter.ywidth;
    F.inv_xw = 1.0f / F.xw; F.inv_yw = 1.0f / F.yw;
    timer_begin(c, "film", s);
    HIPCHK(c, launch_film(F, s));
    timer_end(c, "film", s);
    return PM_OK;
}

int pm_camera_rays(void *ptr, int64_t first, int64_t count, float *rays6, float *film_xy) {
    if (Group *g_ = group_of(ptr)) {
        (void)hipSetDevice(g_->subs[0]->device);
        const int rc_ = pm_camera_rays(g_->subs[0], first, count, rays6, film_xy);
        return rc_ ? group_fail(ptr, g_->subs[0], rc_) : PM_OK;
    }
    GETCTX(ptr);
    if (!c->camera) FAIL(c, PM_ERR_INVALID, "pm_camera_rays: no camera (pm_set_camera)");
    if (first < 0 || count < 0 || first + count > (int64_t)c->W * c->H) FAIL(c, PM_ERR_INVALID, "pm_camera_rays: bad sample range");
    if (count == 0) return PM_OK;
    EyeParams E{};
    eye_camera(c, E);
    DevBuf d_r, d_f;
    int rc = PM_OK;
    hipError_t e = hipSuccess;
    if (rays6) e = d_r.ensure((size_t)count * 6 * sizeof(float));
    if (e == hipSuccess && film_xy) e = d_f.ensure((size_t)count * 2 * sizeof(float));
    if (e == hipSuccess) e = launch_camera_rays(E, first, count, d_r.as<float>(), d_f.as<float>(), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && rays6) e = hipMemcpy(rays6, d_r.p, (size_t)count * 6 * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && film_xy) e = hipMemcpy(film_xy, d_f.p, (size_t)count * 2 * sizeof(float), hipMemcpyDeviceToHost);
    d_r.release(); d_f.release();
    if (e != hipSuccess) { c->err = std::string("pm_camera_rays: ") + hipGetErrorString(e); g_last_error = c->err; rc = PM_ERR_HIP; }
    return rc;
}

/* SceneDev from the committed layout: every section pointer, the counts, the traversal mode and stack */
static void fill_scene_dev(Ctx *c) {
    const SceneLayout &L = c->L;
    const HostScene &hs = c->hs;
    SceneDev &S = c->S;
    const char *base = c->d_scene.as<char>();
    const int64_t ni = (int64_t)hs.insts.size();
    S.blob = base;
    S.blob_bytes = (uint32_t)std::min<size_t>(L.bytes, 0xffffffffu);
    S.lds_bytes = L.bytes <= LDS_SCENE_MAX ? (uint32_t)L.bytes : 0u;
    S.nodes = (const float4 *)(base + L.off[SEC_NODES]); S.refs = (const uint32_t *)(base + L.off[SEC_REFS]);
    S.tri_geo = (const float4 *)(base + L.off[SEC_GEO]); S.tri_shade = (const float4 *)(base + L.off[SEC_SHADE]);
    S.tri_id = (const uint32_t *)(base + L.off[SEC_TID]); S.tri_info = (const int4 *)(base + L.off[SEC_INFO]);
    S.norms = (const float4 *)(base + L.off[SEC_NORMS]); S.disks = (const float4 *)(base + L.off[SEC_DISKS]);
    S.spheres = (const float4 *)(base + L.off[SEC_SPHERES]); S.materials = (const float4 *)(base + L.off[SEC_MATS]);
    S.lights = (const LightDev *)(base + L.off[SEC_LIGHTS]);
    S.n_lights = (int)hs.lights.size(); S.n_nodes = (int)L.n_nodes;
    S.n_refs = (int)L.n_refs;
    S.n_tris = (int)L.n_tris; S.n_disks = (int)(hs.disks.size() / 5); S.n_spheres = (int)(hs.spheres.size() / 4);
    S.tri_geo_g = S.tri_geo; S.tri_id_g = S.tri_id;
    S.tri_pairs_g = L.id_order ? c->d_tripairs.as<float>() : nullptr;
    S.light_tris = c->d_light_tris.as<LightTri>();
    S.tex_recs = c->textured ? c->d_tex_recs.as<TexRec>() : nullptr;
    S.texels = c->textured ? c->d_texels.as<float4>() : nullptr;
    S.mat_tex = c->albedo() ? c->d_mat_tex.as<int>() : nullptr;
    S.mat_spec = c->specular ? c->d_mat_spec.as<float4>() : nullptr;
    S.tri_uv = c->textured ? c->d_tri_uv.as<float4>() : nullptr;
    S.n_inst = (int)ni;
    S.insts = ni ? (const float4 *)(base + L.off[SEC_INSTS]) : nullptr;
    S.obj_v = ni ? (const float4 *)(base + L.off[SEC_OBJV]) : nullptr;
    S.obj_info = ni ? (const int4 *)(base + L.off[SEC_OBJINFO]) : nullptr;
    S.obj_n = ni ? (const float4 *)(base + L.off[SEC_OBJN]) : nullptr;
    S.obj_uv = ni ? (const float4 *)(base + L.off[SEC_OBJUV]) : nullptr;
    S.obj_mesh = ni ? (const int4 *)(base + L.off[SEC_OBJMESH]) : nullptr;
    S.brute = (S.lds_bytes > 0 && L.id_order) ? 1 : 0;
    /* a push happens only when descending a level, so depth + 1 entries suffice;
     * sizing the LDS stack by the actual tree keeps occupancy VGPR-bound */
    S.stack_depth = std::min(BVH_STACK, std::max(2, c->bvh_depth + 2));
    S.wide = L.wide;
    S.wnodes = L.wide ? (const float4 *)(base + L.off[SEC_WNODES]) : nullptr;
    /* wide scenes traverse only the 4-wide tree (traverse() dispatches every
     * MODE_GLOBAL query to traverse4): its exact stack bound sizes the LDS
     * stacks, not the binary tree's depth — k_trace_pool's 256-thread blocks
     * then fit four per CU (its VGPR occupancy) instead of three */
    if (L.wide) S.stack_depth = std::min(L.wide == 3 ? BVH8_STACK : BVH_STACK, std::max(2, L.wide_stack + 1));
}

int pm_commit(void *ptr) {
    GROUP_FWD(ptr, pm_commit(sub));
    GETCTX(ptr);
    std::string err;
    int rc;
    if ((rc = validate_scene(c->hs, err))) FAIL(c, rc, "%s", err.c_str());
    const BuildOptions opt = build_options_from_env();
    const auto t_commit0 = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point a) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
    };
    std::vector<BuildPrim> prims;
    scene_boxes(c->hs, prims, c->bbox_lo, c->bbox_hi);
    /* the distant lights' records, before either builder copies the lights */
    if ((rc = finish_lights(c->hs, c->bbox_lo, c->bbox_hi, c->world_sphere, err))) FAIL(c, rc, "%s", err.c_str());

    bool built = false;
    c->textured = scene_textured(c->hs);
    c->specular = scene_specular(c->hs);
    std::vector<float4> tri_uv; /* textured scenes: SceneDev::tri_uv */
    if (c->hs.insts.empty() && !opt.bvh8 && gpu_bvh_wanted(opt, (int64_t)prims.size())) {
        if ((rc = commit_gpu_bvh(c, prims, opt, c->L, built))) return rc;
        if (opt.times && built) fprintf(stderr, "pm_commit: device build, total %.1f ms\n", since(t_commit0));
        if (built && c->textured) {
            /* the device chose the storage order: without instances a triangle's
             * global id (SEC_TID, per storage slot) is its index */
            std::vector<uint32_t> order((size_t)c->L.n_tris);
            HIPCHK(c, hipMemcpy(order.data(), c->d_scene.as<char>() + c->L.off[SEC_TID], order.size() * sizeof(uint32_t),
                                hipMemcpyDeviceToHost));
            for (uint32_t t : order)
                if (t >= c->hs.tris.size()) FAIL(c, PM_ERR_INVALID, "device build: triangle id %u out of range", t);
            tri_uv = triangle_uvs(c->hs, order.data(), (int64_t)order.size());
        }
    }
    if (!built) {
        SceneBlob blob;
        if ((rc = assemble_scene(c->hs, prims, opt, t_commit0, blob, err))) FAIL(c, rc, "%s", err.c_str());
        const auto t_u0 = std::chrono::steady_clock::now();
        if ((rc = upload(c, c->d_scene, blob.bytes))) return rc;
        if (blob.layout.id_order && (rc = upload(c, c->d_tripairs, blob.tri_pairs))) return rc;
        if (opt.times) fprintf(stderr, "pm_commit: upload %.1f ms (%zu bytes), total %.1f ms\n", since(t_u0), blob.bytes.size(),
                               since(t_commit0));
        c->L = blob.layout;
        c->bvh_depth = blob.bvh_depth;
        if (blob.layout.wide) { c->bvh4_nodes = blob.bvh4_nodes; c->bvh4_depth = blob.bvh4_depth; }
        tri_uv.swap(blob.tri_uv);
    }
    if ((rc = upload(c, c->d_light_tris, c->hs.light_tris))) return rc;
    if (c->textured) {
        if ((rc = upload(c, c->d_tex_recs, c->hs.textures))) return rc;
        if ((rc = upload(c, c->d_texels, c->hs.texels))) return rc;
        if ((rc = upload(c, c->d_tri_uv, tri_uv))) return rc;
    }
    if (c->albedo() && (rc = upload(c, c->d_mat_tex, material_textures(c->hs)))) return rc;
    if (c->specular && (rc = upload(c, c->d_mat_spec, material_specular_table(c->hs)))) return rc;
    fill_scene_dev(c);

    if ((rc = light_summary(c->hs, c->lsum, err))) FAIL(c, rc, "%s", err.c_str());
    if ((rc = upload(c, c->d_light_cdf, c->lsum.cdf))) return rc;
    c->committed = true;
    return PM_OK;
}

/* ------------------------------------------------------------- stages */
int pm_eye_pass(void *ptr, const pm_render_params *p, void *stream) {
    GETCTX(ptr);
    int rc;
    if ((rc = check_params(c, p))) return rc;
    if ((rc = ensure_records(c))) return rc;
    if (!c->pinhole && c->rand2d_total > c->n2d)
        FAIL(c, PM_ERR_INVALID, "eye rays carry %d 2D samples, lights need %d", c->n2d, c->rand2d_total);
    hipStream_t s = pick(c, stream);
    EyeParams E{};
    E.S = c->S;
    E.R = recs(c);
    eye_camera(c, E);
    E.rays = c->d_rays.as<float>(); E.rand2d = c->d_rand2d.as<float>();
    E.eps = p->scene_epsilon; E.r2init = p->initial_radius2; E.max_spec = p->max_specular_depth;
    E.light_seed = p->light_rng_seed;
    E.kd = c->albedo() ? c->d_rkd.as<float4>() : nullptr;
    timer_begin(c, "eye", s);
    HIPCHK(c, launch_eye(E, s));
    timer_end(c, "eye", s);
    c->rec_fresh = false; /* the eye pass writes every record */
    c->tiles.invalidate();
    c->grid_plan.invalidate();
    if (c->view_active && (rc = build_view(c, s))) return rc;
    return PM_OK;
}

int pm_reserve_slots(void *ptr, int64_t n, void **d_slots) {
    GETCTX(ptr);
    int rc;
    if (n < 0) FAIL(c, PM_ERR_INVALID, "negative slot count");
    if (d_slots) { /* the caller may read the buffer from now on: no lazy zero fill on it */
        if ((rc = materialize_slots(c, nullptr))) return rc;
        c->slots_exposed = true;
    }
    if ((size_t)n * sizeof(pm_photon) > c->d_slots.bytes) {
        if (c->d_slots.external)
            FAIL(c, PM_ERR_INVALID, "external slot buffer holds %zu slots, %lld needed",
                 c->d_slots.bytes / sizeof(pm_photon), (long long)n);
        /* keep the contents: grow by copy */
        DevBuf nb;
        HIPCHK(c, nb.ensure((size_t)n * sizeof(pm_photon)));
        if (c->d_slots.p) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, hipMemcpy(nb.p, c->d_slots.p, c->d_slots.bytes, hipMemcpyDeviceToDevice));
            c->d_slots.release();
        }
        c->d_slots = nb;
        nb.p = nullptr;
    }
    if (d_slots) *d_slots = c->d_slots.p;
    return PM_OK;
}

int pm_set_slot_buffer(void *ptr, void *d, int64_t n) {
    GETCTX(ptr);
    int rc;
    if ((rc = materialize_slots(c, nullptr))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->d_slots.release();
    c->fused.valid = false;
    if (d) {
        if (n <= 0) FAIL(c, PM_ERR_INVALID, "external slot buffer needs n_slots > 0");
        c->d_slots.p = d;
        c->d_slots.bytes = (size_t)n * sizeof(pm_photon);
        c->d_slots.external = true;
    }
    c->slots_used = 0;
    return PM_OK;
}

/* radius^2 the grid of a new pass is designed for (pm_plan.h R2Plan): asked
 * only where a photon map's grid is chosen (pm_trace_photons with fused
 * counting, or pm_build_photon_map without), so the trace and the build of
 * one pass agree. A landed histogram sets it; the bins of the previous
 * pass's gathers are reduced on s into host-mapped memory by a one-block
 * kernel (no copy-engine transfer in the stream: a per-pass D2H copy cost
 * ~0.5 ms of C2 step). */
static float grid_radius2(Ctx *c, const pm_render_params *p, hipStream_t s) {
    R2Plan &r = c->grid_plan;
    const float init = p->initial_radius2;
    if (!r.active(p->estimator)) return init;
    if (r.pending && hipEventQuery(c->hist_event) == hipSuccess) {
        uint32_t hist[R2_BINS];
        for (int b = 0; b < R2_BINS; ++b) hist[b] = ((volatile uint32_t *)c->h_hist)[b];
        r.landed(hist, init);
    }
    if (r.reduce_due() && launch_r2hist_reduce(c->d_hist.as<uint32_t>(), c->h_hist_dev, s) == hipSuccess &&
        hipEventRecord(c->hist_event, s) == hipSuccess)
        r.reduce_issued(s);
    r.pass_began(c->rec_fresh);
    return r.radius2(init, c->rec_fresh);
}

static GridDesc make_grid(const Ctx *c, const pm_render_params *p, float radius2) {
    return pm::make_grid(c->bbox_lo, c->bbox_hi, p->estimator, c->cell_span, radius2);
}

static bool same_grid(const GridDesc &a, const GridDesc &b) { return std::memcmp(&a, &b, sizeof(GridDesc)) == 0; }

/* make the first `words` bucket counters zero (a memset only when the last
 * bucket scan did not already leave them cleared) */
static hipError_t count_zeroed(Ctx *c, size_t words, hipStream_t s) {
    if (c->count_zero_ptr == c->d_count.p && c->count_zero_words >= words) return hipSuccess;
    hipError_t e = hipMemsetAsync(c->d_count.p, 0, words * 4, s);
    if (e == hipSuccess) { c->count_zero_words = words; c->count_zero_ptr = c->d_count.p; }
    return e;
}

int pm_trace_photons(void *ptr, const pm_render_params *p, int pass, int64_t path_begin, int64_t path_count,
                     int64_t slot_path_base, void *stream) {
    GETCTX(ptr);
    int rc;
    if ((rc = check_params(c, p))) return rc;
    if (path_count < 0 || path_begin < slot_path_base) FAIL(c, PM_ERR_INVALID, "bad path range");
    if ((uint64_t)(path_begin + path_count) * (uint64_t)p->max_photon_count > 0xffffffffull)
        FAIL(c, PM_ERR_INVALID, "photon slot index exceeds 32 bits (reference pm_index is a uint)");
    const int64_t mpc = p->max_photon_count;
    const int64_t end_slot = (path_begin + path_count - slot_path_base) * mpc;
    hipStream_t s = pick(c, stream);
    const bool fuse = c->fuse_ok && p->gather_structure == PM_GATHER_GRID && path_begin == slot_path_base;
    /* stale slots of an earlier lazy trace: zeroed now unless this fused
     * trace rewrites (or re-marks) every one of them */
    if (c->slots_dirty > 0 && !(fuse && end_slot >= c->slots_dirty) && (rc = materialize_slots(c, s))) return rc;
    c->slots_dirty = 0;
    if ((rc = pm_reserve_slots(c, end_slot, nullptr))) return rc;
    TraceParams T{};
    T.S = c->S;
    T.slots = c->d_slots.as<pm_photon>();
    halton_perm((uint32_t)pass, T.perm);
    {
        const uint32_t base[3] = {3u, 5u, 7u}, off[3] = {2u, 5u, 10u};
        for (int k = 0; k < 3; ++k) {
            T.perm_bits[k] = 0u;
            for (uint32_t d = 0; d < base[k]; ++d) T.perm_bits[k] |= T.perm[off[k] + d] << (3u * d);
        }
    }
    T.path_begin = path_begin; T.path_count = path_count; T.slot_path_base = slot_path_base;
    T.hold = c->trace_hold ? 1 : 0;
    if (T.hold && !c->S.wide) { /* per-lane kernel: only when the held deposits' LDS costs no resident waves */
        const size_t lds = (size_t)c->S.stack_depth * TRACE_BLOCK * 4 + c->S.lds_bytes;
        if (trace_lane_waves_per_cu(c->S, lds, 1) < trace_lane_waves_per_cu(c->S, lds, 0)) T.hold = 0;
    }
    if (c->S.wide) {
        /* pooled kernel: one occupancy round (resident waves per CU from the
         * occupancy API: VGPRs and the LDS stacks) — each wave with a
         * contiguous pool of a multiple of 64 paths. C3 sweep (1M paths, 256 CUs): 4096 waves 5.25 ms, 8192
         * (two rounds) 5.81, 5462 (1.33 rounds) 6.73, 2048 7.22 */
        /* LDS stack entries per lane (env PM_POOL_STACK; 0 = the tree's exact
         * bound): below the bound, deeper entries spill to global memory and
         * the smaller LDS reservation admits more resident blocks */
        const int lstk = c->pool_stack > 0 && c->pool_stack < c->S.stack_depth ? c->pool_stack : c->S.stack_depth;
        T.pool_stack = lstk;
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus <= 0) cus = 256;
        const size_t lds = (size_t)lstk * TRACE_BLOCK * 4 + c->S.lds_bytes;
        const int w8 = c->S.wide == 3;
        int per_cu = trace_pool_waves_per_cu(lds, 0, w8);
        if (T.hold) { /* pooled kernel: the held deposits' LDS must not cost resident waves */
            const int per_cu_h = trace_pool_waves_per_cu(lds, 1, w8);
            if (per_cu_h < per_cu) T.hold = 0;
            else per_cu = per_cu_h;
        }
        const int64_t waves = (int64_t)cus * (per_cu > 0 ? per_cu : 16);
        /* any pool size works (the wave's cursor hands out paths to dead lanes) */
        const int64_t per = std::max<int64_t>(1, (path_count + waves - 1) / waves);
        T.pool_paths = c->trace_pool || c->S.wide == 3 ? per : 0; /* 8-wide: its deeper stacks need the pooled kernel's spill */
        if (lstk < c->S.stack_depth) {
            const int64_t blocks = ((path_count + per - 1) / per + TRACE_BLOCK / 64 - 1) / (TRACE_BLOCK / 64);
            const int64_t threads = blocks * TRACE_BLOCK;
            HIPCHK(c, c->d_spill.ensure((size_t)threads * (size_t)(c->S.stack_depth - lstk) * 4));
            T.spill = c->d_spill.as<int>();
            T.spill_stride = (uint32_t)threads;
        }
    }
    T.pass = pass; T.mpc = (int)mpc; T.max_spec = p->max_specular_depth; T.light_index = p->light_source_index;
    T.eps = p->scene_epsilon; T.seed = p->rng_seed;
    T.light_cdf = c->d_light_cdf.as<float>();
    T.counters = c->d_counters.as<unsigned long long>() + 4;
    T.prof = c->d_counters.as<unsigned long long>() + 8;
    if (c->counting) HIPCHK(c, hipMemsetAsync(T.counters, 0, 32, s));
    /* A call that fills the slot buffer from slot 0 also runs the counting pass
     * of the bucket build (keys, ranks, per-cell counts) at deposit time; the
     * build then skips it (c->fused). Any other slot producer invalidates it. */
    c->fused.valid = false;
    if (fuse) {
        c->fused.r2 = grid_radius2(c, p, s);
        const GridDesc g = make_grid(c, p, c->fused.r2);
        HIPCHK(c, c->d_count.ensure_slack(((size_t)g.ncells + 1) * 4));
        HIPCHK(c, c->d_scratch.ensure_slack(bucket_scratch_words(end_slot, g.ncells) * 4));
        HIPCHK(c, count_zeroed(c, (size_t)g.ncells + 1, s));
        T.bucket = 1;
        T.grid = g;
        T.count = c->d_count.as<uint32_t>();
        T.key = c->d_scratch.as<uint32_t>();
        T.rank = c->d_scratch.as<uint32_t>() + end_slot;
        /* plane-major keys / ranks; the held deposits write a path's four
         * keys as one 16-B store in slot order */
        T.key_np = !T.hold ? path_count : 0;
        T.lazy_zero = c->lazy_zero && !T.hold && !c->d_slots.external && !c->slots_exposed ? 1 : 0;
    }
    timer_begin(c, "trace", s);
    /* the kernel writes all path_count * mpc slots: deposits, then zeros */
    HIPCHK(c, launch_trace(T, c->counting, s));
    timer_end(c, "trace", s);
    if (fuse) { c->fused.valid = true; c->fused.n = end_slot; c->fused.grid = T.grid; c->fused.key_np = T.key_np; c->fused.mpc = (int)mpc; c->count_zero_words = 0; }
    if (T.lazy_zero) {
        if (!c->dirty_event) HIPCHK(c, hipEventCreateWithFlags(&c->dirty_event, hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(c->dirty_event, s));
        c->slots_dirty = end_slot;
        c->dirty_key_np = T.key_np;
        c->dirty_mpc = (int)mpc;
    }
    /* traced photons carry the scene's signs (scene_nonneg); slots outside
     * the traced range keep theirs, so the flag is reset only when this
     * trace rewrote every slot in use */
    if (path_begin == slot_path_base && end_slot >= c->slots_used) c->slots_nonneg = true;
    c->slots_used = std::max(c->slots_used, end_slot);
    return PM_OK;
}

int pm_build_photon_map(void *ptr, const pm_render_params *p, int64_t n_slots, void *stream) {
    GETCTX(ptr);
    int rc;
    if ((rc = check_params(c, p))) return rc;
    if (n_slots <= 0) n_slots = c->slots_used;
    if ((size_t)n_slots * sizeof(pm_photon) > c->d_slots.bytes) FAIL(c, PM_ERR_INVALID, "n_slots beyond slot buffer");
    hipStream_t s = pick(c, stream);
    c->map_slots = n_slots;
    if (p->gather_structure == PM_GATHER_KDTREE && (rc = materialize_slots(c, s))) return rc;
    if (p->gather_structure == PM_GATHER_KDTREE) {
        /* reference path (CreatePhotonMap): DtoH, CPU pbrt KdTree, HtoD */
        timer_begin(c, "build", s, true);
        std::vector<pm_photon> h((size_t)n_slots), nodes;
        HIPCHK(c, hipMemcpyAsync(h.data(), c->d_slots.p, n_slots * sizeof(pm_photon), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        int64_t m = build_kdtree_pbrt(h.data(), n_slots, nodes);
        c->kd_count = m;
        if (m > 0) {
            HIPCHK(c, c->d_kd.ensure(m * sizeof(pm_photon)));
            HIPCHK(c, hipMemcpyAsync(c->d_kd.p, nodes.data(), m * sizeof(pm_photon), hipMemcpyHostToDevice, s));
            HIPCHK(c, hipStreamSynchronize(s));
        }
        timer_end(c, "build", s);
        c->map_kind = PM_GATHER_KDTREE;
        if (m == 0) FAIL(c, PM_ERR_NO_PHOTONS, "0 valid photons");
        return PM_OK;
    }
    /* photon buckets: cell size >= 2 r_max (PPM radii only shrink) */
    GridDesc &g = c->grid;
    /* the grid of the trace's fused counts, if they cover these slots */
    const bool fused_ok = c->fused.valid && c->fused.n == n_slots;
    c->grid_r2 = fused_ok ? c->fused.r2 : grid_radius2(c, p, s);
    g = make_grid(c, p, c->grid_r2);
    const bool counted = fused_ok && same_grid(c->fused.grid, g);
    /* the counting pass below reads every slot's valid bit (and overwrites the keys) */
    if (!counted && (rc = materialize_slots(c, s))) return rc;
    const size_t n = (size_t)n_slots;
    HIPCHK(c, c->d_count.ensure_slack(((size_t)g.ncells + 1) * 4));
    HIPCHK(c, c->d_cell_start.ensure_slack(((size_t)g.ncells + 1) * 4));
    if (!counted) {
        HIPCHK(c, c->d_scratch.ensure_slack(bucket_scratch_words(n_slots, g.ncells) * 4));
        HIPCHK(c, count_zeroed(c, (size_t)g.ncells + 1, s));
    }
    HIPCHK(c, c->d_pha.ensure_slack(n * 16)); HIPCHK(c, c->d_phb.ensure_slack(n * 32));
    timer_begin(c, "build", s);
    HIPCHK(c, launch_bucket_build(c->d_slots.as<pm_photon>(), n_slots, g, c->d_count.as<uint32_t>(),
                                  c->d_cell_start.as<uint32_t>(), c->d_scratch.as<uint32_t>(), c->d_pha.as<float4>(),
                                  c->d_phb.as<float4>(), counted, s, counted ? c->fused.key_np : 0, c->fused.mpc));
    ++c->map_gen; /* kNN pairs repacked on the next kNN gather */
    /* the scan left the counters zeroed */
    c->count_zero_words = (size_t)g.ncells + 1;
    c->count_zero_ptr = c->d_count.p;
    timer_end(c, "build", s);
    c->map_kind = PM_GATHER_GRID;
    return PM_OK;
}


/* ---- the steps of a gather (gather_common), in order ---------------------- */
static int gather_validate(Ctx *c, const pm_render_params *p, bool partials, int64_t rec_begin, int64_t rec_count) {
    int rc;
    if ((rc = check_params(c, p))) return rc;
    if (c->nrec <= 0) FAIL(c, PM_ERR_INVALID, "no records (run pm_eye_pass first)");
    if (c->map_kind != p->gather_structure) FAIL(c, PM_ERR_INVALID, "photon map not built for this gather structure");
    if (p->estimator == PM_ESTIMATOR_KNN && partials)
        FAIL(c, PM_ERR_INVALID, "the kNN estimator is not linear in the photon set: no partial / split gathers "
                                "(multi-GPU: all-gather the photons, then pm_gather_range)");
    if (rec_begin < 0 || rec_count < 0 || rec_begin + rec_count > c->nrec) FAIL(c, PM_ERR_INVALID, "bad record range");
    return PM_OK;
}

/* a pending reset is consumed by a fused gather over all records (it starts
 * from the initial PPM state and writes it: consume); a split partial gather
 * reads the initial radius and leaves the reset to pm_ppm_update_split, which
 * writes every view record; any other gather needs it applied */
static int gather_resolve_reset(Ctx *c, GatherParams &G, bool fused_full, bool split, hipStream_t s, bool &consume) {
    consume = c->rec_fresh && fused_full;
    if (!consume && !(split && c->rec_fresh)) return materialize_reset(c, s);
    G.fresh = 1; /* every radius is r2init, the first group's box comes from the tile's position box */
    G.r2init = c->rec_fresh_r2;
    return PM_OK;
}

/* full-range tile gathers skip the tiles without an active record (their
 * records are neither read nor written, except as partials outside a view) */
static int gather_attach_tiles(Ctx *c, const pm_render_params *p, GatherParams &G, hipStream_t s) {
    TileList &t = c->tiles;
    HIPCHK(c, t.ensure(recs(c), s));
    G.tiles = t.d_list.as<uint32_t>();
    if (t.count_known) { G.n_tiles = t.n; G.n_tiles_dev = nullptr; }
    else { G.n_tiles = (c->nrec + 63) / 64; G.n_tiles_dev = t.d_count.as<uint32_t>(); }
    /* the PPM tile gather and the kNN scalar-stream kernel record the costs */
    if (t.sort && !t.sorted && (p->estimator == PM_ESTIMATOR_PPM || c->knn_ss)) {
        HIPCHK(c, t.d_cost.ensure((size_t)((c->nrec + 63) / 64 + 8) * 2));
        HIPCHK(c, t.d_sorted.ensure(t.d_list.bytes));
        G.tile_cost = t.d_cost.as<uint16_t>();
    }
    return PM_OK;
}

/* a fused PPM tile gather bins the updated radii (R2Plan) — over all
 * records, or over each of a pass's bands (a device's bands in a group
 * render or an all-gather rank): every gather of the pass adds to the same
 * bins, summed once when the next pass chooses its grid (grid_radius2), so
 * the quantile describes every record the context gathers */
static int gather_attach_hist(Ctx *c, const pm_render_params *p, GatherParams &G, hipStream_t s) {
    HIPCHK(c, c->d_hist.ensure(R2_COPIES * R2_BINS * 4));
    if (!c->h_hist) {
        HIPCHK(c, hipHostMalloc((void **)&c->h_hist, R2_BINS * 4, hipHostMallocMapped));
        HIPCHK(c, hipHostGetDevicePointer((void **)&c->h_hist_dev, c->h_hist, 0));
    }
    if (!c->hist_event) HIPCHK(c, hipEventCreateWithFlags(&c->hist_event, hipEventDisableTiming));
    const R2Plan::BinPrep prep = c->grid_plan.before_bin(p->initial_radius2, s);
    /* the reduce may have run on another stream (a trace issued ahead on a
     * second stream chose its grid: dist.py's pipelined passes): without
     * the wait the two race on the bins */
    if (prep.wait) HIPCHK(c, hipStreamWaitEvent(s, c->hist_event, 0));
    if (prep.clear) HIPCHK(c, hipMemsetAsync(c->d_hist.p, 0, R2_COPIES * R2_BINS * 4, s));
    G.r2hist = c->d_hist.as<uint32_t>();
    G.r2hist_inv = 1.0f / p->initial_radius2;
    return PM_OK;
}

static int gather_knn_setup(Ctx *c, const pm_render_params *p, GatherParams &G) {
    G.knn_k = p->knn_lookup;
    G.knn_r2 = p->initial_radius2; /* pbrt's maxDistSquared: the buckets cover it */
    /* every term (kernel <= 3/pi < 1) is <= alpha_max / r_k^2: <= 2^22 of
     * the per-record scale per term (x4 headroom in amax), exact as a float
     * and as an int32, and <= PM_KNN_MAX = 2^6 terms sum below 2^28 —
     * exact in int32 */
    const double amax = flux_bound(c, p) * 4.0;
    G.knn_fx = (float)(std::ldexp(1.0, 24) / std::max(amax, 1e-30));
    G.slots = c->d_slots.as<pm_photon>();
    if (c->knn_ss && !c->counting && c->gather_kernel == PM_GK_TILE) {
        const int64_t nph = (int64_t)(c->d_pha.bytes / 16), pairs = (nph + 1) / 2 + 16;
        const int64_t ntiles = (G.rec_end - G.rec_begin + 63) / 64;
        HIPCHK(c, c->d_knnpk.ensure((size_t)pairs * 80));
        HIPCHK(c, c->d_knnovf.ensure((size_t)(ntiles + KNN_OVF_HDR) * 4));
        G.knn_pk_p = c->d_knnpk.as<float4>();
        G.knn_pk_q = G.knn_pk_p + 2 * pairs;
        G.knn_pk_pairs = pairs;
        G.knn_pack = c->knn_pack_gen != c->map_gen || c->knn_pack_ptr != c->d_knnpk.p;
        c->knn_pack_gen = c->map_gen;
        c->knn_pack_ptr = c->d_knnpk.p;
        G.knn_ovf_n = c->d_knnovf.as<uint32_t>();
        G.knn_ovf = G.knn_ovf_n + KNN_OVF_HDR;
    }
    return PM_OK;
}

/* diagnostic builds (-DPM_TILE_TIMES): env PM_TILE_TIMES=file appends each
 * tile launch's per-wave (start, end, XCC_ID, HW_ID) records (tools/tile_times.py) */
static int tile_times_attach(Ctx *c, GatherParams &G, hipStream_t s) {
#ifdef PM_TILE_TIMES
    const size_t bytes = (size_t)((c->nrec + 63) / 64) * 64;
    if (getenv("PM_TILE_TIMES") && G.tiles) {
        HIPCHK(c, c->d_tile_times.ensure(bytes));
        HIPCHK(c, hipMemsetAsync(c->d_tile_times.p, 0, bytes, s));
        G.tile_times = c->d_tile_times.as<unsigned long long>();
    }
#endif
    return PM_OK;
}

static int tile_times_dump(Ctx *c, const GatherParams &G, hipStream_t s) {
#ifdef PM_TILE_TIMES
    if (!G.tile_times) return PM_OK;
    const int64_t tt_n = (c->nrec + 63) / 64;
    std::vector<unsigned long long> h((size_t)tt_n * 8);
    HIPCHK(c, hipMemcpyAsync(h.data(), G.tile_times, h.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (FILE *f = fopen(getenv("PM_TILE_TIMES"), "ab")) {
        const unsigned long long hdr[4] = {0xffffffffffffffffull, (unsigned long long)tt_n, 0, 0};
        fwrite(hdr, 8, 4, f);
        fwrite(h.data(), 8, h.size(), f);
        fclose(f);
    }
#endif
    return PM_OK;
}

/* env PM_KNN_SS_DEBUG: the tiles k_gather_knn_ss handed back to k_gather_knn_tile */
static int knn_ss_debug_dump(Ctx *c, const GatherParams &G, hipStream_t s) {
    uint32_t nb = 0;
    HIPCHK(c, hipMemcpyAsync(&nb, G.knn_ovf_n, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    fprintf(stderr, "pm knn_ss: %u of %lld tiles handed back\n", nb, (long long)(G.tiles ? G.n_tiles : (G.rec_end - G.rec_begin + 63) / 64));
    std::vector<uint32_t> hdr(KNN_OVF_HDR);
    HIPCHK(c, hipMemcpy(hdr.data(), G.knn_ovf_n, KNN_OVF_HDR * 4, hipMemcpyDeviceToHost));
    if (hdr[1] || hdr[2]) { /* PM_KNN_SS_DBG builds */
        fprintf(stderr, "pm knn_ss dbg: %u bad collects, %u NaN radii\n", hdr[1], hdr[2]);
        for (uint32_t i = 0; i < std::min<uint32_t>(hdr[1], 60); ++i) {
            fprintf(stderr, "  ");
            for (int w = 0; w < 16; ++w) fprintf(stderr, " %u", hdr[64 + 16 * i + w]);
            fprintf(stderr, "\n");
        }
    }
    return PM_OK;
}

static int gather_launch(Ctx *c, const pm_render_params *p, GatherParams &G, bool partials, hipStream_t s) {
    const bool knn = p->estimator == PM_ESTIMATOR_KNN;
    int rc;
    if (!knn && p->gather_structure == PM_GATHER_KDTREE) HIPCHK(c, hipMemsetAsync(G.error, 0, 4, s));
    if ((rc = tile_times_attach(c, G, s))) return rc;
    if (knn) HIPCHK(c, launch_gather_knn(G, c->counting, s));
    else HIPCHK(c, launch_gather(G, p->gather_structure, partials, c->counting, s));
    if ((rc = tile_times_dump(c, G, s))) return rc;
    if (knn && G.knn_ovf_n && getenv("PM_KNN_SS_DEBUG")) return knn_ss_debug_dump(c, G, s);
    return PM_OK;
}

/* after the launch: the tile sort, the kd-tree gather's error word, the state the gather leaves */
static int gather_post(Ctx *c, const pm_render_params *p, GatherParams &G, bool consume, bool hist, hipStream_t s) {
    if (G.tile_cost) { /* the measured wave lifetimes reorder the list for the next gathers */
        HIPCHK(c, launch_tile_sort(G.tiles, G.tile_cost, G.n_tiles_dev, G.n_tiles, c->tiles.d_sorted.as<uint32_t>(), s));
        c->tiles.swap_sorted();
    }
    timer_end(c, "gather", s);
    if (p->estimator != PM_ESTIMATOR_KNN && p->gather_structure == PM_GATHER_KDTREE) {
        /* the reference's path (host kd-tree, synchronous like CreatePhotonMap):
         * a truncated traversal is an error, not a silently darker pixel */
        unsigned int err = 0;
        HIPCHK(c, hipMemcpyAsync(&err, G.error, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        if (err & PM_GATHER_ERR_STACK) FAIL(c, PM_ERR_INVALID, "kd-tree gather: traversal stack of %d entries overflowed", G.kd_stack);
        if (err & PM_GATHER_ERR_TREE) FAIL(c, PM_ERR_INVALID, "kd-tree gather: node links do not form a pbrt kd-tree");
    }
    c->rec_estimator = p->estimator;
    if (consume) c->rec_fresh = false;
    if (hist) c->grid_plan.binned(p->initial_radius2);
    else if (p->estimator == PM_ESTIMATOR_KNN) c->grid_plan.invalidate(); /* r_k^2 replaced the radii */
    return PM_OK;
}

static int gather_common(Ctx *c, const pm_render_params *p, long long *partial, int64_t rec_begin, int64_t rec_count,
                         void *stream, int *count = nullptr, long long *flux = nullptr) {
    const bool split = count != nullptr, partials = partial != nullptr || split;
    int rc;
    if ((rc = gather_validate(c, p, partials, rec_begin, rec_count))) return rc;
    hipStream_t s = pick(c, stream);
    const bool full = rec_begin == 0 && rec_count == c->nrec;
    const bool tile_kernel = c->gather_kernel == PM_GK_TILE && !c->counting && p->gather_structure == PM_GATHER_GRID;
    GatherParams G = gather_params(c, p);
    G.partial = partial;
    G.count = count;
    G.flux = flux;
    G.rec_begin = rec_begin;
    G.rec_end = rec_begin + rec_count;
    bool consume;
    if ((rc = gather_resolve_reset(c, G, full && !partials, split, s, consume))) return rc;
    if (tile_kernel && full && (!partials || c->view_active) && (rc = gather_attach_tiles(c, p, G, s))) return rc;
    if (c->counting) HIPCHK(c, hipMemsetAsync(c->d_counters.p, 0, 32, s));
    const bool hist = tile_kernel && !partials && c->grid_plan.active(p->estimator) && c->grid_plan.wanted;
    if (hist && (rc = gather_attach_hist(c, p, G, s))) return rc;
    timer_begin(c, "gather", s);
    if (p->estimator == PM_ESTIMATOR_KNN && (rc = gather_knn_setup(c, p, G))) return rc;
    if ((rc = gather_launch(c, p, G, partials, s))) return rc;
    return gather_post(c, p, G, consume, hist, s);
}

int pm_gather(void *ptr, const pm_render_params *p, void *stream) {
    GETCTX(ptr);
    return gather_common(c, p, nullptr, 0, c->nrec, stream);
}

int pm_gather_range(void *ptr, const pm_render_params *p, int64_t rec_begin, int64_t rec_count, void *stream) {
    GETCTX(ptr);
    return gather_common(c, p, nullptr, rec_begin, rec_count, stream);
}

int pm_gather_partial(void *ptr, const pm_render_params *p, void *d_partial, void *stream) {
    GETCTX(ptr);
    if (!d_partial) FAIL(c, PM_ERR_INVALID, "null partial buffer");
    return gather_common(c, p, (long long *)d_partial, 0, c->nrec, stream);
}

int pm_gather_split(void *ptr, const pm_render_params *p, void *d_count, void *d_flux, void *stream) {
    GETCTX(ptr);
    if (!d_count || !d_flux) FAIL(c, PM_ERR_INVALID, "null count / flux buffer");
    return gather_common(c, p, nullptr, 0, c->nrec, stream, (int *)d_count, (long long *)d_flux);
}

int pm_ppm_update_split(void *ptr, const pm_render_params *p, const void *d_count, const void *d_flux_chunk,
                        int64_t v_begin, int64_t v_count, void *stream) {
    GETCTX(ptr);
    int rc;
    if ((rc = check_params(c, p))) return rc;
    const int64_t n = view_size(c);
    if (!d_count || (v_count > 0 && !d_flux_chunk) || v_begin < 0 || v_count < 0 || v_begin + v_count > n)
        FAIL(c, PM_ERR_INVALID, "bad view chunk");
    hipStream_t s = pick(c, stream);
    GatherParams G = gather_params(c, p);
    const int fresh = c->rec_fresh ? 1 : 0;
    G.r2init = c->rec_fresh_r2;
    timer_begin(c, "update", s);
    HIPCHK(c, launch_ppm_update_split(G, (const int *)d_count, (const long long *)d_flux_chunk, n, v_begin, v_count,
                                      fresh, s));
    timer_end(c, "update", s);
    c->rec_fresh = false; /* every view record written (records outside the view are inactive) */
    return PM_OK;
}

int pm_ppm_update_split_radius(void *ptr, const pm_render_params *p, const void *d_count, void *d_ratio, void *stream) {
    GETCTX(ptr);
    int rc;
    if ((rc = check_params(c, p))) return rc;
    const int64_t n = view_size(c);
    if (!d_count || !d_ratio) FAIL(c, PM_ERR_INVALID, "null count / ratio buffer");
    hipStream_t s = pick(c, stream);
    GatherParams G = gather_params(c, p);
    const int fresh = c->rec_fresh ? 1 : 0;
    G.r2init = c->rec_fresh_r2;
    timer_begin(c, "update", s);
    HIPCHK(c, launch_ppm_update_radius(G, (const int *)d_count, (float *)d_ratio, n, fresh, s));
    timer_end(c, "update", s);
    c->rec_fresh = false; /* every view record written (records outside the view are inactive) */
    return PM_OK;
}

int pm_ppm_update_split_flux(void *ptr, const pm_render_params *p, const void *d_ratio, const void *d_flux_chunk,
                             int64_t v_begin, int64_t v_count, void *stream) {
    GETCTX(ptr);
    int rc;
    if ((rc = check_params(c, p))) return rc;
    const int64_t n = view_size(c);
    if (!d_ratio || (v_count > 0 && !d_flux_chunk) || v_begin < 0 || v_count < 0 || v_begin + v_count > n)
        FAIL(c, PM_ERR_INVALID, "bad view chunk");
    hipStream_t s = pick(c, stream);
    GatherParams G = gather_params(c, p);
    HIPCHK(c, launch_ppm_update_flux(G, (const float *)d_ratio, (const long long *)d_flux_chunk, v_begin, v_count, s));
    return PM_OK;
}

int pm_ppm_update(void *ptr, const pm_render_params *p, const void *d_partial, int64_t rec_begin, int64_t rec_count,
                  void *stream) {
    GETCTX(ptr);
    int rc;
    if ((rc = check_params(c, p))) return rc;
    if (!d_partial || rec_begin < 0 || rec_count < 0 || rec_begin + rec_count > view_size(c))
        FAIL(c, PM_ERR_INVALID, "bad record range");
    hipStream_t s = pick(c, stream);
    if ((rc = materialize_reset(c, s))) return rc;
    GatherParams G = gather_params(c, p);
    timer_begin(c, "update", s);
    HIPCHK(c, launch_ppm_update(G, (const long long *)d_partial, rec_begin, rec_count, s));
    timer_end(c, "update", s);
    return PM_OK;
}

int pm_get_radius2(void *ptr, int64_t rec_begin, int64_t rec_count, void *d_out, void *stream) {
    GETCTX(ptr);
    if (!d_out || rec_begin < 0 || rec_count < 0 || rec_begin + rec_count > view_size(c))
        FAIL(c, PM_ERR_INVALID, "bad radius2 range");
    int rc;
    if ((rc = materialize_reset(c, pick(c, stream)))) return rc;
    HIPCHK(c, launch_radius2_io(recs(c), (float *)d_out, rec_begin, rec_count, 0, view_list(c), pick(c, stream)));
    return PM_OK;
}

int pm_set_radius2(void *ptr, const void *d_in, int64_t rec_begin, int64_t rec_count, void *stream) {
    GETCTX(ptr);
    if (!d_in || rec_begin < 0 || rec_count < 0 || rec_begin + rec_count > view_size(c))
        FAIL(c, PM_ERR_INVALID, "bad radius2 range");
    int rc;
    if ((rc = materialize_reset(c, pick(c, stream)))) return rc;
    HIPCHK(c, launch_radius2_io(recs(c), (float *)d_in, rec_begin, rec_count, 1, view_list(c), pick(c, stream)));
    c->grid_plan.invalidate(); /* radii may have grown */
    return PM_OK;
}

int pm_final(void *ptr, double emitted, int64_t rec_begin, int64_t rec_count, void *d_out, void *stream) {
    GETCTX(ptr);
    if (!d_out || rec_begin < 0 || rec_count < 0 || rec_begin + rec_count > c->nrec)
        FAIL(c, PM_ERR_INVALID, "bad final range");
    hipStream_t s = pick(c, stream);
    int rc;
    if ((rc = materialize_reset(c, s))) return rc;
    const FinalParams F = final_params(c, emitted, rec_begin, rec_count, (float *)d_out);
    timer_begin(c, "final", s);
    HIPCHK(c, launch_final(F, s));
    timer_end(c, "final", s);
    return PM_OK;
}

/* ------------------------------------------------------------ whole render */
/* the pieces pm_render, group_render and pm_render_simple share; HIP errors
 * are reported on ec (a group's context, or c itself) */

/* valid photons of the map c just built; waits for its stream */
static int valid_photons(Ctx *ec, Ctx *c, const pm_render_params *p, int64_t &nvalid) {
    nvalid = c->kd_count;
    if (p->gather_structure == PM_GATHER_GRID) {
        uint32_t nv = 0;
        HIPCHK(ec, hipMemcpyAsync(&nv, c->d_cell_start.as<uint32_t>() + c->grid.ncells, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(ec, hipStreamSynchronize(c->stream));
        nvalid = nv;
    }
    if (nvalid == 0) FAIL(ec, PM_ERR_NO_PHOTONS, "0 valid photons (photonmappingrenderer.cpp:165-167)");
    return PM_OK;
}

/* c->d_out (nout radiances: the sample raster, or one per ray) -> the host
 * image, through the film when the camera has a filter; waits */
static int deliver_image(Ctx *c, int64_t nout, float *out_rgb) {
    const void *src = c->d_out.p;
    if (has_film(c)) {
        nout = (int64_t)c->cam.width * c->cam.height;
        HIPCHK(c, c->d_img.ensure(nout * 3 * sizeof(float)));
        if (int rc = pm_film(c, c->d_out.p, c->d_img.p, c->stream)) return rc;
        src = c->d_img.p;
    }
    HIPCHK(c, hipMemcpyAsync(out_rgb, src, nout * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PM_OK;
}

/* the stats every photon render reports: paths, valid photons, active records (read back from c) */
static int render_stats(Ctx *ec, Ctx *c, double emitted, int64_t nvalid, pm_stats *st) {
    std::memset(st, 0, sizeof(*st));
    st->paths_emitted = (int64_t)emitted;
    st->photons_valid = nvalid;
    std::vector<float4> pos(c->nrec);
    HIPCHK(ec, hipMemcpy(pos.data(), c->d_pos.p, c->nrec * sizeof(float4), hipMemcpyDeviceToHost));
    for (auto &q : pos) st->gather_points += (fbits_h(q.w) & (PM_REC_MISS | PM_REC_EXCEPTION | PM_REC_INVALID)) == 0;
    return PM_OK;
}

/* one progressive render over the group's devices (Group): per pass every
 * device traces its shard of the global paths into its own slot buffer at
 * the shard's global slot offset, the shards are all-gathered (equal
 * chunks, the last padded with invalid slots), every device builds the full
 * map and gathers its bands; the final pass writes each device's bands into
 * the host image. Bit-identical to one device rendering all the paths (the
 * same valid photons in the map; exact, order-free gather sums). */
static int group_render(Ctx *gc, const pm_render_params *p, float *out_rgb, pm_stats *st) {
    Group &G = *gc->group;
    const int n = (int)G.subs.size();
    if (!p || !out_rgb) FAIL(gc, PM_ERR_INVALID, "null params / output");
    if (p->passes < 1 || p->paths_per_pass < 1) FAIL(gc, PM_ERR_INVALID, "passes and paths_per_pass must be >= 1");
    const int64_t P = p->paths_per_pass, mpc = p->max_photon_count;
    const int64_t chunk = (P + n - 1) / n;                 /* paths per device (the last one may trace fewer) */
    const int64_t total_slots = chunk * n * mpc;
    const size_t chunk_bytes = (size_t)(chunk * mpc) * sizeof(pm_photon);
    int rc;
    auto sub_fail = [&](Ctx *sub, int code) { return group_fail(gc, sub, code); };
    std::vector<pm_photon *> slots(n);
    for (int d = 0; d < n; ++d) {
        Ctx *c = G.subs[d];
        (void)hipSetDevice(c->device);
        if ((rc = pm_eye_pass(c, p, nullptr))) return sub_fail(c, rc);
        if ((rc = pm_reserve_slots(c, total_slots, (void **)&slots[d]))) return sub_fail(c, rc);
    }
    Ctx *c0 = G.subs[0];
    const int64_t nrec = c0->nrec;
    const int64_t unit = c0->pinhole ? (int64_t)((c0->W + 7) / 8) * 64 : 512;
    const auto bands = device_bands(nrec, unit, n);
    int64_t nvalid = 0;
    double t_trace = 0, t_build = 0, t_gather = 0;
    for (int pass = 0; pass < p->passes; ++pass) {
        for (int d = 0; d < n; ++d) {
            Ctx *c = G.subs[d];
            (void)hipSetDevice(c->device);
            const int64_t b = d * chunk, cnt = std::max<int64_t>(0, std::min(chunk, P - b));
            if (cnt > 0 && (rc = pm_trace_photons(c, p, pass, b, cnt, 0, nullptr))) return sub_fail(c, rc);
            if (cnt < chunk) /* padding slots of a short shard: invalid */
                HIPCHK(gc, hipMemsetAsync(slots[d] + (b + cnt) * mpc, 0, (size_t)((chunk - cnt) * mpc) * sizeof(pm_photon),
                                          c->stream));
        }
        /* all-gather of the shards: every buffer gets every device's chunk */
        if (!G.comms.empty()) {
            if (ncclGroupStart() != ncclSuccess) FAIL(gc, PM_ERR_HIP, "ncclGroupStart");
            for (int d = 0; d < n; ++d) {
                Ctx *c = G.subs[d];
                (void)hipSetDevice(c->device);
                const ncclResult_t r = ncclAllGather((const char *)slots[d] + d * chunk_bytes, slots[d], chunk_bytes,
                                                     ncclUint8, G.comms[d], c->stream);
                if (r != ncclSuccess) { (void)ncclGroupEnd(); FAIL(gc, PM_ERR_HIP, "ncclAllGather: %s", ncclGetErrorString(r)); }
            }
            if (ncclGroupEnd() != ncclSuccess) FAIL(gc, PM_ERR_HIP, "ncclGroupEnd");
        } else if (n > 1) {
            for (int d = 0; d < n; ++d) {
                (void)hipSetDevice(G.subs[d]->device);
                HIPCHK(gc, hipEventRecord(G.ev[d], G.subs[d]->stream));
            }
            for (int d = 0; d < n; ++d) {
                Ctx *c = G.subs[d];
                (void)hipSetDevice(c->device);
                for (int q = 0; q < n; ++q) {
                    if (q == d) continue;
                    HIPCHK(gc, hipStreamWaitEvent(c->stream, G.ev[q], 0));
                    HIPCHK(gc, hipMemcpyPeerAsync((char *)slots[d] + q * chunk_bytes, c->device,
                                                  (const char *)slots[q] + q * chunk_bytes, G.subs[q]->device,
                                                  chunk_bytes, c->stream));
                }
            }
        }
        for (int d = 0; d < n; ++d) {
            Ctx *c = G.subs[d];
            (void)hipSetDevice(c->device);
            if ((rc = pm_build_photon_map(c, p, total_slots, nullptr))) {
                if (rc == PM_ERR_NO_PHOTONS) FAIL(gc, PM_ERR_NO_PHOTONS, "0 valid photons (photonmappingrenderer.cpp:165-167)");
                return sub_fail(c, rc);
            }
        }
        (void)hipSetDevice(c0->device);
        if ((rc = valid_photons(gc, c0, p, nvalid))) return rc;
        for (int d = 0; d < n; ++d) {
            Ctx *c = G.subs[d];
            (void)hipSetDevice(c->device);
            for (const auto &bc : bands[d])
                if ((rc = pm_gather_range(c, p, bc.first, bc.second, nullptr))) return sub_fail(c, rc);
        }
        /* the next pass overwrites the slot buffers the peers read */
        for (int d = 0; d < n; ++d) { (void)hipSetDevice(G.subs[d]->device); HIPCHK(gc, hipStreamSynchronize(G.subs[d]->stream)); }
        /* stage times of the slowest device, read once the pass is done (a
         * read inside the loops would wait for one device before the next
         * one's launch) */
        double tt = 0, tb = 0, tg = 0;
        for (int d = 0; d < n; ++d) {
            Ctx *c = G.subs[d];
            if (std::min(chunk, P - d * chunk) > 0) tt = std::max(tt, timer_ms(c, "trace"));
            tb = std::max(tb, timer_ms(c, "build"));
            if (!bands[d].empty()) tg = std::max(tg, timer_ms(c, "gather", bands[d].size()));
        }
        t_trace += tt; t_build += tb; t_gather += tg;
    }
    /* final radiance of each device's bands, straight into the host image */
    const double emitted = (double)P * p->passes;
    const int64_t nout = c0->pinhole ? (int64_t)c0->W * c0->H : nrec;
    /* with a film the bands assemble the sample raster on the host first; it
     * is filmed on the first device below */
    const bool film = has_film(c0);
    std::vector<float> raster;
    float *const img_rgb = out_rgb;
    if (film) { raster.resize((size_t)nout * 3); out_rgb = raster.data(); }
    for (int d = 0; d < n; ++d) {
        Ctx *c = G.subs[d];
        (void)hipSetDevice(c->device);
        if ((rc = materialize_reset(c, c->stream))) return sub_fail(c, rc);
        HIPCHK(gc, c->d_out.ensure(nout * 3 * sizeof(float)));
        for (const auto &bc : bands[d]) {
            FinalParams F = final_params(c, emitted, bc.first, bc.second,
                                         c->pinhole ? c->d_out.as<float>() : c->d_out.as<float>() + 3 * bc.first);
            F.raster = c->pinhole;
            HIPCHK(gc, launch_final(F, c->stream));
            int64_t o0 = bc.first, o1 = bc.first + bc.second; /* output elements of the band */
            if (c->pinhole) {
                const int64_t t0 = bc.first / unit, t1 = (bc.first + bc.second + unit - 1) / unit; /* tile rows */
                o0 = std::min<int64_t>(8 * t0, c->H) * c->W;
                o1 = std::min<int64_t>(8 * t1, c->H) * c->W;
            }
            if (o1 > o0)
                HIPCHK(gc, hipMemcpyAsync(out_rgb + 3 * o0, c->d_out.as<float>() + 3 * o0, (size_t)(o1 - o0) * 3 * sizeof(float),
                                          hipMemcpyDeviceToHost, c->stream));
        }
    }
    for (int d = 0; d < n; ++d) { (void)hipSetDevice(G.subs[d]->device); HIPCHK(gc, hipStreamSynchronize(G.subs[d]->stream)); }
    if (film) {
        (void)hipSetDevice(c0->device);
        HIPCHK(gc, hipMemcpyAsync(c0->d_out.p, raster.data(), raster.size() * sizeof(float), hipMemcpyHostToDevice, c0->stream));
        if ((rc = deliver_image(c0, nout, img_rgb))) return sub_fail(c0, rc);
    }
    if (st) {
        (void)hipSetDevice(c0->device);
        if ((rc = render_stats(gc, c0, emitted, nvalid, st))) return rc;
        st->ms_eye = timer_ms(c0, "eye"); st->ms_trace = t_trace; st->ms_build = t_build; st->ms_gather = t_gather;
    }
    return PM_OK;
}

int pm_render(void *ptr, const pm_render_params *p, float *out_rgb, pm_stats *st) {
    if (group_of(ptr)) return group_render((Ctx *)ptr, p, out_rgb, st);
    GETCTX(ptr);
    int rc;
    if ((rc = check_params(c, p))) return rc;
    if (!out_rgb) FAIL(c, PM_ERR_INVALID, "null output");
    if (p->passes < 1 || p->paths_per_pass < 1) FAIL(c, PM_ERR_INVALID, "passes and paths_per_pass must be >= 1");
    hipStream_t s = c->stream;
    double t_eye = 0, t_trace = 0, t_build = 0, t_gather = 0, t_final = 0;
    if ((rc = pm_eye_pass(c, p, s))) return rc;
    t_eye = timer_ms(c, "eye");
    int64_t nvalid = 0;
    int64_t counters[2] = {0, 0};
    for (int pass = 0; pass < p->passes; ++pass) {
        if ((rc = pm_trace_photons(c, p, pass, 0, p->paths_per_pass, 0, s))) return rc;
        t_trace += timer_ms(c, "trace");
        if ((rc = pm_build_photon_map(c, p, p->paths_per_pass * p->max_photon_count, s))) return rc;
        t_build += timer_ms(c, "build");
        if ((rc = valid_photons(c, c, p, nvalid))) return rc;
        if ((rc = pm_gather(c, p, s))) return rc;
        t_gather += timer_ms(c, "gather");
        if (c->counting) {
            unsigned long long hc[2];
            HIPCHK(c, hipMemcpy(hc, c->d_counters.p, 16, hipMemcpyDeviceToHost));
            counters[0] = (int64_t)hc[0]; counters[1] = (int64_t)hc[1];
        }
    }
    const double emitted = (double)p->paths_per_pass * p->passes;
    const int64_t nout = c->pinhole ? (int64_t)c->W * c->H : c->nrec;
    HIPCHK(c, c->d_out.ensure(nout * 3 * sizeof(float)));
    FinalParams F = final_params(c, emitted, 0, c->nrec, c->d_out.as<float>());
    F.raster = c->pinhole;
    timer_begin(c, "final", s);
    HIPCHK(c, launch_final(F, s));
    timer_end(c, "final", s);
    if ((rc = deliver_image(c, nout, out_rgb))) return rc;
    t_final = timer_ms(c, "final");
    if (st) {
        if ((rc = render_stats(c, c, emitted, nvalid, st))) return rc;
        st->nodes_visited = counters[0];
        st->photons_in_radius = counters[1];
        st->ms_eye = t_eye; st->ms_trace = t_trace; st->ms_build = t_build; st->ms_gather = t_gather;
        st->ms_final = t_final;
    }
    return PM_OK;
}

/* ------------------------------------------------------- simple renderer */
int pm_simple_pass(void *ptr, const pm_render_params *p, void *d_out, void *stream) {
    GETCTX(ptr);
    if (!p) FAIL(c, PM_ERR_INVALID, "null params");
    if (!c->committed) FAIL(c, PM_ERR_INVALID, "scene not committed (call pm_commit)");
    if (!d_out) FAIL(c, PM_ERR_INVALID, "null output");
    const int64_t n = num_records(c);
    if (n <= 0) FAIL(c, PM_ERR_INVALID, "no eye samples (call pm_set_pinhole or pm_set_eye_rays)");
    if (!c->pinhole && c->rand2d_total > c->n2d)
        FAIL(c, PM_ERR_INVALID, "eye rays carry %d 2D samples, lights need %d", c->n2d, c->rand2d_total);
    hipStream_t s = pick(c, stream);
    EyeParams E{};
    E.S = c->S;
    E.R.count = n; /* the simple renderer keeps no records */
    eye_camera(c, E);
    E.rays = c->d_rays.as<float>(); E.rand2d = c->d_rand2d.as<float>();
    E.eps = p->scene_epsilon; E.light_seed = p->light_rng_seed;
    timer_begin(c, "simple", s);
    HIPCHK(c, launch_simple(E, (float *)d_out, s));
    timer_end(c, "simple", s);
    return PM_OK;
}

int pm_render_simple(void *ptr, const pm_render_params *p, float *out_rgb, pm_stats *st) {
    if (Group *g_ = group_of(ptr)) { /* direct light only: one device renders it */
        const int rc_ = pm_render_simple(g_->subs[0], p, out_rgb, st);
        return rc_ ? group_fail(ptr, g_->subs[0], rc_) : PM_OK;
    }
    GETCTX(ptr);
    if (!out_rgb) FAIL(c, PM_ERR_INVALID, "null output");
    const int64_t nout = c->pinhole ? (int64_t)c->W * c->H : c->nrays;
    if (nout > 0) HIPCHK(c, c->d_out.ensure(nout * 3 * sizeof(float)));
    hipStream_t s = c->stream;
    int rc;
    if ((rc = pm_simple_pass(c, p, c->d_out.p, s))) return rc;
    if ((rc = deliver_image(c, nout, out_rgb))) return rc;
    if (st) {
        std::memset(st, 0, sizeof(*st));
        st->gather_points = nout;
        st->ms_eye = timer_ms(c, "simple");
    }
    return PM_OK;
}

/* ------------------------------------------------------- buffers / tests */
int64_t pm_num_records(void *ptr) {
    if (Group *g_ = group_of(ptr)) return pm_num_records(g_->subs[0]);
    Ctx *c = (Ctx *)ptr;
    return c ? num_records(c) : -1;
}

int pm_record_pixel(void *ptr, int64_t r, int64_t *pixel) {
    GETCTX(ptr);
    if (!pixel) FAIL(c, PM_ERR_INVALID, "null output");
    if (!c->pinhole) { *pixel = r; return PM_OK; }
    int64_t tile = r >> 6;
    int lane = (int)(r & 63), tilesX = (c->W + 7) / 8;
    int px = (int)(tile % tilesX) * 8 + (lane & 7), py = (int)(tile / tilesX) * 8 + (lane >> 3);
    *pixel = (px >= c->W || py >= c->H) ? -1 : (int64_t)py * c->W + px;
    return PM_OK;
}

int pm_download_slots(void *ptr, pm_photon *out, int64_t n) {
    GETCTX(ptr);
    int rc;
    if (!out || n < 0 || (size_t)n * sizeof(pm_photon) > c->d_slots.bytes) FAIL(c, PM_ERR_INVALID, "bad slot range");
    if ((rc = materialize_slots(c, nullptr))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->d_slots.p, n * sizeof(pm_photon), hipMemcpyDeviceToHost));
    return PM_OK;
}

int pm_upload_slots(void *ptr, const pm_photon *in, int64_t n) {
    GETCTX(ptr);
    int rc;
    if (!in || n < 0) FAIL(c, PM_ERR_INVALID, "bad slots");
    if ((rc = materialize_slots(c, nullptr))) return rc;
    if ((rc = pm_reserve_slots(c, n, nullptr))) return rc;
    c->fused.valid = false;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->d_slots.p, in, n * sizeof(pm_photon), hipMemcpyHostToDevice));
    c->slots_used = n;
    c->slots_nonneg = true;
    for (int64_t i = 0; i < n && c->slots_nonneg; ++i)
        if (in[i].bits & 1u) /* valid photon */
            c->slots_nonneg = in[i].alpha[0] >= 0.f && in[i].alpha[1] >= 0.f && in[i].alpha[2] >= 0.f;
    return PM_OK;
}

int pm_download_records(void *ptr, pm_record *out, int64_t n) {
    GETCTX(ptr);
    if (!out || n < 0 || n > c->nrec) FAIL(c, PM_ERR_INVALID, "bad record range");
    int rc;
    if ((rc = materialize_reset(c, c->stream))) return rc;
    HIPCHK(c, hipDeviceSynchronize());
    std::vector<float4> pos(n), nrm(n), st(n), dl(n);
    std::vector<float> N(n);
    HIPCHK(c, hipMemcpy(pos.data(), c->d_pos.p, n * 16, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(nrm.data(), c->d_nrm.p, n * 16, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(st.data(), c->d_state.p, n * 16, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(dl.data(), c->d_dl.p, n * 16, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(N.data(), c->d_n.p, n * 4, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) {
        pm_record &r = out[i];
        r.pos[0] = pos[i].x; r.pos[1] = pos[i].y; r.pos[2] = pos[i].z; r.flags = (uint32_t)fbits_h(pos[i].w);
        r.ns[0] = nrm[i].x; r.ns[1] = nrm[i].y; r.ns[2] = nrm[i].z; r.material = fbits_h(nrm[i].w);
        r.flux[0] = st[i].x; r.flux[1] = st[i].y; r.flux[2] = st[i].z; r.radius2 = st[i].w;
        r.dl[0] = dl[i].x; r.dl[1] = dl[i].y; r.dl[2] = dl[i].z; r.photon_count = N[i];
    }
    return PM_OK;
}

int pm_upload_records(void *ptr, const pm_record *in, int64_t n) {
    GETCTX(ptr);
    int rc;
    if (!in || n != num_records(c)) FAIL(c, PM_ERR_INVALID, "record count must equal pm_num_records");
    if ((rc = ensure_records(c))) return rc;
    std::vector<float4> pos(n), nrm(n), st(n), dl(n);
    std::vector<float> N(n);
    for (int64_t i = 0; i < n; ++i) {
        const pm_record &r = in[i];
        pos[i] = f4(r.pos[0], r.pos[1], r.pos[2], ibits((int)r.flags));
        nrm[i] = f4(r.ns[0], r.ns[1], r.ns[2], ibits(r.material));
        st[i] = f4(r.flux[0], r.flux[1], r.flux[2], r.radius2);
        dl[i] = f4(r.dl[0], r.dl[1], r.dl[2], 0.f);
        N[i] = r.photon_count;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->d_pos.p, pos.data(), n * 16, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_nrm.p, nrm.data(), n * 16, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_state.p, st.data(), n * 16, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_dl.p, dl.data(), n * 16, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_n.p, N.data(), n * 4, hipMemcpyHostToDevice));
    c->rec_fresh = false; /* every record overwritten */
    c->tiles.invalidate();
    c->grid_plan.invalidate();
    if (c->view_active && (rc = build_view(c, c->stream))) return rc;
    return PM_OK;
}

int pm_download_record_albedo(void *ptr, float *out_rgb, int64_t n) {
    GETCTX(ptr);
    if (!out_rgb) FAIL(c, PM_ERR_INVALID, "pm_download_record_albedo: null pointer");
    if (!c->committed || !c->albedo())
        FAIL(c, PM_ERR_INVALID, "pm_download_record_albedo: the committed scene has no textured material and none of the physical specular model");
    if (n < 0 || n > c->nrec || !c->d_rkd.p) FAIL(c, PM_ERR_INVALID, "bad record range");
    if (int rc = materialize_reset(c, c->stream)) return rc; /* as pm_download_records does */
    HIPCHK(c, hipDeviceSynchronize());
    std::vector<float4> kd((size_t)n);
    HIPCHK(c, hipMemcpy(kd.data(), c->d_rkd.p, (size_t)n * 16, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) { out_rgb[3 * i] = kd[i].x; out_rgb[3 * i + 1] = kd[i].y; out_rgb[3 * i + 2] = kd[i].z; }
    return PM_OK;
}

int pm_upload_record_albedo(void *ptr, const float *in_rgb, int64_t n) {
    GETCTX(ptr);
    if (!in_rgb) FAIL(c, PM_ERR_INVALID, "pm_upload_record_albedo: null pointer");
    if (!c->committed || !c->albedo())
        FAIL(c, PM_ERR_INVALID, "pm_upload_record_albedo: the committed scene has no textured material and none of the physical specular model");
    /* no record changes: the tile list and the grid plan stay (ensure_records would drop them) */
    if (n != c->nrec || !c->d_rkd.p || (size_t)n * sizeof(float4) > c->d_rkd.bytes)
        FAIL(c, PM_ERR_INVALID, "pm_upload_record_albedo: %lld values for %lld records (run pm_eye_pass or pm_upload_records first)",
             (long long)n, (long long)c->nrec);
    std::vector<float4> kd((size_t)n);
    for (int64_t i = 0; i < n; ++i) kd[i] = f4(in_rgb[3 * i], in_rgb[3 * i + 1], in_rgb[3 * i + 2], 0.f);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->d_rkd.p, kd.data(), (size_t)n * 16, hipMemcpyHostToDevice));
    return PM_OK;
}

int64_t pm_kdtree_nodes(void *ptr) {
    Ctx *c = (Ctx *)ptr;
    return c ? c->kd_count : -1;
}

int pm_download_kdtree(void *ptr, pm_photon *out, int64_t n) {
    GETCTX(ptr);
    if (!out || n < 0 || n > c->kd_count) FAIL(c, PM_ERR_INVALID, "bad kd range");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->d_kd.p, n * sizeof(pm_photon), hipMemcpyDeviceToHost));
    return PM_OK;
}

int pm_gather_counters(void *ptr, int64_t out[4]) {
    GETCTX(ptr);
    unsigned long long h[4];
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h, c->d_counters.p, 32, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) out[i] = (int64_t)h[i];
    return PM_OK;
}

int pm_trace_counters(void *ptr, int64_t out[4]) {
    GETCTX(ptr);
    unsigned long long h[4];
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h, c->d_counters.as<unsigned long long>() + 4, 32, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) out[i] = (int64_t)h[i];
    return PM_OK;
}

int pm_map_info(void *ptr, int64_t out[4]) {
    GETCTX(ptr);
    if (!out) FAIL(c, PM_ERR_INVALID, "null output");
    out[0] = c->map_kind; out[1] = 0; out[2] = c->map_slots; out[3] = 0;
    if (c->map_kind == PM_GATHER_KDTREE) {
        out[1] = c->kd_count;
    } else if (c->map_kind == PM_GATHER_GRID) {
        uint32_t nv = 0;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(&nv, c->d_cell_start.as<uint32_t>() + c->grid.ncells, 4, hipMemcpyDeviceToHost));
        out[1] = nv;
        out[3] = c->grid.ncells;
    }
    return PM_OK;
}

int pm_scene_info(void *ptr, int64_t out[7]) {
    if (Group *g_ = group_of(ptr)) return pm_scene_info(g_->subs[0], out);
    GETCTX(ptr);
    if (!c->S.blob) FAIL(c, PM_ERR_INVALID, "no scene committed");
    const SceneDev &S = c->S;
    out[0] = c->hs.next_tri_id;   /* triangles rendered: meshes + every instance's */
    out[1] = S.n_disks; out[2] = S.n_spheres;
    /* the tree the kernels traverse: the 4-wide BVH when the scene has one
     * (either builder), else the binary SAH tree */
    out[3] = S.wide ? c->bvh4_nodes : S.n_nodes;
    out[4] = S.wide ? c->bvh4_depth : c->bvh_depth;
    out[5] = scene_mode(S) == MODE_BRUTE ? 2 : scene_mode(S) == MODE_LDS ? 1 : scene_mode(S) == MODE_INST ? 3 : 0;
    out[6] = S.blob_bytes;
    return PM_OK;
}

int pm_scene_section(void *ptr, int section, void *out, int64_t max_bytes, int64_t *bytes) {
    if (Group *g_ = group_of(ptr)) return pm_scene_section(g_->subs[0], section, out, max_bytes, bytes);
    GETCTX(ptr);
    if (!c->S.blob) FAIL(c, PM_ERR_INVALID, "no scene committed");
    const SceneDev &S = c->S;
    const SceneLayout &L = c->L;
    const void *src = nullptr;
    int64_t n = 0;
    switch (section) {
    case PM_SCENE_REFS: src = S.refs; n = (int64_t)L.size[SEC_REFS]; break;
    case PM_SCENE_TRI_GEO: src = S.tri_geo; n = (int64_t)L.size[SEC_GEO]; break;
    case PM_SCENE_TRI_SHADE: src = S.tri_shade; n = (int64_t)L.size[SEC_SHADE]; break;
    case PM_SCENE_TRI_ID: src = S.tri_id; n = (int64_t)L.size[SEC_TID]; break;
    case PM_SCENE_TRI_INFO: src = S.tri_info; n = (int64_t)L.size[SEC_INFO]; break;
    case PM_SCENE_BVH4: src = S.wnodes; n = (int64_t)L.size[SEC_WNODES]; break; /* the wide tree, whichever format */
    case PM_SCENE_INSTANCES: src = S.insts; n = (int64_t)L.size[SEC_INSTS]; break;
    case PM_SCENE_OBJ_TRIS: src = S.obj_v; n = (int64_t)L.size[SEC_OBJV]; break;
    case PM_SCENE_LIGHT_TRIS: src = S.light_tris; n = (int64_t)(c->hs.light_tris.size() * sizeof(LightTri)); break;
    case PM_SCENE_LIGHT_CDF: src = c->d_light_cdf.p; n = (int64_t)(c->lsum.cdf.size() * sizeof(float)); break;
    case PM_SCENE_TEXTURES: src = S.tex_recs; n = c->textured ? (int64_t)(c->hs.textures.size() * sizeof(TexRec)) : 0; break;
    case PM_SCENE_MAT_TEX: src = S.mat_tex; n = c->albedo() ? (int64_t)(c->hs.materials.size() * sizeof(int)) : 0; break;
    case PM_SCENE_MAT_SPEC: src = S.mat_spec; n = c->specular ? (int64_t)(c->hs.materials.size() * 2 * sizeof(float4)) : 0; break;
    case PM_SCENE_WORLD_SPHERE: /* a host value */
        if (bytes) *bytes = (int64_t)sizeof c->world_sphere;
        if (out) {
            if (max_bytes < (int64_t)sizeof c->world_sphere) FAIL(c, PM_ERR_INVALID, "scene section needs 16 bytes");
            std::memcpy(out, c->world_sphere, sizeof c->world_sphere);
        }
        return PM_OK;
    default: FAIL(c, PM_ERR_INVALID, "unknown scene section %d", section);
    }
    if (bytes) *bytes = n;
    if (out && n > 0) {
        if (max_bytes < n) FAIL(c, PM_ERR_INVALID, "scene section needs %lld bytes", (long long)n);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(out, src, (size_t)n, hipMemcpyDeviceToHost));
    }
    return PM_OK;
}

int pm_trace_profile(void *ptr, int64_t out[8], int reset) {
    GETCTX(ptr);
    unsigned long long h[8];
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(h, c->d_counters.as<unsigned long long>() + 8, 64, hipMemcpyDeviceToHost));
    for (int i = 0; i < 8; ++i) out[i] = (int64_t)h[i];
    if (reset) HIPCHK(c, hipMemset(c->d_counters.as<unsigned long long>() + 8, 0, 64));
    return PM_OK;
}

int pm_final_view(void *ptr, double emitted, int64_t v_begin, int64_t v_count, void *d_out, void *stream) {
    GETCTX(ptr);
    if (!c->view_active) FAIL(c, PM_ERR_INVALID, "no active-record view (pm_set_record_view)");
    if (!d_out || v_begin < 0 || v_count < 0 || v_begin + v_count > c->n_view) FAIL(c, PM_ERR_INVALID, "bad view range");
    hipStream_t s = pick(c, stream);
    int rc;
    if ((rc = materialize_reset(c, s))) return rc;
    FinalParams F = final_params(c, emitted, v_begin, v_count, (float *)d_out);
    F.view = c->d_vlist.as<uint32_t>();
    timer_begin(c, "final", s);
    HIPCHK(c, launch_final(F, s));
    timer_end(c, "final", s);
    return PM_OK;
}

int pm_record_view_list(void *ptr, void *d_out, void *stream) {
    GETCTX(ptr);
    if (!c->view_active) FAIL(c, PM_ERR_INVALID, "no active-record view (pm_set_record_view)");
    if (!d_out) FAIL(c, PM_ERR_INVALID, "null output");
    if (c->n_view > 0)
        HIPCHK(c, hipMemcpyAsync(d_out, c->d_vlist.p, (size_t)c->n_view * 4, hipMemcpyDeviceToDevice, pick(c, stream)));
    return PM_OK;
}

int pm_set_record_view(void *ptr, int active_only, int64_t *n_view) {
    GETCTX(ptr);
    if (active_only) {
        if (c->nrec <= 0) FAIL(c, PM_ERR_INVALID, "no records (run pm_eye_pass first)");
        int rc;
        HIPCHK(c, hipDeviceSynchronize());
        if ((rc = build_view(c, c->stream))) return rc;
    }
    c->view_active = active_only != 0;
    if (n_view) *n_view = view_size(c);
    return PM_OK;
}

int pm_set_counting(void *ptr, int enabled) {
    GETCTX(ptr);
    c->counting = enabled != 0;
    return PM_OK;
}

int pm_set_stage_timing(void *ptr, const char *stages) {
    GETCTX(ptr);
    if (c->stage_active) FAIL(c, PM_ERR_INVALID, "stage timing changed inside a stage");
    c->timed_stages = stages ? stages : "";
    return PM_OK;
}

int pm_synchronize(void *ptr) {
    GROUP_FWD(ptr, pm_synchronize(sub));
    GETCTX(ptr);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PM_OK;
}

int pm_last_kernel_ms(void *ptr, const char *name, double *ms) {
    GETCTX(ptr);
    if (!name || !ms) FAIL(c, PM_ERR_INVALID, "null argument");
    *ms = timer_ms(c, name);
    if (*ms < 0) FAIL(c, PM_ERR_INVALID, "no timing recorded for '%s'", name);
    return PM_OK;
}

int pm_timing_reset(void *ptr) {
    GETCTX(ptr);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (auto &kv : c->timers) kv.second.used = 0;
    return PM_OK;
}

int pm_timing_total(void *ptr, const char *name, int64_t *count, double *total_ms) {
    GETCTX(ptr);
    if (!name || !count || !total_ms) FAIL(c, PM_ERR_INVALID, "null argument");
    *count = 0;
    *total_ms = 0.0;
    auto it = c->timers.find(name);
    if (it == c->timers.end()) return PM_OK;
    for (size_t i = 0; i < it->second.used; ++i) {
        double ms = pair_ms(it->second.ev[i]);
        if (ms < 0) FAIL(c, PM_ERR_HIP, "event timing failed for '%s'", name);
        *total_ms += ms;
    }
    *count = (int64_t)it->second.used;
    return PM_OK;
}

int pm_reset_records(void *ptr, const pm_render_params *p, void *stream) {
    GETCTX(ptr);
    int rc;
    if ((rc = check_params(c, p))) return rc;
    if (c->nrec <= 0) FAIL(c, PM_ERR_INVALID, "no records (run pm_eye_pass first)");
    (void)stream;
    /* deferred: the next fused full gather starts from the initial state, any
     * other reader applies it first (materialize_reset) */
    c->rec_fresh = true;
    c->rec_fresh_r2 = p->initial_radius2;
    c->grid_plan.invalidate();
    return PM_OK;
}

} /* extern "C" */
