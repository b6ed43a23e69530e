/*
 * pm_api.cpp — the C-ABI of libpmhip.so (declared in include/pm_api.h), the
 * unit of the context: create / destroy, the last error, the stage timers
 * (and the g_stage the launches read), counters, scene / map info and the
 * diagnostic calls, pm_default_params and the small pure exports. The scene
 * calls and pm_commit are in pm_api_scene.cpp, the stages in
 * pm_api_records.cpp, pm_api_photons.cpp, pm_api_gather.cpp and
 * pm_api_fgather.cpp, the whole renders in pm_api_render.cpp; pm_ctx.h holds
 * what they share. Host code only; the kernels live in the .hip files
 * (launchers in pm_kernels.h). No CPU fallback: every compute entry point
 * launches HIP kernels and fails with PM_ERR_HIP when the device is unusable.
 */
#include "pm_ctx.h"

std::string g_last_error;
thread_local pm::StageEvents *pm::g_stage = nullptr;

/* Every stage launch takes a fresh event pair from a per-stage pool. Kernel
 * stages bind the pair to their own dispatches (pm_launch, pm_kernels.h):
 * no marker packets, so timing leaves no idle gap between kernels. A stage
 * of host work / copies (marker = true) records the pair as markers.
 * Nothing synchronizes until a reader asks. */
static bool stage_timed(const Ctx *c, const char *name) {
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
int timer_begin(Ctx *c, const char *name, hipStream_t s, bool marker) {
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
static double pair_ms(const Timer &t) {
    (void)hipEventSynchronize(t.b);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, t.a, t.b) != hipSuccess) return -1.0;
    return ms;
}
/* duration of the most recent launch of a stage (k > 1: the sum of the last k) */
double timer_ms(Ctx *c, const char *name, size_t k) {
    auto it = c->timers.find(name);
    if (it == c->timers.end() || it->second.used == 0) return -1.0;
    double ms = 0;
    for (size_t i = it->second.used - std::min(k, it->second.used); i < it->second.used; ++i) ms += pair_ms(it->second.ev[i]);
    return ms;
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
    if (const char *e = getenv("PM_TRACE_CUS")) c->trace_cus = std::max(1, atoi(e));
    if (const char *e = getenv("PM_KD_STACK")) c->kd_stack = std::max(1, std::min(KD_STACK, atoi(e)));
    if (const char *e = getenv("PM_FG_CHUNK")) c->fg_chunk = std::max<long long>(1, atoll(e));
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
    /* the record sets, bucket maps and tile list release their own; these belong to no struct */
    DevBuf *bufs[] = {&c->d_scene, &c->d_rays, &c->d_rand2d, &c->d_slots, &c->d_vflags, &c->d_vrank, &c->d_vlist, &c->d_vsums,
                      &c->d_tile_times, &c->d_kd, &c->d_out, &c->d_counters, &c->d_hist, &c->d_spill, &c->d_light_tris,
                      &c->d_light_cdf, &c->d_film_table, &c->d_img, &c->d_tex_recs, &c->d_texels, &c->d_mat_tex, &c->d_tri_uv,
                      &c->d_rkd, &c->d_mat_spec, &c->d_fg_li, &c->d_fg_sum};
    for (DevBuf *b : bufs) b->release();
    c->rec.release(); c->fg_rec.release();
    c->map.release(); c->cmap.release();
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

int64_t pm_kdtree_nodes(void *ptr) {
    Ctx *c = (Ctx *)ptr;
    return c ? c->kd_count : -1;
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
    out[0] = c->map_kind; out[1] = 0; out[2] = c->map.slots; out[3] = 0;
    if (c->map_kind == PM_GATHER_KDTREE) {
        out[1] = c->kd_count;
    } else if (c->map_kind == PM_GATHER_GRID) {
        uint32_t nv = 0;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, c->map.valid_photons(&nv));
        out[1] = nv;
        out[3] = c->map.grid.ncells;
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

} /* extern "C" */
