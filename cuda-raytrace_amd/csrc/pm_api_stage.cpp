/*
 * pm_api_stage.cpp — the stage half of the C-ABI: the eye pass, the slot
 * buffer calls, pm_trace_photons (its launch planned by pm_plan.cpp's
 * plan_trace), pm_build_photon_map (the grid each pass gets planned by
 * pm_plan.cpp's R2Plan), the steps of a gather and its entry points, the PPM
 * update and radius calls, pm_final*, the record view, the deferred reset and
 * the record / slot / kd-tree / albedo transfers.
 */
#include "pm_ctx.h"

namespace {

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
    c->fg_passes = 0; /* new primary records: the final-gather sums are another record set's */
    c->cg_passes = 0; /* ... and so are the caustic gather's */
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

/* the parameter block of an eye pass over the context's records (pass 0) */
EyeParams eye_params(Ctx *c, const pm_render_params *p) {
    EyeParams E{};
    E.S = c->S;
    E.R = recs(c);
    eye_camera(c, E);
    E.rays = c->d_rays.as<float>(); E.rand2d = c->d_rand2d.as<float>();
    E.eps = p->scene_epsilon; E.r2init = p->initial_radius2; E.max_spec = p->max_specular_depth;
    E.light_seed = p->light_rng_seed;
    E.kd = c->albedo() ? c->d_rkd.as<float4>() : nullptr;
    return E;
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

} // namespace

/* the final pass over records [begin, begin + count) into out, one radiance
 * per record in record order (callers set raster / view for another layout) */
FinalParams final_params(Ctx *c, double emitted, int64_t begin, int64_t count, float *out) {
    FinalParams F{};
    F.R = recs(c);
    F.knn = c->rec_estimator == PM_ESTIMATOR_KNN; F.materials = c->S.materials;
    F.emitted = (float)emitted; /* gContext["emittingPhotons"]->setFloat((float)totalPhotons) */
    F.rec_begin = begin; F.rec_count = count; F.out = out; F.raster = 0; F.W = c->W;
    F.kd = c->albedo() ? c->d_rkd.as<float4>() : nullptr;
    /* records of a resampled render (pm_eye_resample: PPM, no albedo): dl sums eye_samples samples */
    if (c->eye_samples > 1) { F.n_eye = c->eye_samples; F.resampled = 1; }
    return F;
}

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

extern "C" {

/* ------------------------------------------------------------- stages */
int pm_eye_pass(void *ptr, const pm_render_params *p, void *stream) {
    GETCTX(ptr);
    int rc;
    if ((rc = check_params(c, p))) return rc;
    if ((rc = ensure_records(c))) return rc;
    if (!c->pinhole && c->rand2d_total > c->n2d)
        FAIL(c, PM_ERR_INVALID, "eye rays carry %d 2D samples, lights need %d", c->n2d, c->rand2d_total);
    hipStream_t s = pick(c, stream);
    const EyeParams E = eye_params(c, p);
    timer_begin(c, "eye", s);
    HIPCHK(c, launch_eye(E, s));
    timer_end(c, "eye", s);
    c->rec_fresh = false; /* the eye pass writes every record */
    c->eye_samples = 1;
    c->tiles.invalidate();
    c->grid_plan.invalidate();
    if (c->view_active && (rc = build_view(c, s))) return rc;
    return PM_OK;
}

int pm_eye_resample(void *ptr, const pm_render_params *p, int pass, void *stream) {
    /* what needs no context is checked before the context is */
    if (!p) FAIL((Ctx *)ptr, PM_ERR_INVALID, "pm_eye_resample: null params");
    if (pass < 0) FAIL((Ctx *)ptr, PM_ERR_INVALID, "pm_eye_resample: pass %d is negative", pass);
    GETCTX(ptr);
    int rc;
    if ((rc = check_params(c, p))) return rc;
    if (!c->camera) FAIL(c, PM_ERR_INVALID, "pm_eye_resample: needs the device camera (pm_set_camera)");
    if (c->cam.xsamples != 1 || c->cam.ysamples != 1)
        FAIL(c, PM_ERR_INVALID, "pm_eye_resample: the camera has %d x %d samples per pixel; the passes are the samples (1 x 1)",
             c->cam.xsamples, c->cam.ysamples);
    if (real_filter(c->cam.filter))
        FAIL(c, PM_ERR_INVALID, "pm_eye_resample: the camera has a pixel filter; a record is one pixel (PM_FILTER_NONE)");
    if (p->estimator != PM_ESTIMATOR_PPM)
        FAIL(c, PM_ERR_INVALID, "pm_eye_resample: PM_ESTIMATOR_PPM only (the kNN final applies the Kd of the record's current material)");
    if (c->albedo())
        FAIL(c, PM_ERR_INVALID, "pm_eye_resample: the scene has a textured or physically specular material, whose factor "
                                "pm_final applies once per record: wrong when the hit moves");
    if (pass == 0) return pm_eye_pass(ptr, p, stream);
    if (c->eye_samples < 1 || c->nrec <= 0 || c->nrec != num_records(c))
        FAIL(c, PM_ERR_INVALID, "pm_eye_resample: pass %d before any eye pass wrote this camera's records (pass 0 or pm_eye_pass first)", pass);
    hipStream_t s = pick(c, stream);
    if ((rc = materialize_reset(c, s))) return rc;
    EyeParams E = eye_params(c, p);
    E.pass = (uint32_t)pass;
    timer_begin(c, "eye", s);
    HIPCHK(c, launch_eye_resample(E, s));
    timer_end(c, "eye", s);
    ++c->eye_samples;
    c->fg_passes = 0;
    c->cg_passes = 0;
    c->tiles.invalidate(); /* the flags moved with the hits */
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
    if (c->caustic_map) { /* pm_set_caustic_map: what a marked trace refuses */
        if (p->gather_structure == PM_GATHER_KDTREE)
            FAIL(c, PM_ERR_INVALID, "pm_trace_photons: the caustic map is on and gather_structure is PM_GATHER_KDTREE; the "
                                    "kd-tree build owns the photons' bits word (PM_GATHER_GRID)");
        if (c->albedo())
            FAIL(c, PM_ERR_INVALID, "pm_trace_photons: the caustic map is on and the scene has a textured or physically "
                                    "specular material (final gathering takes neither)");
    }
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
    /* the launch's geometry, decided once (pm_plan.h plan_trace): what the
     * kernel reads of it goes into T, the rest to launch_trace */
    TraceShape sh;
    sh.path_count = path_count; sh.mpc = (int)mpc; sh.slots_aligned = ((uintptr_t)T.slots & 15u) == 0u;
    sh.mode = scene_mode(c->S); sh.wide = c->S.wide; sh.stack_depth = c->S.stack_depth; sh.lds_bytes = c->S.lds_bytes;
    sh.pool_stack = c->pool_stack; sh.trace_pool = c->trace_pool; sh.trace_hold = c->trace_hold;
    sh.mark = c->caustic_map;
    if (c->S.wide && hipDeviceGetAttribute(&sh.cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess) sh.cus = 0;
    const TracePlan plan = plan_trace(sh, trace_waves_per_cu);
    T.hold = plan.hold; T.pool_stack = plan.lstk; T.pool_paths = plan.pool_paths;
    if (plan.spill_entries > 0) {
        HIPCHK(c, c->d_spill.ensure((size_t)plan.spill_stride * (size_t)plan.spill_entries * 4));
        T.spill = c->d_spill.as<int>();
        T.spill_stride = plan.spill_stride;
    }
    T.pass = pass; T.mpc = (int)mpc; T.max_spec = p->max_specular_depth; T.light_index = p->light_source_index;
    T.eps = p->scene_epsilon; T.seed = p->rng_seed;
    T.light_cdf = c->d_light_cdf.as<float>();
    T.mark = c->caustic_map ? 1 : 0;
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
    HIPCHK(c, launch_trace(T, plan, c->counting, s));
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

/* caustic: the scalar stream's pairs and handed-back tiles of the caustic map (G's map is pm_build_caustic_map's) */
static int gather_knn_setup(Ctx *c, const pm_render_params *p, GatherParams &G, bool caustic = false) {
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
        DevBuf &pk = caustic ? c->d_cg_knnpk : c->d_knnpk, &ovf = caustic ? c->d_cg_knnovf : c->d_knnovf;
        uint64_t &pack_gen = caustic ? c->cg_pack_gen : c->knn_pack_gen;
        void *&pack_ptr = caustic ? c->cg_pack_ptr : c->knn_pack_ptr;
        const uint64_t gen = caustic ? c->cg_gen : c->map_gen;
        const int64_t nph = (int64_t)((caustic ? c->d_cg_pha : c->d_pha).bytes / 16), pairs = (nph + 1) / 2 + 16;
        const int64_t ntiles = (G.rec_end - G.rec_begin + 63) / 64;
        HIPCHK(c, pk.ensure((size_t)pairs * 80));
        HIPCHK(c, ovf.ensure((size_t)(ntiles + KNN_OVF_HDR) * 4));
        G.knn_pk_p = pk.as<float4>();
        G.knn_pk_q = G.knn_pk_p + 2 * pairs;
        G.knn_pk_pairs = pairs;
        G.knn_pack = pack_gen != gen || pack_ptr != pk.p;
        pack_gen = gen;
        pack_ptr = pk.p;
        G.knn_ovf_n = ovf.as<uint32_t>();
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

int pm_download_kdtree(void *ptr, pm_photon *out, int64_t n) {
    GETCTX(ptr);
    if (!out || n < 0 || n > c->kd_count) FAIL(c, PM_ERR_INVALID, "bad kd range");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->d_kd.p, n * sizeof(pm_photon), hipMemcpyDeviceToHost));
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

/* ------------------------------------------------------- final gathering */
/* what pm_final_gather_pass and pm_final_gather_rays refuse alike */
static int fg_validate(Ctx *c, const pm_render_params *p, const char *fn) {
    int rc;
    if ((rc = check_params(c, p))) return rc;
    if (p->gather_structure != PM_GATHER_GRID)
        FAIL(c, PM_ERR_INVALID, "%s: the gather rays' kNN estimate runs on the photon buckets (PM_GATHER_GRID)", fn);
    if (p->knn_lookup < 1 || p->knn_lookup > PM_KNN_MAX)
        FAIL(c, PM_ERR_INVALID, "%s: knn_lookup must be in [1, %d]", fn, PM_KNN_MAX);
    if (c->eye_samples < 1 || c->nrec <= 0) FAIL(c, PM_ERR_INVALID, "%s: no records (run pm_eye_pass first)", fn);
    if (c->eye_samples > 1)
        FAIL(c, PM_ERR_INVALID, "%s: the records are pm_eye_resample's (%d eye samples); final gathering starts from one "
                                "eye pass", fn, c->eye_samples);
    if (c->albedo())
        FAIL(c, PM_ERR_INVALID, "%s: the scene has a textured or physically specular material; a secondary hit would "
                                "need its texel or throughput", fn);
    return PM_OK;
}

static FgParams fg_params(Ctx *c, const pm_render_params *p, int n_gather, int pass) {
    FgParams F{};
    F.S = c->S;
    F.P = recs(c);
    F.n_gather = n_gather;
    F.pass = (uint32_t)pass; F.light_seed = p->light_rng_seed;
    F.eps = p->scene_epsilon; F.r2init = p->initial_radius2; F.max_spec = p->max_specular_depth;
    return F;
}

#define FG_ARGS(fn)                                                                                              \
    if (!p) FAIL((Ctx *)ptr, PM_ERR_INVALID, fn ": null params");                                                \
    if (n_gather < 1 || n_gather > PM_FG_MAX)                                                                    \
        FAIL((Ctx *)ptr, PM_ERR_INVALID, fn ": n_gather %d outside 1..%d", n_gather, PM_FG_MAX);                 \
    if (pass < 0) FAIL((Ctx *)ptr, PM_ERR_INVALID, fn ": pass %d is negative", pass)

int pm_final_gather_pass(void *ptr, const pm_render_params *p, int n_gather, int pass, void *stream) {
    FG_ARGS("pm_final_gather_pass"); /* what needs no context is checked before the context is */
    GETCTX(ptr);
    int rc;
    if ((rc = fg_validate(c, p, __func__))) return rc;
    if (c->map_kind != PM_GATHER_GRID) FAIL(c, PM_ERR_INVALID, "pm_final_gather_pass: no photon map built on the buckets (pm_build_photon_map)");
    if (!same_grid(c->grid, pm::make_grid(c->bbox_lo, c->bbox_hi, PM_ESTIMATOR_KNN, c->cell_span, p->initial_radius2)))
        FAIL(c, PM_ERR_INVALID, "pm_final_gather_pass: the photon buckets were not built for PM_ESTIMATOR_KNN with this initial_radius2");
    if (pass > 0 && (c->fg_passes < 1 || c->fg_n != n_gather || c->fg_nrec != c->nrec))
        FAIL(c, PM_ERR_INVALID, "pm_final_gather_pass: pass %d continues no pass 0 of %d rays over these records", pass, n_gather);
    hipStream_t s = pick(c, stream);
    const int64_t N = n_gather, nrec = c->nrec;
    /* whole primary tiles per chunk, at least one */
    const int64_t chunk_recs = std::max<int64_t>(1, c->fg_chunk / (64 * N)) * 64;
    const int64_t cap = std::min(chunk_recs, (nrec + 63) / 64 * 64) * N;
    HIPCHK(c, c->d_fg_pos.ensure(cap * sizeof(float4)));
    HIPCHK(c, c->d_fg_nrm.ensure(cap * sizeof(float4)));
    HIPCHK(c, c->d_fg_state.ensure(cap * sizeof(float4)));
    HIPCHK(c, c->d_fg_n.ensure(cap * sizeof(float)));
    HIPCHK(c, c->d_fg_dl.ensure(cap * sizeof(float4)));
    HIPCHK(c, c->d_fg_li.ensure(cap * 3 * sizeof(float)));
    HIPCHK(c, c->d_fg_sum.ensure(nrec * sizeof(float4)));
    if (pass == 0) { c->fg_passes = 0; c->fg_n = n_gather; c->fg_nrec = nrec; }
    FgParams F = fg_params(c, p, n_gather, pass);
    F.R.pos = c->d_fg_pos.as<float4>(); F.R.nrm = c->d_fg_nrm.as<float4>(); F.R.state = c->d_fg_state.as<float4>();
    F.R.n = c->d_fg_n.as<float>(); F.R.dl = c->d_fg_dl.as<float4>();
    /* the kNN gather and the final over the chunk's records: the context's
     * own records, tile list, view and estimator are not part of either */
    GatherParams G = gather_params(c, p);
    G.view_rank = nullptr; G.view_list = nullptr;
    FinalParams L{};
    L.knn = 1; L.materials = c->S.materials; L.emitted = (float)p->paths_per_pass;
    L.out = c->d_fg_li.as<float>(); L.W = c->W;
    FgSumParams A{};
    A.P = F.P; A.li = L.out; A.sum = c->d_fg_sum.as<float4>(); A.n_gather = n_gather; A.zero = pass == 0;
    for (int64_t r0 = 0; r0 < nrec; r0 += chunk_recs) {
        const int64_t nr = std::min(chunk_recs, nrec - r0);
        F.sec_begin = r0 * N;
        F.R.count = nr * N;
        timer_begin(c, "fgrays", s);
        HIPCHK(c, launch_fg_rays(F, s));
        timer_end(c, "fgrays", s);
        G.R = F.R; G.rec_begin = 0; G.rec_end = F.R.count;
        timer_begin(c, "fgather", s);
        if ((rc = gather_knn_setup(c, p, G))) return rc;
        HIPCHK(c, launch_gather_knn(G, 0, s));
        L.R = F.R; L.rec_begin = 0; L.rec_count = F.R.count;
        HIPCHK(c, launch_final(L, s));
        A.rec_begin = r0; A.rec_count = nr;
        HIPCHK(c, launch_fg_accumulate(A, s));
        timer_end(c, "fgather", s);
    }
    c->fg_chunks = (nrec + chunk_recs - 1) / chunk_recs;
    ++c->fg_passes;
    return PM_OK;
}

int pm_final_gather_resolve(void *ptr, int64_t rec_begin, int64_t rec_count, void *d_out, void *stream) {
    GETCTX(ptr);
    if (c->fg_passes < 1 || c->fg_nrec != c->nrec || c->nrec <= 0)
        FAIL(c, PM_ERR_INVALID, "pm_final_gather_resolve: no final-gather pass over these records (pm_final_gather_pass)");
    if (!d_out || rec_begin < 0 || rec_count < 0 || rec_begin + rec_count > c->nrec)
        FAIL(c, PM_ERR_INVALID, "pm_final_gather_resolve: bad record range");
    hipStream_t s = pick(c, stream);
    FgResolveParams R{};
    R.P = recs(c); R.sum = c->d_fg_sum.as<float4>(); R.materials = c->S.materials;
    R.denom = (float)((int64_t)c->fg_n * c->fg_passes);
    R.rec_begin = rec_begin; R.rec_count = rec_count; R.out = (float *)d_out; R.raster = c->pinhole; R.W = c->W;
    /* pm_set_caustic_map on and pm_caustic_gather run for every pass: Lc beside the direct light */
    const bool caustic = c->caustic_map && c->cg_passes > 0;
    if (caustic && (c->cg_passes != c->fg_passes || c->cg_nrec != c->nrec))
        FAIL(c, PM_ERR_INVALID, "pm_final_gather_resolve: the caustic map is on and pm_caustic_gather ran for %d of the %d "
                                "final-gather passes", c->cg_passes, c->fg_passes);
    timer_begin(c, "final", s);
    if (caustic) HIPCHK(c, launch_fg_resolve_caustic(R, (float)c->cg_emitted, s));
    else HIPCHK(c, launch_fg_resolve(R, s));
    timer_end(c, "final", s);
    return PM_OK;
}

/* ------------------------------------------------------- the caustic map */
int pm_set_caustic_map(void *ptr, int on) {
    GETCTX(ptr);
    if (on && c->committed && c->albedo())
        FAIL(c, PM_ERR_INVALID, "pm_set_caustic_map: the scene has a textured or physically specular material (final "
                                "gathering takes neither)");
    c->caustic_map = on != 0;
    c->cg_built = false;
    c->cg_passes = 0;
    return PM_OK;
}

int pm_build_caustic_map(void *ptr, void *stream) {
    GETCTX(ptr);
    if (!c->caustic_map) FAIL(c, PM_ERR_INVALID, "pm_build_caustic_map: the caustic map is off (pm_set_caustic_map)");
    if (c->map_kind != PM_GATHER_GRID || c->map_slots <= 0)
        FAIL(c, PM_ERR_INVALID, "pm_build_caustic_map: no photon map built on the buckets (pm_build_photon_map first)");
    if ((size_t)c->map_slots * sizeof(pm_photon) > c->d_slots.bytes)
        FAIL(c, PM_ERR_INVALID, "pm_build_caustic_map: the slot buffer no longer holds the map's %lld slots", (long long)c->map_slots);
    hipStream_t s = pick(c, stream);
    int rc;
    if ((rc = materialize_slots(c, s))) return rc; /* the count reads every slot's bits */
    const GridDesc g = c->grid; /* the full map's grid: the kNN estimator's for the build's initial_radius2 */
    const size_t n = (size_t)c->map_slots, nc = (size_t)g.ncells + 1;
    const bool fresh_count = !(c->d_cg_count.p && nc * 4 <= c->d_cg_count.bytes);
    HIPCHK(c, c->d_cg_count.ensure_slack(nc * 4));
    HIPCHK(c, c->d_cg_cell_start.ensure_slack(nc * 4));
    HIPCHK(c, c->d_cg_scratch.ensure_slack(caustic_scratch_words((int64_t)n, g.ncells) * 4));
    HIPCHK(c, c->d_cg_pha.ensure_slack(n * 16));
    HIPCHK(c, c->d_cg_phb.ensure_slack(n * 32));
    /* a new counter buffer starts zeroed; afterwards every build's scan leaves it so */
    if (fresh_count) HIPCHK(c, hipMemsetAsync(c->d_cg_count.p, 0, c->d_cg_count.bytes, s));
    timer_begin(c, "caustic", s);
    HIPCHK(c, launch_caustic_build(c->d_slots.as<pm_photon>(), (int64_t)n, g, c->d_cg_count.as<uint32_t>(),
                                   c->d_cg_cell_start.as<uint32_t>(), c->d_cg_scratch.as<uint32_t>(),
                                   c->d_cg_pha.as<float4>(), c->d_cg_phb.as<float4>(), s));
    timer_end(c, "caustic", s);
    c->cg_grid = g;
    c->cg_slots = (int64_t)n;
    c->cg_built = true;
    ++c->cg_gen;
    return PM_OK;
}

int pm_caustic_gather(void *ptr, const pm_render_params *p, int pass, void *stream) {
    if (!p) FAIL((Ctx *)ptr, PM_ERR_INVALID, "pm_caustic_gather: null params");
    if (pass < 0) FAIL((Ctx *)ptr, PM_ERR_INVALID, "pm_caustic_gather: pass %d is negative", pass);
    GETCTX(ptr);
    int rc;
    if ((rc = fg_validate(c, p, __func__))) return rc;
    if (!c->caustic_map) FAIL(c, PM_ERR_INVALID, "pm_caustic_gather: the caustic map is off (pm_set_caustic_map)");
    if (!c->cg_built) FAIL(c, PM_ERR_INVALID, "pm_caustic_gather: no caustic map built (pm_build_caustic_map)");
    if (!same_grid(c->cg_grid, pm::make_grid(c->bbox_lo, c->bbox_hi, PM_ESTIMATOR_KNN, c->cell_span, p->initial_radius2)))
        FAIL(c, PM_ERR_INVALID, "pm_caustic_gather: the caustic map was not built on PM_ESTIMATOR_KNN buckets with this initial_radius2");
    if (pass > 0 && (c->cg_passes < 1 || c->cg_nrec != c->nrec))
        FAIL(c, PM_ERR_INVALID, "pm_caustic_gather: pass %d continues no pass 0 over these records", pass);
    hipStream_t s = pick(c, stream);
    /* a GatherParams of its own, as pm_final_gather_pass makes for its secondary records: the primary records
     * against the caustic map, every tile, no view */
    pm_render_params q = *p;
    q.estimator = PM_ESTIMATOR_KNN;
    GatherParams G = gather_params(c, &q);
    G.view_rank = nullptr; G.view_list = nullptr;
    G.grid = c->cg_grid;
    G.cell_start = c->d_cg_cell_start.as<uint32_t>();
    G.ph_a = c->d_cg_pha.as<float4>(); G.ph_b = c->d_cg_phb.as<float4>();
    G.rec_begin = 0; G.rec_end = c->nrec;
    if (pass == 0) { /* pass 0 starts the sums: flux 0, photon_count 0 */
        G.fresh = 1;
        G.r2init = p->initial_radius2;
        c->cg_passes = 0; c->cg_nrec = c->nrec; c->cg_emitted = 0;
    } else if ((rc = materialize_reset(c, s))) return rc;
    timer_begin(c, "caustic", s);
    if ((rc = gather_knn_setup(c, &q, G, true))) return rc;
    HIPCHK(c, launch_gather_knn(G, 0, s));
    timer_end(c, "caustic", s);
    c->rec_fresh = false;
    c->rec_estimator = PM_ESTIMATOR_KNN; /* the records hold kNN sums */
    c->grid_plan.invalidate();           /* r_k^2 replaced the radii */
    ++c->cg_passes;
    c->cg_emitted += (double)p->paths_per_pass;
    return PM_OK;
}

int64_t pm_caustic_map_count(void *ptr) {
    Ctx *c = (Ctx *)ptr;
    if (!c || c->group || !c->cg_built) return -1;
    (void)hipSetDevice(c->device);
    uint32_t nv = 0;
    if (hipStreamSynchronize(c->stream) != hipSuccess ||
        hipMemcpy(&nv, c->d_cg_cell_start.as<uint32_t>() + c->cg_grid.ncells, 4, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return (int64_t)nv;
}

int pm_download_caustic_slots(void *ptr, uint32_t *out, int64_t n) {
    GETCTX(ptr);
    if (!out) FAIL(c, PM_ERR_INVALID, "pm_download_caustic_slots: null pointer");
    if (!c->cg_built) FAIL(c, PM_ERR_INVALID, "pm_download_caustic_slots: no caustic map built (pm_build_caustic_map)");
    const int64_t have = pm_caustic_map_count(c);
    if (n < 0 || n > have)
        FAIL(c, PM_ERR_INVALID, "pm_download_caustic_slots: %lld indices asked, %lld held", (long long)n, (long long)have);
    std::vector<float4> b((size_t)n * 2);
    HIPCHK(c, hipMemcpy(b.data(), c->d_cg_phb.p, (size_t)n * 32, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) std::memcpy(&out[i], &b[2 * (size_t)i + 1].y, 4);
    return PM_OK;
}

int pm_download_caustic_cell_start(void *ptr, uint32_t *out, int64_t n) {
    GETCTX(ptr);
    if (!out) FAIL(c, PM_ERR_INVALID, "pm_download_caustic_cell_start: null pointer");
    if (!c->cg_built) FAIL(c, PM_ERR_INVALID, "pm_download_caustic_cell_start: no caustic map built (pm_build_caustic_map)");
    if (n < 0 || n > (int64_t)c->cg_grid.ncells + 1)
        FAIL(c, PM_ERR_INVALID, "pm_download_caustic_cell_start: %lld words asked, %lld held", (long long)n, (long long)c->cg_grid.ncells + 1);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->d_cg_cell_start.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PM_OK;
}

int pm_download_caustic_radiance(void *ptr, float *out_rgb, int64_t n) {
    GETCTX(ptr);
    if (!out_rgb) FAIL(c, PM_ERR_INVALID, "pm_download_caustic_radiance: null pointer");
    if (c->cg_passes < 1 || n < 0 || n > c->cg_nrec || c->cg_nrec != c->nrec)
        FAIL(c, PM_ERR_INVALID, "pm_download_caustic_radiance: %lld radiances asked, %lld held (pm_caustic_gather)", (long long)n,
             (long long)(c->cg_passes < 1 ? 0 : c->cg_nrec));
    if (n == 0) return PM_OK;
    DevBuf d;
    HIPCHK(c, d.ensure((size_t)n * 3 * sizeof(float)));
    FgResolveParams R{};
    R.P = recs(c); R.materials = c->S.materials; R.rec_begin = 0; R.rec_count = n; R.out = d.as<float>();
    hipError_t e = launch_caustic_radiance(R, (float)c->cg_emitted, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out_rgb, d.p, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    d.release();
    HIPCHK(c, e);
    return PM_OK;
}

int pm_final_gather_rays(void *ptr, const pm_render_params *p, int n_gather, int pass, int64_t first, int64_t count,
                         float *rays6) {
    FG_ARGS("pm_final_gather_rays");
    GETCTX(ptr);
    int rc;
    if ((rc = fg_validate(c, p, __func__))) return rc;
    if (!rays6 || first < 0 || count < 0 || first + count > c->nrec * (int64_t)n_gather)
        FAIL(c, PM_ERR_INVALID, "pm_final_gather_rays: bad ray range");
    if (count == 0) return PM_OK;
    DevBuf d;
    HIPCHK(c, d.ensure((size_t)count * 6 * sizeof(float)));
    const FgParams F = fg_params(c, p, n_gather, pass);
    hipError_t e = launch_fg_ray_dump(F, first, count, d.as<float>(), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(rays6, d.p, (size_t)count * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    d.release();
    HIPCHK(c, e);
    return PM_OK;
}

int pm_download_gather_sum(void *ptr, float *out_rgb, int64_t n) {
    GETCTX(ptr);
    if (!out_rgb) FAIL(c, PM_ERR_INVALID, "pm_download_gather_sum: null pointer");
    if (c->fg_passes < 1 || n < 0 || n > c->fg_nrec || !c->d_fg_sum.p)
        FAIL(c, PM_ERR_INVALID, "pm_download_gather_sum: %lld sums asked, %lld held (pm_final_gather_pass)", (long long)n,
             (long long)(c->fg_passes < 1 ? 0 : c->fg_nrec));
    HIPCHK(c, hipDeviceSynchronize());
    std::vector<float4> a((size_t)n);
    HIPCHK(c, hipMemcpy(a.data(), c->d_fg_sum.p, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) { out_rgb[3 * i] = a[i].x; out_rgb[3 * i + 1] = a[i].y; out_rgb[3 * i + 2] = a[i].z; }
    return PM_OK;
}

} /* extern "C" */
