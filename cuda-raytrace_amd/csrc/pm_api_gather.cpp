/*
 * pm_api_gather.cpp — the gathers of the stage calls: the parameter block of
 * a gather over the context's photon map (gather_params) and the kNN scalar
 * stream's buffers on either bucket map (gather_knn_setup), the named steps
 * of a gather, the four pm_gather* entry points and the four pm_ppm_update*
 * calls.
 */
#include "pm_ctx.h"

/* cells per axis of a box of width 2 r' (r' of radius2) on grid g: the tile
 * kernel's run count (GatherParams::span), clamped to its instances 2..5
 * (larger boxes scan per lane) */
static int grid_span(const GridDesc &g, float radius2) {
    const double rq = sqrt((double)radius2) * 1.0001 + 1e-4;
    const double w = 2.0 * rq * (double)g.inv_cs * (1.0 + 1e-6);
    return std::max(2, std::min(5, (int)std::floor(w) + 2));
}

/* the largest alpha a deposit can carry: the emission (LightSummary's bound
 * for this call's light_source_index), max_photon_count Lambert weights and
 * max_specular_depth lobe colours of the physical specular model (spec_max is
 * 1, and the factor exactly 1, without such a material) */
static double flux_bound(Ctx *c, const pm_render_params *p) {
    const double emit = p->light_source_index == PM_ALL_LIGHTS ? c->lsum.emit_max_all : c->lsum.emit_max;
    return emit * std::pow(c->lsum.kd_max, (double)p->max_photon_count) *
           std::pow(c->lsum.spec_max, (double)std::max(p->max_specular_depth, 0));
}

GatherParams gather_params(Ctx *c, const pm_render_params *p) {
    GatherParams G{};
    G.R = recs(c);
    G.materials = c->S.materials;
    G.ppm_alpha = p->ppm_alpha;
    c->map.attach(G);
    G.kd_nodes = c->d_kd.as<pm_photon>(); G.kd_count = c->kd_count;
    G.counters = c->d_counters.as<unsigned long long>();
    G.kernel = c->gather_kernel;
    G.kd_stack = c->kd_stack;
    G.error = reinterpret_cast<unsigned int *>(c->d_counters.as<unsigned long long>() + 16);
    G.fx_nonneg = c->lsum.scene_nonneg && c->slots_nonneg ? 1 : 0;
    G.span = grid_span(c->map.grid, c->grid_r2 > 0.f ? c->grid_r2 : p->initial_radius2);
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

/* the kNN estimator's part of G, and the scalar stream's pairs and handed-back tiles of the map m G points at */
int gather_knn_setup(Ctx *c, const pm_render_params *p, GatherParams &G, BucketMap &m) {
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
        const int64_t nph = (int64_t)(m.ph_a.bytes / 16), pairs = (nph + 1) / 2 + 16;
        const int64_t ntiles = (G.rec_end - G.rec_begin + 63) / 64;
        HIPCHK(c, m.knn_pk.ensure((size_t)pairs * 80));
        HIPCHK(c, m.knn_ovf.ensure((size_t)(ntiles + KNN_OVF_HDR) * 4));
        G.knn_pk_p = m.knn_pk.as<float4>();
        G.knn_pk_q = G.knn_pk_p + 2 * pairs;
        G.knn_pk_pairs = pairs;
        G.knn_pack = m.pack_gen != m.gen || m.pack_ptr != m.knn_pk.p;
        m.pack_gen = m.gen;
        m.pack_ptr = m.knn_pk.p;
        G.knn_ovf_n = m.knn_ovf.as<uint32_t>();
        G.knn_ovf = G.knn_ovf_n + KNN_OVF_HDR;
    }
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
    if (p->estimator == PM_ESTIMATOR_KNN && (rc = gather_knn_setup(c, p, G, c->map))) return rc;
    if ((rc = gather_launch(c, p, G, partials, s))) return rc;
    return gather_post(c, p, G, consume, hist, s);
}

extern "C" {

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

} /* extern "C" */
