/*
 * pm_api_fgather.cpp — final gathering and the caustic map: the passes over
 * the secondary records of a chunk (pm_final_gather_pass), their resolve and
 * diagnostic downloads (gather rays, the sums), pm_set_caustic_map,
 * pm_build_caustic_map, pm_caustic_gather over the primary records and the
 * caustic map's count and downloads.
 */
#include "pm_ctx.h"

#include <functional>

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

/* what a diagnostic launch writes into a temporary device buffer of `bytes`, copied to the host on the context's
 * stream and waited for; the temporary is released before an error is reported */
static int launch_to_host(Ctx *c, void *out, size_t bytes, const std::function<hipError_t(float *)> &launch) {
    DevBuf d;
    HIPCHK(c, d.ensure(bytes));
    hipError_t e = launch(d.as<float>());
    if (e == hipSuccess) e = hipMemcpyAsync(out, d.p, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    d.release();
    HIPCHK(c, e);
    return PM_OK;
}

#define FG_ARGS(fn)                                                                                              \
    if (!p) FAIL((Ctx *)ptr, PM_ERR_INVALID, fn ": null params");                                                \
    if (n_gather < 1 || n_gather > PM_FG_MAX)                                                                    \
        FAIL((Ctx *)ptr, PM_ERR_INVALID, fn ": n_gather %d outside 1..%d", n_gather, PM_FG_MAX);                 \
    if (pass < 0) FAIL((Ctx *)ptr, PM_ERR_INVALID, fn ": pass %d is negative", pass)

extern "C" {

/* ------------------------------------------------------- final gathering */
int pm_final_gather_pass(void *ptr, const pm_render_params *p, int n_gather, int pass, void *stream) {
    FG_ARGS("pm_final_gather_pass"); /* what needs no context is checked before the context is */
    GETCTX(ptr);
    int rc;
    if ((rc = fg_validate(c, p, __func__))) return rc;
    if (c->map_kind != PM_GATHER_GRID) FAIL(c, PM_ERR_INVALID, "pm_final_gather_pass: no photon map built on the buckets (pm_build_photon_map)");
    if (!same_grid(c->map.grid, pm::make_grid(c->bbox_lo, c->bbox_hi, PM_ESTIMATOR_KNN, c->cell_span, p->initial_radius2)))
        FAIL(c, PM_ERR_INVALID, "pm_final_gather_pass: the photon buckets were not built for PM_ESTIMATOR_KNN with this initial_radius2");
    if (pass > 0 && (c->fg_passes < 1 || c->fg_n != n_gather || c->fg_nrec != c->nrec))
        FAIL(c, PM_ERR_INVALID, "pm_final_gather_pass: pass %d continues no pass 0 of %d rays over these records", pass, n_gather);
    hipStream_t s = pick(c, stream);
    const int64_t N = n_gather, nrec = c->nrec;
    /* whole primary tiles per chunk, at least one */
    const int64_t chunk_recs = std::max<int64_t>(1, c->fg_chunk / (64 * N)) * 64;
    const int64_t cap = std::min(chunk_recs, (nrec + 63) / 64 * 64) * N;
    HIPCHK(c, c->fg_rec.ensure(cap));
    HIPCHK(c, c->d_fg_li.ensure(cap * 3 * sizeof(float)));
    HIPCHK(c, c->d_fg_sum.ensure(nrec * sizeof(float4)));
    if (pass == 0) { c->fg_passes = 0; c->fg_n = n_gather; c->fg_nrec = nrec; }
    FgParams F = fg_params(c, p, n_gather, pass);
    F.R = c->fg_rec.dev(0); /* each chunk sets its count */
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
        if ((rc = gather_knn_setup(c, p, G, c->map))) return rc;
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

int pm_final_gather_rays(void *ptr, const pm_render_params *p, int n_gather, int pass, int64_t first, int64_t count,
                         float *rays6) {
    FG_ARGS("pm_final_gather_rays");
    GETCTX(ptr);
    int rc;
    if ((rc = fg_validate(c, p, __func__))) return rc;
    if (!rays6 || first < 0 || count < 0 || first + count > c->nrec * (int64_t)n_gather)
        FAIL(c, PM_ERR_INVALID, "pm_final_gather_rays: bad ray range");
    if (count == 0) return PM_OK;
    return launch_to_host(c, rays6, (size_t)count * 6 * sizeof(float), [&](float *d) {
        return launch_fg_ray_dump(fg_params(c, p, n_gather, pass), first, count, d, c->stream);
    });
}

int pm_download_gather_sum(void *ptr, float *out_rgb, int64_t n) {
    GETCTX(ptr);
    if (!out_rgb) FAIL(c, PM_ERR_INVALID, "pm_download_gather_sum: null pointer");
    if (c->fg_passes < 1 || n < 0 || n > c->fg_nrec || !c->d_fg_sum.p)
        FAIL(c, PM_ERR_INVALID, "pm_download_gather_sum: %lld sums asked, %lld held (pm_final_gather_pass)", (long long)n,
             (long long)(c->fg_passes < 1 ? 0 : c->fg_nrec));
    return download_rgb(c, c->d_fg_sum, out_rgb, n);
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
    if (c->map_kind != PM_GATHER_GRID || c->map.slots <= 0)
        FAIL(c, PM_ERR_INVALID, "pm_build_caustic_map: no photon map built on the buckets (pm_build_photon_map first)");
    if ((size_t)c->map.slots * sizeof(pm_photon) > c->d_slots.bytes)
        FAIL(c, PM_ERR_INVALID, "pm_build_caustic_map: the slot buffer no longer holds the map's %lld slots", (long long)c->map.slots);
    hipStream_t s = pick(c, stream);
    int rc;
    if ((rc = materialize_slots(c, s))) return rc; /* the count reads every slot's bits */
    BucketMap &m = c->cmap;
    const GridDesc g = c->map.grid; /* the full map's grid: the kNN estimator's for the build's initial_radius2 */
    const size_t n = (size_t)c->map.slots, nc = (size_t)g.ncells + 1;
    const bool fresh_count = !(m.count.p && nc * 4 <= m.count.bytes);
    HIPCHK(c, m.count.ensure_slack(nc * 4));
    HIPCHK(c, m.cell_start.ensure_slack(nc * 4));
    HIPCHK(c, m.scratch.ensure_slack(caustic_scratch_words((int64_t)n, g.ncells) * 4));
    HIPCHK(c, m.ph_a.ensure_slack(n * 16));
    HIPCHK(c, m.ph_b.ensure_slack(n * 32));
    /* a new counter buffer starts zeroed; afterwards every build's scan leaves it so */
    if (fresh_count) HIPCHK(c, hipMemsetAsync(m.count.p, 0, m.count.bytes, s));
    timer_begin(c, "caustic", s);
    HIPCHK(c, launch_caustic_build(c->d_slots.as<pm_photon>(), (int64_t)n, g, m.count.as<uint32_t>(),
                                   m.cell_start.as<uint32_t>(), m.scratch.as<uint32_t>(), m.ph_a.as<float4>(),
                                   m.ph_b.as<float4>(), s));
    timer_end(c, "caustic", s);
    m.grid = g;
    m.slots = (int64_t)n;
    c->cg_built = true;
    ++m.gen;
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
    if (!same_grid(c->cmap.grid, pm::make_grid(c->bbox_lo, c->bbox_hi, PM_ESTIMATOR_KNN, c->cell_span, p->initial_radius2)))
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
    c->cmap.attach(G);
    G.rec_begin = 0; G.rec_end = c->nrec;
    if (pass == 0) { /* pass 0 starts the sums: flux 0, photon_count 0 */
        G.fresh = 1;
        G.r2init = p->initial_radius2;
        c->cg_passes = 0; c->cg_nrec = c->nrec; c->cg_emitted = 0;
    } else if ((rc = materialize_reset(c, s))) return rc;
    timer_begin(c, "caustic", s);
    if ((rc = gather_knn_setup(c, &q, G, c->cmap))) return rc;
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
    if (hipStreamSynchronize(c->stream) != hipSuccess || c->cmap.valid_photons(&nv) != hipSuccess) return -1;
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
    HIPCHK(c, hipMemcpy(b.data(), c->cmap.ph_b.p, (size_t)n * 32, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) std::memcpy(&out[i], &b[2 * (size_t)i + 1].y, 4);
    return PM_OK;
}

int pm_download_caustic_cell_start(void *ptr, uint32_t *out, int64_t n) {
    GETCTX(ptr);
    if (!out) FAIL(c, PM_ERR_INVALID, "pm_download_caustic_cell_start: null pointer");
    if (!c->cg_built) FAIL(c, PM_ERR_INVALID, "pm_download_caustic_cell_start: no caustic map built (pm_build_caustic_map)");
    const int64_t have = (int64_t)c->cmap.grid.ncells + 1;
    if (n < 0 || n > have)
        FAIL(c, PM_ERR_INVALID, "pm_download_caustic_cell_start: %lld words asked, %lld held", (long long)n, (long long)have);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->cmap.cell_start.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PM_OK;
}

int pm_download_caustic_radiance(void *ptr, float *out_rgb, int64_t n) {
    GETCTX(ptr);
    if (!out_rgb) FAIL(c, PM_ERR_INVALID, "pm_download_caustic_radiance: null pointer");
    if (c->cg_passes < 1 || n < 0 || n > c->cg_nrec || c->cg_nrec != c->nrec)
        FAIL(c, PM_ERR_INVALID, "pm_download_caustic_radiance: %lld radiances asked, %lld held (pm_caustic_gather)", (long long)n,
             (long long)(c->cg_passes < 1 ? 0 : c->cg_nrec));
    if (n == 0) return PM_OK;
    return launch_to_host(c, out_rgb, (size_t)n * 3 * sizeof(float), [&](float *d) {
        FgResolveParams R{};
        R.P = recs(c); R.materials = c->S.materials; R.rec_begin = 0; R.rec_count = n; R.out = d;
        return launch_caustic_radiance(R, (float)c->cg_emitted, c->stream);
    });
}

} /* extern "C" */
