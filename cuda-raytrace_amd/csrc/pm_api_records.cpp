/*
 * pm_api_records.cpp — the record half of the stage calls: check_params, the
 * eye pass and its resample, the record view, the deferred reset, the radius
 * calls, pm_final / pm_final_view, and the record and albedo transfers.
 */
#include "pm_ctx.h"

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

static int ensure_records(Ctx *c) {
    int64_t n = num_records(c);
    if (n <= 0) FAIL(c, PM_ERR_INVALID, "no eye samples (call pm_set_pinhole or pm_set_eye_rays)");
    HIPCHK(c, c->rec.ensure(n));
    /* the albedo factors, only for a textured or physically specular scene; a new buffer starts as
     * all ones (records uploaded without an eye pass keep their flux as it is) */
    if (c->albedo() && !(c->d_rkd.p && (size_t)n * sizeof(float4) <= c->d_rkd.bytes)) {
        HIPCHK(c, c->d_rkd.ensure(n * sizeof(float4)));
        const std::vector<float4> ones((size_t)n, f4(1.f, 1.f, 1.f, 0.f));
        HIPCHK(c, hipMemcpy(c->d_rkd.p, ones.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice));
    }
    c->nrec = n;
    c->records_replaced();
    return PM_OK;
}

/* the parameter block of an eye pass over the context's records (pass 0) */
static EyeParams eye_params(Ctx *c, const pm_render_params *p) {
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

/* (re)builds the active-record view from the current records; synchronizes to read its size */
static int build_view(Ctx *c, hipStream_t s) {
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

/* n float4 of a device buffer as packed RGB on the host, once the device is idle */
int download_rgb(Ctx *c, const DevBuf &d, float *out_rgb, int64_t n) {
    HIPCHK(c, hipDeviceSynchronize());
    std::vector<float4> a((size_t)n);
    HIPCHK(c, hipMemcpy(a.data(), d.p, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) { out_rgb[3 * i] = a[i].x; out_rgb[3 * i + 1] = a[i].y; out_rgb[3 * i + 2] = a[i].z; }
    return PM_OK;
}

hipError_t RecordBufs::download(pm_record *out, int64_t cnt) const {
    std::vector<float4> p(cnt), ns(cnt), st(cnt), d(cnt);
    std::vector<float> N(cnt);
    hipError_t e = hipMemcpy(p.data(), pos.p, cnt * 16, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(ns.data(), nrm.p, cnt * 16, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(st.data(), state.p, cnt * 16, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(d.data(), dl.p, cnt * 16, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(N.data(), n.p, cnt * 4, hipMemcpyDeviceToHost);
    for (int64_t i = 0; i < cnt && e == hipSuccess; ++i) {
        pm_record &r = out[i];
        r.pos[0] = p[i].x; r.pos[1] = p[i].y; r.pos[2] = p[i].z; r.flags = (uint32_t)fbits_h(p[i].w);
        r.ns[0] = ns[i].x; r.ns[1] = ns[i].y; r.ns[2] = ns[i].z; r.material = fbits_h(ns[i].w);
        r.flux[0] = st[i].x; r.flux[1] = st[i].y; r.flux[2] = st[i].z; r.radius2 = st[i].w;
        r.dl[0] = d[i].x; r.dl[1] = d[i].y; r.dl[2] = d[i].z; r.photon_count = N[i];
    }
    return e;
}

hipError_t RecordBufs::upload(const pm_record *in, int64_t cnt) {
    std::vector<float4> p(cnt), ns(cnt), st(cnt), d(cnt);
    std::vector<float> N(cnt);
    for (int64_t i = 0; i < cnt; ++i) {
        const pm_record &r = in[i];
        p[i] = f4(r.pos[0], r.pos[1], r.pos[2], ibits((int)r.flags));
        ns[i] = f4(r.ns[0], r.ns[1], r.ns[2], ibits(r.material));
        st[i] = f4(r.flux[0], r.flux[1], r.flux[2], r.radius2);
        d[i] = f4(r.dl[0], r.dl[1], r.dl[2], 0.f);
        N[i] = r.photon_count;
    }
    hipError_t e = hipMemcpy(pos.p, p.data(), cnt * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(nrm.p, ns.data(), cnt * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(state.p, st.data(), cnt * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dl.p, d.data(), cnt * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(n.p, N.data(), cnt * 4, hipMemcpyHostToDevice);
    return e;
}

/* pm_final (view == nullptr) and pm_final_view: the ranges are checked by the callers */
static int final_range(Ctx *c, double emitted, int64_t begin, int64_t count, void *d_out, const uint32_t *view,
                       void *stream) {
    hipStream_t s = pick(c, stream);
    int rc;
    if ((rc = materialize_reset(c, s))) return rc;
    FinalParams F = final_params(c, emitted, begin, count, (float *)d_out);
    F.view = view;
    timer_begin(c, "final", s);
    HIPCHK(c, launch_final(F, s));
    timer_end(c, "final", s);
    return PM_OK;
}

extern "C" {

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
    c->records_replaced(); /* the hits moved, and the tile flags with them */
    if (c->view_active && (rc = build_view(c, s))) return rc;
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

int pm_record_view_size(void *ptr, int64_t *n_view) {
    if (!n_view) FAIL((Ctx *)ptr, PM_ERR_INVALID, "pm_record_view_size: null pointer");
    if (!ptr) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "pm_record_view_size: null context");
    GETCTX(ptr);
    if (!c->view_active) FAIL(c, PM_ERR_INVALID, "pm_record_view_size: no active-record view (pm_set_record_view)");
    *n_view = c->n_view;
    return PM_OK;
}

int pm_download_tile_list(void *ptr, uint32_t *out, int64_t max_n, int64_t *n, int *sorted) {
    if (!n || !sorted) FAIL((Ctx *)ptr, PM_ERR_INVALID, "pm_download_tile_list: null pointer");
    if (max_n < 0) FAIL((Ctx *)ptr, PM_ERR_INVALID, "pm_download_tile_list: negative size %lld", (long long)max_n);
    if (!ptr) FAIL((Ctx *)nullptr, PM_ERR_INVALID, "pm_download_tile_list: null context");
    GETCTX(ptr);
    if (c->nrec <= 0) FAIL(c, PM_ERR_INVALID, "pm_download_tile_list: no records (run pm_eye_pass first)");
    TileList &t = c->tiles;
    HIPCHK(c, t.ensure(recs(c), c->stream));
    HIPCHK(c, hipDeviceSynchronize()); /* the list may have been built or sorted on a caller's stream */
    uint32_t cnt = 0;
    HIPCHK(c, hipMemcpy(&cnt, t.d_count.p, 4, hipMemcpyDeviceToHost));
    const int64_t tiles = (c->nrec + 63) / 64;
    if ((int64_t)cnt > tiles || (size_t)cnt * 4 > t.d_list.bytes)
        FAIL(c, PM_ERR_INVALID, "pm_download_tile_list: the list claims %u of %lld tiles", cnt, (long long)tiles);
    *n = (int64_t)cnt;
    *sorted = t.sorted ? 1 : 0;
    if (!out) return PM_OK;
    if (max_n < (int64_t)cnt)
        FAIL(c, PM_ERR_INVALID, "pm_download_tile_list: room for %lld entries, %u held", (long long)max_n, cnt);
    if (cnt) HIPCHK(c, hipMemcpy(out, t.d_list.p, (size_t)cnt * 4, hipMemcpyDeviceToHost));
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
    return final_range(c, emitted, rec_begin, rec_count, d_out, nullptr, stream);
}

int pm_final_view(void *ptr, double emitted, int64_t v_begin, int64_t v_count, void *d_out, void *stream) {
    GETCTX(ptr);
    if (!c->view_active) FAIL(c, PM_ERR_INVALID, "no active-record view (pm_set_record_view)");
    if (!d_out || v_begin < 0 || v_count < 0 || v_begin + v_count > c->n_view) FAIL(c, PM_ERR_INVALID, "bad view range");
    return final_range(c, emitted, v_begin, v_count, d_out, c->d_vlist.as<uint32_t>(), stream);
}

int pm_download_records(void *ptr, pm_record *out, int64_t n) {
    GETCTX(ptr);
    if (!out || n < 0 || n > c->nrec) FAIL(c, PM_ERR_INVALID, "bad record range");
    int rc;
    if ((rc = materialize_reset(c, c->stream))) return rc;
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, c->rec.download(out, n));
    return PM_OK;
}

int pm_upload_records(void *ptr, const pm_record *in, int64_t n) {
    GETCTX(ptr);
    int rc;
    if (!in || n != num_records(c)) FAIL(c, PM_ERR_INVALID, "record count must equal pm_num_records");
    if ((rc = ensure_records(c))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->rec.upload(in, n));
    c->rec_fresh = false; /* every record overwritten */
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
    return download_rgb(c, c->d_rkd, out_rgb, n);
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

} /* extern "C" */
