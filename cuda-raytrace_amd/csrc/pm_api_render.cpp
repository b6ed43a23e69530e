/*
 * pm_api_render.cpp — the whole renders of the C-ABI, built from the stage
 * calls: pm_film and the image delivery, pm_render on one device,
 * group_render over the devices of a multi-device context, and the simple
 * (direct light) renderer.
 */
#include "pm_ctx.h"

extern "C" {

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

/* ------------------------------------------------------------ whole render */
/* the pieces pm_render, group_render and pm_render_simple share; HIP errors
 * are reported on ec (a group's context, or c itself) */

/* valid photons of the map c just built; waits for its stream */
static int valid_photons(Ctx *ec, Ctx *c, const pm_render_params *p, int64_t &nvalid) {
    nvalid = c->kd_count;
    if (p->gather_structure == PM_GATHER_GRID) {
        uint32_t nv = 0;
        HIPCHK(ec, c->map.valid_photons(&nv, c->stream));
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
    HIPCHK(ec, hipMemcpy(pos.data(), c->rec.pos.p, c->nrec * sizeof(float4), hipMemcpyDeviceToHost));
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

/* pm_render's loop with a fresh eye sample per pass in front of the trace
 * (stochastic progressive photon mapping: one record per pixel, moved under
 * its statistics); the final divides the summed direct light by the passes */
int pm_render_resampled(void *ptr, const pm_render_params *p, float *out_rgb, pm_stats *st) {
    GETCTX(ptr);
    int rc;
    if ((rc = check_params(c, p))) return rc;
    if (!out_rgb) FAIL(c, PM_ERR_INVALID, "null output");
    if (p->passes < 1 || p->paths_per_pass < 1) FAIL(c, PM_ERR_INVALID, "passes and paths_per_pass must be >= 1");
    hipStream_t s = c->stream;
    double t_eye = 0, t_trace = 0, t_build = 0, t_gather = 0, t_final = 0;
    int64_t nvalid = 0;
    int64_t counters[2] = {0, 0};
    for (int pass = 0; pass < p->passes; ++pass) {
        if ((rc = pm_eye_resample(c, p, pass, s))) return rc;
        t_eye += timer_ms(c, "eye");
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
    const int64_t nout = (int64_t)c->W * c->H; /* one stratum, no film: the sample raster is the image */
    HIPCHK(c, c->d_out.ensure(nout * 3 * sizeof(float)));
    FinalParams F = final_params(c, emitted, 0, c->nrec, c->d_out.as<float>());
    F.raster = 1;
    F.n_eye = p->passes; F.resampled = 1; /* also for a single pass, where it is pm_render's final */
    timer_begin(c, "final", s);
    HIPCHK(c, launch_final(F, s));
    timer_end(c, "final", s);
    if ((rc = deliver_image(c, nout, out_rgb))) return rc;
    t_final = timer_ms(c, "final");
    if (st) {
        if ((rc = render_stats(c, c, emitted, nvalid, st))) return rc; /* gather_points: the last pass's */
        st->nodes_visited = counters[0];
        st->photons_in_radius = counters[1];
        st->ms_eye = t_eye; st->ms_trace = t_trace; st->ms_build = t_build; st->ms_gather = t_gather;
        st->ms_final = t_final;
    }
    return PM_OK;
}

/* pm_render's loop with pm_final_gather_pass in the place of the primary
 * records' gather, and the resolve in the place of the final. The buckets are
 * built for the kNN estimator, whatever params->estimator says. Under
 * pm_set_caustic_map each pass also builds the caustic map and gathers it at
 * the primary records; the resolve then adds Lc. */
int pm_render_final_gather(void *ptr, const pm_render_params *p, int n_gather, float *out_rgb, pm_stats *st) {
    if (!p) FAIL((Ctx *)ptr, PM_ERR_INVALID, "pm_render_final_gather: null params");
    if (n_gather < 1 || n_gather > PM_FG_MAX)
        FAIL((Ctx *)ptr, PM_ERR_INVALID, "pm_render_final_gather: n_gather %d outside 1..%d", n_gather, PM_FG_MAX);
    GETCTX(ptr);
    int rc;
    pm_render_params q = *p;
    q.estimator = PM_ESTIMATOR_KNN;
    if ((rc = check_params(c, &q))) return rc;
    if (!out_rgb) FAIL(c, PM_ERR_INVALID, "null output");
    if (q.passes < 1 || q.paths_per_pass < 1) FAIL(c, PM_ERR_INVALID, "passes and paths_per_pass must be >= 1");
    if (c->albedo())
        FAIL(c, PM_ERR_INVALID, "pm_render_final_gather: the scene has a textured or physically specular material; a "
                                "secondary hit would need its texel or throughput");
    hipStream_t s = c->stream;
    double t_eye = 0, t_trace = 0, t_build = 0, t_gather = 0, t_final = 0;
    if ((rc = pm_eye_pass(c, &q, s))) return rc;
    t_eye = timer_ms(c, "eye");
    int64_t nvalid = 0;
    for (int pass = 0; pass < q.passes; ++pass) {
        if ((rc = pm_trace_photons(c, &q, pass, 0, q.paths_per_pass, 0, s))) return rc;
        t_trace += timer_ms(c, "trace");
        if ((rc = pm_build_photon_map(c, &q, q.paths_per_pass * q.max_photon_count, s))) return rc;
        t_build += timer_ms(c, "build");
        if ((rc = valid_photons(c, c, &q, nvalid))) return rc;
        if ((rc = pm_final_gather_pass(c, &q, n_gather, pass, s))) return rc;
        /* every chunk of the pass; a stage that is not timed (pm_set_stage_timing) adds nothing */
        t_gather += std::max(0.0, timer_ms(c, "fgrays", (size_t)c->fg_chunks)) +
                    std::max(0.0, timer_ms(c, "fgather", (size_t)c->fg_chunks));
        if (c->caustic_map) { /* the caustic map of this pass's photons, looked up at the eye hits */
            if ((rc = pm_build_caustic_map(c, s))) return rc;
            if ((rc = pm_caustic_gather(c, &q, pass, s))) return rc;
            t_gather += std::max(0.0, timer_ms(c, "caustic", 2)); /* the build and the gather */
        }
    }
    const double emitted = (double)q.paths_per_pass * q.passes;
    const int64_t nout = c->pinhole ? (int64_t)c->W * c->H : c->nrec;
    HIPCHK(c, c->d_out.ensure(nout * 3 * sizeof(float)));
    if ((rc = pm_final_gather_resolve(c, 0, c->nrec, c->d_out.p, s))) return rc;
    if ((rc = deliver_image(c, nout, out_rgb))) return rc;
    t_final = timer_ms(c, "final");
    if (st) {
        if ((rc = render_stats(c, c, emitted, nvalid, st))) return rc;
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

} /* extern "C" */
