/*
 * pm_api_photons.cpp — the photon half of the stage calls: the slot buffer
 * calls and the deferred zero fill of a lazy trace, pm_trace_photons (its
 * launch planned by pm_plan.cpp's plan_trace), pm_build_photon_map (the grid
 * each pass gets planned by pm_plan.cpp's R2Plan), and the slot and kd-tree
 * transfers.
 */
#include "pm_ctx.h"

/* the deferred zero fill of a lazy_zero trace, on stream s after the trace
 * (s == nullptr: on the trace's own stream, waited for) */
int materialize_slots(Ctx *c, hipStream_t s) {
    if (c->slots_dirty <= 0) return PM_OK;
    const bool wait = s == nullptr;
    if (wait) s = c->stream;
    HIPCHK(c, hipStreamWaitEvent(s, c->dirty_event, 0));
    HIPCHK(c, launch_zero_invalid_slots(c->d_slots.as<pm_photon>(), c->map.scratch.as<uint32_t>(), c->slots_dirty,
                                        c->dirty_key_np, c->dirty_mpc, s));
    c->slots_dirty = 0;
    if (wait) HIPCHK(c, hipStreamSynchronize(s));
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

/* make the first `words` bucket counters zero (a memset only when the last
 * bucket scan did not already leave them cleared) */
static hipError_t count_zeroed(Ctx *c, size_t words, hipStream_t s) {
    if (c->count_zero_ptr == c->map.count.p && c->count_zero_words >= words) return hipSuccess;
    hipError_t e = hipMemsetAsync(c->map.count.p, 0, words * 4, s);
    if (e == hipSuccess) { c->count_zero_words = words; c->count_zero_ptr = c->map.count.p; }
    return e;
}

extern "C" {

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
    if (c->trace_cus > 0) sh.cus = c->trace_cus; /* env PM_TRACE_CUS: pools, grid and spill stride follow together */
    else if (c->S.wide && hipDeviceGetAttribute(&sh.cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess) sh.cus = 0;
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
        BucketMap &m = c->map;
        c->fused.r2 = grid_radius2(c, p, s);
        const GridDesc g = make_grid(c, p, c->fused.r2);
        HIPCHK(c, m.count.ensure_slack(((size_t)g.ncells + 1) * 4));
        HIPCHK(c, m.scratch.ensure_slack(bucket_scratch_words(end_slot, g.ncells) * 4));
        HIPCHK(c, count_zeroed(c, (size_t)g.ncells + 1, s));
        T.bucket = 1;
        T.grid = g;
        T.count = m.count.as<uint32_t>();
        T.key = m.scratch.as<uint32_t>();
        T.rank = m.scratch.as<uint32_t>() + end_slot;
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
    BucketMap &m = c->map;
    m.slots = n_slots;
    if (p->gather_structure == PM_GATHER_KDTREE && (rc = materialize_slots(c, s))) return rc;
    if (p->gather_structure == PM_GATHER_KDTREE) {
        /* reference path (CreatePhotonMap): DtoH, CPU pbrt KdTree, HtoD */
        timer_begin(c, "build", s, true);
        std::vector<pm_photon> h((size_t)n_slots), nodes;
        HIPCHK(c, hipMemcpyAsync(h.data(), c->d_slots.p, n_slots * sizeof(pm_photon), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        int64_t nk = build_kdtree_pbrt(h.data(), n_slots, nodes);
        c->kd_count = nk;
        if (nk > 0) {
            HIPCHK(c, c->d_kd.ensure(nk * sizeof(pm_photon)));
            HIPCHK(c, hipMemcpyAsync(c->d_kd.p, nodes.data(), nk * sizeof(pm_photon), hipMemcpyHostToDevice, s));
            HIPCHK(c, hipStreamSynchronize(s));
        }
        timer_end(c, "build", s);
        c->map_kind = PM_GATHER_KDTREE;
        if (nk == 0) FAIL(c, PM_ERR_NO_PHOTONS, "0 valid photons");
        return PM_OK;
    }
    /* photon buckets: cell size >= 2 r_max (PPM radii only shrink) */
    GridDesc &g = m.grid;
    /* the grid of the trace's fused counts, if they cover these slots */
    const bool fused_ok = c->fused.valid && c->fused.n == n_slots;
    c->grid_r2 = fused_ok ? c->fused.r2 : grid_radius2(c, p, s);
    g = make_grid(c, p, c->grid_r2);
    const bool counted = fused_ok && same_grid(c->fused.grid, g);
    /* the counting pass below reads every slot's valid bit (and overwrites the keys) */
    if (!counted && (rc = materialize_slots(c, s))) return rc;
    const size_t n = (size_t)n_slots;
    HIPCHK(c, m.count.ensure_slack(((size_t)g.ncells + 1) * 4));
    HIPCHK(c, m.cell_start.ensure_slack(((size_t)g.ncells + 1) * 4));
    if (!counted) {
        HIPCHK(c, m.scratch.ensure_slack(bucket_scratch_words(n_slots, g.ncells) * 4));
        HIPCHK(c, count_zeroed(c, (size_t)g.ncells + 1, s));
    }
    HIPCHK(c, m.ph_a.ensure_slack(n * 16)); HIPCHK(c, m.ph_b.ensure_slack(n * 32));
    timer_begin(c, "build", s);
    HIPCHK(c, launch_bucket_build(c->d_slots.as<pm_photon>(), n_slots, g, m.count.as<uint32_t>(),
                                  m.cell_start.as<uint32_t>(), m.scratch.as<uint32_t>(), m.ph_a.as<float4>(),
                                  m.ph_b.as<float4>(), counted, s, counted ? c->fused.key_np : 0, c->fused.mpc));
    ++m.gen; /* kNN pairs repacked on the next kNN gather */
    /* the scan left the counters zeroed */
    c->count_zero_words = (size_t)g.ncells + 1;
    c->count_zero_ptr = m.count.p;
    timer_end(c, "build", s);
    c->map_kind = PM_GATHER_GRID;
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

/* ---- test hooks: the bucket map of the last pm_build_photon_map, read only.
 * What needs no context is checked before the context is. */
#define MAP_HOOK(fn, null_arg)                                                                    \
    if (null_arg) FAIL((Ctx *)ptr, PM_ERR_INVALID, fn ": null pointer");                          \
    if (!ptr) FAIL((Ctx *)nullptr, PM_ERR_INVALID, fn ": null context");                          \
    GETCTX(ptr);                                                                                  \
    if (c->map_kind != PM_GATHER_GRID || !c->map.cell_start.p)                                    \
        FAIL(c, PM_ERR_INVALID, fn ": no photon map built on the buckets (pm_build_photon_map)"); \
    HIPCHK(c, hipStreamSynchronize(c->stream))

int pm_map_grid(void *ptr, int32_t dims[3], float origin[3], uint32_t *inv_cs_bits) {
    MAP_HOOK("pm_map_grid", !dims || !origin || !inv_cs_bits);
    const GridDesc &g = c->map.grid;
    dims[0] = g.dx; dims[1] = g.dy; dims[2] = g.dz;
    origin[0] = g.gx; origin[1] = g.gy; origin[2] = g.gz;
    std::memcpy(inv_cs_bits, &g.inv_cs, 4);
    return PM_OK;
}

int pm_download_map_cell_start(void *ptr, uint32_t *out, int64_t n) {
    if (n < 0) FAIL((Ctx *)ptr, PM_ERR_INVALID, "pm_download_map_cell_start: negative size %lld", (long long)n);
    MAP_HOOK("pm_download_map_cell_start", !out);
    const int64_t have = (int64_t)c->map.grid.ncells + 1;
    if (n > have || (size_t)n * 4 > c->map.cell_start.bytes)
        FAIL(c, PM_ERR_INVALID, "pm_download_map_cell_start: %lld words asked, %lld held", (long long)n, (long long)have);
    HIPCHK(c, hipMemcpy(out, c->map.cell_start.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PM_OK;
}

int pm_download_map_counters(void *ptr, uint32_t *out, int64_t n) {
    if (n < 0) FAIL((Ctx *)ptr, PM_ERR_INVALID, "pm_download_map_counters: negative size %lld", (long long)n);
    MAP_HOOK("pm_download_map_counters", !out);
    const int64_t have = (int64_t)c->map.grid.ncells + 1;
    if (n > have || !c->map.count.p || (size_t)n * 4 > c->map.count.bytes)
        FAIL(c, PM_ERR_INVALID, "pm_download_map_counters: %lld words asked, %lld held", (long long)n, (long long)have);
    HIPCHK(c, hipMemcpy(out, c->map.count.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PM_OK;
}

int pm_download_map_photons(void *ptr, float *ph_a, float *ph_b, int64_t n) {
    if (n < 0) FAIL((Ctx *)ptr, PM_ERR_INVALID, "pm_download_map_photons: negative size %lld", (long long)n);
    MAP_HOOK("pm_download_map_photons", !ph_a || !ph_b);
    uint32_t nv = 0;
    HIPCHK(c, c->map.valid_photons(&nv));
    /* the photons the scan counted, and never more than the build sized the arrays for */
    const int64_t have = std::min<int64_t>((int64_t)nv, c->map.slots);
    if (n > have || (size_t)n * 16 > c->map.ph_a.bytes || (size_t)n * 32 > c->map.ph_b.bytes)
        FAIL(c, PM_ERR_INVALID, "pm_download_map_photons: %lld photons asked, %lld held", (long long)n, (long long)have);
    if (n == 0) return PM_OK;
    HIPCHK(c, hipMemcpy(ph_a, c->map.ph_a.p, (size_t)n * 16, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(ph_b, c->map.ph_b.p, (size_t)n * 32, hipMemcpyDeviceToHost));
    return PM_OK;
}
#undef MAP_HOOK

int pm_download_kdtree(void *ptr, pm_photon *out, int64_t n) {
    GETCTX(ptr);
    if (!out || n < 0 || n > c->kd_count) FAIL(c, PM_ERR_INVALID, "bad kd range");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->d_kd.p, n * sizeof(pm_photon), hipMemcpyDeviceToHost));
    return PM_OK;
}

} /* extern "C" */
