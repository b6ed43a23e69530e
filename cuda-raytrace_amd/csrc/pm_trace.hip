/*
 * pm_trace.hip — photon-pass kernels (HIP/CDNA4).
 *
 *   k_trace_lane   photon emission + bounce, one path per lane, <=
 *                  max_photon_count deposits per path into owner-written
 *                  slots                         (photontracing.cu:80-185)
 *   k_trace_pool   the same paths for scenes traversed from HBM: a wave's
 *                  lanes take paths from a pool and keep their traversals
 *                  alive across its loop (k_trace_pool8: the 8-wide tree)
 * (eye pass: pm_eye.hip; photon buckets: pm_bucket.hip; gathers:
 * pm_gather.hip, pm_gather_knn.hip; PPM update of partials / final:
 * pm_records.hip)
 */
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pm_kernels.h"
#include "pm_plan.h"
#include "pm_sample.h"
#include "pm_shade.h"
#include "pm_trav_step.h"

#pragma clang fp contract(off)

namespace pm {

/* ====================================================================== */
/* photon pass                                                            */
/* ====================================================================== */
/* bits = valid | caustic << 1 (pm_api.h pm_set_caustic_map): 1 from every kernel but the MARK ones */
PMD void store_photon(pm_photon *dst, uint32_t bits, v3 p, v3 a, v3 wi) {
    /* 40-B slot, 8-B aligned: five 8-byte stores */
    float2 *q = reinterpret_cast<float2 *>(dst);
    q[0] = make_float2(__uint_as_float(bits), p.x);
    q[1] = make_float2(p.y, p.z);
    q[2] = make_float2(a.x, a.y);
    q[3] = make_float2(a.z, wi.x);
    q[4] = make_float2(wi.y, wi.z);
}

/* Photon paths (photontracing.cu:80-185) split into ray steps so a block can
 * compact its live paths between steps. Per-path state (12 words) lives in
 * registers and moves through LDS only at compaction. */
struct PathState {
    Ray ray;         /* tmax is RT_DEFAULT_MAX at every step */
    v3 alpha;
    uint32_t pid;    /* global path id */
    uint32_t nI;     /* photons-in-path counter (reference nI) */
    uint32_t spec;   /* specular bounces so far */
    uint32_t stored; /* slots [0, stored) written */
    /* fused counting: the bucket rank of the last deposit is stored one deposit
     * later (or when the path ends), so the wave never waits for the returning
     * atomic right after issuing it */
    uint32_t pslot;  /* slot of the pending rank, PSLOT_NONE if none */
    uint32_t prank;
    uint32_t diff;   /* MARK kernels only: a diffuse hit has happened (spec > 0 && nI == 1 also holds for L D S D) */
};
constexpr uint32_t PSLOT_NONE = 0xffffffffu;
/* path pid's place in the launch's slot buffer, in paths: its slots start at mpc times this */
PMD size_t path_slot_base(const TraceParams &P, uint32_t pid) { return (size_t)(pid - (uint64_t)P.slot_path_base); }
/* where the fused bucket count keeps deposit k of path pid: plane-major
 * (k * key_np + path) when key_np > 0, so that the lanes of a wave — paths
 * next to each other — store their keys and ranks into the same lines
 * instead of one 4-B store per 16-B path block; else the slot index */
PMD size_t key_index(const TraceParams &P, uint32_t pid, uint32_t k) {
    const size_t path = path_slot_base(P, pid);
    return P.key_np > 0 ? (size_t)k * (size_t)P.key_np + path : path * (size_t)P.mpc + k;
}
PMD void flush_rank(const TraceParams &P, PathState &st) {
    if (st.pslot != PSLOT_NONE) { P.rank[st.pslot] = st.prank; st.pslot = PSLOT_NONE; }
}

/* HOLD kernels (k_trace_lane, k_trace_pool when max_photon_count is 4): a
 * path's first three deposits wait in LDS until the path ends, then its
 * 160-B slot block is written with 16-B stores, with its four bucket keys
 * and ranks as one 16-B store each (the fourth deposit ends the path, so it
 * is stored at once, next to the block's other writes). Writing each deposit
 * as it happens (photontracing.cu:141-151's owner-writes) stored five 8-B
 * pieces at a 160-B lane stride at different times, so L2 wrote partial lines
 * back several times (PMC: 2.2x the slot + key + rank bytes at C2, 2.9x at
 * C3). Registers were not an option: holding 36 words cost ~90 VGPRs in
 * the brute-force trace (4 -> 3 waves/SIMD). LDS: HOLD_WORDS x TRACE_BLOCK
 * words after the stacks and the scene blob, a column per thread. */
/* HOLD_MPC, HOLD_WORDS: pm_plan_pod.h */
struct Held {
    uint32_t *col;    /* this thread's LDS column: word i at col[i * TRACE_BLOCK] */
    uint4 key, rank;  /* shift registers, .x the newest deposit's; those beyond the path's count are never read */
};
PMD void held_put(Held &h, const TraceParams &P, size_t slot, uint32_t k, v3 p, v3 a, v3 wi, uint32_t key,
                  uint32_t rank) {
    if (k < 3u) {
        uint32_t *c = h.col + 9u * k * TRACE_BLOCK;
        c[0 * TRACE_BLOCK] = __float_as_uint(p.x); c[1 * TRACE_BLOCK] = __float_as_uint(p.y);
        c[2 * TRACE_BLOCK] = __float_as_uint(p.z); c[3 * TRACE_BLOCK] = __float_as_uint(a.x);
        c[4 * TRACE_BLOCK] = __float_as_uint(a.y); c[5 * TRACE_BLOCK] = __float_as_uint(a.z);
        c[6 * TRACE_BLOCK] = __float_as_uint(wi.x); c[7 * TRACE_BLOCK] = __float_as_uint(wi.y);
        c[8 * TRACE_BLOCK] = __float_as_uint(wi.z);
    } else {
        store_photon(P.slots + slot, 1u, p, a, wi); /* the last deposit: the block is written right after */
    }
    h.key = make_uint4(key, h.key.x, h.key.y, h.key.z);
    h.rank = make_uint4(rank, h.rank.x, h.rank.y, h.rank.z);
}
/* the path's slot block (16-B aligned: 160 B per path from a 16-B aligned
 * buffer, plan_trace's hold_launch): slots 0..2 from LDS (zero past the n
 * deposits), slot 3 zero unless its deposit was stored; with fused counting
 * the key and rank quads (key 0xffffffff past n) */
PMD void held_write(const TraceParams &P, uint32_t pid, const Held &h, uint32_t n) {
    const size_t path = path_slot_base(P, pid);
    uint32_t w[HOLD_WORDS];
#pragma unroll
    for (int i = 0; i < HOLD_WORDS; ++i) w[i] = (uint32_t)(i / 9) < n ? h.col[i * TRACE_BLOCK] : 0u;
    const uint32_t va = n > 0u, vb = n > 1u, vc = n > 2u;
    uint4 *dst = reinterpret_cast<uint4 *>(P.slots + path * HOLD_MPC);
    dst[0] = make_uint4(va, w[0], w[1], w[2]);
    dst[1] = make_uint4(w[3], w[4], w[5], w[6]);
    dst[2] = make_uint4(w[7], w[8], vb, w[9]);
    dst[3] = make_uint4(w[10], w[11], w[12], w[13]);
    dst[4] = make_uint4(w[14], w[15], w[16], w[17]);
    dst[5] = make_uint4(vc, w[18], w[19], w[20]);
    dst[6] = make_uint4(w[21], w[22], w[23], w[24]);
    if (n > 3u) {
        reinterpret_cast<uint2 *>(dst + 7)[0] = make_uint2(w[25], w[26]); /* slot 3 already stored */
    } else {
        dst[7] = make_uint4(w[25], w[26], 0u, 0u);
        dst[8] = make_uint4(0u, 0u, 0u, 0u);
        dst[9] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (P.bucket) {
        /* slot j = push n - 1 - j (wraps for j >= n: invalid) */
        const uint32_t q0 = n - 1u, q1 = n - 2u, q2 = n - 3u, q3 = n - 4u;
#define PICKQ(V, Q, DEF) ((Q) == 0u ? V.x : (Q) == 1u ? V.y : (Q) == 2u ? V.z : (Q) == 3u ? V.w : (DEF))
        reinterpret_cast<uint4 *>(P.key)[path] = make_uint4(PICKQ(h.key, q0, 0xffffffffu), PICKQ(h.key, q1, 0xffffffffu),
                                                            PICKQ(h.key, q2, 0xffffffffu), PICKQ(h.key, q3, 0xffffffffu));
        reinterpret_cast<uint4 *>(P.rank)[path] = make_uint4(PICKQ(h.rank, q0, 0u), PICKQ(h.rank, q1, 0u),
                                                             PICKQ(h.rank, q2, 0u), PICKQ(h.rank, q3, 0u));
#undef PICKQ
    }
}

/* Phase profile of k_trace (profiling builds only: `make prof` ->
 * lib/libpmhip_prof.so): per-wave s_memtime cycles accumulated per phase,
 * summed over waves into TraceParams::prof (pm_trace_profile). */
struct TProf {
#ifdef PM_TRACE_PROFILE
    uint64_t last = 0, start = 0, acc[6] = {0, 0, 0, 0, 0, 0};
    PMD void begin() { start = last = __builtin_amdgcn_s_memtime(); }
    PMD void mark(int i) {
        const uint64_t t = __builtin_amdgcn_s_memtime();
        acc[i] += t - last;
        last = t;
    }
    PMD void flush(unsigned long long *out) {
        if (!out || (threadIdx.x & 63) != 0) return;
        for (int i = 0; i < 6; ++i) atomicAdd(&out[i], (unsigned long long)acc[i]);
        atomicAdd(&out[6], (unsigned long long)(last - start));
        atomicAdd(&out[7], 1ull);
    }
#else
    PMD void begin() {}
    PMD void mark(int) {}
    PMD void flush(unsigned long long *) {}
#endif
};

/* PM_ALL_LIGHTS: the light a path starts on, the first l with
 * cdf[l] > min(u, 1 - 2^-24) of the light selection table (pm_api.h
 * pm_light_selection_cdf; u held below 1 so that the bin found is never
 * empty), and the probability of that pick as the float difference of its
 * table entries. The search is sample_light_mesh's: its trip count depends
 * on n alone, so the lanes of a wave stay together and only their addresses
 * differ (a few floats that L2 / TCP keep). */
PMD int pick_light(const float *cdf, int n, float u, float *pmf) {
    u = fminf(u, 0x1.fffffep-1f);
    int lo = 0, len = n;
    while (len > 1) {
        const int half = len >> 1;
        lo = cdf[lo + half - 1] > u ? lo : lo + half;
        len -= half;
    }
    *pmf = cdf[lo] - (lo > 0 ? cdf[lo - 1] : 0.f);
    return lo;
}

/* emission: Halton light sample -> first ray (photontracing.cu:88-117).
 * ALL (PM_ALL_LIGHTS, uniform per launch: a template argument, so the
 * fixed-light kernels keep their code and registers): the light is picked per
 * path with the sequence's fifth dimension — base 11, table perm + 17, at the
 * same index; permuted_radical_inverse itself (its modulo and the n *= invBase
 * quirk at every index: no floor shortcut to prove) — and the weight is
 * divided by the pick's probability last, so a probability of 1 leaves it bit
 * for bit. The other four dimensions and the bounce stream do not change: the
 * path is otherwise the path pid of the picked light. */
template <int ALL>
PMD bool emit_path(const TraceParams &P, const SceneDev &S, const uint32_t *perm, uint32_t pid, PathState &st) {
    const uint32_t pm_index = pid * (uint32_t)P.mpc;
    float smp[4];
    permuted_halton4(pm_index, perm, P.perm_bits, smp);
    int light = P.light_index;
    float pmf = 1.0f;
    if (ALL) light = pick_light(P.light_cdf, S.n_lights, permuted_radical_inverse(pm_index, 11u, perm + 17), &pmf);
    const LightDev Lt = S.lights[light];
    v3 N1; float pdf;
    v3 Le = sample_le(Lt, S.light_tris, smp[0], smp[1], smp[2], smp[3], P.eps, &st.ray, &N1, &pdf);
    st.pid = pid; st.nI = 0; st.spec = 0; st.stored = 0; st.pslot = PSLOT_NONE;
    if (pdf == 0.0f || is_black(Le)) return false;
    st.ray.tmax = RT_DEFAULT_MAX;
    st.alpha = (absdot(N1, st.ray.d) * Le) / pdf;
    /* an IEEE division per component (v3 / float multiplies by the reciprocal: two roundings) */
    if (ALL) st.alpha = mk(st.alpha.x / pmf, st.alpha.y / pmf, st.alpha.z / pmf);
    return true;
}

/* one ray of a path: trace, then specular continuation or diffuse deposit +
 * Lambert bounce (photontracing.cu:119-183); false when the path ends */
template <int HOLD, bool INST = false, bool TEX = false, bool SPEC = false, bool MARK = false>
PMD bool path_shade(const TraceParams &P, const SceneDev &S, PathState &st, const Hit &h, TProf &prof, Held &held);

template <int MODE, int HOLD, bool TEX, bool SPEC, bool MARK, class C>
PMD bool path_step(const TraceParams &P, const SceneDev &S, int *stack, PathState &st, C &cen, TProf &prof,
                   Held &held) {
    Hit h;
    const bool hit = traverse<false, MODE>(S, st.ray, h, stack, TRACE_BLOCK, cen);
    prof.mark(1);
    if (!hit) return false;
    return path_shade<HOLD, MODE == MODE_INST, TEX, SPEC, MARK>(P, S, st, h, prof, held);
}

/* the hit of a path's ray: specular continuation, or diffuse deposit +
 * Lambert bounce (photontracing.cu:119-183); false when the path ends.
 * HOLD: the deposit goes to `held` (written at path end, held_write).
 * TEX (a scene with a textured material): the Lambert bounce takes Kd from
 * the texture at the hit, so a photon off a red texel carries red.
 * SPEC (a scene with a material of the physical specular model, always with
 * TEX): such a material's step picks its lobe with a Philox draw of the
 * bounce stream's key at word 2 = the path's specular count (>= 1; the
 * Lambert bounce has 0 there) and scales alpha by the lobe's weight.
 * MARK (pm_set_caustic_map; never with HOLD, TEX or SPEC): a deposit made
 * before the path's first diffuse hit — at least one hit before it (nI >= 1)
 * and every one of them specular — is a caustic photon and gets bit 1 of its
 * bits word; st.diff carries "a diffuse hit has happened". Everything else
 * the kernel writes is the unmarked kernel's */
template <int HOLD, bool INST, bool TEX, bool SPEC, bool MARK>
PMD bool path_shade(const TraceParams &P, const SceneDev &S, PathState &st, const Hit &h, TProf &prof, Held &held) {
    static_assert(!MARK || (!HOLD && !TEX && !SPEC), "the MARK instantiations store per deposit in plain scenes");
    const uint32_t mpc = (uint32_t)P.mpc;
    Geo g = shade<INST>(S, st.ray, h);
    v3 hit_point = st.ray.o + h.t * st.ray.d;
    float4 m = S.materials[g.material];
    int mtype = fbits(m.w);
    prof.mark(3);
    if (is_specular(mtype)) {
        v3 wi;
        float4 sa, sb;
        bool pbrt = false;
        if (SPEC) {
            sa = S.mat_spec[2 * g.material]; sb = S.mat_spec[2 * g.material + 1];
            pbrt = fbits(sb.w) != 0;
        }
        if (SPEC && pbrt) {
            /* the counters first (the reference's model steps, then counts): the
             * draw below is keyed by spec and nI after their increments; a path
             * ends either way, so the order changes no outcome */
            if ((int)++st.spec > P.max_spec) return false;
            if (st.nI == 0) st.nI++;
            float u = 0.f;
            if (mtype == PM_GLASS) { /* nI >= 1 here, so path pid's counters never meet path pid + 1's */
                uint32_t o4[4];
                pmdm_philox4x32_10(st.pid * mpc + st.nI, (uint32_t)P.pass, st.spec, 0u, P.seed, 0u, o4);
                u = pmdm_u01(o4[0]);
            }
            v3 w; float eta2;
            if (!material_specular_pbrt(mtype, sa, sb, g, -st.ray.d, u, &wi, &w, &eta2)) return false;
            st.alpha = st.alpha * w; /* flux: no (ei / et)^2 (pbrt-v3's correction of v2) */
        } else {
            if (!material_specular(mtype, g, -st.ray.d, &wi)) return false;
            if ((int)++st.spec > P.max_spec) return false;
            if (st.nI == 0) st.nI++;
        }
        st.ray.o = hit_point; st.ray.d = wi; st.ray.tmin = P.eps; st.ray.tmax = RT_DEFAULT_MAX;
        return true;
    }
    v3 wo = -st.ray.d;
    if (st.nI >= 1) {
        const size_t slot = path_slot_base(P, st.pid) * mpc + (st.nI - 1);
        /* MARK is never built with HOLD (the static_assert above), so a MARK kernel always stores here */
        if (!HOLD) store_photon(P.slots + slot, MARK && !st.diff ? 3u : 1u, hit_point, st.alpha, wo);
        st.stored = st.nI;
        uint32_t key = 0xffffffffu, rank = 0u;
        if (P.bucket) { /* fused counting pass of the bucket build (pm_bucket.hip k_bucket_count) */
            const GridDesc &g = P.grid;
            const uint32_t cx = cell_axis(hit_point.x, g.gx, g.inv_cs, g.dx);
            const uint32_t cy = cell_axis(hit_point.y, g.gy, g.inv_cs, g.dy);
            const uint32_t cz = cell_axis(hit_point.z, g.gz, g.inv_cs, g.dz);
            key = (cz * (uint32_t)g.dy + cy) * (uint32_t)g.dx + cx;
            rank = atomicAdd(&P.count[key], 1u);
            if (!HOLD) {
                const size_t ki = key_index(P, st.pid, st.nI - 1);
                P.key[ki] = key;
                flush_rank(P, st);
                st.prank = rank; st.pslot = (uint32_t)ki;
            }
        }
        /* HOLD: the returned rank is first read at the path's end */
        if (HOLD) held_put(held, P, slot, st.nI - 1, hit_point, st.alpha, wo, key, rank);
    }
    if (MARK) st.diff = 1u;
    prof.mark(4);
    if (st.nI >= mpc) return false;
    const uint32_t pm_index = st.pid * mpc;
    uint32_t o4[4];
    pmdm_philox4x32_10(pm_index + st.nI, (uint32_t)P.pass, 0u, 0u, P.seed, 0u, o4);
    float u1 = pmdm_u01(o4[0]), u2 = pmdm_u01(o4[1]);
    v3 wiw; float bpdf;
    v3 kd = xyz(m);
    if (TEX) kd = hit_kd<INST>(S, h, hit_point, g.material, kd);
    v3 fr = sample_f(kd, g, wo, u1, u2, &wiw, &bpdf);
    if (is_black(fr) || bpdf == 0.f) return false;
    v3 anew = st.alpha * fr * absdot(wiw, g.ns) / bpdf;
    st.alpha = anew;
    st.nI++;
    st.ray.o = hit_point; st.ray.d = wiw; st.ray.tmin = P.eps; st.ray.tmax = RT_DEFAULT_MAX;
    prof.mark(5);
    return true;
}

/* a finished path's unused slots are invalid = zero (the reference leaves
 * them stale, DESIGN.md divergences); written here instead of a memset pass */
template <int HOLD = 0>
PMD void finish_path(const TraceParams &P, PathState &st, const Held *held = nullptr) {
    if (HOLD) { held_write(P, st.pid, *held, st.stored); return; }
    flush_rank(P, st);
    const uint32_t mpc = (uint32_t)P.mpc;
    pm_photon *slots = P.slots + path_slot_base(P, st.pid) * mpc;
    const float2 z = make_float2(0.f, 0.f);
    for (uint32_t k = st.stored; k < mpc; ++k) {
        float2 *q = reinterpret_cast<float2 *>(slots + k);
        /* lazy_zero (fused counting, env PM_LAZY_ZERO=1; off by default):
         * the invalid key alone marks the slot; the bucket fill never reads
         * it, and pm_api zeroes it before any other reader. 20-50 MB fewer
         * trace stores per pass, but no faster C2 trace on a same-box A/B and
         * a slower C4 bucket fill (46.5 -> 69 us; profiles/r05/trace_writes) */
        if (!P.lazy_zero) { q[0] = z; q[1] = z; q[2] = z; q[3] = z; q[4] = z; }
        if (P.bucket) P.key[key_index(P, st.pid, k)] = 0xffffffffu;
    }
}

/* the COUNT kernels' last act: the block's census into P.counters */
PMD void census_tail(const TraceParams &, const NoCensus &, uint32_t, uint32_t) {}
PMD void census_tail(const TraceParams &P, const Census &cen, uint32_t rays, uint32_t deposits) {
    count4(P.counters, rays, cen.nodes, cen.prims, deposits);
}

/* Per-lane photon tracer: one path per lane, no block barriers; a wave lives
 * as long as its longest path (C2: one occupancy round of 4,096 waves, 3.46
 * rays per path on average). Pools of several paths per lane, refilled as
 * lanes finish, and a block-compacting variant were measured slower (DESIGN.md
 * §5) and removed. HOLD: deposits held in LDS and written per path.
 * COUNT: census [rays traced, BVH nodes entered, primitive tests, photons
 * deposited], one atomic per wave (counting launches only, never timed). */
template <int COUNT, int MODE, int HOLD, int ALL, bool TEX, bool SPEC, bool MARK = false>
PMD void trace_lane_body(const TraceParams &P) {
    extern __shared__ __attribute__((aligned(16))) int stk[];
    __shared__ uint32_t perm[28];
    const int tid = threadIdx.x;
    if (tid < 28) perm[tid] = P.perm[tid];
    const SceneDev S = scene_view<mode_lds(MODE)>(P.S, reinterpret_cast<uint4 *>(stk + P.S.stack_depth * TRACE_BLOCK),
                                                       tid, TRACE_BLOCK);
    __syncthreads();
    int *stack = stk + tid;
    typename std::conditional<COUNT != 0, Census, NoCensus>::type cen;
    TProf prof;
    uint32_t rays = 0, deposits = 0;
    const int64_t path = (int64_t)blockIdx.x * TRACE_BLOCK + tid;
    PathState st;
    Held held;
    if (HOLD) /* after the stacks and the (16-B padded) scene blob: the layout plan_trace (pm_plan.cpp lane_lds) sizes */
        held.col = reinterpret_cast<uint32_t *>(stk + P.S.stack_depth * TRACE_BLOCK + (mode_lds(MODE) ? (int)((P.S.lds_bytes + 15u) / 4u & ~3u) : 0)) + tid;
    prof.begin();
    if (path < P.path_count) {
        bool alive = emit_path<ALL>(P, S, perm, (uint32_t)(P.path_begin + path), st);
        if (MARK) st.diff = 0u;
        prof.mark(0);
        while (alive) {
            ++rays;
            alive = path_step<MODE, HOLD, TEX, SPEC, MARK>(P, S, stack, st, cen, prof, held);
            prof.mark(2);
        }
        if (COUNT) deposits += st.stored;
        finish_path<HOLD>(P, st, &held);
    }
    prof.flush(P.prof);
    census_tail(P, cen, rays, deposits);
}

template <int COUNT, int MODE, int HOLD, int ALL = 0, bool TEX = false>
__global__ __launch_bounds__(TRACE_BLOCK) void k_trace_lane(TraceParams P) { trace_lane_body<COUNT, MODE, HOLD, ALL, TEX, false>(P); }
template <int COUNT, int MODE, int HOLD, int ALL>
__global__ __launch_bounds__(TRACE_BLOCK) void k_trace_lane_spec(TraceParams P) { trace_lane_body<COUNT, MODE, HOLD, ALL, true, true>(P); }
/* pm_set_caustic_map: k_trace_lane<COUNT, MODE, 0, ALL> that marks caustic photons */
template <int COUNT, int MODE, int ALL>
__global__ __launch_bounds__(TRACE_BLOCK) void k_trace_lane_mark(TraceParams P) { trace_lane_body<COUNT, MODE, 0, ALL, false, false, true>(P); }

/* Pooled photon tracer for scenes traversed from HBM with the 4-wide BVH
 * (C3). A ray's traversal lives across iterations of the wave's loop
 * (TravState: node, stack in LDS, pending leaves, best hit), so lanes whose
 * ray ended do not idle until the wave's longest ray ends: they wait until
 * at least POOL_SHADE_MIN lanes are ready (or nothing traverses), then those
 * lanes shade their hits together (deposit / bounce -> next ray) and lanes
 * without a path take the next ones of the wave's pool [wbegin, wend). The
 * rest of the time every iteration runs POOL_STEPS traversal steps for the
 * traversing lanes. Paths, slots and bucket counts are the per-lane
 * kernel's (owner-writes; the fused bucket ranks' order is immaterial). */
constexpr int POOL_SHADE_MIN = 16, POOL_STEPS = 4;
enum { PHASE_DEAD = 0, PHASE_TRAV = 1, PHASE_SHADE = 2 };
/* 5 waves/SIMD: 96 VGPRs with 28 B of scratch (104 B with held deposits;
 * unconstrained the kernel takes more registers and fits 4 waves); with
 * the LDS stacks capped at 31 entries (PM_POOL_STACK, the rest spilled) five
 * 256-thread blocks fit a CU. C3 trace (same box): 4.59-4.61 ms at 4 waves,
 * 4.41-4.42 ms at 5 (stack 31 or 24); 6 (80 VGPRs, 100 B of scratch) 4.58 */
constexpr int POOL_EU = 5;
/* the 8-wide walk: 4 waves/SIMD (102 VGPRs, 115 with held deposits, no
 * scratch); at 5 it spilled 88 B */
constexpr int POOL8_EU = 4;
#define POOL_OCC __attribute__((amdgpu_waves_per_eu(POOL_EU, POOL_EU)))
#define POOL8_OCC __attribute__((amdgpu_waves_per_eu(POOL8_EU, POOL8_EU)))

/* W8: the 8-wide tree (S.wide == 3, TravState8); ALL: emit_path's; TEX, SPEC, MARK: path_shade's */
template <int COUNT, int HOLD, int W8, int ALL, bool TEX, bool SPEC, bool MARK = false>
__device__ __forceinline__ void trace_pool_body(TraceParams P) {
    extern __shared__ __attribute__((aligned(16))) int stk[];
    __shared__ uint32_t perm[28];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 28) perm[tid] = P.perm[tid];
    const SceneDev &S = P.S;
    __syncthreads();
    int *stack = stk + tid;
    /* LDS stack entries per lane (P.pool_stack, else the tree's bound); deeper ones spill to global memory.
     * plan_trace (pm_plan.cpp) sizes the launch's LDS for this lstk (+ the held columns) and the spill
     * area for grid x TRACE_BLOCK threads (P.spill_stride) */
    const int lstk = P.pool_stack > 0 && P.pool_stack < P.S.stack_depth ? P.pool_stack : P.S.stack_depth;
    const SpillStack sstk{stack, TRACE_BLOCK, lstk, P.spill, P.spill_stride, (uint32_t)(blockIdx.x * TRACE_BLOCK + tid)};
    typename std::conditional<COUNT != 0, Census, NoCensus>::type cen;
    TProf prof;
    uint32_t rays = 0, deposits = 0;
    const int64_t wave_id = ((int64_t)blockIdx.x * TRACE_BLOCK + tid) >> 6;
    const int64_t wbegin = wave_id * P.pool_paths;
    const int64_t wend = wbegin + P.pool_paths < P.path_count ? wbegin + P.pool_paths : P.path_count;
    int64_t cursor = wbegin; /* wave-uniform: next unassigned path of the pool */
    PathState st;
    typename std::conditional<W8 != 0, TravState8, TravState>::type tr;
    Held held;
    if (HOLD) held.col = reinterpret_cast<uint32_t *>(stk + lstk * TRACE_BLOCK) + tid; /* after the stacks */
    int phase = PHASE_DEAD;
    while (true) {
        const unsigned long long travm = __ballot(phase == PHASE_TRAV);
        const unsigned long long shadem = __ballot(phase == PHASE_SHADE);
        const unsigned long long deadm = __ballot(phase == PHASE_DEAD);
        const bool pool_left = cursor < wend;
        if (travm == 0ull && shadem == 0ull && !pool_left) break; /* every lane reaches it together */
        const int waiting = __popcll(shadem) + (pool_left ? __popcll(deadm) : 0);
        if (travm == 0ull || waiting >= POOL_SHADE_MIN) {
            if (phase == PHASE_SHADE) {
                ++rays;
                const bool alive = tr.best.ref != 0xffffffffu && path_shade<HOLD, false, TEX, SPEC, MARK>(P, S, st, tr.best, prof, held);
                if (alive) {
                    trav_begin(st.ray, tr);
                    phase = PHASE_TRAV;
                } else {
                    if (COUNT) deposits += st.stored;
                    finish_path<HOLD>(P, st, &held);
                    phase = PHASE_DEAD;
                }
            }
            const unsigned long long dm = __ballot(phase == PHASE_DEAD);
            if (cursor < wend) {
                const int64_t mine = cursor + __popcll(dm & ((1ull << lane) - 1ull));
                if (phase == PHASE_DEAD && mine < wend) {
                    const bool emitted = emit_path<ALL>(P, S, perm, (uint32_t)(P.path_begin + mine), st);
                    if (MARK) st.diff = 0u;
                    if (emitted) {
                        trav_begin(st.ray, tr);
                        phase = PHASE_TRAV;
                    } else {
                        finish_path<HOLD>(P, st, &held);
                    }
                }
                cursor = cursor + __popcll(dm) < wend ? cursor + __popcll(dm) : wend;
            }
            continue;
        }
#pragma unroll 1
        for (int k = 0; k < POOL_STEPS; ++k)
            if (phase == PHASE_TRAV && !trav_step(S, st.ray, tr, sstk, cen)) phase = PHASE_SHADE;
    }
    census_tail(P, cen, rays, deposits);
}

template <int COUNT, int HOLD, int ALL = 0, bool TEX = false>
__global__ __launch_bounds__(TRACE_BLOCK) POOL_OCC void k_trace_pool(TraceParams P) { trace_pool_body<COUNT, HOLD, 0, ALL, TEX, false>(P); }
template <int COUNT, int HOLD, int ALL>
__global__ __launch_bounds__(TRACE_BLOCK) POOL_OCC void k_trace_pool_spec(TraceParams P) { trace_pool_body<COUNT, HOLD, 0, ALL, true, true>(P); }
template <int COUNT, int HOLD, int ALL = 0, bool TEX = false>
__global__ __launch_bounds__(TRACE_BLOCK) POOL8_OCC void k_trace_pool8(TraceParams P) { trace_pool_body<COUNT, HOLD, 1, ALL, TEX, false>(P); }
template <int COUNT, int HOLD, int ALL>
__global__ __launch_bounds__(TRACE_BLOCK) POOL8_OCC void k_trace_pool8_spec(TraceParams P) { trace_pool_body<COUNT, HOLD, 1, ALL, true, true>(P); }
/* pm_set_caustic_map: k_trace_pool<COUNT, 0, ALL> / k_trace_pool8<COUNT, 0, ALL> that mark caustic photons */
template <int COUNT, int ALL>
__global__ __launch_bounds__(TRACE_BLOCK) POOL_OCC void k_trace_pool_mark(TraceParams P) { trace_pool_body<COUNT, 0, 0, ALL, false, false, true>(P); }
template <int COUNT, int ALL>
__global__ __launch_bounds__(TRACE_BLOCK) POOL8_OCC void k_trace_pool8_mark(TraceParams P) { trace_pool_body<COUNT, 0, 1, ALL, false, false, true>(P); }

/* MAT: which instantiations a scene runs: 0 = the plain ones, 1 = TEX (a
 * textured material), 2 = SPEC (a material of the physical specular model),
 * 3 = MARK (a plain scene under pm_set_caustic_map; HOLD is 0 by the plan,
 * so the HOLD = 1 arms below name the same kernel and never launch) */
template <int COUNT, int MODE, int HOLD, int ALL, int MAT>
static auto lane_kernel() {
    if constexpr (MAT == 3) return &k_trace_lane_mark<COUNT, MODE, ALL>;
    else if constexpr (MAT == 2) return &k_trace_lane_spec<COUNT, MODE, HOLD, ALL>;
    else return &k_trace_lane<COUNT, MODE, HOLD, ALL, MAT == 1>;
}
template <int COUNT, int HOLD, int W8, int ALL, int MAT>
static auto pool_kernel() {
    if constexpr (W8 != 0) {
        if constexpr (MAT == 3) return &k_trace_pool8_mark<COUNT, ALL>;
        else if constexpr (MAT == 2) return &k_trace_pool8_spec<COUNT, HOLD, ALL>;
        else return &k_trace_pool8<COUNT, HOLD, ALL, MAT == 1>;
    } else {
        if constexpr (MAT == 3) return &k_trace_pool_mark<COUNT, ALL>;
        else if constexpr (MAT == 2) return &k_trace_pool_spec<COUNT, HOLD, ALL>;
        else return &k_trace_pool<COUNT, HOLD, ALL, MAT == 1>;
    }
}
/* f(std::integral_constant<int, MAT>): dispatch_flag (pm_kernels.h) for the four-valued MAT of this unit */
template <class F>
static void dispatch_mat(int mat, F &&f) {
    switch (mat) {
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    default: f(std::integral_constant<int, 0>{}); break;
    }
}
/* f(kernel) for the kernel of a family: the pooled ones by tree width, the
 * per-lane ones by traversal mode (instances: the per-lane kernel, the pooled
 * one walks only one level; plan_trace asks trace_waves_per_cu for
 * TRACE_LANE_GLOBAL's occupancy in their place, never TRACE_LANE_INST's) */
template <int COUNT, int HOLD, int ALL, int MAT, class F>
static void dispatch_family(TraceFamily family, F &&f) {
    if (family == TRACE_POOL || family == TRACE_POOL8) {
        dispatch_flag(family == TRACE_POOL8, [&](auto W8) { f(pool_kernel<COUNT, HOLD, decltype(W8)::value, ALL, MAT>()); });
    } else {
        const int mode = family == TRACE_LANE_BRUTE ? MODE_BRUTE : family == TRACE_LANE_LDS ? MODE_LDS
                         : family == TRACE_LANE_INST ? MODE_INST : MODE_GLOBAL;
        dispatch_mode(mode, [&](auto MODE) { f(lane_kernel<COUNT, decltype(MODE)::value, HOLD, ALL, MAT>()); });
    }
}

/* resident waves per CU of a trace kernel family at `lds` bytes of dynamic
 * LDS (0 if unknown): the occupancy plan_trace (pm_plan.h) asks for. The
 * bytes are the plan's; this only picks the kernel */
int trace_waves_per_cu(TraceFamily family, bool hold, size_t lds) {
    int blocks = 0;
    dispatch_flag(hold, [&](auto HOLD) {
        dispatch_family<0, decltype(HOLD)::value, 0, 0>(family, [&](auto kernel) {
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kernel, TRACE_BLOCK, lds) != hipSuccess) blocks = 0;
        });
    });
    return blocks * (TRACE_BLOCK / 64);
}

/* kernel, grid and LDS bytes are the plan's (plan_trace, pm_plan.h: the one
 * place they are computed); p carries the same plan's pool_stack, pool_paths,
 * hold and spill_stride to the kernel. A scene with a material of the
 * physical specular model (SceneDev::mat_spec) runs the SPEC instantiations,
 * one with a textured material (SceneDev::tex_recs) the TEX ones, a plain one
 * under pm_set_caustic_map the MARK ones (deposits stored one by one:
 * plan_trace under TraceShape::mark); every other scene the kernels it ran
 * before any of these existed */
hipError_t launch_trace(const TraceParams &p, const TracePlan &pl, int count, hipStream_t s) {
    if (p.path_count <= 0) return hipSuccess;
    const int mat = p.mark ? 3 : p.S.mat_spec ? 2 : p.S.tex_recs ? 1 : 0;
    /* PM_ALL_LIGHTS: the ALL instantiations; a fixed light is an index into S.lights */
    const bool all = p.light_index == PM_ALL_LIGHTS;
    if ((p.mark && (p.S.mat_spec || p.S.tex_recs || pl.hold_launch || p.hold)) || (mat == 2 && !p.S.mat_tex) ||
        (all ? !p.light_cdf : p.light_index < 0 || p.light_index >= p.S.n_lights) ||
        (pl.pooled && pl.spill_entries > 0 && !p.spill))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)pl.grid_blocks);
    const size_t lds = pl.hold_launch ? pl.lds_hold : pl.lds;
    dispatch_flag(count != 0, [&](auto COUNT) { dispatch_flag(pl.hold_launch, [&](auto HOLD) { dispatch_flag(all, [&](auto ALL) {
        dispatch_mat(mat, [&](auto MAT) {
            dispatch_family<decltype(COUNT)::value, decltype(HOLD)::value, decltype(ALL)::value, decltype(MAT)::value>(
                pl.family, [&](auto kernel) { pm_launch(kernel, grid, dim3(TRACE_BLOCK), lds, s, p); });
        });
    }); }); });
    return hipGetLastError();
}

} // namespace pm
