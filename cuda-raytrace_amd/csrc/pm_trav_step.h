/*
 * pm_trav_step.h — the resumable closest-hit walks of the pooled trace
 * kernels (pm_trace.hip k_trace_pool / k_trace_pool8, their only user): a
 * ray's traversal kept alive across iterations of an outer loop (TravState,
 * TravState8), advanced a step at a time (trav_step), its stack in LDS with a
 * spill area in global memory (SpillStack).
 */
#pragma once
#include "pm_traverse.h"

#pragma clang fp contract(off)

namespace pm {

/* a lane's traversal stack: entries below cap in its LDS column, deeper ones (rare: the bound is exact, typical
 * depths are far below it) in a global spill area, entry i of thread gid at spill[(i - cap) * sstride + gid] — so the
 * LDS a block reserves can be sized for occupancy, not the worst ray */
struct SpillStack {
    int *lds;
    int stride, cap;
    int *spill;
    uint32_t sstride, gid;
    PMD void put(int i, int v) const {
        if (i < cap) lds[i * stride] = v;
        else spill[(size_t)(i - cap) * sstride + gid] = v;
    }
    PMD int get(int i) const { return i < cap ? lds[i * stride] : spill[(size_t)(i - cap) * sstride + gid]; }
};

/* Resumable closest-hit traversal for kernels that keep a ray's traversal alive across iterations of an outer loop
 * (k_trace_pool): trav_step advances by one node visit or one leaf and returns false once the ray is done (best holds
 * its closest hit, if any); the result equals traverse4's / traverse8's (same culling, same leaf tests, same
 * tie-break). */
/* the 8-wide walk's state: no pending queue (the registers of eight queued leaves spilled the pooled kernel), a visit
 * tests its hit leaves itself */
struct TravState8 {
    RaySlab rs; /* the high planes' offset is rebuilt per visit (ray_oinv_hi) */
    Hit best;
    int cur, sp, guard;
};
/* the 4-wide walk's: and the pending leaves */
struct TravState : TravState8 {
    LeafQueue leaves;
};
PMD void trav_begin(const Ray &ray, TravState8 &t) {
    best_begin(t.best, ray.tmax);
    t.best.beta = t.best.gamma = 0.f;
    t.rs = ray_slab(ray);
    t.cur = 0; t.sp = 0; t.guard = 0;
}
PMD void trav_begin(const Ray &ray, TravState &t) {
    trav_begin(ray, static_cast<TravState8 &>(t));
    t.leaves.clear();
}

template <class C>
PMD bool trav_step(const SceneDev &S, const Ray &ray, TravState &T, const SpillStack &stk, C &cen) {
    /* (requesting the node before the pending leaf's test, so a wave's leaf and node loads overlap, measured slower:
     * C3 trace 4.14 -> 4.22-4.27 ms, 88 B of scratch at 5 waves/SIMD or 4.23-4.26 ms at 4; profiles/r05/trace_c3) */
    if (T.leaves.n0 != 0) {
        leaf_isect<false, true>(S, T.leaves.s0, T.leaves.n0, ray, T.best, cen);
        T.leaves.pop();
        /* the last pending leaf done: this step also visits the next node, so a lane's leaf tests share steps with
         * node visits (the wave runs both codes whenever its lanes differ anyway). Against a step that ends after
         * every leaf, C3 trace per 1M paths 4.42-4.43 -> 4.07-4.10 ms (same box, round 3); also testing the first
         * leaf a visit finds in the same step: 4.44 (the second leaf code costs every step) */
        if (T.leaves.n0 != 0) return true;
    }
    if (T.cur < 0 || T.guard > S.n_nodes) return false;
    ++T.guard;
    cen.node();
    float t[4];
    int c[4], n[4];
    node4_test(S, T.cur, T.rs, ray_oinv_hi(T.rs, ray.o), ray.tmin, T.best.t, t, c, n);
    /* the pending-leaf queue is empty here (a visit follows the last pending leaf's test): the hit leaves, in child
     * order, enter it by shifting from the back — selects only, no branch per child. (traverse4's chain of
     * first-free-slot tests measured slower here: C3 trace 3.86-3.88 vs 3.81-3.85 ms, profiles/r05/trace_c3
     * pool_tuning.) */
    T.leaves.clear();
#pragma unroll
    for (int k = 3; k >= 0; --k)
        if (t[k] != INF && n[k] > 0) T.leaves.push_front((uint32_t)~c[k], (uint32_t)n[k]);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (n[k] != 0) t[k] = INF;
    /* next4 written out: called here it cost two counting pooled kernels 8 B more scratch (124 -> 132, 204 -> 212) */
    auto cs = [&](int a, int b) {
        if (t[b] < t[a]) { const float tt = t[a]; t[a] = t[b]; t[b] = tt; const int cc = c[a]; c[a] = c[b]; c[b] = cc; }
    };
    cs(0, 1); cs(2, 3); cs(0, 2); cs(1, 3); cs(1, 2);
    if (t[3] != INF) { stk.put(T.sp, c[3]); ++T.sp; }
    if (t[2] != INF) { stk.put(T.sp, c[2]); ++T.sp; }
    if (t[1] != INF) { stk.put(T.sp, c[1]); ++T.sp; }
    if (t[0] != INF) T.cur = c[0];
    else T.cur = pop_or_done(stk, T.sp);
    return T.leaves.n0 != 0 || T.cur >= 0;
}
/* one node visit per step, its hit leaves tested in the same step */
template <class C>
PMD bool trav_step(const SceneDev &S, const Ray &ray, TravState8 &T, const SpillStack &stk, C &cen) {
    if (T.cur < 0 || T.guard > S.n_nodes) return false;
    ++T.guard;
    cen.node();
    int next = -1;
    visit8<false>(S, T.cur, ray, T.rs, T.best, cen, next, [&](int v) { stk.put(T.sp, v); ++T.sp; });
    T.cur = next >= 0 ? next : pop_or_done(stk, T.sp);
    return T.cur >= 0;
}

} // namespace pm
