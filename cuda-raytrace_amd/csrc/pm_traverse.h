/*
 * pm_traverse.h — the one-call closest-hit and any-hit ray queries: the
 * binary walk (traverse2), the quantized 4-wide walk (traverse4) with the
 * instance walk (blas_isect), the 8-wide walk (visit8, traverse8) and the
 * traverse<ANY, MODE> front that picks one. Boxes: pm_slab.h; primitives:
 * pm_leaf.h. Included by the units that trace rays: pm_trace.hip (through
 * pm_trav_step.h, its resumable walk) and, through pm_eye_dev.h, pm_eye.hip
 * and pm_fgather.hip.
 */
#pragma once
#include "pm_leaf.h"
#include "pm_slab.h"

#pragma clang fp contract(off)

namespace pm {

/* a lane's traversal stack: a column of LDS, entry i at col[i * stride] */
struct LaneStack {
    int *col, stride;
    PMD void put(int i, int v) const { col[i * stride] = v; }
    PMD int get(int i) const { return col[i * stride]; }
};
/* the tail of every walk's visit: the deepest pushed node, or -1 when none is left */
template <class Stk>
PMD int pop_or_done(const Stk &stk, int &sp) {
    if (sp > 0) { --sp; return stk.get(sp); }
    return -1;
}
/* a 4-wide node's hit internal children (every other child's t set to INF) ordered near to far with a sorting
 * network, (0,1) (2,3) (0,2) (1,3) (1,2); the farther ones are pushed far to near, and the nearest — else the stack's
 * top, else -1 — is the node to enter next */
template <class Stk>
PMD int next4(float t[4], int c[4], const Stk &stk, int &sp) {
    auto cs = [&](int a, int b) {
        if (t[b] < t[a]) { const float tt = t[a]; t[a] = t[b]; t[b] = tt; const int cc = c[a]; c[a] = c[b]; c[b] = cc; }
    };
    cs(0, 1); cs(2, 3); cs(0, 2); cs(1, 3); cs(1, 2);
#pragma unroll
    for (int k = 3; k >= 1; --k)
        if (t[k] != INF) { stk.put(sp, c[k]); ++sp; }
    return t[0] != INF ? c[0] : pop_or_done(stk, sp);
}

/* Leaves found while descending are postponed (at most the four children of one node: first ref and count, count 0 =
 * none) and tested in a separate loop, so a wave runs the primitive code once for all lanes that reached leaves
 * instead of once per node iteration for a few of them (Aila & Laine's "while-while"). Culling is unchanged: a
 * postponed leaf's box was hit within the current best t. */
struct LeafQueue {
    uint32_t s0, n0, s1, n1, s2, n2, s3, n3;
    PMD void clear() { s0 = n0 = s1 = n1 = s2 = n2 = s3 = n3 = 0; }
    PMD void pop() { s0 = s1; n0 = n1; s1 = s2; n1 = n2; s2 = s3; n2 = n3; n3 = 0; }
    PMD void push(uint32_t s, uint32_t n) { /* traverse4's: into the first free slot */
        if (n0 == 0) { s0 = s; n0 = n; }
        else if (n1 == 0) { s1 = s; n1 = n; }
        else if (n2 == 0) { s2 = s; n2 = n; }
        else { s3 = s; n3 = n; }
    }
    PMD void push_front(uint32_t s, uint32_t n) { /* trav_step's (pm_trav_step.h, with the measurement) */
        s3 = s2; n3 = n2; s2 = s1; n2 = n1; s1 = s0; n1 = n0; s0 = s; n0 = n;
    }
};

/* BVH traversal with a per-lane stack column in LDS (stack[depth*stride]). Closest hit (ANY=false) or occlusion
 * (ANY=true). Node = 4 float4: (l.lo, l.hi.x) (l.hi.yz, r.lo.xy) (r.lo.z, r.hi) (left, right, lcount, rcount); child
 * >= 0 internal node, child < 0 leaf with refs start ~child. */
template <bool ANY, class C>
PMD bool traverse2(const SceneDev &S, const Ray &ray, Hit &best, int *stack, int stride, C &cen) {
    best_begin(best, ray.tmax);
    const RaySlab rs = ray_slab(ray);
    const LaneStack stk{stack, stride};
    int sp = 0, cur = 0; /* cur: next node to enter; -1: none left */
    /* its two pending leaves as scalars: a queue struct cost the MODE_LDS trace kernels 36 B of scratch, two a wave */
    uint32_t l0s = 0, l0n = 0, l1s = 0, l1n = 0;
    int guard = 0; /* every node is entered at most once per ray: a bound every lane reaches */
    while (true) {
        while (cur >= 0 && l0n == 0 && guard <= S.n_nodes) {
            ++guard;
            cen.node();
            const float4 *nd = S.nodes + 4 * cur;
            float4 a = nd[0], b = nd[1], c = nd[2];
            int4 ch = *reinterpret_cast<const int4 *>(nd + 3);
            const v3 oinvH = ray_oinv_hi(rs, ray.o);
            float tl = box_near(a.x, a.y, a.z, a.w, b.x, b.y, rs, oinvH, ray.tmin, best.t);
            float tr = box_near(b.z, b.w, c.x, c.y, c.z, c.w, rs, oinvH, ray.tmin, best.t);
            bool hl = tl != INF && ch.z >= 0;
            bool hr = tr != INF && ch.w >= 0;
            if (hl && ch.x < 0) { l0s = (uint32_t)~ch.x; l0n = (uint32_t)ch.z; hl = false; }
            if (hr && ch.y < 0) {
                if (l0n == 0) { l0s = (uint32_t)~ch.y; l0n = (uint32_t)ch.w; }
                else { l1s = (uint32_t)~ch.y; l1n = (uint32_t)ch.w; }
                hr = false;
            }
            if (hl && hr && sp < S.stack_depth) {
                int nearc = ch.x, farc = ch.y;
                if (tr < tl) { nearc = ch.y; farc = ch.x; }
                stk.put(sp, farc);
                ++sp;
                cur = nearc;
            } else if (hl) {
                cur = ch.x;
            } else if (hr) {
                cur = ch.y;
            } else {
                cur = pop_or_done(stk, sp);
            }
        }
        while (l0n != 0) {
            if (leaf_isect<ANY>(S, l0s, l0n, ray, best, cen)) return true;
            l0s = l1s; l0n = l1n; l1n = 0;
        }
        if (cur < 0 || guard > S.n_nodes) break;
    }
    return found<ANY>(best);
}

/* 4-wide traversal (MODE_GLOBAL scenes with S.wide == 2): one 64-B node per visit, its four boxes tested at once; hit
 * internal children are ordered near to far, the nearest entered next and the rest pushed (next4; the stack is sized
 * by the builder's max_stack); hit leaves are postponed and tested together as in traverse2() (at most four per
 * node). INST: the scene's top-level tree, whose leaves may hold instances (MODE_INST). */
template <bool ANY, class C, bool INST = false>
PMD bool traverse4(const SceneDev &S, const Ray &ray, Hit &best, int *stack, int stride, C &cen) {
    best_begin(best, ray.tmax);
    const RaySlab rs = ray_slab(ray);
    const LaneStack stk{stack, stride};
    int sp = 0, cur = 0, guard = 0;
    LeafQueue leaves;
    leaves.clear();
    while (true) {
        while (cur >= 0 && leaves.n0 == 0 && guard <= S.n_nodes) {
            ++guard;
            cen.node();
            float t[4];
            int c[4], n[4];
            node4_test(S, cur, rs, ray_oinv_hi(rs, ray.o), ray.tmin, best.t, t, c, n);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (t[k] != INF && n[k] > 0) leaves.push((uint32_t)~c[k], (uint32_t)n[k]); /* leaf: postpone */
                if (n[k] != 0) t[k] = INF; /* only internal children stay */
            }
            cur = next4(t, c, stk, sp);
        }
        while (leaves.n0 != 0) {
            /* instance trees use the stack entries above the ones in use */
            if (leaf_isect<ANY, true, C, INST>(S, leaves.s0, leaves.n0, ray, best, cen, stack + sp * stride, stride))
                return true;
            leaves.pop();
        }
        if (cur < 0 || guard > S.n_nodes) break;
    }
    return found<ANY>(best);
}

/* ------------------------------------------------------ instance trees */
/* Closest hit (or any hit) among an instance's triangles. The object tree is walked in object space: the ray taken
 * through w2o (o' = w2o o, d' = w2o d; the same t parameterises both, the transform being affine) and every box
 * widened by pad = 1e-5 (a (2 |o| + W) + k B), a = |w2o| (row sums), W the instance's world extent, k = |o2w| |w2o|,
 * B the object's extent (both per instance, I[7]) — beyond the rounding of o', d' and of the world vertices mapped
 * back (~3 ulps of those magnitudes), so culling is conservative: every triangle that can win is tested. Triangles
 * are rebuilt in world space (inst_tri) and tested with the world ray like a flattened mesh's, so hits equal the
 * flattened scene's bit for bit. The stack entries above the caller's hold the walk (collapse_bvh4's bound). */
template <bool ANY, class C>
PMD bool blas_isect(const SceneDev &S, uint32_t inst, const Ray &ray, Hit &best, int *stack, int stride, C &cen) {
    const float4 *I = S.insts + 8 * inst;
    const float4 hd = I[6], pk = I[7];
    const uint32_t gid0 = (uint32_t)__float_as_int(hd.z);
    const float4 w0 = I[3], w1 = I[4], w2 = I[5];
    const v3 o = inst_point(I + 3, ray.o.x, ray.o.y, ray.o.z);
    const v3 d = mk((w0.x * ray.d.x + w0.y * ray.d.y) + w0.z * ray.d.z, (w1.x * ray.d.x + w1.y * ray.d.y) + w1.z * ray.d.z,
                    (w2.x * ray.d.x + w2.y * ray.d.y) + w2.z * ray.d.z);
    const float on = fmaxf(fabsf(ray.o.x), fmaxf(fabsf(ray.o.y), fabsf(ray.o.z)));
    const float pad = 1e-5f * (pk.y * (2.f * on) + pk.z);
    const v3 inv = safe_inv(d);
    const RaySlab rs{inv, mk((o.x + pad) * inv.x, (o.y + pad) * inv.y, (o.z + pad) * inv.z)};
    const v3 oH = mk((o.x - pad) * inv.x, (o.y - pad) * inv.y, (o.z - pad) * inv.z);
    const LaneStack stk{stack, stride};
    int sp = 0, cur = __float_as_int(hd.x), guard = 0;
    while (cur >= 0 && guard <= S.n_nodes) {
        ++guard;
        cen.node();
        float t[4];
        int c[4], n[4];
        node4_test(S, cur, rs, oH, ray.tmin, best.t, t, c, n);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (t[k] == INF || n[k] <= 0) continue;
            /* a leaf: its triangles at object slots [~c, ~c + count) (LEAF_TRIS) */
            const uint32_t s0 = (uint32_t)~c[k], cnt = (uint32_t)n[k] & 0x3fffu;
            for (uint32_t q = s0; q < s0 + cnt; ++q) {
                cen.prim();
                v3 p0, p1, p2;
                float4 g[3];
                inst_tri(S, I, q, p0, p1, p2, g);
                float tt, bb, gg;
                const bool ok = isect_tri_v(g[0], g[1], g[2], ray, &tt, &bb, &gg);
                if (ANY) { if (ok) return true; continue; }
                if (!ok || tt > best.t) continue;
                consider(best, tt, bb, gg, (PRIM_INST << 30) | q, gid0 + (uint32_t)__float_as_int(S.obj_v[3 * q].w));
            }
            t[k] = INF;
        }
        cur = next4(t, c, stk, sp); /* internal children: nearest next, the others pushed */
    }
    return false;
}

/* ------------------------------------------------------- 8-wide trees */
/* a node's hit internal children near to far: 32-bit keys (the entry t's bits — non-negative floats order like their
 * bits — with the low three replaced by the child's slot; misses and leaves sort last as ~0) through Batcher's
 * odd-even merge network for 8 (19 min/max pairs). The order only steers the walk; hits do not depend on it
 * (lowest-id tie-break). */
PMD void sort8_keys(uint32_t k[8]) {
    auto cs = [&](int a, int b) { const uint32_t lo = min(k[a], k[b]), hi = max(k[a], k[b]); k[a] = lo; k[b] = hi; };
    cs(0, 1); cs(2, 3); cs(4, 5); cs(6, 7);
    cs(0, 2); cs(1, 3); cs(4, 6); cs(5, 7);
    cs(1, 2); cs(5, 6);
    cs(0, 4); cs(1, 5); cs(2, 6); cs(3, 7);
    cs(2, 4); cs(3, 5);
    cs(1, 2); cs(3, 4); cs(5, 6);
}
PMD int child8(const int c[8], uint32_t slot) { /* c[slot & 7] by selects (no dynamic register index) */
    const int a = (slot & 1u) ? c[1] : c[0], b = (slot & 1u) ? c[3] : c[2];
    const int d = (slot & 1u) ? c[5] : c[4], e = (slot & 1u) ? c[7] : c[6];
    const int f = (slot & 2u) ? b : a, g = (slot & 2u) ? e : d;
    return (slot & 4u) ? g : f;
}
/* one node visit of the 8-wide walk: the hit leaves tested at once (every lane's, in one pass of the wave), the hit
 * internal children sorted, the nearest returned in `next` (-1: none) and the others pushed far to near */
template <bool ANY, class C, class Put>
PMD bool visit8(const SceneDev &S, int node, const Ray &ray, const RaySlab &rs, Hit &best, C &cen, int &next,
                Put &&stack_put) {
    float t[8];
    int c[8];
    node8_test(S, node, rs, ray_oinv_hi(rs, ray.o), ray.tmin, best.t, t, c);
    uint32_t key[8], lm = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (t[k] != INF && c[k] < 0) lm |= 1u << k;
        key[k] = t[k] != INF && c[k] >= 0 ? (__float_as_uint(t[k]) & ~7u) | (uint32_t)k : 0xffffffffu;
    }
    /* the hit leaves, one per lane per round: as many rounds as the lane with the most (unrolled per slot, the wave
     * ran the leaf code for every slot any lane hit) */
    while (lm != 0u) {
        const uint32_t k = (uint32_t)__builtin_ctz(lm);
        lm &= lm - 1u;
        if (leaf8_isect<ANY>(S, child8(c, k), ray, best, cen) && ANY) return true;
    }
    sort8_keys(key);
#pragma unroll
    for (int k = 7; k >= 1; --k)
        if (key[k] != 0xffffffffu) stack_put(child8(c, key[k]));
    next = key[0] != 0xffffffffu ? child8(c, key[0]) : -1;
    return false;
}
/* one-call closest / any hit on the 8-wide tree (eye pass, shadow rays, per-lane kernels) */
template <bool ANY, class C>
PMD bool traverse8(const SceneDev &S, const Ray &ray, Hit &best, int *stack, int stride, C &cen) {
    best_begin(best, ray.tmax);
    const RaySlab rs = ray_slab(ray);
    const LaneStack stk{stack, stride};
    int sp = 0, cur = 0, guard = 0;
    while (cur >= 0 && guard <= S.n_nodes) {
        ++guard;
        cen.node();
        int next = -1;
        if (visit8<ANY>(S, cur, ray, rs, best, cen, next, [&](int v) { stk.put(sp, v); ++sp; })) return true;
        cur = next >= 0 ? next : pop_or_done(stk, sp);
    }
    return found<ANY>(best);
}

/* the query every kernel calls: the walk of the scene's traversal mode */
template <bool ANY, int MODE, class C>
PMD bool traverse(const SceneDev &S, const Ray &ray, Hit &best, int *stack, int stride, C &cen) {
    if constexpr (MODE == MODE_BRUTE) {
        best_begin(best, ray.tmax);
        cen.node();
        if (brute_isect<ANY>(S, ray, best, cen)) return true;
        return found<ANY>(best);
    } else if constexpr (MODE == MODE_INST) {
        return traverse4<ANY, C, true>(S, ray, best, stack, stride, cen);
    } else {
        if constexpr (MODE == MODE_GLOBAL) {
            if (S.wide == 3) return traverse8<ANY>(S, ray, best, stack, stride, cen);
            if (S.wide) return traverse4<ANY>(S, ray, best, stack, stride, cen);
        }
        return traverse2<ANY>(S, ray, best, stack, stride, cen);
    }
}
template <bool ANY, int MODE>
PMD bool traverse(const SceneDev &S, const Ray &ray, Hit &best, int *stack, int stride) {
    NoCensus none;
    return traverse<ANY, MODE>(S, ray, best, stack, stride, none);
}

} // namespace pm
