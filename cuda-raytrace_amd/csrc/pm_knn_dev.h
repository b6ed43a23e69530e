/*
 * pm_knn_dev.h — device-inline code shared by the kNN gather kernels
 * (pm_gather_knn.hip: k_gather_knn, k_gather_knn_tile; pm_gather_knn_ss.hip:
 * k_gather_knn_ss), which compute one estimate bit for bit: the exact
 * fixed-point term (Kx3, knn_rnd, knn_facing, knn_add, knn_scale), a lane's
 * cell box (knn_cells), the per-lane row scan (KnnGrid, cell_gap), the row
 * map's pitch (rowmap_bits) and the leader groups' reach (KT_GROUP_R).
 * Only what more than one kernel uses lives here.
 */
#pragma once
#include "pm_gather_dev.h"

#pragma clang fp contract(off)

namespace pm {
#define PM_INLINE __attribute__((always_inline))
PMD float sq(float x) { return x * x; }
/* kNN sums: each term round(c * sc) is an integer <= 2^22
 * (knn_fx), at most PM_KNN_MAX = 2^6 of them per record, so their int32 sum
 * is exact (< 2^28): order-free like the PPM gather's int64 fixed point, at
 * one rounding, one conversion and one integer add per channel (round 4
 * summed terms <= 2^47 in double: two double-rate operations per term; the
 * scalar-stream SUM pass is 41 % of the kNN gather) */
struct Kx3 { int x, y, z; };
/* a kNN term to the nearest integer, floor(x + 0.5) in one instruction
 * (v_cvt_rpi_i32_f32): an error of at most half a unit of the record's fixed
 * point per term, without the one-sided bias of truncation (round 6) */
PMD int knn_rnd(float x) {
    int r;
    asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
/* Dot(Faceforward(ns, wo), wi) > 0 for the photon's wi = (wx, b.w, wz) */
PMD bool knn_facing(v3 ns, bool back, const float4 &b, float wx, float wz) {
    float dn = dot(ns, mk(wx, b.w, wz));
    if (back) dn = -dn;
    return dn > 0.f;
}
/* pbrt kernel() 3/pi (1 - d^2/r_k^2)^2 / r_k^2 times alpha, inv = 1/r_k^2,
 * in the record's fixed point sc */
PMD void knn_add(Kx3 &a, float d2, float inv, float sc, const float4 &b) {
    const float s = 1.f - d2 * inv;
    const float kk = 3.f * INV_PI * s * s;
    /* sc is a power of two: k * (inv * sc) * alpha rounds like (k * inv * alpha) * sc;
     * terms are rounded to the nearest integer (knn_rnd: <= 1/2 unit each) */
    const float ks = kk * (inv * sc);
    a.x += knn_rnd(ks * b.x); a.y += knn_rnd(ks * b.y); a.z += knn_rnd(ks * b.z);
}
/* distance, in cell units, from coordinate u (cell units) to cell c of an
 * axis with dim cells — the border cells extend to infinity (cell_axis
 * clamps) — less a 1e-3 margin that covers the float rounding of u and of the
 * photons' own d^2, so pruning with it never drops a photon that counts */
PMD float cell_gap(float u, uint32_t c, int dim) {
    const float lo = c == 0 ? -INFINITY : (float)c, hi = (int)c + 1 == dim ? INFINITY : (float)(c + 1);
    return fmaxf(fmaxf(lo - u, u - hi) - 1e-3f, 0.f);
}
PMD float next_up(float x) { return __uint_as_float(__float_as_uint(x) + 1u); } /* x >= 0, finite */
/* per-record fixed-point scale: the power of two below knn_fx * r_k^2 */
PMD float knn_scale(float fx, float md2) {
    return md2 == 0.f ? 1.f : __uint_as_float(__float_as_uint(fx * md2) & 0xff800000u);
}
constexpr uint32_t KT_GROUP_R = 1; /* lane boxes span <= 5 cells: a group's union <= 7 per axis */

/* the tile kernels' row map: union row u = ((cz - Z0) << LY) + (cy - Y0) with
 * LY = rowmap_bits(Y0, Y1), the bits of the y extent */
PMD uint32_t rowmap_bits(uint32_t Y0, uint32_t Y1) { return Y1 > Y0 ? 32u - (uint32_t)__builtin_clz(Y1 - Y0) : 0u; }
/* the cells [x0, x1] x [y0, y1] x [z0, z1] of a lane's box [p - r', p + r'],
 * r' = sqrt(r2) with a margin for its own rounding and the photons' (sqrtf:
 * pm_gather.hip's box_reach is a different number) */
PMD void knn_cells(const GridDesc &g, v3 p, float r2, uint32_t &x0, uint32_t &x1, uint32_t &y0, uint32_t &y1,
                   uint32_t &z0, uint32_t &z1) {
    const float rq = sqrtf(r2) * 1.0001f + 1e-4f;
    x0 = cell_axis(p.x - rq, g.gx, g.inv_cs, g.dx); x1 = cell_axis(p.x + rq, g.gx, g.inv_cs, g.dx);
    y0 = cell_axis(p.y - rq, g.gy, g.inv_cs, g.dy); y1 = cell_axis(p.y + rq, g.gy, g.inv_cs, g.dy);
    z0 = cell_axis(p.z - rq, g.gz, g.inv_cs, g.dz); z1 = cell_axis(p.z + rq, g.gz, g.inv_cs, g.dz);
}

/* the bucket rows around p within sqrt(maxd2), nearest rings first; bound()
 * (in world units^2) is re-read per row; visit(j, d2) per photon of the kept
 * cells. Returns nothing; COUNT census through vis / rows. */
struct KnnGrid {
    GridDesc g; /* a copy: a pointer into the kernel arguments would force them into scratch */
    uint32_t x0, x1, y0, y1, z0, z1;
    int cyc, czc, rings;
    float ux, uy, uz, inv2;
    PMD void init(const GridDesc &G, v3 p, float maxd2) {
        g = G;
        knn_cells(G, p, maxd2, x0, x1, y0, y1, z0, z1);
        cyc = (int)cell_axis(p.y, G.gy, G.inv_cs, G.dy); czc = (int)cell_axis(p.z, G.gz, G.inv_cs, G.dz);
        /* the query point in cell units (cell_axis before the floor) */
        ux = (p.x - G.gx) * G.inv_cs; uy = (p.y - G.gy) * G.inv_cs; uz = (p.z - G.gz) * G.inv_cs;
        inv2 = G.inv_cs * G.inv_cs;
        rings = max((int)(y1 - y0), (int)(z1 - z0));
    }
    template <class B, class V>
    PMD void scan(const uint32_t *cell_start, const float4 *ph_a, v3 p, B bound, V visit, unsigned long long &vis,
                  unsigned long long &rows) const {
        for (int ring = 0; ring <= rings; ++ring)
            for (uint32_t cz = z0; cz <= z1; ++cz)
                for (uint32_t cy = y0; cy <= y1; ++cy) {
                    if (max(abs((int)cy - cyc), abs((int)cz - czc)) != ring) continue;
                    const float gy = cell_gap(uy, cy, g.dy), gz = cell_gap(uz, cz, g.dz);
                    const float lim = bound() * inv2 - (gy * gy + gz * gz);
                    if (lim < 0.f) continue;
                    uint32_t xa = x0, xb = x1;
                    while (xa <= xb && sq(cell_gap(ux, xa, g.dx)) > lim) ++xa;
                    while (xb > xa && sq(cell_gap(ux, xb, g.dx)) > lim) --xb;
                    if (xa > xb) continue;
                    const uint32_t row = (cz * (uint32_t)g.dy + cy) * (uint32_t)g.dx;
                    const uint32_t b = cell_start[row + xa], e = cell_start[row + xb + 1];
                    vis += e - b; rows++;
                    for (uint32_t j = b; j < e; ++j) {
                        const float4 a = ph_a[j];
                        const v3 diff = p - xyz(a);
                        visit(j, a, diff.x * diff.x + diff.y * diff.y + diff.z * diff.z);
                    }
                }
    }
};

} // namespace pm
