"""CPU tests of the float64 ray-query reference and its generators
(ray_query_ref.py): the decided shares and caps the GPU tests rely on, the
reference against longdouble and exact rational arithmetic, the generators'
claims, and the slab-test bound of pm_slab.h (box_near with the per-ray
pad) in emulated fp32 on the far-origin group."""
from fractions import Fraction

import numpy as np
import pytest

import ray_query_ref as Q

HBM_PAD = 300


def test_control_group_is_decided():
    """(a) and the caps: the reference alone fixes the tested share"""
    c = Q.control_case()
    assert Q.undecided_share(c, HBM_PAD) <= 0.01
    for n in (1, 2, 3, 63, 64, 65, 66):
        c = Q.count_case(n)
        assert len(c.tris) == n and Q.undecided_share(c, HBM_PAD) <= c.cap
    for c in (Q.slow_small_case(), Q.slow_huge_case()):
        assert Q.undecided_share(c, HBM_PAD) <= c.cap


@pytest.mark.parametrize("make", [Q.control_case, Q.axis_case, Q.grazing_case, Q.tie_case, Q.shifted_case,
                                  lambda: Q.far_case(1e4)])
def test_no_ray_reaches_the_padding(make):
    c = make()
    a = Q.query(c.prims(HBM_PAD), c.rays, Q.EPS, Q.TMAX)
    assert np.isfinite(c.rays).all()
    assert (a.state[:, c.n_prims():] == Q.SURE_MISS).all()


def test_decided_answers_hold_in_longdouble():
    """(b) the same rays in numpy.longdouble: no decided answer changes"""
    for c in (Q.control_case(), Q.far_case(1e3), Q.axis_case()):
        a = Q.query(c.prims(), c.rays, Q.EPS, Q.TMAX)
        ld = Q.nominal_tri_hit(c.tris, c.rays, Q.EPS, Q.TMAX, np.longdouble)
        assert a.decided.any() and np.array_equal(ld[a.decided], a.hit[a.decided])


def test_decided_answers_hold_in_exact_arithmetic():
    """(b) a few hundred rays with fractions.Fraction"""
    c = Q.control_case()
    a = Q.query(c.prims(), c.rays, Q.EPS, Q.TMAX)
    pick = np.concatenate([np.flatnonzero(a.decided & (a.hit >= 0))[:150], np.flatnonzero(a.decided & (a.hit < 0))[:50]])
    eps, tmax = Fraction(Q.EPS), Fraction(Q.TMAX)
    for r in pick:
        best, best_t = Q.MISS, None
        for k, tri in enumerate(c.tris):
            e = Q.tri_exact(tri, c.rays[r])
            if e is None:
                continue
            t, b1, b2 = e
            if eps < t < tmax and b1 >= 0 and b2 >= 0 and b1 + b2 <= 1 and (best_t is None or t < best_t):
                best, best_t = k, t
        assert best == a.hit[r]
        if best >= 0:
            assert abs(float(best_t) - a.t_hit[r]) <= 1e-12 * max(1.0, abs(a.t_hit[r]))


def test_generators_are_deterministic_and_true():
    """(c)"""
    for make in (Q.control_case, Q.tie_case, Q.axis_case, Q.grazing_case, Q.slow_small_case):
        a, b = make(), make()
        assert np.array_equal(a.rays.view(np.uint32), b.rays.view(np.uint32)) and np.array_equal(a.tris, b.tris)
    # non-overlapping: every pair of triangles sits in its own grid cell
    tris = Q.grid_triangles().astype(np.float64)
    cells = np.floor(tris.mean(axis=1) * [4, 4, 3]).astype(int)
    assert len({tuple(c) for c in cells}) == len(tris)
    assert np.array_equal(np.floor(tris.min(axis=1) * [4, 4, 3]), np.floor(tris.max(axis=1) * [4, 4, 3]))
    # edge-aimed targets: within 2e-4 (barycentric) of an edge, in exact arithmetic on the float64 target
    k, tgt, b = Q.bary_targets(Q.grid_triangles(), 300, 3, edge=2e-4)
    for i in range(300):
        P = [[Fraction(float(v)) for v in p] for p in Q.grid_triangles()[k[i]]]
        bb = [Fraction(float(v)) for v in b[i]]
        assert sum(bb) == 1 or abs(float(sum(bb)) - 1.0) < 1e-15
        assert min(abs(v) for v in bb) <= Fraction(2, 10000)
        q = [sum(bb[j] * P[j][a] for j in range(3)) for a in range(3)]
        assert max(abs(float(q[a]) - tgt[i][a]) for a in range(3)) < 1e-14
    # the far rays start `dist` from the centre and pass within 1e-3 of their target's triangle plane point
    r = Q.far_rays(Q.grid_triangles(), 64, 1e4, 9).astype(np.float64)
    assert np.allclose(np.linalg.norm(r[:, :3] - 0.5, axis=1), 1e4, rtol=1e-6)
    # grazing rays: within 1e-4 rad (plus the fp32 rounding of the direction) of the plane
    tr = Q.grid_triangles()
    g = Q.grazing_case().rays.astype(np.float64)
    kk, _, _ = Q.bary_targets(tr, len(g), 109)
    P = tr.astype(np.float64)[kk]
    nrm = Q.unit(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]))
    assert np.abs(np.sum(nrm * g[:, 3:], axis=1)).max() <= 1e-4 + 1e-6
    # the tie rays: exact ties by construction, expected winners inside the reference's candidate set
    c = Q.tie_case()
    a = Q.query(c.prims(), c.rays, Q.EPS, Q.TMAX)
    for order in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
        e = Q.tie_expected(c, order)
        assert a.cand[np.arange(len(e)), np.where(e < 0, a.cand.shape[1] - 1, e)].all()
    assert (Q.tie_expected(c, (0, 1, 2)) != Q.tie_expected(c, (2, 1, 0))).any()
    # the slow-path triangles: a normal below 2^-125, above 2^125, and a zero area
    n32 = lambda t: np.cross(np.float32(t[0]) - np.float32(t[2]), np.float32(t[1]) - np.float32(t[0]))
    assert 0 < np.abs(np.float64(Q.TINY)).max() and np.abs(n32(Q.TINY).astype(np.float64)).max() < 2.0 ** -125
    assert np.abs(n32(Q.slow_huge_case().tris[0])).max() >= 2.0 ** 125
    assert not n32(Q.FLAT).any()
    # the light lies off every surface's plane
    for c in (Q.control_case(), Q.tie_case(), Q.axis_case()):
        P = c.tris.astype(np.float64)
        nr = Q.unit(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]))
        assert np.abs(np.sum(nr * (c.light.astype(np.float64) - P[:, 0]), axis=1)).min() > 1e-3


# ------------------------------------------------------ the slab-test bound
f32 = np.float32


def slab_accepts(lo, hi, o, d, t_hit, ray_pad):
    """box_near in emulated fp32 on the box [lo, hi] padded as pm_commit pads
    it, with an exact reciprocal rounded to fp32 (the hardware's is within an
    ulp of it): does the box's [tn, tf] survive, with tmax = the hit's own t?
    ray_pad: the per-ray pad 2^-20 max|o| (pm_slab.h ray_pad2, ray_slab, ray_oinv_hi) or none."""
    lo, hi = Q.padded_box(lo, hi)
    dd = np.where(np.abs(d) < f32(1e-20), np.copysign(f32(1e-20), d), d).astype(f32)
    inv = (1.0 / dd.astype(np.float64)).astype(f32)
    pad = (f32(2.0 ** -20) * np.abs(o).max(axis=1, keepdims=True)).astype(f32) if ray_pad else f32(0) * o
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)
    oinv = ((o + pad).astype(f32) * inv).astype(f32)
    oinv_h = fma(-(f32(2) * pad).astype(f32), inv, oinv)
    t0, t1 = fma(lo, inv, -oinv), fma(hi, inv, -oinv_h)
    tn = np.maximum(np.minimum(t0, t1).max(axis=1), f32(Q.EPS))
    tf = np.minimum(np.maximum(t0, t1).min(axis=1), t_hit.astype(f32))
    return tn <= tf


def test_slab_bound_over_far_origins():
    """No hit the float64 reference is sure of may be culled by the hit
    triangle's own padded box, at any distance of the far-origin group; the
    commit pad alone (the code before the per-ray pad) does cull some from
    1e4 on, which is what the per-ray pad is for."""
    lost_before = 0
    for dist in Q.FAR_DISTANCES + (1e6, 1e8):
        tris = Q.grid_triangles()
        rays = Q.far_rays(tris, 20000, dist, 211)
        t, b1, b2 = Q.tri_terms(tris, rays[:, :3], rays[:, 3:])
        with np.errstate(invalid="ignore"):
            ok = (t > Q.EPS) & (b1 >= -2e-4) & (b2 >= -2e-4) & (b1 + b2 <= 1 + 2e-4)   # accepted, or within the edge band
        r, k = np.nonzero(ok)
        lo, hi = tris.min(axis=1)[k], tris.max(axis=1)[k]
        # tmax as the kernels hold it: the hit's t, an fp32 value up to m_t off the float64 one
        th = (t[r, k] * (1.0 + 64 * Q.U)).astype(np.float32)
        kept = slab_accepts(lo, hi, rays[r, :3], rays[r, 3:], th, ray_pad=True)
        assert kept.all(), f"distance {dist:g}: {(~kept).sum()} of {len(kept)} hits culled by their own box"
        lost_before += int((~slab_accepts(lo, hi, rays[r, :3], rays[r, 3:], th, ray_pad=False)).sum())
    assert lost_before > 0, "the emulation no longer shows the culling the per-ray pad removes"
