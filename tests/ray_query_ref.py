"""float64 reference of the renderer's one ray query (closest hit / any hit of
a ray against triangles, disks and spheres) and the ray and scene generators of
tests/test_ray_query.py (CPU) and tests/test_ray_query_gpu.py (GPU).

This is not a restatement of the device's intersectors (pm_isect.h) or walkers
(pm_slab.h, pm_leaf.h, pm_traverse.h, pm_trav_step.h): triangles are intersected with the
textbook Moller-Trumbore test on edge vectors taken from the vertices
(e1 = p1 - p0, e2 = p2 - p0, pvec = d x e2, ...), disks and spheres
analytically, everything in float64 on the fp32 input values widened. No
precomputed (e0, e1, n) record, no inv * (p0 - o) ordering, no fp32 anywhere.

The margin m
------------
A float64 answer can be compared with an fp32 kernel only where the answer
does not hinge on the fp32 rounding. isect_tri_v computes

    den = n.d                      3 mul, 2 add       <= 3 u |n||d|
    inv = 1 / den                  1 rounding         (relative u, after
                                                       den's 3 u / |cos|)
    s   = p0 - o                   1 sub              <= u (|o| + |p0|)
    e2  = inv * s                  1 mul
    i   = d x e2                   2 mul, 1 sub       <= 3 u |d||e2|
    beta = i.e1, gamma = i.e0      3 mul, 2 add       <= 3 u |i||e|
    t   = n.e2                     3 mul, 2 add       <= 3 u |n||e2|

on a record whose e0, e1 carry one rounding each and whose n = e1 x e0
carries three (u = 2^-24, the unit roundoff of fp32). That is 20 roundings on
the way to a barycentric coordinate. Each is relative to a product of norms,
not to the result, so against beta = ((d x s).e) / (n.d) the error is
bounded by 20 u |d||s||e| / (|n||d||cos|), cos the cosine between the ray and
the normal. With |n| = |e||e'| sin A = |e| h (h the triangle's height over
that edge), |s| <= |o| + |p| and the relative terms (which scale with beta
<= 1 itself and with the edge length L that n's cancellation is relative to)
this is

    m = K u (|o| + |p| + L) / (h |cos|),        K = 32, u = 2^-24

with h the smallest height (twice the area over the longest edge L), |p| the
largest vertex norm. K = 32 leaves a factor 1.6 over the count of 20 for
norms against components. A barycentric slip of m moves the hit by at most
m L in the plane, so the same bound in t is m_t = m L / |d|; the recorded
point o + d t adds its own two roundings, 2 u (|o| + |d| t) / |d|.
Disks and spheres use the same form with their radius for h and L. One m
everywhere; nothing here was tuned against the kernels.

A ray is *decided* when every inequality that fixes its answer (t > tmin,
t < tmax, beta >= 0, gamma >= 0, beta + gamma <= 1, radius / phimax /
discriminant, and t below the runner-up's) clears its threshold by more than
m. For the others the reference returns the candidate set: every primitive
(and "miss") that is the answer under some perturbation within m.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
K = 32.0
MISS = -1

SURE_MISS, MAYBE, SURE_HIT = 0, 1, 2


class Prims:
    """tris (n, 3, 3) float32; disks [(o, x, y, z, inner, phimax)]; spheres
    [(radius, w2o 4x4)]. Global ids: triangles, then disks, then spheres."""

    def __init__(self, tris, disks=(), spheres=()):
        self.tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
        self.disks = [tuple(np.asarray(v, np.float32) for v in d) for d in disks]
        self.spheres = [(np.float32(r), np.asarray(w, np.float32).reshape(4, 4)) for r, w in spheres]

    def __len__(self):
        return len(self.tris) + len(self.disks) + len(self.spheres)


def _norm(a):
    return np.sqrt(np.sum(a * a, axis=-1))


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _classify(t, mt, inside_sure, outside_sure, tmin, tmax, dead):
    """state, tlo, thi of one primitive kind from its t, its margin in t and its in/out verdicts"""
    with np.errstate(invalid="ignore"):
        t_in = (t - mt > tmin) & (t + mt < tmax)
        t_out = (t + mt < tmin) | (t - mt > tmax)
        state = np.full(t.shape, MAYBE, np.int8)
        state[inside_sure & t_in] = SURE_HIT
        state[outside_sure | t_out | dead] = SURE_MISS
        bad = ~np.isfinite(t) | ~np.isfinite(mt)
        state[bad & ~dead] = MAYBE
        tlo = np.where(bad, -np.inf, t - mt)
        thi = np.where(bad, np.inf, t + mt)
    return state, np.where(bad, np.nan, t), tlo, thi


def tri_terms(tris, o, d, ft=np.float64):
    """Moller-Trumbore on vertices: (t, b1, b2) of every ray against every
    triangle in the float type ft (float64, or numpy.longdouble for test b)"""
    P = tris.astype(ft)
    p0, e1, e2 = P[None, :, 0], (P[:, 1] - P[:, 0])[None], (P[:, 2] - P[:, 0])[None]
    o, d = o.astype(ft)[:, None, :], d.astype(ft)[:, None, :]
    pvec = _cross(d, e2)
    det = _dot(e1, pvec)
    tvec = o - p0
    qvec = _cross(tvec, e1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return _dot(e2, qvec) / det, _dot(tvec, pvec) / det, _dot(d, qvec) / det


def _tris(tris, o, d, tmin, tmax, dir_err):
    P = tris.astype(np.float64)
    e1, e2, e3 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], P[:, 2] - P[:, 1]
    nrm = _cross(e1, e2)
    area2 = _norm(nrm)
    L = np.maximum(np.maximum(_norm(e1), _norm(e2)), _norm(e3))
    pmax = _norm(P).max(axis=1)
    dead = (area2 == 0.0)[None, :]                       # zero area: never hit
    t, b1, b2 = tri_terms(tris, o, d)
    dn = _norm(d)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        h = area2 / L
        cos = np.abs(_dot(nrm[None], d[:, None, :])) / (area2[None] * dn)
        reach = _norm(o)[:, None] + pmax[None] + L[None]
        m = (K * U * reach + dir_err * _norm(o[:, None, :] - P[None, :, 0])) / (h[None] * cos)
        mt = m * L[None] / dn + 2.0 * U * (_norm(o)[:, None] + dn * np.abs(t)) / dn
        b0 = 1.0 - b1 - b2
        inside = (b1 > m) & (b2 > m) & (b0 > 2.0 * m)
        outside = (b1 < -m) | (b2 < -m) | (b0 < -2.0 * m)
    return _classify(t, mt, inside, outside, tmin, tmax, dead | np.zeros(t.shape, bool))


def _disks(disks, o, d, tmin, tmax, dir_err):
    out = []
    on, dn = _norm(o), _norm(d)
    for c, x, y, z, inner, phimax in disks:
        c, x, y, z = (v.astype(np.float64) for v in (c, x, y, z))
        inner, phimax = float(inner), float(phimax)
        with np.errstate(invalid="ignore", divide="ignore"):
            zd = _dot(d, z)
            t = _dot(c - o, z) / zd
            cos = np.abs(zd) / (_norm(z) * dn)
            loc = o + t[:, None] * d - c
            lu, lv = _dot(loc, x) / _dot(x, x), _dot(loc, y) / _dot(y, y)
            dist = np.sqrt(lu * lu + lv * lv)
            r = min(_norm(x), _norm(y))
            m = (K * U * (on + _norm(c) + r) + dir_err * _norm(o - c)) / (r * cos)
            mt = m * r / dn + 2.0 * U * (on + dn * np.abs(t)) / dn
            inside = (dist < 1.0 - m) & ((inner <= 0.0) | (dist > inner + m))
            outside = (dist > 1.0 + m) | ((inner > 0.0) & (dist < inner - m))
            if phimax < 2.0 * math.pi:
                phi = np.mod(np.arctan2(lv, lu), 2.0 * math.pi)
                ma = m / np.maximum(dist, 1e-300)
                inside &= (phi > ma) & (phi < phimax - ma)
                outside |= (phi > phimax + ma) & (phi < 2.0 * math.pi - ma)
        out.append(_classify(t, mt, inside, outside, tmin, tmax, np.zeros(t.shape, bool)))
    return out


def _spheres(spheres, o, d, tmin, tmax, dir_err):
    out = []
    for rad, w2o in spheres:
        W, rad = w2o.astype(np.float64), float(rad)
        oo, dd = o @ W[:3, :3].T + W[:3, 3], d @ W[:3, :3].T
        dn, on = _norm(dd), _norm(oo)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            tc = -_dot(oo, dd) / (dn * dn)                 # closest approach to the centre
            q = _norm(oo + tc[:, None] * dd) / rad
            m = (K * U * (on + _norm(W[:3, 3]) + rad) + dir_err * on) / rad
            hc = rad * np.sqrt(np.maximum(1.0 - q * q, 0.0))
            mt = (m * rad + np.where(hc > 0, m * rad * rad / np.maximum(hc, 1e-300), np.inf)) / dn \
                + 2.0 * U * (on + dn * np.abs(tc)) / dn
            t0, t1 = tc - hc / dn, tc + hc / dn
            line_hit, line_miss = q < 1.0 - m, q > 1.0 + m
            first_in = (t0 - mt > tmin) & (t0 + mt < tmax)
            first_below = t0 + mt < tmin
            second_in = (t1 - mt > tmin) & (t1 + mt < tmax)
            sure = line_hit & (first_in | (first_below & second_in))
            miss = line_miss | (line_hit & ((t0 - mt > tmax) | (t1 + mt < tmin) | (first_below & (t1 - mt > tmax))))
        t = np.where(first_in | ~first_below, t0, t1)
        state = np.full(t.shape, MAYBE, np.int8)
        state[sure] = SURE_HIT
        state[miss] = SURE_MISS
        grey = state == MAYBE
        tlo = np.where(grey, np.where(np.isfinite(t0 - mt), np.minimum(t0 - mt, t1 - mt), -np.inf), t - mt)
        thi = np.where(grey, np.inf, t + mt)
        out.append((state, t, tlo, thi))
    return out


class Answer:
    """state / t / tlo / thi: [rays, prims]; hit: the closest primitive by the
    float64 numbers (MISS = -1) and its t; decided; cand [rays, prims + 1]:
    the candidate set, the last column standing for a miss."""


def query(prims, rays, tmin, tmax, dir_err=0.0):
    """The closest-hit answer of every ray (o, d rows of `rays`, float32).
    tmin, tmax: scalars or per ray. dir_err: a relative uncertainty of the
    direction itself (the photon side's restated Halton direction)."""
    rays = np.asarray(rays, np.float32).reshape(-1, 6)
    o, d = rays[:, :3].astype(np.float64), rays[:, 3:].astype(np.float64)
    n = len(rays)
    tmin = np.broadcast_to(np.asarray(tmin, np.float64), (n,))[:, None]
    tmax = np.broadcast_to(np.asarray(tmax, np.float64), (n,))[:, None]
    cols = []
    if len(prims.tris):
        cols.append(_tris(prims.tris, o, d, tmin, tmax, dir_err))
    for st, t, lo, hi in _disks(prims.disks, o, d, tmin[:, 0], tmax[:, 0], dir_err) + \
            _spheres(prims.spheres, o, d, tmin[:, 0], tmax[:, 0], dir_err):
        cols.append((st[:, None], t[:, None], lo[:, None], hi[:, None]))
    a = Answer()
    a.state, a.t, a.tlo, a.thi = (np.concatenate([c[k] for c in cols], axis=1) for k in range(4))
    sure = a.state == SURE_HIT
    best_hi = np.where(sure, a.thi, np.inf).min(axis=1)
    cand = (a.state != SURE_MISS) & (a.tlo <= best_hi[:, None])
    a.cand = np.concatenate([cand, ~sure.any(axis=1, keepdims=True)], axis=1)
    a.decided = a.cand.sum(axis=1) == 1
    a.hit = np.where(a.decided, np.where(a.cand[:, -1], MISS, a.cand[:, :-1].argmax(axis=1)), -2)   # -2: undecided
    a.t_hit = np.where(a.hit >= 0, a.t[np.arange(n), np.maximum(a.hit, 0)], np.inf)
    a.mt_hit = np.where(a.hit >= 0, (a.thi - a.tlo)[np.arange(n), np.maximum(a.hit, 0)] / 2.0, 0.0)
    a.occluded_sure = sure.any(axis=1)
    a.clear_sure = (a.state == SURE_MISS).all(axis=1)
    return a


def nominal_tri_hit(tris, rays, tmin, tmax, ft=np.float64):
    """The closest triangle (MISS: none) by the plain comparisons, no margin,
    in the float type ft: what test (b) holds the decided answers against."""
    rays = np.asarray(rays, np.float32).reshape(-1, 6)
    t, b1, b2 = tri_terms(tris, rays[:, :3], rays[:, 3:], ft)
    with np.errstate(invalid="ignore"):
        ok = (t > tmin) & (t < tmax) & (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= 1)
    tt = np.where(ok, t, np.inf)
    return np.where(ok.any(axis=1), tt.argmin(axis=1), MISS)


def tri_exact(tri, ray):
    """(t, b1, b2) of one ray and one triangle in exact rational arithmetic (None: parallel)"""
    P = [[Fraction(float(v)) for v in p] for p in np.asarray(tri, np.float32)]
    o, d = [Fraction(float(v)) for v in ray[:3]], [Fraction(float(v)) for v in ray[3:]]
    sub = lambda a, b: [x - y for x, y in zip(a, b)]
    dot = lambda a, b: sum(x * y for x, y in zip(a, b))
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    e1, e2 = sub(P[1], P[0]), sub(P[2], P[0])
    pvec = cross(d, e2)
    det = dot(e1, pvec)
    if det == 0:
        return None
    tvec = sub(o, P[0])
    qvec = cross(tvec, e1)
    return dot(e2, qvec) / det, dot(tvec, pvec) / det, dot(d, qvec) / det


# ---------------------------------------------------------------- generators
def grid_triangles(n=40, seed=11, cells=(4, 4, 3), lo=0.0, size=1.0):
    """n triangles in [lo, lo + size]^3, one per cell of a grid and held 10% of
    the cell off its walls, so no two touch: no equal-t ties. None is thinner
    than height / longest edge = 0.25."""
    rng = np.random.RandomState(seed)
    cx, cy, cz = cells
    pick = rng.permutation(cx * cy * cz)[:n]
    out = []
    for c in pick:
        i, j, k = c % cx, (c // cx) % cy, c // (cx * cy)
        base = np.array([i / cx, j / cy, k / cz])
        ext = np.array([1.0 / cx, 1.0 / cy, 1.0 / cz])
        while True:
            P = base + ext * (0.1 + 0.8 * rng.uniform(size=(3, 3)))
            e = [P[1] - P[0], P[2] - P[0], P[2] - P[1]]
            L = max(np.linalg.norm(v) for v in e)
            if np.linalg.norm(np.cross(e[0], e[1])) / L >= 0.25 * L:
                break
        out.append(lo + size * P)
    return np.asarray(out, np.float32)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def sphere_dirs(rng, n):
    return unit(rng.normal(size=(n, 3)))


def random_rays(n, seed, lo=0.0, size=1.0):
    """half from inside the cube, half from the shell just outside it (up to
    20% of its size away), directions uniform over the sphere"""
    rng = np.random.RandomState(seed)
    o = rng.uniform(0.0, 1.0, size=(n, 3))
    shell = np.arange(n) % 2 == 1
    ax = rng.randint(0, 3, size=n)
    off = np.where(rng.uniform(size=n) < 0.5, -rng.uniform(0.01, 0.2, size=n), 1.0 + rng.uniform(0.01, 0.2, size=n))
    o[shell, ax[shell]] = off[shell]
    return np.concatenate([lo + size * o, sphere_dirs(rng, n)], axis=1).astype(np.float32)


def bary_targets(tris, n, seed, edge=None):
    """(triangle index, point) of n targets: uniform inside the triangles, or
    with `edge` within that barycentric distance of an edge or a vertex (one
    coordinate in [-edge, edge]; every third one with two such coordinates)"""
    rng = np.random.RandomState(seed)
    k = rng.randint(0, len(tris), size=n)
    r1, r2 = np.sqrt(rng.uniform(size=n)), rng.uniform(size=n)
    b = np.stack([1.0 - r1, r1 * (1.0 - r2), r1 * r2], 1)
    if edge is not None:
        small = rng.uniform(-edge, edge, size=n)
        which = rng.randint(0, 3, size=n)
        rest = rng.uniform(0.05, 0.95, size=n) * (1.0 - small)
        b = np.zeros((n, 3))
        idx = np.arange(n)
        b[idx, which] = small
        b[idx, (which + 1) % 3] = rest
        b[idx, (which + 2) % 3] = 1.0 - small - rest
        vtx = idx % 3 == 2
        s2 = rng.uniform(-edge, edge, size=n)
        b[vtx, (which[vtx] + 1) % 3] = s2[vtx]
        b[vtx, (which[vtx] + 2) % 3] = 1.0 - small[vtx] - s2[vtx]
    P = np.asarray(tris, np.float32).astype(np.float64)[k]
    return k, np.einsum("nk,nkc->nc", b, P), b


def aimed_rays(origins, targets):
    """float32 rays from `origins` through `targets` (unit directions, rounded to float32)"""
    o = np.asarray(origins, np.float32)
    d = unit(np.asarray(targets, np.float64) - o.astype(np.float64))
    return np.concatenate([o, d.astype(np.float32)], axis=1).astype(np.float32)


def far_rays(tris, n, dist, seed, centre=(0.5, 0.5, 0.5), edge=2e-4):
    """n rays from `dist` away from the scene's centre (directions over the
    whole sphere), half aimed at triangle interiors, half within `edge`
    (barycentric) of edges and vertices"""
    rng = np.random.RandomState(seed)
    org = np.asarray(centre) + dist * sphere_dirs(rng, n)
    _, p_in, _ = bary_targets(tris, n, seed + 1)
    _, p_ed, _ = bary_targets(tris, n, seed + 2, edge=edge)
    tgt = np.where((np.arange(n) % 2 == 0)[:, None], p_in, p_ed)
    return aimed_rays(org, tgt)


def grazing_rays(tris, n, seed, angle=1e-4):
    """rays that meet a triangle's plane within `angle` radians of it, from
    about one longest edge away, aimed at interior points"""
    rng = np.random.RandomState(seed)
    k, tgt, _ = bary_targets(tris, n, seed)
    P = np.asarray(tris, np.float32).astype(np.float64)[k]
    nrm = unit(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]))
    inplane = unit(np.cross(nrm, sphere_dirs(rng, n)))
    a = rng.uniform(-angle, angle, size=n)
    back = inplane * np.cos(a)[:, None] + nrm * np.sin(a)[:, None]
    return aimed_rays(tgt + 0.5 * back, tgt)


def padding_spheres(count, at=(120.0, -77.0, 33.0)):
    """`count` tiny spheres (64 B each) parked in a row far from every ray:
    they only raise the primitive count and the scene's size into the next
    traversal mode"""
    out = []
    for i in range(count):
        w2o = np.eye(4, dtype=np.float32)
        w2o[:3, 3] = (-(at[0] + 0.5 * i), -at[1], -at[2])
        out.append((np.float32(1e-3), w2o))
    return out


# --------------------------------------------------------------------- cases
EPS = 1e-3          # scene_epsilon of every case (tmin of eye and photon rays)
TMAX = 1e27         # RT_DEFAULT_MAX
LIGHT = (0.5234, 0.4671, 0.5512)


class Case:
    """One scene and its rays. tris [n, 3, 3] in insertion (= global id)
    order; cap: the largest undecided share the case may have (None: an
    adversarial group, no cap); shadow: whether dl is read as an any-hit probe."""

    def __init__(self, name, tris, rays, disks=(), spheres=(), light=LIGHT, cap=None, shadow=True):
        self.name, self.cap, self.shadow = name, cap, shadow
        self.tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
        self.disks, self.spheres = list(disks), list(spheres)
        self.light = np.asarray(light, np.float32)
        self.rays = np.asarray(rays, np.float32).reshape(-1, 6)

    def prims(self, pad=0):
        return Prims(self.tris, self.disks, self.spheres + padding_spheres(pad))

    def n_prims(self):
        return len(self.tris) + len(self.disks) + len(self.spheres)


def mixed_rays(tris, n, seed, lo=0.0, size=1.0):
    """half random (random_rays), half from random origins at interior points"""
    a = random_rays(n // 2, seed, lo, size)
    b = random_rays(n - n // 2, seed + 1, lo, size)
    _, tgt, _ = bary_targets(tris, len(b), seed + 2)
    return np.concatenate([a, aimed_rays(b[:, :3], tgt)])


def control_case():
    tris = grid_triangles()
    return Case("control", tris, mixed_rays(tris, 4000, 5), cap=0.01)


def count_case(n):
    tris = grid_triangles(n, seed=23, cells=(5, 4, 4))
    return Case(f"count{n}", tris, mixed_rays(tris, 1536, 31 + n), cap=0.05)


TINY = np.float32([[1e-20, 0, 0], [0, 2e-20, 0], [0, 0, 3e-20]])       # normal ~1e-40: below 2^-125
FLAT = np.float32([[0.2, 0.2, 0.2], [0.4, 0.4, 0.4], [0.3, 0.3, 0.3]])  # zero area


def slow_small_case():
    """five ordinary triangles, the tiny one and a zero-area one; rays at the
    ordinary ones, at the origin corner and along the zero-area segment"""
    tris = grid_triangles(5, seed=41, cells=(2, 2, 2))
    rays = mixed_rays(tris, 1024, 43)
    rng = np.random.RandomState(47)
    org = 0.5 + 0.6 * sphere_dirs(rng, 256)
    at_tiny = aimed_rays(org[:48], np.float64(TINY).mean(axis=0)[None] + np.zeros((48, 3)))
    at_flat = aimed_rays(org[48:], 0.2 + 0.2 * rng.uniform(size=(208, 1)) + np.zeros((208, 3)))
    return Case("slow-small", np.concatenate([tris, TINY[None], FLAT[None]]), np.concatenate([rays, at_tiny, at_flat]), cap=0.05)


def slow_huge_case():
    """three triangles of order 1e19 (normals ~1e38: above 2^125), seen from
    from origins of order 1e5 (inside the C-ABI's bound on origins)"""
    s = 1e19
    tris = np.float32([[[-0.2 * s, -0.2 * s, 0.25 * s], [1.0 * s, -0.2 * s, 0.25 * s], [-0.2 * s, 0.9 * s, 0.25 * s]],
                       [[0, 0, 0.5 * s], [0, 0.8 * s, 0.5 * s], [1.1 * s, 0, 0.5 * s]],
                       [[0, 0, -0.5 * s], [0.9 * s, 0, -0.5 * s], [0, 1.0 * s, -0.6 * s]]])
    rng = np.random.RandomState(53)
    org = np.clip(1e5 * rng.normal(size=(1024, 3)), -1e6, 1e6)   # inside the C-ABI's bound on origins
    k, tgt, _ = bary_targets(tris, 1024, 59)
    return Case("slow-huge", tris, aimed_rays(org, tgt), light=(0.31 * s, 0.27 * s, 0.23 * s), cap=0.05, shadow=False)


def tie_case():
    """coplanar triangles in z = 0.5 whose fp32 normals are powers of two (so
    a ray along -z has the same t bits on all): T0 and T2 share T0's
    hypotenuse, T1 overlaps both; a disk in the plane and a sphere tangent to
    it from below at (0.25, 0.25). Vertical rays through the overlap, the
    shared edge and the tangent point, and oblique rays at the same targets."""
    z = 0.5
    tris = np.float32([[[0, 0, z], [0.5, 0, z], [0, 0.5, z]],
                       [[0.125, 0.125, z], [0.625, 0.125, z], [0.125, 1.125, z]],
                       [[0.5, 0, z], [0.5, 0.5, z], [0, 0.5, z]]])
    disk = (np.float32([0.25, 0.25, z]), np.float32([0.25, 0, 0]), np.float32([0, 0.25, 0]), np.float32([0, 0, 1]),
            np.float32(0.0), np.float32(2.0 * math.pi))
    w2o = np.eye(4, dtype=np.float32)
    w2o[:3, 3] = (-0.25, -0.25, -0.25)
    rng = np.random.RandomState(61)
    g = rng.randint(0, 65, size=(768, 2)) / 64.0 * 0.75          # dyadic targets over the patch
    s = rng.randint(0, 33, size=256) / 64.0
    edge = np.stack([s, 0.5 - s], 1)                             # on the shared edge, exactly
    xy = np.concatenate([g, edge, [[0.25, 0.25]] * 8])
    tgt = np.concatenate([xy, np.full((len(xy), 1), z)], 1)
    down = np.concatenate([tgt + [0, 0, 0.5], np.tile([0.0, 0.0, -1.0], (len(tgt), 1))], 1)
    org = tgt + np.abs(rng.normal(size=tgt.shape)) * [0.3, 0.3, 0.6] + [0, 0, 0.1]
    return Case("ties", tris, np.concatenate([down.astype(np.float32), aimed_rays(org, tgt)]), disks=[disk],
                spheres=[(np.float32(0.25), w2o)], light=(0.31, 0.77, 0.93))


def tie_expected(case, order):
    """for the vertical rays of tie_case: the primitive that must win when the
    triangles are inserted in `order` (ids: triangles by insertion, disk,
    sphere) — the first inserted among those containing the point, computed
    exactly (every coordinate is a small dyadic number)"""
    n = len(case.rays) // 2
    xy = case.rays[:n, :2].astype(np.float64)
    x, y = xy[:, 0], xy[:, 1]
    inside = np.stack([(x >= 0) & (y >= 0) & (x + y <= 0.5),
                       (x >= 0.125) & (y >= 0.125) & ((x - 0.125) * 2 + (y - 0.125) <= 1.0),
                       (x <= 0.5) & (y <= 0.5) & (x + y >= 0.5),
                       (x - 0.25) ** 2 + (y - 0.25) ** 2 <= 0.0625,
                       (x == 0.25) & (y == 0.25)], 1)
    rank = np.array([list(order).index(k) for k in range(3)] + [3, 4])
    score = np.where(inside, rank[None, :], 99)
    return np.where(inside.any(axis=1), score.argmin(axis=1), MISS)


COMMIT_PAD = np.float32(1e-4)


def padded_box(lo, hi):
    """a primitive box as pm_commit pads it, in float32 as it computes it:
    both planes of an axis move by 1e-4 max(1, |lo|, |hi|)"""
    lo, hi = np.float32(lo), np.float32(hi)
    pad = (COMMIT_PAD * np.maximum(np.float32(1.0), np.maximum(np.abs(lo), np.abs(hi)))).astype(np.float32)
    return (lo - pad).astype(np.float32), (hi + pad).astype(np.float32)


def vertex_normals(tris, seed=131):
    """distinct unit normals for the three vertices of every triangle (float32):
    the face normal tilted by up to ~35 degrees, so the shading normal of a
    hit depends on both barycentrics"""
    rng = np.random.RandomState(seed)
    P = np.asarray(tris, np.float32).astype(np.float64)
    face = unit(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]))
    return unit(face[:, None, :] + 0.7 * sphere_dirs(rng, 3 * len(P)).reshape(len(P), 3, 3) / np.sqrt(3.0) * 1.2).astype(np.float32)


def shading_normal(tris, normals, rays, hit):
    """float64 interpolated unit normal of each ray at triangle hit[ray]: the
    weight of vertex 1 is Moller-Trumbore's u, of vertex 2 its v"""
    rays = np.asarray(rays, np.float32)
    _, b1, b2 = tri_terms(tris, rays[:, :3], rays[:, 3:])
    r = np.arange(len(rays))
    b1, b2 = b1[r, hit], b2[r, hit]
    N = np.asarray(normals, np.float32).astype(np.float64)[hit]
    return unit(N[:, 0] * (1.0 - b1 - b2)[:, None] + N[:, 1] * b1[:, None] + N[:, 2] * b2[:, None])


def axis_case():
    """group 5 on the control triangles plus two axis-aligned quads sharing an
    edge: directions with zero, -0.0 and 1e-30 components; origins on a padded
    box face, on a triangle's plane, inside a leaf box; rays along the shared
    edge; surfaces just below and just above scene_epsilon"""
    tris = grid_triangles()
    q = np.float32([[[1.25, 0, 0], [1.75, 0, 0], [1.75, 0.5, 0]], [[1.25, 0, 0], [1.75, 0.5, 0], [1.25, 0.5, 0]],
                    [[1.75, 0, 0], [1.75, 0, 0.5], [1.75, 0.5, 0.5]], [[1.75, 0, 0], [1.75, 0.5, 0.5], [1.75, 0.5, 0]]])
    tris = np.concatenate([tris, q])
    rng = np.random.RandomState(71)
    rays = []
    k, tgt, _ = bary_targets(tris, 1536, 73)
    for i, small in enumerate((0.0, -0.0, 1e-30, -1e-30)):      # one or two components replaced
        sl = slice(i * 384, (i + 1) * 384)
        d = sphere_dirs(rng, 384)
        ax = rng.randint(0, 3, size=384)
        d[np.arange(384), ax] = small
        two = np.arange(384) % 2 == 0
        d[two, (ax[two] + 1) % 3] = small
        d = unit(d)
        d[np.arange(384), ax] = small
        d[two, (ax[two] + 1) % 3] = small
        o = tgt[sl] - d * rng.uniform(0.3, 1.5, size=(384, 1))
        rays.append(np.concatenate([o, d], 1).astype(np.float32))
    P = tris.astype(np.float64)
    lo, hi = tris.min(axis=1), tris.max(axis=1)
    lo_f, hi_f = padded_box(lo, hi)
    k, tgt, _ = bary_targets(tris, 768, 79)
    ax = rng.randint(0, 3, size=768)
    side = rng.randint(0, 2, size=768)
    o = tgt + 0.4 * sphere_dirs(rng, 768)
    o = o.astype(np.float32)
    o[np.arange(768), ax] = np.where(side == 0, lo_f[k, ax], hi_f[k, ax])   # exactly on a padded face
    rays.append(aimed_rays(o, tgt))
    k, tgt, b = bary_targets(tris, 512, 83)                     # origin on the triangle's plane (inside it)
    rays.append(np.concatenate([tgt, sphere_dirs(rng, 512)], 1).astype(np.float32))
    inplane = unit(P[k, 1] - P[k, 0])
    rays.append(np.concatenate([tgt[:256] - 0.5 * inplane[:256], inplane[:256]], 1).astype(np.float32))
    k, tgt, _ = bary_targets(tris, 256, 89)                     # inside a leaf box, off the plane by less than the pad
    nrm = unit(np.cross(P[k, 1] - P[k, 0], P[k, 2] - P[k, 0]))
    rays.append(np.concatenate([tgt + 5e-5 * nrm, sphere_dirs(rng, 256)], 1).astype(np.float32))
    s = rng.uniform(-0.2, 0.7, size=128)                        # along the quads' shared edge x = 1.75, z = 0
    e = np.stack([np.full(128, 1.75), s, np.zeros(128)], 1)
    rays.append(np.concatenate([e - [0, 1.0, 0], np.tile([0.0, 1.0, 0.0], (128, 1))], 1).astype(np.float32))
    rays.append(np.concatenate([e + [0.3, 0, 0.3], np.tile(unit([-1.0, 0, -1.0]), (128, 1))], 1).astype(np.float32))
    k, tgt, _ = bary_targets(tris, 512, 97)                     # the surface at t = eps (1 +- 1e-3 .. 1e-6)
    nrm = unit(np.cross(P[k, 1] - P[k, 0], P[k, 2] - P[k, 0]))
    f = 1.0 + np.where(np.arange(512) % 2 == 0, -1.0, 1.0) * 10.0 ** -rng.uniform(3, 6, size=512)
    rays.append(np.concatenate([tgt + (EPS * f)[:, None] * nrm, -nrm], 1).astype(np.float32))
    return Case("axis", tris, np.concatenate(rays), light=(0.5234, 0.4671, 0.7512))


FAR_DISTANCES = (1e1, 1e2, 1e3, 1e4, 1e5)


def far_case(dist):
    tris = grid_triangles()
    return Case(f"far{dist:g}", tris, far_rays(tris, 1024, dist, 101))


def shifted_case(shift=3000.0):
    """the control geometry at coordinates near `shift`, seen from near zero"""
    tris = grid_triangles(lo=shift)
    rng = np.random.RandomState(103)
    _, p_in, _ = bary_targets(tris, 1024, 105)
    _, p_ed, _ = bary_targets(tris, 1024, 107, edge=2e-4)
    tgt = np.where((np.arange(1024) % 2 == 0)[:, None], p_in, p_ed)
    return Case("shifted", tris, aimed_rays(rng.uniform(-1.0, 1.0, size=(1024, 3)), tgt),
                light=tuple(shift + np.float64(LIGHT)))


def grazing_case():
    tris = grid_triangles()
    return Case("grazing", tris, grazing_rays(tris, 2048, 109))


def undecided_share(case, pad=0):
    return 1.0 - float(query(case.prims(pad), case.rays, EPS, TMAX).decided.mean())
