"""What a correct photon slot buffer is, in float64: the second reference of
the photon trace (csrc/pm_trace.hip), next to the oracle's bit-for-bit one.
tests/test_trace_directed.py certifies the checkers on the CPU (the oracle's
slots pass, every corruption of a list is rejected);
tests/test_trace_directed_gpu.py holds the kernels' slots to them.

Nothing here restates the kernels or the oracle: no Halton, no Philox, no
fp32. The closest-hit answers come from ray_query_ref.query (Moller-Trumbore
on the vertices in float64, with its own margin for what fp32 cannot decide);
this module adds the distance of a point from a primitive and the rules below.

A path owns mpc consecutive slots. Deposit k of a path has position p_k, flux
alpha_k and direction wi_k, the direction the photon arrived FROM (the negated
ray direction, stored bit for bit).

Layout (assert_layout; exact, any scene)
  the valid bits (bits & 1) of a path form a prefix; every slot after it is
  forty zero bytes; a valid slot's bits word is 1, or under the caustic map 1
  or 3, and within a path no 3 follows a 1 (a deposit is a caustic photon only
  before the path's first diffuse hit).

Geometry (assert_paths; scenes of constant-colour materials)
  | |wi_k| - 1 | <= UNIT_BOUND;
  p_k lies on a matte primitive: its float64 distance from the nearest one is
  <= POS_BOUND;
  for k >= 1 the segment is direct when p_{k-1} - p_k = L wi_k to within
  DIR_BOUND world units (L the segment's length: the photon's ray missed
  p_{k-1} sideways by no more than that). In a scene without mirrors or glass,
  and under max_specular_depth = 0, every segment must be direct; with them a
  segment may bend at specular hits. For a direct segment the float64 closest
  hit of the ray the kernel traced, (p_{k-1}, -wi_k) with tmin the scene
  epsilon, is at p_k: at distance L to within DIST_BOUND, on a primitive no
  further than POS_BOUND from p_k (the same one, or one tied with it);
  for k = 0, and for a segment that is not direct, the float64 closest hit of
  (p_k, wi_k) exists: the photon came from somewhere (the unrecorded first
  hit x_0, or the last specular surface).

Flux
  alpha_0 is finite and non-negative (so is alpha_0 / Kd(x_0), whatever x_0
  is). Cosine-sampled Lambert makes f cos / pdf = Kd, and the reference's
  mirrors and glass weigh 1, so alpha_k / alpha_{k-1} is, per channel, the Kd
  of a primitive that holds p_{k-1} (one within POS_BOUND of it), to within
  KD_BOUND. On the Cornell box the white, red and green walls make that
  discriminating: a deposit stored one bounce late, or against another wall's
  material, fails it.

Exemptions
  Only a deposit whose ray ray_query_ref.query calls undecided (an edge, a tie
  between primitives at different distances, grazing) is exempt, and only from
  the closest-hit rules; every other rule still holds for it. assert_paths
  refuses a buffer whose exempt share exceeds `cap` (1 %).

Bounds
  Each residual was measured on the oracle's slots of the cases of
  test_trace_directed.py (CASES below: every scene of the GPU file that has an
  oracle, 3,000 paths at mpc 4 and 1,000 at mpc 8, pass 0 and pass 1; half as
  many on the scenes of thousands of triangles, whose checks are dense), on the
  CPU, and the bound is that worst residual times 4: the slack between two
  correct fp32 evaluations of the same path. MEASURED holds the worst values,
  test_trace_directed.py::test_bounds_are_four_times_the_oracle_residuals
  measures them again.
"""
import numpy as np

import ray_query_ref as R
from pmrender import scenes as S
from pmrender.abi import PM_MATTE, PHOTON_DTYPE

# worst residuals of the oracle's slots over CASES (see the module docstring); world units are the Cornell box's
# (coordinates up to 560, so one fp32 ulp of a position is 6.1e-5)
MEASURED = {
    "unit": 8.4048153e-07,   # | |wi| - 1 |  (2.3e-7 without mirrors or glass; a refraction's direction is less exact)
    "pos": 1.5595823e-04,    # distance of p_k from its primitive
    "dir": 1.2529968e-04,    # | p_{k-1} - p_k - L wi_k |
    "dist": 2.9425581e-04,   # | t |d| - L | of the float64 closest hit
    "kd": 2.6559627e-06,     # | alpha_k / alpha_{k-1} - Kd |  (4.5e-7 outside the instanced scene)
}
SLACK = 4.0
UNIT_BOUND = SLACK * MEASURED["unit"]
POS_BOUND = SLACK * MEASURED["pos"]
DIR_BOUND = SLACK * MEASURED["dir"]
DIST_BOUND = SLACK * MEASURED["dist"]
KD_BOUND = SLACK * MEASURED["kd"]
EXEMPT_CAP = 0.01

NEAR = 1.0        # candidate primitives of a point: those whose box, grown by NEAR, holds it
RAY_CHUNK = 256   # rays per ray_query_ref.query call (it works on dense [rays, primitives] arrays)


# ---------------------------------------------------------------------------------------------- layout
def valid(slots):
    return (slots["bits"] & 1) != 0


def by_path(slots, mpc):
    assert len(slots) % mpc == 0, f"{len(slots)} slots are no multiple of mpc {mpc}"
    return slots.reshape(-1, mpc)


def assert_layout(slots, mpc, marked=False):
    """the exact rules of the module docstring; returns the deposits per path"""
    slots = np.ascontiguousarray(slots, dtype=PHOTON_DTYPE)
    sp = by_path(slots, mpc)
    v = valid(sp)
    n = v.sum(axis=1)
    prefix = np.arange(mpc)[None, :] < n[:, None]
    bad = np.flatnonzero((v != prefix).any(axis=1))
    assert bad.size == 0, f"{bad.size} paths whose valid slots are no prefix, first path {bad[0]}: bits {sp['bits'][bad[0]].tolist()}"
    words = slots.view(np.uint32).reshape(-1, mpc, PHOTON_DTYPE.itemsize // 4)
    dirty = words.any(axis=2) & ~v
    bad = np.argwhere(dirty)
    assert bad.size == 0, f"{len(bad)} dead slots are not zero, first path {bad[0][0]} slot {bad[0][1]}: " \
                          f"{words[bad[0][0], bad[0][1]].tolist()}"
    bits = sp["bits"]
    allowed = (bits == 1) | ((bits == 3) if marked else False)
    bad = np.argwhere(v & ~allowed)
    assert bad.size == 0, f"{len(bad)} valid slots with a bits word outside {'1, 3' if marked else '1'}, first path " \
                          f"{bad[0][0]} slot {bad[0][1]}: {int(bits[bad[0][0], bad[0][1]])}"
    if marked and mpc > 1:
        late = v[:, 1:] & (bits[:, 1:] == 3) & (bits[:, :-1] == 1)
        bad = np.argwhere(late)
        assert bad.size == 0, f"{len(bad)} caustic marks after a path's first diffuse hit, first path {bad[0][0]} slot {bad[0][1] + 1}"
    return n


def assert_same_slots(a, b, what="slots"):
    """bit for bit; names the first path and slot that differ (mpc: slots per path, for the message)"""
    a, b = np.ascontiguousarray(a, dtype=PHOTON_DTYPE), np.ascontiguousarray(b, dtype=PHOTON_DTYPE)
    assert len(a) == len(b), f"{what}: {len(a)} slots against {len(b)}"
    ua, ub = a.view(np.uint32).reshape(len(a), -1), b.view(np.uint32).reshape(len(b), -1)
    bad = np.flatnonzero((ua != ub).any(axis=1))
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {len(a)} slots differ, first slot {i}\n got  {a[i]}\n want {b[i]}")


def slot_of(path, k, mpc):
    return path * mpc + k


# ------------------------------------------------------------------------------------------ the scene
class Geometry:
    """The primitives of a pmrender Scene as ray_query_ref.Prims (triangles of the meshes and of the flattened
    instances, then disks, then spheres) with, per primitive, its material's type and Kd, and its box."""

    def __init__(self, scene):
        tris, mats = [], []
        meshes = list(scene.meshes) + [scene.flattened(k) for k in range(len(scene.instances))]
        for m in meshes:
            P = np.asarray(m["P"], np.float32).reshape(-1, 3)
            t = P[np.asarray(m["idx"], np.int64).reshape(-1, 3)]
            tris.append(t)
            mats += [m["material"]] * len(t)
        disks = []
        for o, x, y, z, inner, phimax, mat, _ in scene.disks:
            if float(phimax) < 2.0 * np.pi - 1e-6:
                raise NotImplementedError("partial disks: no distance of a point from one here")
            disks.append((o, x, y, z, inner, phimax))
            mats.append(mat)
        spheres = []
        for r, _, w2o, mat, _ in scene.spheres:
            spheres.append((r, np.asarray(w2o, np.float32).reshape(4, 4)))
            mats.append(mat)
        self.prims = R.Prims(np.concatenate(tris) if tris else np.zeros((0, 3, 3), np.float32), disks, spheres)
        for mtype, rgb in scene.materials:
            if not isinstance(rgb, np.ndarray):
                raise NotImplementedError("assert_paths takes scenes of constant-colour materials of the reference's model")
        self.mtype = np.array([scene.materials[m][0] for m in mats])
        self.kd = np.array([scene.materials[m][1] for m in mats], np.float64)
        self.matte = self.mtype == PM_MATTE
        self.specular = bool((~self.matte).any())
        T = self.prims.tris.astype(np.float64)
        lo, hi = [T.min(axis=1)], [T.max(axis=1)]
        for o, x, y, z, _, _ in self.prims.disks:
            o, r = o.astype(np.float64), max(np.linalg.norm(x), np.linalg.norm(y))
            lo.append((o - r)[None]); hi.append((o + r)[None])
        for r, w2o in self.prims.spheres:
            c = -np.linalg.solve(w2o[:3, :3].astype(np.float64), w2o[:3, 3].astype(np.float64))
            lo.append((c - float(r))[None]); hi.append((c + float(r))[None])
        self.lo, self.hi = np.concatenate(lo), np.concatenate(hi)

    def __len__(self):
        return len(self.prims)

    # ---- the distance of a point from a primitive
    @staticmethod
    def _segment(p, a, b):
        ab = b - a
        den = np.maximum((ab * ab).sum(-1), 1e-300)
        t = np.clip(((p - a) * ab).sum(-1) / den, 0.0, 1.0)
        return np.linalg.norm(p - (a + t[:, None] * ab), axis=-1)

    def _tri_dist(self, p, k):
        T = self.prims.tris.astype(np.float64)[k]
        a, b, c = T[:, 0], T[:, 1], T[:, 2]
        n = np.cross(b - a, c - a)
        nn = np.maximum(np.linalg.norm(n, axis=-1), 1e-300)
        plane = ((p - a) * n).sum(-1) / nn
        q = p - (plane / nn)[:, None] * n
        # q inside the triangle: on the inner side of its three edges
        inside = np.ones(len(p), bool)
        for u, v in ((a, b), (b, c), (c, a)):
            inside &= (np.cross(v - u, q - u) * n).sum(-1) >= 0.0
        edge = np.minimum(np.minimum(self._segment(p, a, b), self._segment(p, b, c)), self._segment(p, c, a))
        return np.where(inside, np.abs(plane), edge)

    def _disk_dist(self, p, d):
        o, x, y, z, inner, _ = (np.asarray(v, np.float64) for v in self.prims.disks[d])
        zn = z / np.linalg.norm(z)
        h = ((p - o) * zn).sum(-1)
        q = p - o - h[:, None] * zn
        u, v = (q * x).sum(-1) / (x * x).sum(), (q * y).sum(-1) / (y * y).sum()
        rho = np.sqrt(u * u + v * v)
        r = min(np.linalg.norm(x), np.linalg.norm(y))
        radial = np.maximum(np.maximum(rho - 1.0, float(inner) - rho), 0.0) * r
        return np.sqrt(h * h + radial * radial)

    def _sphere_dist(self, p, s):
        r, w2o = self.prims.spheres[s]
        W = w2o.astype(np.float64)
        return np.abs(np.linalg.norm(p @ W[:3, :3].T + W[:3, 3], axis=-1) - float(r))

    def near(self, points):
        """(point index, primitive, distance) of every pair whose box, grown by NEAR, holds the point: sorted by point"""
        p = np.asarray(points, np.float64).reshape(-1, 3)
        pi, ki = [], []
        for s in range(0, len(p), 1024):
            c = p[s:s + 1024, None, :]
            m = ((c >= self.lo[None] - NEAR) & (c <= self.hi[None] + NEAR)).all(axis=2)
            a, b = np.nonzero(m)
            pi.append(a + s); ki.append(b)
        pi, ki = np.concatenate(pi), np.concatenate(ki)
        d = np.full(len(pi), np.inf)
        nt, nd = len(self.prims.tris), len(self.prims.disks)
        t = ki < nt
        d[t] = self._tri_dist(p[pi[t]], ki[t])
        for j in range(nd):
            sel = ki == nt + j
            d[sel] = self._disk_dist(p[pi[sel]], j)
        for j in range(len(self.prims.spheres)):
            sel = ki == nt + nd + j
            d[sel] = self._sphere_dist(p[pi[sel]], j)
        return pi, ki, d

    def query(self, o, d, eps, own=None):
        """ray_query_ref.query over chunks of rays -> (decided, hit primitive or MISS, t |d|).

        own[i]: the triangles that hold ray i's origin (a deposit). query() leaves most rays that leave their
        own surface at a grazing angle undecided: its margin in t, K u |o| L / (h cos), passes the scene
        epsilon below cos ~ 0.06, though the origin lies on that plane and the float64 t is ~1e-4. Such a ray
        is asked again without the triangles of `own` that it meets in float64 at |t| < eps / 2 (a plane is met
        once: they cannot be the hit beyond eps), which only ever turns an exempt deposit into a checked one."""
        n = len(o)
        decided, hit, dist = np.zeros(n, bool), np.full(n, R.MISS), np.full(n, np.inf)
        rays = np.concatenate([o, d], axis=1).astype(np.float32)
        dn = np.linalg.norm(rays[:, 3:].astype(np.float64), axis=1)
        for s in range(0, n, RAY_CHUNK):
            a = R.query(self.prims, rays[s:s + RAY_CHUNK], float(eps), R.TMAX)
            decided[s:s + RAY_CHUNK] = a.decided
            hit[s:s + RAY_CHUNK] = np.where(a.decided, a.hit, R.MISS)
            dist[s:s + RAY_CHUNK] = a.t_hit * dn[s:s + RAY_CHUNK]
        if own is not None:
            for i in np.flatnonzero(~decided):
                ks = np.asarray(own[i], np.int64)
                if len(ks) == 0:
                    continue
                t, _, _ = R.tri_terms(self.prims.tris[ks], rays[i:i + 1, :3], rays[i:i + 1, 3:])
                ks = ks[np.abs(t[0]) < 0.5 * float(eps)]
                if len(ks) == 0:
                    continue
                tris = self.prims.tris.copy()
                tris[ks] = 0.0   # zero area: never hit
                a = R.query(R.Prims(tris, self.prims.disks, self.prims.spheres), rays[i:i + 1], float(eps), R.TMAX)
                if a.decided[0]:
                    decided[i], hit[i], dist[i] = True, a.hit[0], a.t_hit[0] * dn[i]
        return decided, hit, dist


_geometries = {}


def geometry(scene):
    """one Geometry per Scene object (the tests share scenes)"""
    g = _geometries.get(id(scene))
    if g is None or g[0] is not scene:
        g = _geometries[id(scene)] = (scene, Geometry(scene))
    return g[1]


# ------------------------------------------------------------------------------------------ the paths
class Residuals(dict):
    """worst residual per rule, deposits checked, exempt ones"""


def _first(mask, path, k):
    i = int(np.flatnonzero(mask)[0])
    return f"first path {int(path[i])} slot {int(k[i])}"


def measure_paths(scene, params, slots, marked=False):
    """Everything assert_paths asserts, as numbers: Residuals with the worst residual of every rule ('unit',
    'pos', 'dir', 'dist', 'kd'), the counts ('deposits', 'exempt', 'bent') and, under 'fail', the violations that
    are no matter of a bound (message strings)."""
    g = geometry(scene)
    mpc, eps = int(params.max_photon_count), float(params.scene_epsilon)
    slots = np.ascontiguousarray(slots, dtype=PHOTON_DTYPE)
    assert_layout(slots, mpc, marked)
    sp = by_path(slots, mpc)
    v = valid(sp)
    path, k = np.nonzero(v)
    out = Residuals(unit=0.0, pos=0.0, dir=0.0, dist=0.0, kd=0.0, deposits=len(path), exempt=0, bent=0, fail=[])
    if len(path) == 0:
        return out
    p = sp["p"][path, k].astype(np.float64)
    wi = sp["wi"][path, k].astype(np.float64)
    al = sp["alpha"][path, k].astype(np.float64)
    fail = out["fail"]
    if not (np.isfinite(p).all() and np.isfinite(wi).all()):
        fail.append("a deposit with a position or direction that is not finite")
        return out
    out["unit"] = float(np.abs(np.linalg.norm(wi, axis=1) - 1.0).max())
    bad = ~np.isfinite(al).all(axis=1) | (al < 0.0).any(axis=1)
    if bad.any():
        fail.append(f"{int(bad.sum())} deposits whose flux is negative or not finite, {_first(bad, path, k)}")

    # every deposit lies on a matte primitive
    pi, ki, dk = g.near(p)
    nearest = np.full(len(p), np.inf)
    np.minimum.at(nearest, pi, dk)
    out["pos"] = float(nearest.max())
    held = dk <= POS_BOUND                      # the primitives that hold a deposit
    on_matte = np.zeros(len(p), bool)
    np.logical_or.at(on_matte, pi[held], g.matte[ki[held]])
    off = np.isfinite(nearest) & (nearest <= POS_BOUND) & ~on_matte
    holds_tri = held & (ki < len(g.prims.tris))

    class Own:  # the triangles that hold the deposits `rows`, by ray
        def __init__(self, rows):
            self.rows = rows

        def __getitem__(self, i):
            return ki[holds_tri & (pi == self.rows[i])]
    if off.any():
        fail.append(f"{int(off.sum())} deposits on a mirror or glass primitive, {_first(off, path, k)}")

    # k >= 1: the segment from the deposit before (the previous row: rows are sorted by path, then slot)
    later = np.flatnonzero(k >= 1)
    prev = later - 1
    seg = p[prev] - p[later]
    L = np.linalg.norm(seg, axis=1)
    side = np.linalg.norm(seg - L[:, None] * wi[later], axis=1)
    direct = side <= DIR_BOUND
    may_bend = g.specular and int(params.max_specular_depth) > 0
    if may_bend:
        out["bent"] = int((~direct).sum())
        out["dir"] = float(side[direct].max()) if direct.any() else 0.0
    else:
        out["dir"] = float(side.max()) if len(side) else 0.0
    # flux: alpha_k / alpha_{k-1} is the Kd of a primitive that holds p_{k-1}
    if len(later):
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(al[prev] != 0.0, al[later] / al[prev], np.where(al[later] == 0.0, np.nan, np.inf))
        row_of = np.full(len(p), -1)
        row_of[prev] = np.arange(len(later))
        sel = held & (row_of[pi] >= 0)
        rows = row_of[pi[sel]]
        err = np.abs(ratio[rows] - g.kd[ki[sel]])
        err = np.where(np.isnan(ratio[rows]), 0.0, err).max(axis=1)   # a channel that was 0 stays 0
        best = np.full(len(later), np.inf)
        np.minimum.at(best, rows, err)
        has = np.isfinite(nearest[prev]) & (nearest[prev] <= POS_BOUND)
        out["kd"] = float(best[has].max()) if has.any() else 0.0

    # the closest hit of the ray the kernel traced, for direct segments
    exempt = np.zeros(len(p), bool)
    fwd = later[direct]
    if len(fwd):
        dec, hit, dist = g.query(sp["p"][path[fwd - 1], k[fwd - 1]], -sp["wi"][path[fwd], k[fwd]], eps, Own(fwd - 1))
        exempt[fwd[~dec]] = True
        miss = dec & (hit == R.MISS)
        if miss.any():
            fail.append(f"{int(miss.sum())} deposits whose ray hits nothing in float64, {_first(miss, path[fwd], k[fwd])}")
        ok = dec & (hit != R.MISS)
        # the hit lies on the ray at `dist`, the deposit at L to within DIR_BOUND of the ray: at the same distance
        # the two are the same point, on the hit primitive or on one tied with it
        out["dist"] = float(np.abs(dist[ok] - L[direct][ok]).max()) if ok.any() else 0.0
    # where the photon came from: the first deposit of a path and every bent segment
    back = np.concatenate([np.flatnonzero(k == 0), later[~direct]])
    if len(back):
        dec, hit, _ = g.query(sp["p"][path[back], k[back]], sp["wi"][path[back], k[back]], eps, Own(back))
        exempt[back[~dec]] = True
        miss = dec & (hit == R.MISS)
        if miss.any():
            fail.append(f"{int(miss.sum())} deposits that came from nowhere (no float64 hit along wi), "
                        f"{_first(miss, path[back], k[back])}")
    out["exempt"] = int(exempt.sum())
    return out


def assert_paths(scene, params, slots, marked=False, cap=EXEMPT_CAP, what="slots"):
    """the rules of the module docstring on `slots` (the slots of whole paths, params.max_photon_count each) of a
    trace of `scene` under `params`; returns the Residuals"""
    return assert_residuals(measure_paths(scene, params, slots, marked), scene, params, cap, what)


def assert_residuals(r, scene, params, cap=EXEMPT_CAP, what="slots"):
    """measure_paths' numbers against the bounds; cap None: the exempt share is not held (a buffer of a few
    deposits, every one of them part of a larger buffer that is)"""
    g = geometry(scene)
    assert not r["fail"], f"{what}: " + "; ".join(r["fail"])
    assert r["unit"] <= UNIT_BOUND, f"{what}: | |wi| - 1 | = {r['unit']:.3g} > {UNIT_BOUND:.3g}"
    assert r["pos"] <= POS_BOUND, f"{what}: a deposit {r['pos']:.3g} off every primitive > {POS_BOUND:.3g}"
    if not (g.specular and int(params.max_specular_depth) > 0):
        assert r["dir"] <= DIR_BOUND, f"{what}: wi misses the deposit before by {r['dir']:.3g} > {DIR_BOUND:.3g}"
    assert r["dist"] <= DIST_BOUND, f"{what}: the float64 closest hit is {r['dist']:.3g} from the deposit > {DIST_BOUND:.3g}"
    assert r["kd"] <= KD_BOUND, f"{what}: alpha_k / alpha_k-1 is {r['kd']:.3g} off the Kd under p_k-1 > {KD_BOUND:.3g}"
    if cap is not None:
        assert r["exempt"] <= cap * r["deposits"], f"{what}: {r['exempt']} of {r['deposits']} deposits undecided, over {cap:.0%}"
    return r


# ------------------------------------------------------------------------------------------ the scenes
def sphere_soup(n_tris):
    """triangle_soup with one glass and one mirror sphere (the reference's model: both weigh 1)"""
    sc = S.triangle_soup(n_tris, 16, 16)
    glass = sc.material(S.PM_GLASS, (1.0, 1.0, 1.0))
    mirror = sc.material(S.PM_MIRROR, (0.9, 0.9, 0.9))
    for (x, y, z), r, m in (((370.0, 100.0, 250.0), 100.0, glass), ((150.0, 90.0, 380.0), 90.0, mirror)):
        o2w, w2o = S.translate(x, y, z)
        sc.spheres.append((np.float32(r), o2w, w2o, m, -1))
    return sc


def figures_instanced():
    """instanced_scene's three figure instances (one a mirror) without its two shading-normal quads: their
    vertex normals are not unit vectors and the reference's shading does not normalise what it interpolates, so
    a bounce off them has |wi| != 1 and f cos / pdf != Kd, in the oracle as on the device (measured: | |wi| - 1 |
    up to 0.46). That is the shading's contract with its input, not the trace's; test_gpu_parity.py keeps those
    quads bit-exact against the oracle."""
    sc = S.instanced_scene(16, 16)
    del sc.instances[3:]
    return sc


LDS_TRIS, HBM_TRIS = 60, 2000  # triangle_soup sizes: an LDS-resident tree, and one traversed from HBM (pooled)

SCENES = {
    "cornell": lambda: S.cornell_box(16, 16),               # brute force
    "soup_lds": lambda: S.triangle_soup(LDS_TRIS, 16, 16),
    "soup_hbm": lambda: S.triangle_soup(HBM_TRIS, 16, 16),
    "instanced": lambda: figures_instanced(),               # two-level; one mirror object among the instances
    "spheres_lds": lambda: sphere_soup(LDS_TRIS),
    "spheres_hbm": lambda: sphere_soup(HBM_TRIS),
}
MODE = {"cornell": "brute", "soup_lds": "bvh-lds", "soup_hbm": "bvh-hbm", "instanced": "bvh-instanced",
        "spheres_lds": "bvh-lds", "spheres_hbm": "bvh-hbm"}
_scenes = {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = SCENES[name]()
    return _scenes[name]


# the cases the bounds were measured on: (scene, paths, mpc, pass, max_specular_depth)
CASES = [(s, n // (2 if MODE[s] in ("bvh-hbm", "bvh-instanced") else 1), mpc, ps, 10)
         for s in SCENES for n, mpc, ps in ((3000, 4, 0), (1000, 8, 1))] + \
        [(s, 1000, 4, 0, d) for s in ("spheres_lds", "instanced") for d in (0, 1)]
