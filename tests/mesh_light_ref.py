"""float64 numpy restatement of the triangle-mesh area light (pm_add_light_mesh,
pm_shade.h sample_light_mesh / sample_le / sample_l_shading), and of the disk
light's same formulas, driven by the random numbers the GPU uses: the permuted
Halton emission samples (index pid * max_photon_count) and the Philox light
samples of the pinhole eye pass (pixel, slot, light_rng_seed). The oracle has
no mesh lights; both random streams are pinned to it bit for bit by the
existing tests, so this file is the yardstick of tests/test_mesh_light_gpu.py.
"""
import numpy as np

import oracle
from pmrender import scenes
from pmrender.abi import PM_MATTE, PM_MIRROR

LE = (17.0, 11.0, 5.0)


# ------------------------------------------------------------------ meshes
def light_meshes():
    """The four light meshes of the issue, planar in z = 0 and wound to face
    +z: (a) one triangle, (b) a quad of two equal triangles (cdf[0] = 0.5
    exactly), (c) a 7-triangle fan with areas spanning 1 : 1000 and one
    zero-area triangle (a repeated vertex), (d) a 33-triangle strip."""
    out = {}
    out["a"] = (np.float32([[0, 0, 0], [30, 0, 0], [0, 20, 0]]), np.int32([[0, 1, 2]]))
    out["b"] = (np.float32([[-10, -10, 0], [10, -10, 0], [10, 10, 0], [-10, 10, 0]]), np.int32([[0, 1, 2], [0, 2, 3]]))
    ang = [0.0, 0.001, 0.5, 1.2, 2.0, 3.0, 4.5]
    P = [[0.0, 0.0, 0.0]] + [[20.0 * np.cos(a), 20.0 * np.sin(a), 0.0] for a in ang]
    rim = [1, 2, 3, 4, 4, 5, 6, 7]                       # rim[4] == rim[3]: triangle 3 has zero area
    out["c"] = (np.float32(P), np.int32([[0, rim[i], rim[i + 1]] for i in range(7)]))
    V = np.float32([[2.0 * i - 34.0, (8.0 if i % 2 else -8.0) + 0.25 * (i % 5), 0.0] for i in range(35)])
    idx = []
    for i in range(33):
        a, b, c = i, i + 1, i + 2
        e1, e2 = V[b] - V[a], V[c] - V[a]
        idx.append((a, b, c) if e1[0] * e2[1] - e1[1] * e2[0] > 0 else (b, a, c))
    out["d"] = (V, np.int32(idx))
    return out


def table_ref(P, idx, reverse=False):
    """(cdf float32, total area, unit normals) as include/pm_api.h states them."""
    P = np.asarray(P, np.float32).astype(np.float64)
    p0, p1, p2 = P[idx[:, 0]], P[idx[:, 1]], P[idx[:, 2]]
    n = np.cross(p1 - p0, p2 - p0)
    ln = np.linalg.norm(n, axis=1)
    run = np.cumsum(0.5 * ln)                            # np.cumsum adds in index order
    cdf = (run / run[-1]).astype(np.float32)
    cdf[-1] = 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        nn = np.where(ln[:, None] > 0, n / ln[:, None], 0.0)
    return cdf, float(run[-1]), -nn if reverse else nn


def ulp_distance(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------ samplers
def pick(cdf, u):
    """first k with cdf[k] > u"""
    return np.searchsorted(cdf, u, side="right")


def mesh_points(P, idx, cdf, u1, u2):
    """(k, point) for samples (u1, u2): `cdf` is the device's own table."""
    P = np.asarray(P, np.float32).astype(np.float64)
    u1 = np.minimum(np.asarray(u1, np.float32), np.float32(1.0 - 2.0 ** -24))   # held below 1: the bin is never empty
    c = np.asarray(cdf, np.float32)
    k = pick(c, u1)
    u1, u2 = u1.astype(np.float64), np.asarray(u2, np.float32).astype(np.float64)
    c = c.astype(np.float64)
    prev = np.where(k > 0, c[np.maximum(k - 1, 0)], 0.0)
    su = np.sqrt((u1 - prev) / (c[k] - prev))
    b0, b1 = 1.0 - su, u2 * su
    p0, p1, p2 = P[idx[k, 0]], P[idx[k, 1]], P[idx[k, 2]]
    return k, p0 + b1[:, None] * (p1 - p0) + (1.0 - b0 - b1)[:, None] * (p2 - p0)


def concentric_disk(u1, u2):
    """util.cu.h:23-65 in float64"""
    sx, sy = 2.0 * np.asarray(u1, np.float64) - 1.0, 2.0 * np.asarray(u2, np.float64) - 1.0
    r, th = np.zeros_like(sx), np.zeros_like(sx)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = (sx >= -sy) & (sx > sy)
        r[a], th[a] = sx[a], np.where(sy[a] > 0, sy[a] / sx[a], 8.0 + sy[a] / sx[a])
        b = (sx >= -sy) & ~(sx > sy)
        r[b], th[b] = sy[b], 2.0 - sx[b] / sy[b]
        c = ~(sx >= -sy) & (sx <= sy)
        r[c], th[c] = -sx[c], 4.0 + sy[c] / sx[c]
        d = ~(sx >= -sy) & ~(sx <= sy)
        r[d], th[d] = -sy[d], 6.0 - sx[d] / sy[d]
    th = np.where((sx == 0) & (sy == 0), 0.0, th) * (np.pi / 4.0)
    r = np.where((sx == 0) & (sy == 0), 0.0, r)
    return r * np.cos(th), r * np.sin(th)


def uniform_sphere(u1, u2, n):
    """cudalight.cu.h:66-73 in float64, flipped to n's side"""
    u1, u2 = np.asarray(u1, np.float64), np.asarray(u2, np.float64)
    z = 1.0 - 2.0 * u1
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = 2.0 * np.pi * u2
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)
    flip = np.sum(d * n, 1) < 0
    d[flip] = -d[flip]
    return d


def emission_samples(n_paths, mpc=4, pass_index=0):
    """The four Halton dimensions of path pid: index pid * max_photon_count of
    the pass's permutation (photontracing.cu:88-96; pm_trace.hip emit_path)."""
    perm = oracle.halton_permutation(pass_index)
    return np.stack([oracle.halton_sample(pid * mpc, perm) for pid in range(n_paths)]).astype(np.float32)


def philox_uv(pixels, slot, seed):
    """(u1, u2) of the pinhole eye pass's light sample: Philox counter (pixel, slot, 0, 0), key (seed, 0)."""
    out = np.zeros((len(pixels), 2), np.float32)
    for i, px in enumerate(pixels):
        o = oracle.philox((int(px), int(slot), 0, 0), (int(seed), 0))
        out[i] = (np.float32(o[0] >> 8) * np.float32(1.0 / 16777216.0), np.float32(o[1] >> 8) * np.float32(1.0 / 16777216.0))
    return out


# ------------------------------------------------------------------ scenes
MIRROR_Z, CATCH_Z = 50.0, -50.0
EXTENT = 8000.0        # the mirror scene's extent (the catcher's side): positions are compared relative to it
FLOOR_EXTENT = 600.0   # the floor scene's


def _padding(s, pad):
    """Matte primitives behind the catcher, out of every path's reach: spheres
    (64 B each: more than BRUTE_MAX_PRIMS primitives still fit the LDS budget),
    or one instanced triangle (two-level mode)."""
    grey = s.material(PM_MATTE, (0.5, 0.5, 0.5))
    if pad == "inst":
        s.objects.append(dict(P=np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), idx=np.int32([[0, 1, 2]]), N=None, uv=None,
                              material=grey, light=-1))
        s.instances.append((0, *scenes.translate(0.0, 0.0, -200.0)))
        return
    for i in range(int(pad)):
        o2w, w2o = scenes.translate(-300.0 + 30.0 * (i % 20), -300.0 + 30.0 * (i // 20), -200.0)
        s.spheres.append((np.float32(5.0), o2w, w2o, grey, -1))


def mirror_scene(light, pad=0):
    """The light in z = 0 facing +z, a large mirror at z = 50 above it, a
    matte catcher at z = -50 below: slot 4 pid is the path's first deposit and
    carries the emission alpha. light: ("mesh", P, idx) or ("disk", radius)."""
    s = scenes.Scene()
    mir = s.material(PM_MIRROR, (1.0, 1.0, 1.0))
    grey = s.material(PM_MATTE, (0.5, 0.5, 0.5))
    m, c = 2000.0, EXTENT / 2
    s.add_quads([[(-m, -m, MIRROR_Z), (m, -m, MIRROR_Z), (m, m, MIRROR_Z), (-m, m, MIRROR_Z)]], mir)
    s.add_quads([[(-c, -c, CATCH_Z), (c, -c, CATCH_Z), (c, c, CATCH_Z), (-c, c, CATCH_Z)]], grey)
    if light[0] == "mesh":
        s.lights.append(("mesh", light[1], light[2], np.float32(LE), 1, False))   # the emitter alone: nothing to see
    else:
        r = np.float32(light[1])
        area = np.float32(np.float32(2.0 * np.pi) * np.float32(0.5) * np.float32(r * r))
        s.lights.append(("disk", np.float32([0, 0, 0]), np.float32([r, 0, 0]), np.float32([0, r, 0]),
                         np.float32([0, 0, 1]), np.float32(LE), area, 1))
    if pad:
        _padding(s, pad)
    s.camera = scenes.pinhole(64, 48, eye=(0.0, 0.0, 40.0), look=(0.0, 0.0, -50.0), up=(0.0, 1.0, 0.0))
    return s


def unfold(slots):
    """Emission origin (in z = 0) and direction of each first deposit, the
    mirror at z = MIRROR_Z unfolded: the deposit's wi is minus the direction of
    travel after the reflection."""
    p, r = slots["p"].astype(np.float64), -slots["wi"].astype(np.float64)
    d = r * np.array([1.0, 1.0, -1.0])
    q = p.copy()
    q[:, 2] = 2.0 * MIRROR_Z - p[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = q[:, 2] / d[:, 2]
    return q - t[:, None] * d, d


def to_floor(P, height=100.0):
    """the z = 0, +z facing mesh as a ceiling light: (x, y, 0) -> (x, height, y), facing -y"""
    P = np.asarray(P, np.float32)
    return np.stack([P[:, 0], np.full(len(P), np.float32(height)), P[:, 1]], 1).astype(np.float32)


KD = (0.5, 0.25, 0.75)


def floor_scene(light, nsamples=1, slab=False, reverse=False, look_up=False, W=64, H=48):
    """A matte floor (y = 0) under the light at y = 100 (facing down), seen
    from y = 40 looking down; slab: an opaque slab at y = 50 under the whole
    light; look_up: the camera looks up at the light instead."""
    s = scenes.Scene()
    fl = s.material(PM_MATTE, KD)
    f = FLOOR_EXTENT / 2
    s.add_quads([[(-f, 0, -f), (-f, 0, f), (f, 0, f), (f, 0, -f)]], fl)
    if slab:
        s.add_quads([[(-250, 50, -250), (250, 50, -250), (250, 50, 250), (-250, 50, 250)]], fl)
    if light[0] == "mesh":
        s.add_mesh_light(to_floor(light[1]), light[2], LE, nsamples, reverse)
    else:
        r = np.float32(light[1])
        black = s.material(PM_MATTE, (0.0, 0.0, 0.0))
        o, x, y, n = np.float32([0, 100, 0]), np.float32([r, 0, 0]), np.float32([0, 0, r]), np.float32([0, -1, 0])
        area = np.float32(np.float32(2.0 * np.pi) * np.float32(0.5) * np.float32(r * r))
        s.lights.append(("disk", o, x, y, n, np.float32(LE), area, nsamples))
        s.disks.append((o, x, y, n, np.float32(0.0), np.float32(2.0 * np.pi), black, 0))
    if look_up:
        s.camera = ("pinhole", np.float32([0, 20, 0]), np.float32([0, 1, 0]), np.float32([0.6, 0, 0]),
                    np.float32([0, 0, 0.45]), W, H)
    else:
        s.camera = ("pinhole", np.float32([0, 40, 0]), np.float32([0, -1, 0]), np.float32([2.4, 0, 0]),
                    np.float32([0, 0, 1.8]), W, H)
    return s


def direct_light(pos, ns, pts, normals, area, nsamples, pdf_division=True):
    """sum over the samples of |ns.wi| Kd/pi Le / (pdf nS), pdf = d^2 / (cos A),
    for unoccluded records (cudalight.cu.h:18-64, raytracing.cu:49-84).
    pts, normals: [nS][records, 3] sampled points and their emitting normals."""
    pos, ns = pos.astype(np.float64), ns.astype(np.float64)
    L = np.zeros((len(pos), 3))
    fv = np.float32(KD).astype(np.float64) / np.pi
    for p, n in zip(pts, normals):
        uwi = p - pos
        d2 = np.sum(uwi * uwi, 1)
        wi = uwi / np.sqrt(d2)[:, None]
        cos = -np.sum(n * wi, 1)
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.abs(np.sum(ns * wi, 1)) / (d2 / (cos * area) * nsamples if pdf_division else 1.0)
        L += np.where(cos > 0, w, 0.0)[:, None] * fv[None, :] * np.float32(LE).astype(np.float64)[None, :]
    return L
