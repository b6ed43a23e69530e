"""float64 numpy restatement of the distant light (include/pm_api.h
pm_add_light_distant; pm_shade.h sample_le, sample_l_shading; pm_scene.cpp
world_sphere, finish_lights), driven by the random numbers the GPU uses
(mesh_light_ref.emission_samples). The oracle has no such light: this file
is the yardstick of tests/test_delta_lights*.py.
"""
import math

import numpy as np

import mesh_light_ref as M
from pmrender import scenes
from pmrender.abi import (PM_LIGHT_AREA_DISK, PM_LIGHT_AREA_MESH, PM_LIGHT_DISTANT, PM_LIGHT_POINT,
                          PM_MATTE, PM_MIRROR)

KD = M.KD


def unit(v):
    v = np.asarray(v, np.float32).astype(np.float64)
    return v / math.sqrt(float(v @ v))


def unit32(v):
    """the unit vector as the library stores it: normalised in double, rounded to float"""
    return unit(v).astype(np.float32).astype(np.float64)


def coordinate_system(v):
    """pbrt-v2 CoordinateSystem(v, &v1, &v2)"""
    v = np.asarray(v, np.float64)
    if abs(v[0]) > abs(v[1]):
        inv = 1.0 / math.sqrt(v[0] * v[0] + v[2] * v[2])
        v1 = np.array([-v[2] * inv, 0.0, v[0] * inv])
    else:
        inv = 1.0 / math.sqrt(v[1] * v[1] + v[2] * v[2])
        v1 = np.array([0.0, v[2] * inv, -v[1] * inv])
    return v1, np.cross(v, v1)


def world_sphere(points):
    """(centre, radius) of pm_commit's world sphere for a scene whose bounds are those of `points`"""
    P = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    lo, hi = P.min(0), P.max(0)
    c = (0.5 * (lo + hi)).astype(np.float32).astype(np.float64)
    return c, math.sqrt(float(np.sum(np.maximum(np.abs(hi - c), np.abs(lo - c)) ** 2)))


def distant_record(to_light, centre, R):
    """(disk centre, p1, p2, area) of the distant light's record"""
    w = unit32(to_light)
    v1, v2 = coordinate_system(w)
    return centre + R * w, R * v1, R * v2, math.pi * R * R


def distant_emission(to_light, L, centre, R, lu1, lu2):
    w = unit32(to_light)
    o, p1, p2, area = distant_record(to_light, centre, R)
    x, y = M.concentric_disk(np.asarray(lu1, np.float32), np.asarray(lu2, np.float32))
    org = o[None, :] + x[:, None] * p1[None, :] + y[:, None] * p2[None, :]
    d = np.broadcast_to(-w, org.shape)
    alpha = np.broadcast_to(np.asarray(L, np.float32).astype(np.float64) * area, org.shape)
    return org, d, alpha


def distant_direct(to_light, L, ns):
    w = unit32(to_light)
    return np.abs(np.asarray(ns, np.float64) @ w)[:, None] * (np.float32(KD).astype(np.float64) / np.pi)[None, :] * \
        np.asarray(L, np.float32).astype(np.float64)[None, :]


def luminance(c):
    c = np.asarray(c, np.float32).astype(np.float64)
    return 0.212671 * c[0] + 0.715160 * c[1] + 0.072169 * c[2]


def power_table(types, le, areas):
    """pm_light_selection_cdf in float64 (pbrt's Power() per light), as float32"""
    w = []
    for t, c, a in zip(types, np.asarray(le, np.float32).reshape(-1, 3), np.asarray(areas, np.float32)):
        y = luminance(c)
        if t == PM_LIGHT_POINT:
            w.append(y * 4.0 * math.pi)
        elif t in (PM_LIGHT_AREA_DISK, PM_LIGHT_AREA_MESH):
            w.append(y * (math.pi * float(a)))
        else:
            assert t == PM_LIGHT_DISTANT
            w.append(y * float(a))
    run = np.cumsum(np.maximum(np.array(w), 0.0))
    cdf = (run / run[-1]).astype(np.float32)
    cdf[-1] = 1.0
    return cdf


# ------------------------------------------------------------------ scenes
def mirror_scene(light, pad=0):
    """mesh_light_ref.mirror_scene's arrangement with a delta light.
    light: ("distant", to_light, L) | ("point", I) at the origin"""
    s = M.mirror_scene(("disk", 1.0), pad)
    del s.lights[:]
    add_light(s, light, pos=(0.0, 0.0, 0.0))
    return s


def add_light(s, light, pos):
    if light[0] == "distant":
        return s.add_distant_light(light[1], (0.0, 0.0, 0.0), light[2])
    if light[0] == "point":
        s.lights.append(("point", np.float32(pos), np.float32(light[1])))
        return len(s.lights) - 1
    raise ValueError(light[0])


def floor_scene(light, slab=None, W=64, H=48, height=100.0, wall=False):
    """floor_scene's floor (y = 0, 600 x 600) seen from y = 40 looking down, lit
    by a delta light at (0, height, 0). slab: (x0, x1, z0, z1) of an opaque
    slab at y = 50; wall: a wall at x = -96, just outside the view, facing +x."""
    s = scenes.Scene()
    fl = s.material(PM_MATTE, KD)
    f = M.FLOOR_EXTENT / 2
    s.add_quads([[(-f, 0, -f), (-f, 0, f), (f, 0, f), (f, 0, -f)]], fl)
    if slab:
        x0, x1, z0, z1 = slab
        s.add_quads([[(x0, 50, z0), (x1, 50, z0), (x1, 50, z1), (x0, 50, z1)]], fl)
    if wall:
        s.add_quads([[(-96, 0, -f), (-96, 200, -f), (-96, 200, f), (-96, 0, f)]], fl)
    add_light(s, light, pos=(0.0, height, 0.0))
    s.camera = ("pinhole", np.float32([0, 40, 0]), np.float32([0, -1, 0]), np.float32([2.4, 0, 0]),
                np.float32([0, 0, 1.8]), W, H)
    return s


def scene_points(s):
    """every world vertex of a Scene's meshes (no disks, spheres or instances)"""
    assert not s.disks and not s.spheres and not s.instances
    return np.concatenate([np.asarray(m["P"], np.float32).reshape(-1, 3) for m in s.meshes])


def segment_hits_rect(p, q, y, x0, x1, z0, z1, margin=0.0):
    """does the segment p -> q cross the axis-aligned rectangle at height y? Returns (hit, near):
    near marks crossings within `margin` of the rectangle's edge."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (y - p[:, 1]) / (q[:, 1] - p[:, 1])
    x = p[:, 0] + t * (q[:, 0] - p[:, 0])
    z = p[:, 2] + t * (q[:, 2] - p[:, 2])
    ok = (t > 0.001) & (t < 0.999)
    inside = ok & (x >= x0) & (x <= x1) & (z >= z0) & (z <= z1)
    edge = np.minimum(np.minimum(np.abs(x - x0), np.abs(x - x1)), np.minimum(np.abs(z - z0), np.abs(z - z1)))
    wide = ok & (x >= x0 - margin) & (x <= x1 + margin) & (z >= z0 - margin) & (z <= z1 + margin)
    return inside, wide & (edge <= margin)
