"""Independent restatements of csrc/pm_plan.cpp for tests/test_pass_plan.py:
the photon grid of a radius in numpy.float32 arithmetic (every operation
rounded to float32, in the order pm_plan.h states), the histogram quantile
in float64, and the scene box pm_commit hands to make_grid."""
import struct

import numpy as np

f32 = np.float32
R2_BINS, R2_PER_OCTAVE = 64, 8
PM_ESTIMATOR_PPM, PM_ESTIMATOR_KNN = 0, 1


def bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def from_bits(u):
    return f32(struct.unpack("<f", struct.pack("<I", u))[0])


def scene_bbox(scene):
    """The box of a Scene's mesh vertices, disk corners o +- x +- y and the
    transformed corners of each sphere's cube (scene_boxes, pm_scene.cpp)."""
    assert not scene.instances
    pts = [np.asarray(m["P"], f32).reshape(-1, 3)[np.asarray(m["idx"]).ravel()] for m in scene.meshes]
    for o, x, y, *_ in scene.disks:
        o, x, y = (np.asarray(v, f32) for v in (o, x, y))
        pts.append(np.stack([(o + f32(sx) * x) + f32(sy) * y for sx in (-1, 1) for sy in (-1, 1)]))
    for r, o2w, *_ in scene.spheres:
        m, r = np.asarray(o2w, f32).reshape(4, 4), f32(r)
        corners = [(r if k & 1 else -r, r if k & 2 else -r, r if k & 4 else -r) for k in range(8)]
        pts.append(np.array([[((m[a, 0] * x + m[a, 1] * y) + m[a, 2] * z) + m[a, 3] for a in range(3)]
                             for x, y, z in corners], f32))
    pts = np.concatenate(pts).astype(f32)
    return pts.min(0), pts.max(0)


def make_grid(lo, hi, estimator, cell_span, radius2):
    """(dx, dy, dz, ncells, bits of inv_cs)"""
    rq = np.sqrt(f32(radius2)) * f32(1.0001) + f32(1e-4)
    f = f32(0.5) if estimator == PM_ESTIMATOR_KNN else f32(2.0) / f32(cell_span - 1)
    cs = (f * rq) * f32(1.001)
    ext = [max(f32(hi[a]) - f32(lo[a]), f32(1e-3)) for a in range(3)]
    while True:
        dims = [max(1, int(np.ceil(e / cs)) + 1) for e in ext]
        if dims[0] * dims[1] * dims[2] <= 1 << 25:
            break
        cs = cs * f32(1.25)
    assert type(cs) is f32 and type(rq) is f32
    return dims[0], dims[1], dims[2], dims[0] * dims[1] * dims[2], bits(f32(1.0) / cs)


def quantile_radius2(hist, init, quantile):
    """(bin, radius^2): bins b.. hold r^2 / init <= 2^(-b/8); the largest b
    whose tail still holds the quantile, a 1 % margin, never above init."""
    total = sum(hist)
    best, above = 0, total
    for b in range(R2_BINS):
        if above < quantile * total:
            break
        best = b
        above -= hist[b]
    if total == 0:
        return best, f32(0.0)
    return best, min(f32(init), f32(float(init) * 2.0 ** (-best / R2_PER_OCTAVE) * 1.01))
