"""Shared pieces of the final-gathering tests (tests/test_fgather.py on the CPU,
tests/test_fgather_gpu.py on the GPU): the float32 numpy restatement of the
gather rays of include/pm_api.h (the rotated Hammersley set, pbrt's
CoordinateSystem and CosineSampleHemisphere, the direction), the Philox draws
through the oracle module's Philox4x32-10, and the accumulate / resolve
arithmetic.
"""
import numpy as np

import oracle
from pmrender.abi import PM_REC_BACKFACE, PM_REC_EXCEPTION, PM_REC_INVALID, PM_REC_MISS

F32 = np.float32
ONE_MINUS = F32(1.0 - 2.0 ** -24)
INACTIVE = PM_REC_MISS | PM_REC_EXCEPTION | PM_REC_INVALID


def u01(word):
    return F32(word >> 8) * F32(1.0 / 16777216.0)


def philox_u01(ctr, key):
    """pmdm_u01 of the four words of pmdm_philox4x32_10(ctr; key)"""
    o = oracle.philox(tuple(int(v) & 0xffffffff for v in ctr), tuple(int(v) & 0xffffffff for v in key))
    return [u01(w) for w in o]


def rotation(r, pass_, seed):
    """(ru, rv) of primary record r: counter (lo32 r, hi32 r, 3, pass), key (light_rng_seed, 0)"""
    u = philox_u01((r, r >> 32, 3, pass_), (seed, 0))
    return u[0], u[1]


def light_rand2d(first, count, n2d, pass_, seed):
    """(count, n2d, 2): the light samples of secondary records first ..: counter (lo32 s, hi32 s, 0, pass),
    key (light_rng_seed, slot)"""
    out = np.zeros((count, n2d, 2), F32)
    for i in range(count):
        s = first + i
        for t in range(n2d):
            out[i, t] = philox_u01((s, s >> 32, 0, pass_), (seed, t))[:2]
    return out


def bitreverse32(j):
    return int("{:032b}".format(int(j))[::-1], 2)


def samples32(n, ru, rv):
    """(u1, u2) of rays 0 .. n - 1 under the rotation (ru, rv), float32 in the header's order"""
    j = np.arange(n)
    a = (j.astype(F32) + F32(0.5)) / F32(n) + F32(ru)
    b = np.array([bitreverse32(k) for k in j], np.float64).astype(F32) * F32(2.0 ** -32) + F32(rv)
    u1 = np.minimum(a - np.floor(a), ONE_MINUS).astype(F32)
    u2 = np.minimum(b - np.floor(b), ONE_MINUS).astype(F32)
    return u1, u2


def disk32(u1, u2):
    """the concentric disk map as the device evaluates it (pm_sample.h), float32; sin / cos are numpy's"""
    u1, u2 = np.asarray(u1, F32), np.asarray(u2, F32)
    sx, sy = F32(2) * u1 - F32(1), F32(2) * u2 - F32(1)
    r, num, base = np.ones_like(sx), np.zeros_like(sx), np.zeros_like(sx)
    a = (sx >= -sy) & (sx > sy)
    b = (sx >= -sy) & ~(sx > sy)
    c = ~(sx >= -sy) & (sx <= sy)
    d = ~(sx >= -sy) & ~(sx <= sy)
    r[a], num[a], base[a] = sx[a], sy[a], np.where(sy[a] > 0, F32(0), F32(8))
    r[b], num[b], base[b] = sy[b], -sx[b], F32(2)
    r[c], num[c], base[c] = -sx[c], -sy[c], F32(4)
    r[d], num[d], base[d] = -sy[d], sx[d], F32(6)
    zero = (sx == 0) & (sy == 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        theta = (base + num / r).astype(F32)
    theta = (theta.astype(np.float64) * (np.pi / 4.0)).astype(F32)
    dx, dy = (r * np.cos(theta)).astype(F32), (r * np.sin(theta)).astype(F32)
    return np.where(zero, F32(0), dx), np.where(zero, F32(0), dy)


def frame32(n):
    """pbrt's CoordinateSystem(n) in float32: (v1, v2)"""
    n = np.asarray(n, F32)
    if abs(n[0]) > abs(n[1]):
        il = F32(1) / np.sqrt(n[0] * n[0] + n[2] * n[2])
        v1 = np.array([-n[2] * il, F32(0), n[0] * il], F32)
    else:
        il = F32(1) / np.sqrt(n[1] * n[1] + n[2] * n[2])
        v1 = np.array([F32(0), n[2] * il, -n[1] * il], F32)
    v2 = np.array([n[1] * v1[2] - n[2] * v1[1], n[2] * v1[0] - n[0] * v1[2], n[0] * v1[1] - n[1] * v1[0]], F32)
    return v1, v2


def directions32(ns, backface, n, ru, rv):
    """(n, 3) float32 directions of a record's rays and the mask of the traced ones (z != 0)"""
    nn = -np.asarray(ns, F32) if backface else np.asarray(ns, F32)
    u1, u2 = samples32(n, ru, rv)
    dx, dy = disk32(u1, u2)
    z = np.sqrt(np.maximum(F32(0), F32(1) - dx * dx - dy * dy)).astype(F32)
    v1, v2 = frame32(nn)
    v = ((dx[:, None] * v1[None] + dy[:, None] * v2[None]) + z[:, None] * nn[None]).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = F32(1) / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    d = (v * inv[:, None]).astype(F32)
    traced = z != 0
    d[~traced] = 0
    return d, traced


def rays32(recs, n, pass_, seed):
    """(len(recs) * n, 6): what pm_final_gather_rays returns, restated"""
    out = np.zeros((len(recs), n, 6), F32)
    for r, rec in enumerate(recs):
        if rec["flags"] & INACTIVE:
            continue
        ru, rv = rotation(r, pass_, seed)
        d, traced = directions32(rec["ns"], bool(rec["flags"] & PM_REC_BACKFACE), n, ru, rv)
        out[r, :, :3] = rec["pos"]
        out[r, :, 3:] = d
    return out.reshape(-1, 6)


def accumulate32(acc, li):
    """A += Li_j in ascending j, float32: acc (nrec, 3), li (nrec, n, 3)"""
    acc = np.array(acc, F32)
    for j in range(li.shape[1]):
        acc = (acc + li[:, j].astype(F32)).astype(F32)
    return acc


def sanitize32(out):
    with np.errstate(all="ignore"):
        y = F32(0.212671) * out[:, 0] + F32(0.715160) * out[:, 1] + F32(0.072169) * out[:, 2]
    bad = np.isnan(out).any(axis=1) | (y < F32(-1e-5)) | np.isinf(y)
    out = out.copy()
    out[bad] = 0
    return out


def resolve32(recs, kd, acc, n, passes):
    """out_r = dl_r + Kd_r x (A_r / (float)(N P)), sanitised; inactive records black. (nrec, 3), record order"""
    with np.errstate(all="ignore"):
        out = (recs["dl"].astype(F32) + np.asarray(kd, F32) * (np.asarray(acc, F32) / F32(n * passes))).astype(F32)
    out = sanitize32(out)
    out[(recs["flags"] & INACTIVE) != 0] = 0
    return out
