"""Yardstick of the camera and film tests (tests/test_film.py, test_film_gpu.py):
the filter functions in float64, the film in two forms (fp32 in the order
include/pm_api.h pins: the bit-exact target; and float64), and the camera ray
formula of pm_set_camera in float64. The jitter and lens randoms are Philox
through the oracle module, as tests/mesh_light_ref.py takes its light samples.
"""
import numpy as np

import oracle
from mesh_light_ref import concentric_disk, ulp_distance  # noqa: F401  (ulp_distance: re-exported)
from pmrender.abi import (PM_FILM_TABLE, PM_FILTER_BOX, PM_FILTER_GAUSSIAN, PM_FILTER_MITCHELL, PM_FILTER_TRIANGLE)

F32 = np.float32
T = PM_FILM_TABLE


# ------------------------------------------------------------------ filters
def mitchell_1d(x, B, C):
    t = np.abs(2.0 * np.asarray(x, np.float64))
    hi = ((-B - 6 * C) * t ** 3 + (6 * B + 30 * C) * t ** 2 + (-12 * B - 48 * C) * t + (8 * B + 24 * C)) / 6.0
    lo = ((12 - 9 * B - 6 * C) * t ** 3 + (-18 + 12 * B + 6 * C) * t ** 2 + (6 - 2 * B)) / 6.0
    return np.where(t > 1.0, hi, lo)


def filter_eval(ftype, xw, yw, a, b, x, y):
    """F(x, y) in float64 from the float32 parameters, as include/pm_api.h states it."""
    xw, yw, a, b = (float(F32(v)) for v in (xw, yw, a, b))
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if ftype == PM_FILTER_BOX:
        return np.ones(np.broadcast(x, y).shape)
    if ftype == PM_FILTER_TRIANGLE:
        return np.maximum(0.0, xw - np.abs(x)) * np.maximum(0.0, yw - np.abs(y))
    if ftype == PM_FILTER_GAUSSIAN:
        def g(t, w):
            return np.maximum(0.0, np.exp(-a * t * t) - np.exp(-a * w * w))
        return g(x, xw) * g(y, yw)
    if ftype == PM_FILTER_MITCHELL:
        return mitchell_1d(x / xw, a, b) * mitchell_1d(y / yw, a, b)
    raise ValueError(ftype)


def filter_table64(ftype, xw, yw, a=0.0, b=0.0):
    """table[j, i] = F((i + 0.5) / 16 xw, (j + 0.5) / 16 yw), float64 (not yet rounded)."""
    c = (np.arange(T) + 0.5) / T
    return filter_eval(ftype, xw, yw, a, b, (c * float(F32(xw)))[None, :], (c * float(F32(yw)))[:, None])


# ------------------------------------------------------------------ samples
def philox_u01(q, seed):
    """the four uniforms of sample q: counter (lo32 q, hi32 q, 1, 0), key (seed, 0); float32"""
    out = np.zeros((len(q), 4), F32)
    for i, v in enumerate(q):
        o = oracle.philox((int(v) & 0xffffffff, int(v) >> 32, 1, 0), (int(seed), 0))
        out[i] = [F32(w >> 8) * F32(1.0 / 16777216.0) for w in o]
    return out


def sample_randoms(W, H, xs, ys, jitter, seed):
    """(ju, jv, lu, lv) float32 per sample of the (W xs) x (H ys) raster, raster order"""
    n = W * xs * H * ys
    u = philox_u01(np.arange(n), seed)
    if not jitter:
        u[:, 0] = u[:, 1] = 0.5
    return u


def film_positions32(W, H, xs, ys, u):
    """(fx, fy) as the device computes them: fp32 (ix + ju) / xs"""
    WS, HS = W * xs, H * ys
    iy, ix = np.divmod(np.arange(WS * HS), WS)
    fx = (ix.astype(F32) + u[:, 0]) / F32(xs)
    fy = (iy.astype(F32) + u[:, 1]) / F32(ys)
    return fx.astype(F32), fy.astype(F32)


# ------------------------------------------------------------------ film
def _membership(fx, fy, xw, yw):
    """per sample the pixel box [x0, x1] x [y0, y1] and (dx, dy), all fp32 as pinned"""
    xw, yw = F32(xw), F32(yw)
    dx, dy = fx - F32(0.5), fy - F32(0.5)
    return (np.ceil(dx - xw), np.floor(dx + xw), np.ceil(dy - yw), np.floor(dy + yw), dx, dy)


def film32(samples, fx, fy, W, H, table, xw, yw):
    """The film in fp32 in the pinned order: per pixel the samples in ascending
    q, sum w L and sum w in fp32, one division per channel. Returns (image
    (H, W, 3) float32, footprint sizes (H, W)). Vectorised over pixels: step k
    adds every pixel's k-th member, so each pixel's order is ascending q."""
    samples = np.asarray(samples, F32).reshape(-1, 3)
    table = np.asarray(table, F32).reshape(T, T)
    x0, x1, y0, y1, dx, dy = _membership(fx, fy, xw, yw)
    inv_xw, inv_yw = F32(1.0) / F32(xw), F32(1.0) / F32(yw)
    pix, smp = [], []
    for q in range(len(fx)):  # (pixel, sample) pairs in ascending q
        xa, xb = int(max(x0[q], 0)), int(min(x1[q], W - 1))
        ya, yb = int(max(y0[q], 0)), int(min(y1[q], H - 1))
        if xa > xb or ya > yb:
            continue
        yy, xx = np.mgrid[ya:yb + 1, xa:xb + 1]
        pix.append((yy * W + xx).ravel())
        smp.append(np.full(pix[-1].size, q))
    pix, smp = np.concatenate(pix), np.concatenate(smp)
    order = np.argsort(pix, kind="stable")  # stable: ascending q inside a pixel
    pix, smp = pix[order], smp[order]
    px, py = (pix % W).astype(F32), (pix // W).astype(F32)
    jx = np.minimum(np.floor(np.abs((px - dx[smp]) * inv_xw * F32(T))).astype(np.int64), T - 1)
    jy = np.minimum(np.floor(np.abs((py - dy[smp]) * inv_yw * F32(T))).astype(np.int64), T - 1)
    w = table[jy, jx]
    start = np.searchsorted(pix, np.arange(W * H), side="left")
    count = np.searchsorted(pix, np.arange(W * H), side="right") - start
    sw, sl = np.zeros(W * H, F32), np.zeros((W * H, 3), F32)
    for k in range(int(count.max()) if count.size else 0):
        act = np.nonzero(count > k)[0]
        i = start[act] + k
        sl[act] = sl[act] + (w[i][:, None] * samples[smp[i]]).astype(F32)
        sw[act] = sw[act] + w[i]
    with np.errstate(invalid="ignore", divide="ignore"):
        img = np.where(sw[:, None] == 0, F32(0), np.maximum(F32(0), sl / sw[:, None])).astype(F32)
    return img.reshape(H, W, 3), count.reshape(H, W)


def film64(samples, fx, fy, W, H, table, xw, yw):
    """The same film with float64 sums (membership and table index as pinned in
    fp32: they select, they do not round the result). Returns (image float64
    (H, W, 3), sum |w| |L| (H, W, 3), sum w (H, W), sum |w| (H, W), n (H, W))."""
    samples = np.asarray(samples, F32).reshape(-1, 3).astype(np.float64)
    table = np.asarray(table, F32).reshape(T, T).astype(np.float64)
    x0, x1, y0, y1, dx, dy = _membership(fx, fy, xw, yw)
    inv_xw, inv_yw = F32(1.0) / F32(xw), F32(1.0) / F32(yw)
    sl, sa = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    sw, saw, n = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W), np.int64)
    for q in range(len(fx)):
        xa, xb = int(max(x0[q], 0)), int(min(x1[q], W - 1))
        ya, yb = int(max(y0[q], 0)), int(min(y1[q], H - 1))
        if xa > xb or ya > yb:
            continue
        xx, yy = np.arange(xa, xb + 1).astype(F32), np.arange(ya, yb + 1).astype(F32)
        jx = np.minimum(np.floor(np.abs((xx - dx[q]) * inv_xw * F32(T))).astype(np.int64), T - 1)
        jy = np.minimum(np.floor(np.abs((yy - dy[q]) * inv_yw * F32(T))).astype(np.int64), T - 1)
        w = table[jy[:, None], jx[None, :]]
        sl[ya:yb + 1, xa:xb + 1] += w[..., None] * samples[q]
        sa[ya:yb + 1, xa:xb + 1] += np.abs(w)[..., None] * np.abs(samples[q])
        sw[ya:yb + 1, xa:xb + 1] += w
        saw[ya:yb + 1, xa:xb + 1] += np.abs(w)
        n[ya:yb + 1, xa:xb + 1] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        img = np.where(sw[..., None] == 0, 0.0, np.maximum(0.0, sl / sw[..., None]))
    return img, sa, sw, saw, n


# ------------------------------------------------------------------ camera
def camera_rays64(eye, fwd, right, up, W, H, xs, ys, u, lens_radius=0.0, focal_distance=0.0):
    """(origins, directions, fx, fy) in float64 from the float32 camera and the
    float32 randoms u (sample_randoms), the formula of include/pm_api.h."""
    eye, fwd, right, up = (np.asarray(v, F32).astype(np.float64) for v in (eye, fwd, right, up))
    WS, HS = W * xs, H * ys
    iy, ix = np.divmod(np.arange(WS * HS), WS)
    u = np.asarray(u, F32).astype(np.float64)
    sx = 2.0 * (ix + u[:, 0]) / WS - 1.0
    sy = 1.0 - 2.0 * (iy + u[:, 1]) / HS
    d0 = fwd[None] + sx[:, None] * right[None] + sy[:, None] * up[None]
    fx, fy = (ix + u[:, 0]) / xs, (iy + u[:, 1]) / ys
    lens_radius, focal_distance = float(F32(lens_radius)), float(F32(focal_distance))
    if lens_radius > 0.0:
        cx, cy = concentric_disk(u[:, 2], u[:, 3])
        o = eye[None] + lens_radius * (cx[:, None] * (right / np.linalg.norm(right))[None] +
                                       cy[:, None] * (up / np.linalg.norm(up))[None])
        pf = eye[None] + d0 * (focal_distance / np.linalg.norm(fwd))
        d = pf - o
    else:
        o = np.broadcast_to(eye, d0.shape).copy()
        d = d0
    return o, d / np.linalg.norm(d, axis=1, keepdims=True), fx, fy
