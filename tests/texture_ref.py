"""float64 restatement of the texture lookup (csrc/pm_texture.h, pm_api.h
pm_add_texture_*): the UVMapping2D, the wrap modes, the level-0 bilinear
lookup in the stated lerp form a + f (b - a), the checkerboard and the scale;
and the (u, v) of a triangle hit from its world position. Written from the
contract in pm_api.h, vectorised over points."""
import numpy as np

REPEAT, BLACK, CLAMP = 0, 1, 2
WRAPS = {"repeat": REPEAT, "black": BLACK, "clamp": CLAMP}


def _texel(img, x, y, wrap):
    h, w = img.shape[:2]
    if wrap == REPEAT:
        return img[np.mod(y, h), np.mod(x, w)]
    if wrap == CLAMP:
        return img[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    out = img[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].copy()
    out[~inside] = 0.0
    return out


def image(img, u, v, wrap="repeat", mapping=(1.0, 1.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)):
    """img (h, w, 3), row 0 at v = 0; u, v arrays -> (n, 3) float64."""
    img = np.asarray(img, np.float64)
    wrap = WRAPS[wrap] if isinstance(wrap, str) else wrap
    su, sv, du, dv = (float(np.float32(m)) for m in mapping)
    h, w = img.shape[:2]
    s, t = su * np.asarray(u, np.float64) + du, sv * np.asarray(v, np.float64) + dv
    x, y = s * w - 0.5, t * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)
    a, b = _texel(img, ix, iy, wrap), _texel(img, ix + 1, iy, wrap)
    c, d = _texel(img, ix, iy + 1, wrap), _texel(img, ix + 1, iy + 1, wrap)
    r0, r1 = a + fx * (b - a), c + fx * (d - c)
    return (r0 + fy * (r1 - r0)) * np.asarray(np.float32(scale), np.float64)


def checker_first(u, v, mapping):
    """True where the checkerboard picks its first operand."""
    su, sv, du, dv = (float(np.float32(m)) for m in mapping)
    s, t = su * np.asarray(u, np.float64) + du, sv * np.asarray(v, np.float64) + dv
    return (np.floor(s).astype(np.int64) + np.floor(t).astype(np.int64)) % 2 == 0


def checker_edge_distance(u, v, mapping):
    """distance in (s, t) to the nearest checker edge (an integer s or t)"""
    su, sv, du, dv = (float(np.float32(m)) for m in mapping)
    s, t = su * np.asarray(u, np.float64) + du, sv * np.asarray(v, np.float64) + dv
    return np.minimum(np.abs(s - np.round(s)), np.abs(t - np.round(t)))


def evaluate(tex, u, v):
    """tex: ("const", rgb) | ("image", img, wrap, mapping, scale) | ("checker", op1, op2, mapping) |
    ("scale", op1, op2), operands being const / image tuples."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    if tex[0] == "const":
        return np.broadcast_to(np.asarray(np.float32(tex[1]), np.float64), (len(u), 3)).copy()
    if tex[0] == "image":
        return image(tex[1], u, v, tex[2], tex[3], tex[4])
    if tex[0] == "checker":
        first = checker_first(u, v, tex[3])
        return np.where(first[:, None], evaluate(tex[1], u, v), evaluate(tex[2], u, v))
    if tex[0] == "scale":
        return evaluate(tex[1], u, v) * evaluate(tex[2], u, v)
    raise ValueError(tex[0])


def triangle_uv(p, p0, p1, p2, uv0=(0.0, 0.0), uv1=(1.0, 0.0), uv2=(0.0, 1.0)):
    """(u, v) of world points p (n, 3) on triangle (p0, p1, p2): barycentrics by
    least squares in float64, then b0 uv0 + b1 uv1 + b2 uv2. Also returns (b1, b2)."""
    p, p0, p1, p2 = (np.asarray(a, np.float64) for a in (p, p0, p1, p2))
    e1, e2 = p1 - p0, p2 - p0
    d = p - p0
    a11, a12, a22 = e1 @ e1, e1 @ e2, e2 @ e2
    r1, r2 = d @ e1, d @ e2
    det = a11 * a22 - a12 * a12
    b1, b2 = (a22 * r1 - a12 * r2) / det, (a11 * r2 - a12 * r1) / det
    b0 = 1.0 - b1 - b2
    uv0, uv1, uv2 = (np.asarray(a, np.float64) for a in (uv0, uv1, uv2))
    uv = b0[:, None] * uv0 + b1[:, None] * uv1 + b2[:, None] * uv2
    return uv[:, 0], uv[:, 1], b1, b2


def mesh_uv(p, P, idx, uv=None, tol=1e-3, with_distance=False, with_margin=False):
    """(u, v, hit) of points p on the mesh (P, idx, per-vertex uv or None): of the triangles that
    contain a point (barycentrics within tol, its plane within tol x the mesh's size) the one whose
    plane is nearest, and among coplanar ones the one the point lies deepest inside; hit False where
    none does. with_distance: also that plane distance (inf: no hit); with_margin: also the point's
    smallest barycentric there (its distance to the triangle's edges, where default uvs jump)."""
    p = np.asarray(p, np.float64)
    P = np.asarray(P, np.float64).reshape(-1, 3)
    idx = np.asarray(idx).reshape(-1, 3)
    u, v, best, margin = np.zeros(len(p)), np.zeros(len(p)), np.full(len(p), np.inf), np.full(len(p), -np.inf)
    for tri in idx:
        p0, p1, p2 = P[tri]
        n = np.cross(p1 - p0, p2 - p0)
        n /= np.linalg.norm(n)
        corners = ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0)) if uv is None else tuple(np.asarray(uv, np.float64).reshape(-1, 2)[tri])
        tu, tv, b1, b2 = triangle_uv(p, p0, p1, p2, *corners)
        dist = np.abs((p - p0) @ n)
        mb = np.minimum(np.minimum(b1, b2), 1.0 - b1 - b2)
        on = (dist < tol * max(1.0, np.abs(P).max())) & (mb >= -tol)
        on &= (dist < best - 1e-6) | ((dist <= best + 1e-6) & (mb > margin))
        u[on], v[on], best[on], margin[on] = tu[on], tv[on], dist[on], mb[on]
    hit = np.isfinite(best)
    out = (u, v, hit)
    if with_distance:
        out += (best,)
    if with_margin:
        out += (margin,)
    return out


def disk_uv(p, o, x, y, inner=0.0, phimax=2.0 * np.pi):
    """pbrt-v2 Disk: u = phi / phiMax, v = 1 - (r - r_i) / (R - r_i) of world points p on the disk with
    centre o and radius vectors x, y (inner: r_i / R); also returns phi"""
    p, o, x, y = (np.asarray(a, np.float64) for a in (p, o, x, y))
    d = p - o
    lx, ly = d @ x / (x @ x), d @ y / (y @ y)
    phi = np.arctan2(ly, lx)
    phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    r = np.hypot(lx, ly)
    return phi / float(phimax), 1.0 - (r - inner) / (1.0 - inner), phi


def sphere_uv(p, w2o):
    """pbrt-v2 full Sphere: u = phi / 2 pi, v = (theta - pi) / (0 - pi) of world points p, taken to object
    space with the row-major 4 x 4 w2o; also returns (phi, theta)"""
    p = np.asarray(p, np.float64)
    m = np.asarray(w2o, np.float64).reshape(4, 4)
    q = p @ m[:3, :3].T + m[:3, 3]
    phi = np.arctan2(q[:, 1], q[:, 0])
    phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    theta = np.arccos(np.clip(q[:, 2] / np.linalg.norm(q, axis=1), -1.0, 1.0))
    return phi / (2 * np.pi), (theta - np.pi) / (0.0 - np.pi), phi, theta
