"""Reference for power-weighted light selection (PM_ALL_LIGHTS): the light
selection table in float64 as include/pm_api.h states it
(pm_light_selection_cdf), the fifth Halton dimension (base 11, table entries
17..27) restated in numpy float32 with the reference's `n *= invBase` quirk,
the pick itself, and the scenes of tests/test_multi_light*.py.

The restated radical inverse is proved before it is used (prove_restatement):
the same function with bases 3, 5, 7 must give dimensions 1-3 of
oracle.halton_sample bit for bit, around indices 0, 12,582,912 (where the
quirk's truncated product first leaves floor(n / base)) and 2^24.
"""
import functools
import math

import numpy as np

import mesh_light_ref as MR
import oracle
from pmrender import scenes
from pmrender.abi import PM_LIGHT_AREA_DISK, PM_LIGHT_AREA_MESH, PM_LIGHT_POINT, PM_MATTE

U24 = 2.0 ** -24
# (base, first table entry) of the Halton dimensions (PermutedHalton(5, ...): 2 + 3 + 5 + 7 + 11 = 28 entries)
DIMS = ((2, 0), (3, 2), (5, 5), (7, 10), (11, 17))
QUIRK_EDGES = (0, 12582912, 1 << 24)


# ------------------------------------------------------------------ table
def weights(types, le_rgb, areas):
    """selection weight per light, float64 from the float32 inputs (pm_api.h)"""
    le = np.asarray(le_rgb, np.float32).reshape(-1, 3).astype(np.float64)
    ar = np.asarray(areas, np.float32).astype(np.float64)
    w = []
    for t, c, a in zip(types, le, ar):
        y = 0.212671 * c[0] + 0.715160 * c[1] + 0.072169 * c[2]
        if t == PM_LIGHT_POINT:
            x = y * (4.0 * math.pi)
        elif t in (PM_LIGHT_AREA_DISK, PM_LIGHT_AREA_MESH):
            x = y * (math.pi * a)
        else:
            raise ValueError(f"unknown light type {t}")
        w.append(0.0 if x < 0.0 else x)
    return np.asarray(w, np.float64)


def table_ref(types, le_rgb, areas):
    """cdf float32: running sum in light order, cdf[l] = (float)(sum[l] / sum[n-1]), cdf[n-1] = 1"""
    run = np.cumsum(weights(types, le_rgb, areas))       # np.cumsum adds in index order
    if len(run) == 0 or not (run[-1] > 0.0) or not np.isfinite(run[-1]):
        raise ValueError("total selection weight is 0 or not finite")
    cdf = (run / run[-1]).astype(np.float32)
    cdf[-1] = 1.0
    return cdf


def pmf_of(cdf):
    """float32 pick probabilities: cdf[l] - (l ? cdf[l-1] : 0)"""
    cdf = np.asarray(cdf, np.float32)
    return (cdf - np.concatenate([np.float32([0.0]), cdf[:-1]])).astype(np.float32)


def light_sets():
    """(types, le_rgb [n, 3], areas [n]) of the issue's light sets"""
    P, D, M = PM_LIGHT_POINT, PM_LIGHT_AREA_DISK, PM_LIGHT_AREA_MESH
    rng = np.random.RandomState(11)
    out = {
        "one": ([D], [[17, 17, 17]], [13273.0]),
        "zero_second": ([D, M], [[17, 11, 5], [0, 0, 0]], [1256.5, 400.0]),
        # weights about 1 : 30 : 1000 (point 4 pi y, disk pi A y, mesh pi A y)
        "mixed3": ([P, D, M], [[1.0, 1.0, 1.0], [3.0, 2.0, 1.0], [5.0, 9.0, 20.0]], [0.0, 57.0, 447.0]),
    }
    for n in (5, 33):
        types = [(P, D, M)[i % 3] for i in range(n)]
        out[f"n{n}"] = (types, rng.uniform(0.0, 20.0, (n, 3)), rng.uniform(1.0, 500.0, n))
    return {k: (list(t), np.asarray(c, np.float32), np.asarray(a, np.float32)) for k, (t, c, a) in out.items()}


# ------------------------------------------------------------------ Halton
def radical_inverse_f32(n, base, table):
    """permuted_radical_inverse (photontracing.cu:19-31; pm_sample.h) over an
    array of indices, every operation in float32 as the device performs it:
    val += p[n % base] * invBi; n = (uint)((float)n * invBase); invBi *= invBase."""
    n = np.asarray(n, np.uint32).copy()
    table = np.asarray(table, np.uint32)
    inv_base = np.float32(1.0) / np.float32(base)
    val = np.zeros(n.shape, np.float32)
    inv_bi = inv_base
    while np.any(n > 0):
        live = n > 0
        d = table[n % np.uint32(base)].astype(np.float32)
        val = np.where(live, (val + (d * inv_bi).astype(np.float32)).astype(np.float32), val)
        n = np.where(live, (n.astype(np.float32) * inv_base).astype(np.float32).astype(np.uint32), n)
        inv_bi = np.float32(inv_bi * inv_base)
    return val


def edge_indices(span=40):
    idx = []
    for e in QUIRK_EDGES:
        idx.extend(range(max(0, e - span), e + span))
    return np.asarray(idx, np.uint32)


@functools.lru_cache(maxsize=None)
def prove_restatement(pass_index=0):
    """radical_inverse_f32 with bases 3, 5, 7 == dimensions 1-3 of
    oracle.halton_sample, bit for bit, around every edge. Returns the number
    of indices compared."""
    perm = oracle.halton_permutation(pass_index)
    idx = edge_indices()
    ref = np.stack([oracle.halton_sample(int(i), perm) for i in idx]).astype(np.float32)
    for dim in (1, 2, 3):
        base, off = DIMS[dim]
        got = radical_inverse_f32(idx, base, perm[off:off + base])
        bad = np.nonzero(got.view(np.uint32) != ref[:, dim].view(np.uint32))[0]
        assert bad.size == 0, f"base {base}: restated radical inverse differs from the oracle at index {idx[bad[:4]]}"
    return len(idx)


def u5(path_ids, mpc=4, pass_index=0):
    """the selection sample of each path: base 11, table perm[17:28], index pid * mpc (uint32 wrap)"""
    prove_restatement(pass_index)
    perm = oracle.halton_permutation(pass_index)
    idx = (np.asarray(path_ids, np.uint64) * np.uint64(mpc)).astype(np.uint32)
    return radical_inverse_f32(idx, 11, perm[17:28])


def pick(cdf, u):
    """first l with cdf[l] > min(u, 1 - 2^-24)"""
    u = np.minimum(np.asarray(u, np.float32), np.float32(1.0 - U24))
    return np.searchsorted(np.asarray(cdf, np.float32), u, side="right")


# ------------------------------------------------------------------ rounding bound
def alpha_bound(bounces):
    """Relative bound between a PM_ALL_LIGHTS deposit's alpha and alpha_k / pmf
    of the same path traced from its light k alone, after `bounces` Lambert
    bounces. Both are the same real product; path_shade applies three float
    roundings to alpha per Lambert bounce (alpha * fr: one per component;
    * absdot: one; * rcp(bpdf): one — the reciprocal itself does not depend on
    alpha; a specular continuation leaves alpha alone), and the all-lights
    emission one more (the division by pmf). So R_k = 3 b, R_all = 3 b + 1, and
    the quotient of the two lies within (1 + u)^(R_all + R_k) - 1, u = 2^-24 / (1 - 2^-24)."""
    u = U24 / (1.0 - U24)
    return (1.0 + u) ** (6 * np.asarray(bounces, np.float64) + 1) - 1.0


# ------------------------------------------------------------------ scenes
PAD_Z = 700.0   # behind the back wall (z = 559.2): no path gets there


def _pad(s, pad):
    """matte primitives behind the back wall, out of every path's reach, to
    push the scene into each traversal mode (as mesh_light_ref._padding)"""
    grey = s.material(PM_MATTE, (0.5, 0.5, 0.5))
    if pad == "inst":
        s.objects.append(dict(P=np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), idx=np.int32([[0, 1, 2]]), N=None, uv=None,
                              material=grey, light=-1))
        s.instances.append((0, *scenes.translate(100.0, 100.0, PAD_Z)))
        return
    for i in range(int(pad)):
        o2w, w2o = scenes.translate(20.0 + 25.0 * (i % 20), 20.0 + 25.0 * (i // 20), PAD_Z)
        s.spheres.append((np.float32(5.0), o2w, w2o, grey, -1))


def mixed_scene(W=64, H=48, pad=0, mesh_le=scenes.WALL_LIGHT_LE):
    """Three lights of mixed type and distinct colours in a matte Cornell
    enclosure with a mirror sphere (scenes.feature_scene: the ceiling disk, 2
    shadow samples, then a point light) plus the blue wall quad as a mesh
    light: lights (disk, point, mesh)."""
    s = scenes.feature_scene(W, H)
    s.add_mesh_light(scenes.WALL_LIGHT, [(0, 1, 2), (0, 2, 3)], mesh_le, 1)
    if pad:
        _pad(s, pad)
    return s


def one_light_scene(W=64, H=48):
    return scenes.cornell_box(W, H)


def zero_second_scene(W=64, H=48):
    """two lights, the second one with Le = 0: cdf [1, 1], every pick is light 0 with pmf 1"""
    s = scenes.cornell_box(W, H)
    s.add_mesh_light(scenes.WALL_LIGHT, [(0, 1, 2), (0, 2, 3)], (0.0, 0.0, 0.0), 1)
    return s


def scene_light_arrays(scene):
    """(types, le_rgb, areas) of a Scene's lights as pm_commit hands them to pm_light_selection_cdf"""
    types, le, areas = [], [], []
    for L in scene.lights:
        if L[0] == "point":
            types.append(PM_LIGHT_POINT); le.append(L[2]); areas.append(0.0)
        elif L[0] == "mesh":
            types.append(PM_LIGHT_AREA_MESH); le.append(L[3])
            areas.append(np.float32(MR.table_ref(L[1], L[2])[1]))
        else:
            types.append(PM_LIGHT_AREA_DISK); le.append(L[5]); areas.append(L[6])
    return types, np.asarray(le, np.float32), np.asarray(areas, np.float32)


def emission_bounds(scene, cdf=None):
    """the emitted-weight bound of the fixed-point scales (pm_scene.cpp light_summary):
    max over the lights of max|Le| * (4 pi | 2 pi area), each divided by its
    float pmf (lights with pmf > 0 only) when `cdf` is given"""
    types, le, areas = scene_light_arrays(scene)
    pmf = np.ones(len(types), np.float32) if cdf is None else pmf_of(cdf)
    em = 0.0
    for t, c, a, p in zip(types, le, areas, pmf):
        if not p > 0:
            continue
        b = float(np.abs(c).max()) * (4.0 * math.pi if t == PM_LIGHT_POINT else float(a) * 2.0 * math.pi)
        em = max(em, b / float(p))
    return max(em, 1e-30)


def ppm_fixed_unit(scene, cdf, max_photon_count=4):
    """one unit of the PPM gather's fixed point under PM_ALL_LIGHTS (pm_api_gather.cpp
    gather_params): 2^-S, S = floor(log2(2^40 / cmax)), cmax = emission bound *
    kd_max^mpc * kd_max / pi * 4"""
    kd = 1.0
    for mtype, rgb in scene.materials:
        if mtype == PM_MATTE:
            kd = max(kd, float(np.max(rgb)))
    cmax = emission_bounds(scene, cdf) * kd ** max_photon_count * (kd / math.pi) * 4.0
    S = int(math.floor(math.log2(2.0 ** 40 / max(cmax, 1e-30))))
    return 2.0 ** -max(-60, min(60, S))
