"""Shared pieces of the resampling tests (tests/test_resample.py on the CPU,
tests/test_resample_gpu.py on the GPU): the composition scene, the Philox
randoms of eye pass k restated through the oracle module's Philox4x32-10 (as
tests/film_ref.py takes pass 0's), its camera rays in float64 and their hits
through tests/ray_query_ref.py, and the fp32 restatement of the resampled
final.
"""
import numpy as np

import film_ref as R
import oracle
import ray_query_ref as Q
from pmrender import scenes
from pmrender.abi import PM_MATTE, PM_REC_EXCEPTION, PM_REC_INVALID, PM_REC_MISS

F32 = np.float32
INV_PI = F32(0.31830988618379067154)  # pm_math.h INV_PI

# the composition test's inputs (the issue fixes image, passes, paths; lens, seed and quad are chosen so that
# some pixels hit in an earlier pass and miss in the last one and some the other way round: test_resample.py)
W, H, PASSES, PATHS = 20, 12, 3, 4096
CAMERA = dict(lens_radius=30.0, focal_distance=900.0, sample_seed=5, jitter=True)
# a free-standing quad facing the eye, left of the box's green wall (x = 0) where the 20 x 12 view is open
QUAD = [(-60.0, 150.0, 100.0), (-150.0, 150.0, 100.0), (-150.0, 400.0, 100.0), (-60.0, 400.0, 100.0)]
POINT_LIGHT = ("point", np.float32([278.0, 500.0, 279.5]), np.float32([150000.0, 150000.0, 150000.0]))


def composition_scene(light="point", w=W, h=H, **camera):
    """The Cornell box plus QUAD in front of the open background, through the thin-lens device camera;
    light: "point" (tests/test_gpu_configs.py's point light instead of the disk) or "disk" (the ceiling disk)."""
    s = scenes.cornell_box(w, h)
    if light == "point":
        s.lights = [POINT_LIGHT]
        s.disks = []
    s.add_quads([QUAD], s.material(PM_MATTE, (0.6, 0.6, 0.2)))
    s.camera = scenes.device_camera(w, h, **{**CAMERA, **camera})
    return s


def philox_u01(counters, key):
    """pmdm_u01 of the four words of pmdm_philox4x32_10(counter; key, 0), float32, per counter row"""
    out = np.zeros((len(counters), 4), F32)
    for i, c in enumerate(counters):
        o = oracle.philox(tuple(int(v) & 0xffffffff for v in c), (int(key), 0))
        out[i] = [F32(w >> 8) * F32(1.0 / 16777216.0) for w in o]
    return out


def camera_randoms(n, seed, pass_):
    """(ju, jv, lu, lv) of samples 0 .. n - 1 in eye pass pass_: counter (lo32 q, hi32 q, 1, pass_), key (seed, 0)"""
    return philox_u01([(q, q >> 32, 1, pass_) for q in range(n)], seed)


def light_rand2d(n, n2d, light_seed, pass_):
    """(n, n2d, 2): the light samples of eye pass pass_: counter (q, slot, 0, pass_), key (light_rng_seed, 0)"""
    u = philox_u01([(q, s, 0, pass_) for q in range(n) for s in range(n2d)], light_seed)
    return np.ascontiguousarray(u[:, :2].reshape(n, n2d, 2))


def scene_prims(scene):
    tris = np.concatenate([np.asarray(m["P"], F32)[np.asarray(m["idx"])] for m in scene.meshes])
    return Q.Prims(tris, disks=[d[:6] for d in scene.disks])


def pass_hits(scene, pass_, eps=0.1):
    """Per pixel of the scene's camera in eye pass pass_: 1 a decided hit, 0 a decided miss, -1 undecided,
    from the float64 rays of tests/film_ref.py and the float64 ray query (no fp32 anywhere)."""
    _, eye, fwd, right, up, w, h, kw = scene.camera
    u = camera_randoms(w * h, kw["sample_seed"], pass_)
    if not kw["jitter"]:
        u[:, 0] = u[:, 1] = 0.5
    o, d, _, _ = R.camera_rays64(eye, fwd, right, up, w, h, 1, 1, u, kw["lens_radius"], kw["focal_distance"])
    # the device's fp32 ray differs from the float64 one by a few ulp: a relative direction uncertainty
    a = Q.query(scene_prims(scene), np.concatenate([o, d], axis=1).astype(F32), eps, 1e30, dir_err=1e-5)
    return np.where(a.hit >= 0, 1, np.where(a.hit == Q.MISS, 0, -1))


def final_resampled32(recs, n_eye, emitted):
    """The final of a resampled render over downloaded records, fp32 in the order include/pm_api.h pins:
    dl / n + (flux (1 / pi)) (1 / (radius2 emitted)), the second term 0 while photon_count is 0; NaN, a
    luminance below -1e-5 or infinite -> black; padding records black. (n_records, 3) in record order."""
    dl, flux = recs["dl"].astype(F32), recs["flux"].astype(F32)
    with np.errstate(all="ignore"):
        inv = F32(1.0) / (recs["radius2"].astype(F32) * F32(emitted))
        idl = np.where((recs["photon_count"] != 0)[:, None], (flux * INV_PI) * inv[:, None], F32(0)).astype(F32)
        out = (dl / F32(n_eye) + idl).astype(F32)
        y = F32(0.212671) * out[:, 0] + F32(0.715160) * out[:, 1] + F32(0.072169) * out[:, 2]
    bad = np.isnan(out).any(axis=1) | (y < F32(-1e-5)) | np.isinf(y) | ((recs["flags"] & PM_REC_INVALID) != 0)
    out[bad] = 0
    return out


def inactive(recs):
    return (recs["flags"] & (PM_REC_MISS | PM_REC_EXCEPTION | PM_REC_INVALID)) != 0
