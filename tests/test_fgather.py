"""Final gathering (pm_final_gather_pass, pm_render_final_gather), the parts
that need no device: the sample set, the frame and the direction of
tests/fgather_ref.py, the accumulate and resolve arithmetic, and the argument
checks the C-ABI makes before it looks at the context.
"""
import ctypes
import json
import os
import subprocess

import numpy as np

import fgather_ref as G
from pmrender import hip
from pmrender.abi import PM_ERR_INVALID, PM_REC_MISS, RECORD_DTYPE, RenderParams

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_render_cli")
SCENES = os.path.join(ROOT, "cuda-raytrace_amd", "scenes")


def test_samples_stay_in_the_unit_square():
    """u1, u2 in [0, 1) at the extremes of the rotation and of j: a exactly 1 (j + 0.5 = N / 2, ru = 0.5),
    a just below 2, b = rv + bitreverse32(j) 2^-32 with rv at its largest"""
    top = G.ONE_MINUS
    for n in (1, 2, 5, 64, 256):
        for ru in (F32(0), F32(0.5), top, F32(2.0 ** -24)):
            for rv in (F32(0), F32(0.5), top):
                u1, u2 = G.samples32(n, ru, rv)
                assert u1.dtype == u2.dtype == np.float32
                assert (u1 >= 0).all() and (u1 <= top).all() and (u2 >= 0).all() and (u2 <= top).all()
    u1, _ = G.samples32(2, F32(0.25), F32(0))  # j = 1: a = 0.75 + 0.25 = 1 exactly -> 0
    assert u1[1] == 0
    u1, _ = G.samples32(1, top, F32(0))        # a = 0.5 + (1 - 2^-24) -> 0.5 after the wrap (rounded)
    assert 0.49 < u1[0] < 0.51


def test_hammersley_mean_cosine():
    """Cosine-weighted directions have E[z] = 2 / 3. z = sqrt(1 - r^2) depends on the radius of the concentric
    map alone, a function of bounded variation of (u1, u2), so the N = 64 rotated Hammersley set (star discrepancy
    <= (1 + log2 N) / N = 7 / 64) integrates it to within 7 / 64 by Koksma-Hlawka; float64 throughout"""
    n = 64
    for ru, rv in ((0.0, 0.0), (0.3, 0.7), (0.999, 0.123)):
        j = np.arange(n)
        u1 = np.mod((j + 0.5) / n + ru, 1.0)
        u2 = np.mod(np.array([G.bitreverse32(k) for k in j]) * 2.0 ** -32 + rv, 1.0)
        dx, dy = G.disk32(u1.astype(F32), u2.astype(F32))
        z = np.sqrt(np.maximum(0.0, 1.0 - dx.astype(np.float64) ** 2 - dy.astype(np.float64) ** 2))
        assert abs(z.mean() - 2.0 / 3.0) <= 7.0 / 64.0


def test_frame_and_direction():
    rng = np.random.default_rng(7)
    normals = list(rng.normal(size=(32, 3))) + [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, -1, 0], [1, 1, 0]]
    for n in normals:
        n = (np.asarray(n, np.float64) / np.linalg.norm(n)).astype(F32)
        v1, v2 = G.frame32(n)
        m = np.stack([v1, v2, n]).astype(np.float64)
        assert np.abs(m @ m.T - np.eye(3)).max() < 1e-6  # orthonormal
        assert np.linalg.det(m) > 0.999                   # right-handed: v1 x v2 = n
        for back in (False, True):
            d, traced = G.directions32(n, back, 16, F32(0.37), F32(0.81))
            assert traced.all() and d.dtype == np.float32
            assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6
            assert ((d @ (-n if back else n)) > 0).all()


def test_rays_of_inactive_records_are_zero():
    recs = np.zeros(3, RECORD_DTYPE)
    recs["ns"] = [0, 1, 0]
    recs["pos"] = [[1, 2, 3], [4, 5, 6], [7, 8, 9]]
    recs["flags"][1] = PM_REC_MISS
    rays = G.rays32(recs, 4, 0, 0).reshape(3, 4, 6)
    assert not rays[1].any() and (rays[0][:, :3] == [1, 2, 3]).all() and rays[2][:, 3:].any(axis=1).all()
    again = G.rays32(recs, 4, 1, 0).reshape(3, 4, 6)
    assert (again[0] != rays[0]).any()  # another pass, another rotation


def test_accumulate_and_resolve_arithmetic():
    li = np.array([[[1e8, 1, 0], [1, 1e-8, 0], [-1e8, 1, 3]]], F32)
    acc = G.accumulate32(np.zeros((1, 3), F32), li)
    want = np.zeros(3, F32)
    for j in range(3):
        want = (want + li[0, j]).astype(F32)
    assert np.array_equal(acc[0], want) and acc[0, 0] == 0  # ascending j in float32: the 1 is lost
    recs = np.zeros(2, RECORD_DTYPE)
    recs["dl"] = [[0.5, 0.5, 0.5], [9, 9, 9]]
    recs["flags"][1] = PM_REC_MISS
    out = G.resolve32(recs, np.array([[0.5, 1, 0]] * 2, F32), np.array([[3, 3, 3]] * 2, F32), 3, 2)
    assert np.array_equal(out[0], F32(0.5) + np.array([0.5, 1, 0], F32) * (F32(3) / F32(6))) and not out[1].any()
    out = G.resolve32(recs[:1], np.ones((1, 3), F32), np.array([[np.nan, 0, 0]], F32), 1, 1)
    assert not out.any()  # sanitised


def test_argument_checks_come_before_the_context():
    lib = hip.load_library()
    p = RenderParams.defaults()
    ref = ctypes.byref(p)
    err = lambda: lib.pm_last_error(None)
    for n in (0, -3, 257):
        assert lib.pm_final_gather_pass(None, ref, n, 0, None) == PM_ERR_INVALID and b"n_gather" in err()
        assert lib.pm_final_gather_rays(None, ref, n, 0, 0, 1, None) == PM_ERR_INVALID and b"n_gather" in err()
        assert lib.pm_render_final_gather(None, ref, n, None, None) == PM_ERR_INVALID and b"n_gather" in err()
    assert lib.pm_final_gather_pass(None, ref, 4, -1, None) == PM_ERR_INVALID and b"negative" in err()
    assert lib.pm_final_gather_rays(None, ref, 4, -2, 0, 1, None) == PM_ERR_INVALID and b"negative" in err()
    assert lib.pm_final_gather_pass(None, None, 4, 0, None) == PM_ERR_INVALID and b"null params" in err()
    assert lib.pm_render_final_gather(None, None, 4, None, None) == PM_ERR_INVALID and b"null params" in err()
    assert lib.pm_final_gather_pass(None, ref, 4, 0, None) == PM_ERR_INVALID and b"null context" in err()
    assert lib.pm_final_gather_resolve(None, 0, 0, None, None) == PM_ERR_INVALID and b"null context" in err()
    out = np.zeros(3, F32)
    assert lib.pm_download_gather_sum(None, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 1) == PM_ERR_INVALID
    assert b"null context" in err()


# ------------------------------------------------------------------ parser
SCENE = """
LookAt 278 273 -800  278 273 0  0 1 0
Camera "perspective" "float fov" [39.3]
Film "image" "integer xresolution" [16] "integer yresolution" [16] "string filename" "fg.pfm"
Renderer "cuda" "string rendername" "photonmapping" "integer paths" [4096] "integer finalgathersamples" [%d]
WorldBegin
LightSource "point" "point from" [278 500 279.5] "rgb I" [150000 150000 150000]
Material "matte" "rgb Kd" [0.5 0.5 0.5]
Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0  556 0 0  556 0 559]
WorldEnd
"""


def dump(path, *flags):
    r = subprocess.run([CLI, "--pbrt", str(path), "--dump", *flags], capture_output=True, text=True, timeout=60)
    return r, (json.loads(r.stdout) if r.returncode == 0 else None)


def test_finalgathersamples_key(tmp_path):
    f = tmp_path / "fg.pbrt"
    f.write_text(SCENE % 12)
    r, d = dump(f)
    assert r.returncode == 0, r.stderr
    assert d["final_gather"] == 12 and d["warnings"] == 0 and d["resample"] == 0 and d["paths"] == 4096
    r, d = dump(f, "--final-gather", "4")       # the command line wins over the file
    assert d["final_gather"] == 4 and d["warnings"] == 0
    r, d = dump(f, "--final-gather", "0")       # ... also to switch it off
    assert d["final_gather"] == 0
    r, d = dump(os.path.join(SCENES, "cornell-box.pbrt"))  # nothing parsed today changes
    assert d["final_gather"] == 0 and d["warnings"] == 0
    f.write_text(SCENE % 257)
    r, _ = dump(f)
    assert r.returncode != 0 and "finalgathersamples" in r.stderr
    r = subprocess.run([CLI, "--pbrt", str(f), "--dump", "--final-gather", "300"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--final-gather" in r.stderr
