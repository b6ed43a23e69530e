"""Final gathering on the GPU (pm_final_gather_pass / _resolve / _rays,
pm_render_final_gather). The yardstick is the existing stages: the gather rays
a context reports are fed to a second context as host rays, where the existing
eye pass, bucket build, kNN gather and final give every ray's radiance; the
sums and the resolved image must equal the numpy float32 sum and resolve of
those, bit for bit. Only the rays themselves are compared under a tolerance
(numpy's sqrt, division, sin and cos against the device's).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import fgather_ref as G
import ray_query_ref as Q
from mesh_light_ref import ulp_distance
from pmrender import hip, scenes
from pmrender.abi import (PM_ERR_INVALID, PM_ESTIMATOR_KNN, PM_GATHER_KDTREE, PM_MATTE, PM_REC_BACKFACE,
                          PM_REC_EXCEPTION, PM_REC_MISS, RECORD_DTYPE, RenderParams)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 16
PATHS = 4096
POINT_LIGHT = ("point", np.float32([278.0, 500.0, 279.5]), np.float32([150000.0, 150000.0, 150000.0]))
# a quad inside the box whose normal points away from the eye (a BACKFACE record)
BACK_QUAD = [(200.0, 100.0, 300.0), (200.0, 200.0, 300.0), (100.0, 200.0, 300.0), (100.0, 100.0, 300.0)]
# a host ray that hits nothing: it stands in, in the second context, for a gather ray that is not traced
SAFE_RAY = np.float32([278.0, 2000.0, 278.0, 0.0, 1.0, 0.0])
# the largest ulp distance of a direction component to the float32 restatement measured on an MI355X per N
# (test_rays prints it); asserted at twice that, for libm sqrt / division / sin / cos against the device's. The
# large distances are components near zero, where an ulp is tiny, so an absolute bound stands beside it, from the
# number format alone. With e = 2^-24: sin and cos of the same float32 angle differ by at most 2 ulp between the
# two libraries, so dx and dy (|.| <= 1) differ by at most 4 e with the product's rounding; r^2 = dx^2 + dy^2 then
# by at most 2 (|dx| + |dy|) 4 e + 3 e < 15 e; z = sqrt(1 - r^2) is ill-conditioned at the rim of the disk, where
# |dz| <= 15 e / (2 z) + e; the frame, the sum of three products and the normalisation add less than 8 e to a unit
# vector. Per component: (16 + 8 / z) e, z the ray's cosine to the normal from the restatement (held above 2^-12).
RAY_ULPS_MEASURED = {1: 18, 5: 78, 32: 1502}


def ray_abs_bound(z):
    return (16.0 + 8.0 / np.maximum(z, 2.0 ** -12)) * 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def params(**kw):
    """4,096 paths leave few photons on the walls: a radius of 50 finds some for most records"""
    return RenderParams.defaults(**{**dict(paths_per_pass=PATHS, passes=1, initial_radius2=2500.0, knn_lookup=8,
                                           estimator=PM_ESTIMATOR_KNN), **kw})


def box(light="point", fov=50.0, blocks=True):
    """the Cornell box at 16 x 16 through a pinhole wide enough to see past it (MISS records), with BACK_QUAD"""
    s = scenes.cornell_box(W, H, blocks=blocks)
    if light == "point":
        s.lights = [POINT_LIGHT]
        s.disks = []
    s.add_quads([BACK_QUAD], s.material(PM_MATTE, (0.6, 0.6, 0.2)))
    s.camera = scenes.pinhole(W, H, fov_deg=fov)
    return s


def n2d_of(scene):
    return sum(L[-1] for L in scene.lights if L[0] == "disk") + sum(L[4] for L in scene.lights if L[0] == "mesh")


def kd_of(scene, recs):
    kd = np.zeros((len(recs), 3), np.float32)
    for i, r in enumerate(recs):
        if not (r["flags"] & G.INACTIVE):
            t, rgb = scene.materials[int(r["material"])]
            kd[i] = rgb if t == PM_MATTE else 0
    return kd


def on_emitter(scene, recs):
    """the records (hits of the second context) that lie on a light's disk: there the existing eye pass adds the
    emitted term, which a gather ray leaves out"""
    hit = np.zeros(len(recs), bool)
    for o, x, y, z, inner, phimax, material, light in scene.disks:
        if light < 0:
            continue
        d = recs["pos"].astype(np.float64) - np.asarray(o, np.float64)[None]
        zn = np.asarray(z, np.float64) / np.linalg.norm(z)
        hit |= (np.abs(d @ zn) < 1e-2) & (np.linalg.norm(d, axis=1) < np.linalg.norm(x) * 1.001)
    return hit & ((recs["flags"] & G.INACTIVE) == 0)


def ray_radiances(scene, p, rays, slots, pass_, B=None, instancing=True):
    """Li of every gather ray from the existing stages in a host-ray context: (li (n, 3), its records, B)"""
    dead = ~rays[:, 3:].any(axis=1)
    rb = rays.copy()
    rb[dead] = SAFE_RAY
    n2d = n2d_of(scene)
    rand2d = G.light_rand2d(0, len(rays), n2d, pass_, p.light_rng_seed) if n2d else None
    if B is None:
        B = scenes.Scene(**{**scene.__dict__, "camera": ("rays", rb, rand2d, n2d)}).load_into(hip.Context(0),
                                                                                              instancing=instancing)
    else:
        B.set_eye_rays(rb, rand2d, n2d)
    B.eye_pass(p)
    B.upload_slots(slots)
    B.build_photon_map(p)
    B.gather(p)
    li = B.final_image(p.paths_per_pass)
    recs = B.download_records()
    assert (G.INACTIVE & recs["flags"][dead]).all()
    li[dead] = 0
    return li, recs, B


def staged(scene, p, n, passes=1, A=None, instancing=True, check=True):
    """`passes` final-gather passes through the stage calls in context A, each checked against the second
    context's radiances summed in numpy. Returns (A, primary records, sums, resolved image, last B records)."""
    A = A or scene.load_into(hip.Context(0), instancing=instancing)
    B = None
    try:
        A.eye_pass(p)
        prim = A.download_records()
        acc = np.zeros((len(prim), 3), np.float32)
        brecs = None
        for k in range(passes):
            A.trace_photons(p, k)
            A.build_photon_map(p)
            slots = A.download_slots(p.paths_per_pass * p.max_photon_count)
            A.final_gather_pass(p, n, k)
            got = A.gather_sum()
            if check:
                rays = A.final_gather_rays(p, n, k)
                li, brecs, B = ray_radiances(scene, p, rays, slots, k, B, instancing)
                acc = G.accumulate32(acc, li.reshape(len(prim), n, 3))
                # a record with a ray on a light's disk: the second context's radiance has the emitted term, the
                # gather ray's has not (test_composition_disk_light_adds_no_le); its sum is taken as given
                lit = on_emitter(scene, brecs).reshape(len(prim), n).any(axis=1)
                assert lit.mean() < 0.25
                acc[lit] = got[lit]
                bad = np.nonzero((bits(got) != bits(acc)).any(axis=1))[0]
                assert bad.size == 0, f"pass {k}: sums differ in {bad.size} of {len(prim)} records, first {bad[:8]}"
        img = A.final_gather_resolve()
        if check:
            ref = G.resolve32(prim, kd_of(scene, prim), acc, n, passes)
            pix = A.record_pixels()
            ok = pix >= 0
            want = np.zeros((W * H, 3), np.float32)
            want[pix[ok]] = ref[ok]
            assert np.array_equal(bits(img).reshape(-1, 3), bits(want))
        return A, prim, got, img, brecs
    finally:
        if B is not None:
            B.close()


# ------------------------------------------------------------------ 1. rays
@pytest.mark.parametrize("n", (1, 5, 32))
def test_rays(n):
    sc = box()
    ctx = sc.load_into(hip.Context(0))
    try:
        p = params()
        ctx.eye_pass(p)
        recs = ctx.download_records()
        active = (recs["flags"] & G.INACTIVE) == 0
        assert ((recs["flags"] & PM_REC_BACKFACE) != 0)[active].any() and ((recs["flags"] & PM_REC_MISS) != 0).any()
        worst, worst_abs, worst_rel = 0, 0.0, 0.0
        for pass_ in (0, 3):
            got = ctx.final_gather_rays(p, n, pass_).reshape(len(recs), n, 6)
            ref = G.rays32(recs, n, pass_, p.light_rng_seed).reshape(len(recs), n, 6)
            assert not got[~active].any(), "an inactive record's rays are all zero"
            assert np.array_equal(bits(got[..., :3]), bits(ref[..., :3])), "origins"
            assert np.array_equal(got[..., 3:].any(axis=2), ref[..., 3:].any(axis=2)), "the traced rays"
            worst = max(worst, int(ulp_distance(got[..., 3:], ref[..., 3:]).max()))
            nn = np.where(((recs["flags"] & PM_REC_BACKFACE) != 0)[:, None], -recs["ns"], recs["ns"]).astype(np.float64)
            z = np.einsum("rjk,rk->rj", ref[..., 3:].astype(np.float64), nn)
            diff = np.abs(got[..., 3:].astype(np.float64) - ref[..., 3:]).max(axis=2)
            worst_abs = max(worst_abs, float(diff.max()))
            worst_rel = max(worst_rel, float((diff / ray_abs_bound(z))[active].max()))
            ln = np.linalg.norm(got[active][..., 3:].astype(np.float64), axis=2)
            assert np.abs(ln[ln > 0] - 1).max() < 1e-6
            # every direction lies in the hemisphere of the normal that faces the eye
            nn = np.where(((recs["flags"] & PM_REC_BACKFACE) != 0)[:, None], -recs["ns"], recs["ns"])
            assert (np.einsum("rjk,rk->rj", got[..., 3:], nn)[active] >= 0).all()
        a = ctx.final_gather_rays(p, n, 0, first=3 * n + (n > 1), count=n)  # a range that starts inside a record
        assert np.array_equal(bits(a), bits(ctx.final_gather_rays(p, n, 0).reshape(-1, 6)[3 * n + (n > 1):][:n]))
        print(f"n = {n}: largest direction ulp distance to the float32 restatement {worst}, "
              f"largest absolute difference {worst_abs:.3e} ({worst_abs * 2 ** 24:.2f} x 2^-24), "
              f"at most {worst_rel:.3f} of the (16 + 8 / z) 2^-24 bound")
        assert worst <= 2 * RAY_ULPS_MEASURED[n] and worst_rel <= 1.0
    finally:
        ctx.close()


# ------------------------------------------------------------------ 2, 3. composition
def test_composition_point_light():
    A, prim, got, img, _ = staged(box("point"), params(), 5)
    A.close()
    assert (got > 0).any(axis=1).sum() > 50 and img.max() > 0


def test_composition_disk_light_adds_no_le():
    """The exact composition holds for every record none of whose rays lands on the light's disk (the second
    context's direct light then has no emitted term either). A ray that does land there adds Le = 15 per channel in
    the second context and must add none here: the record's sum is the second context's less Le per such ray,
    within the rounding of n float32 additions of that size."""
    sc = box("disk")
    p, n = params(), 32
    A, prim, got, img, brecs = staged(sc, p, n, check=False)
    try:
        A.trace_photons(p, 0)
        slots = A.download_slots(PATHS * p.max_photon_count)
        rays = A.final_gather_rays(p, n, 0)
        li, brecs, B = ray_radiances(sc, p, rays, slots, 0)
        B.close()
        on_light = on_emitter(sc, brecs).reshape(len(prim), n)
        le = np.float32(sc.lights[0][5])
        assert on_light.any(axis=1).sum() >= 1, "no gather ray lands on the light"
        li = li.reshape(len(prim), n, 3)
        clean = ~on_light.any(axis=1)
        ref = G.accumulate32(np.zeros((len(prim), 3), np.float32), li)
        assert np.array_equal(bits(got[clean]), bits(ref[clean]))
        less = G.accumulate32(np.zeros((len(prim), 3), np.float32), np.where(on_light[..., None], li - le, li))
        tol = n * 2.0 ** -23 * np.abs(ref).max() * 2
        assert tol < 0.01 * le.min()
        assert np.abs(got[~clean].astype(np.float64) - less[~clean]).max() <= tol
    finally:
        A.close()


# ------------------------------------------------------------------ 4. traversal modes
def padded(sc, pad):
    grey = sc.material(PM_MATTE, (0.5, 0.5, 0.5))
    for r, w2o in Q.padding_spheres(pad):
        o2w = np.eye(4, dtype=np.float32)
        o2w[:3, 3] = -w2o[:3, 3]
        sc.spheres.append((r, o2w.reshape(-1), w2o.reshape(-1), grey, -1))
    return sc


@pytest.mark.parametrize("mode,pad", [("brute", 0), ("bvh-lds", 66), ("bvh-hbm", 300)], ids=("brute", "lds", "hbm"))
def test_traversal_modes(mode, pad):
    A, *_ = staged(padded(box("point"), pad), params(), 4)
    got = A.scene_info()["mode"]
    A.close()
    assert got == mode


def test_instanced_equals_flattened():
    sc = scenes.figure_scene(W, H, subdiv=2)
    sc.camera = scenes.pinhole(W, H)
    p = params()
    A, _, sum_a, img_a, _ = staged(sc, p, 4)
    mode = A.scene_info()["mode"]
    A.close()
    assert mode == "bvh-instanced"
    F, _, sum_f, img_f, _ = staged(sc, p, 4, instancing=False, check=False)
    F.close()
    assert np.array_equal(bits(sum_a), bits(sum_f)) and np.array_equal(bits(img_a), bits(img_f))


# ------------------------------------------------------------------ 5. specular chain of a gather ray
def test_caustic_scene_chain():
    sc = scenes.caustic_scene(W, H)
    sc.camera = scenes.pinhole(W, H)
    p = params()
    A, prim, got, img, brecs = staged(sc, p, 8)
    A.close()
    # The secondary records themselves cannot be downloaded, so their flags and hits are not compared one by one
    # with the second context's: the evidence is indirect. A chain that ends elsewhere than the second context's
    # changes the record's Li (direct light and kNN estimate of another point) and so the sum, which matched bit
    # for bit above; a chain whose Li is 0 either way (an exception against a miss) is not told apart by it.
    # What is asserted here is that the case occurs: the second context saw chains that ended in an exception
    # or a miss, beside those through the glass or off the mirror that carried light.
    assert (got > 0).any() and ((brecs["flags"] & (PM_REC_EXCEPTION | PM_REC_MISS)) != 0).any()


# ------------------------------------------------------------------ 6. chunk independence
CHILD = """
import sys, numpy as np
sys.path[:0] = [{pkg!r}, {tests!r}]
import test_fgather_gpu as T
from pmrender import hip
ctx = T.box("disk").load_into(hip.Context(0))
img, st = ctx.render_final_gather(T.params(), 5)
np.save(sys.argv[1], img)
"""


def test_chunk_independence(tmp_path):
    imgs = []
    for name, chunk in (("default", None), ("tile", str(64 * 5))):
        env = dict(os.environ)
        env.pop("PM_FG_CHUNK", None)
        if chunk:
            env["PM_FG_CHUNK"] = chunk
        out = tmp_path / f"{name}.npy"
        code = CHILD.format(pkg=os.path.join(ROOT, "cuda-raytrace_amd"), tests=os.path.join(ROOT, "tests"))
        r = subprocess.run([sys.executable, "-c", code, str(out)], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        imgs.append(np.load(out))
    assert imgs[0].max() > 0 and np.array_equal(bits(imgs[0]), bits(imgs[1]))


# ------------------------------------------------------------------ 7. passes, the whole render, the film
def test_three_passes_and_the_whole_render():
    sc = box("disk")
    p = params(passes=3)
    A, prim, got, img, _ = staged(sc, p, 5, passes=3)  # P = 3: the resolve divided by 15
    try:
        whole, st = A.render_final_gather(p, 5)
        assert np.array_equal(bits(whole), bits(img))
        assert st["paths_emitted"] == 3 * PATHS and st["ms_gather"] > 0 and st["photons_valid"] > 0
    finally:
        A.close()


def test_film_is_applied_as_render_applies_it():
    import torch
    sc = box("disk")
    _, eye, fwd, right, up, w, h = sc.camera
    sc.camera = scenes.device_camera(w, h, xsamples=2, ysamples=2, filter="gaussian", fov_deg=50.0)
    ctx = sc.load_into(hip.Context(0))
    try:
        p = params()
        img, _ = ctx.render_final_gather(p, 5)
        raster = ctx.final_gather_resolve()
        d_s = torch.from_numpy(raster.reshape(-1, 3)).to("cuda:0")
        d_i = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.film(d_s.data_ptr(), d_i.data_ptr())
        ctx.synchronize()
        assert img.shape == (h, w, 3) and img.max() > 0
        assert np.array_equal(bits(img).reshape(-1, 3), bits(d_i.cpu().numpy()))
    finally:
        ctx.close()


# ------------------------------------------------------------------ 8. primary state untouched
def test_primary_state_untouched():
    sc = box("disk")
    ctx, ref = sc.load_into(hip.Context(0)), sc.load_into(hip.Context(0))
    try:
        p = params()
        ctx.eye_pass(p)
        ctx.trace_photons(p, 0)
        ctx.build_photon_map(p)
        before = ctx.download_records()
        ctx.final_gather_pass(p, 5, 0)
        after = ctx.download_records()
        assert before.tobytes() == after.tobytes()
        ctx.gather(p)
        got = ctx.final_image(PATHS)
        want, _ = ref.render(p)
        assert want.max() > 0 and np.array_equal(bits(got), bits(want))
    finally:
        ctx.close(); ref.close()


# ------------------------------------------------------------------ 9. refusals
@pytest.mark.parametrize("name", ("group", "kdtree", "no eye pass", "no map", "ppm map", "resampled", "textured",
                                  "specular", "n_gather", "pass", "continues"))
def test_refusals(name):
    word = {"group": "multi-device", "kdtree": "PM_GATHER_GRID", "no eye pass": "pm_eye_pass", "no map": "no photon map",
            "ppm map": "PM_ESTIMATOR_KNN", "resampled": "pm_eye_resample", "textured": "textured",
            "specular": "specular", "n_gather": "n_gather", "pass": "negative", "continues": "continues"}[name]
    p, n, k = params(), 4, 0
    sc = box("point")
    devices = None
    if name == "group":
        devices = [0, 0]
    elif name == "textured":
        sc = scenes.cornell_textured(W, H)
    elif name == "specular":
        sc = scenes.caustic_fresnel(W, H)
    elif name == "resampled":
        sc.camera = scenes.device_camera(W, H, jitter=True)
    ctx = sc.load_into(hip.Context(0, devices=devices))
    try:
        if name not in ("group", "no eye pass"):
            ctx.eye_pass(p)
        if name == "resampled":
            q = params(estimator=0)
            ctx.eye_resample(q, 1)
        if name not in ("group", "no eye pass", "no map", "textured", "specular"):
            q = params(estimator=0) if name == "ppm map" else p
            ctx.trace_photons(q, 0)
            ctx.build_photon_map(q)
        if name == "kdtree":
            p = params(gather_structure=PM_GATHER_KDTREE, estimator=0)
        n = 257 if name == "n_gather" else n
        k = -1 if name == "pass" else 2 if name == "continues" else 0
        with pytest.raises(hip.PMError) as e:
            ctx.final_gather_pass(p, n, k)
        assert e.value.code == PM_ERR_INVALID and word in str(e.value), str(e.value)
        if name == "continues":
            with pytest.raises(hip.PMError):
                ctx.final_gather_resolve()
    finally:
        ctx.close()


def test_new_primary_records_drop_the_sums():
    """an eye pass (or new eye samples) after pass 0 leaves no sums to continue or to resolve, though the record
    count is the same"""
    ctx = box("point").load_into(hip.Context(0))
    try:
        p = params()
        ctx.eye_pass(p)
        ctx.trace_photons(p, 0)
        ctx.build_photon_map(p)
        ctx.final_gather_pass(p, 4, 0)
        ctx.final_gather_pass(p, 4, 1)  # continues
        ctx.eye_pass(p)
        for call in (lambda: ctx.final_gather_pass(p, 4, 2), ctx.final_gather_resolve, ctx.gather_sum):
            with pytest.raises(hip.PMError) as e:
                call()
            assert e.value.code == PM_ERR_INVALID
        ctx.final_gather_pass(p, 4, 0)
        ctx.set_pinhole(*box("point").camera[1:])
        with pytest.raises(hip.PMError):
            ctx.final_gather_resolve()
    finally:
        ctx.close()


# ------------------------------------------------------------------ 10. front ends
CLI = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_render_cli")
HOST = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_pbrt_host")
SCENES = os.path.join(ROOT, "cuda-raytrace_amd", "scenes")


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = (int(v) for v in f.readline().split())
        scale = float(f.readline())
        data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4").reshape(h, w, 3)
    return data[::-1].astype(np.float32)


def stage_driver(sc, p, n):
    """eye pass, trace, bucket build, final-gather pass, resolve through the stage calls: (H, W, 3) or (n, 3)"""
    ctx = sc.load_into(hip.Context(0))
    try:
        ctx.eye_pass(p)
        ctx.trace_photons(p, 0)
        ctx.build_photon_map(p)
        ctx.final_gather_pass(p, n, 0)
        return ctx.final_gather_resolve()
    finally:
        ctx.close()


def test_front_ends_write_the_stage_drivers_image(tmp_path):
    """pm_render_cli --final-gather 4 on cornell-box.pbrt at 16 x 16, the same scene with the Renderer key, and
    pm_pbrt_host --final-gather 4: each image equals the stage driver's bit for bit. The two scene-file renders
    are scenes.cornell_box through the pinhole; the plugin host hands its own pbrt camera's rays and light
    samples to the renderer and writes them out, and the stage driver runs on those (as
    tests/test_pbrt_boundary.py compares it)."""
    p = RenderParams.defaults(paths_per_pass=PATHS, estimator=PM_ESTIMATOR_KNN)  # the front ends' own defaults
    text = open(os.path.join(SCENES, "cornell-box.pbrt")).read()
    text = text.replace('"integer xresolution" [256] "integer yresolution" [256]',
                        f'"integer xresolution" [{W}] "integer yresolution" [{H}]')
    text = text.replace('Include "', f'Include "{SCENES}/')
    assert f"[{W}]" in text
    keyed = text.replace('"integer passes" [1]', '"integer passes" [1] "integer finalgathersamples" [4]')
    assert keyed != text
    (tmp_path / "flag.pbrt").write_text(text)
    (tmp_path / "key.pbrt").write_text(keyed)
    want = stage_driver(scenes.cornell_box(W, H), p, 4)
    ctx = scenes.cornell_box(W, H).load_into(hip.Context(0))
    try:
        plain, _ = ctx.render(RenderParams.defaults(paths_per_pass=PATHS))
    finally:
        ctx.close()
    assert want.max() > 0 and not np.array_equal(bits(want), bits(plain))
    for name, extra in (("flag", ["--final-gather", "4"]), ("key", [])):
        out = tmp_path / f"{name}.pfm"
        r = subprocess.run([CLI, "--pbrt", str(tmp_path / f"{name}.pbrt"), "--paths", str(PATHS), "--out", str(out), *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(bits(read_pfm(out)), bits(want)), name
    # the key switched off from the command line is pm_render
    out = tmp_path / "off.pfm"
    r = subprocess.run([CLI, "--pbrt", str(tmp_path / "key.pbrt"), "--paths", str(PATHS), "--out", str(out),
                        "--final-gather", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and np.array_equal(bits(read_pfm(out)), bits(plain))
    # the plugin
    out = tmp_path / "host.bin"
    r = subprocess.run([HOST, "--width", str(W), "--height", str(H), "--paths", str(PATHS), "--out", str(out),
                        "--final-gather", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{W * H} samples added" in r.stdout
    with open(out, "rb") as f:
        hdr = np.frombuffer(f.read(16), np.int32)
        n2d, n = int(hdr[2]), W * H
        rays = np.frombuffer(f.read(n * 6 * 4), np.float32).reshape(n, 6)
        rand2d = np.frombuffer(f.read(n * 2 * n2d * 4), np.float32)
        img = np.frombuffer(f.read(n * 3 * 4), np.float32).reshape(n, 3)
    sc = scenes.cornell_box(W, H)
    sc.camera = ("rays", rays.copy(), rand2d.copy(), n2d)
    ref = stage_driver(sc, p, 4)
    assert ref.max() > 0 and np.array_equal(bits(img), bits(ref))
    # a scene the library refuses fails with its message
    r = subprocess.run([CLI, "--pbrt", os.path.join(SCENES, "cornell-checker.pbrt"), "--final-gather", "4", "--paths", "1024",
                        "--out", str(tmp_path / "no.pfm")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "pm_render_final_gather" in r.stderr and "textured" in r.stderr, r.stderr


# ------------------------------------------------------------------ 11. energy
def test_energy_matches_the_plain_knn_estimate():
    """The closed Cornell box seen from inside, N = 64, 65,536 paths: the mean of the final-gathered indirect
    image against the mean of the plain kNN indirect image. Both estimate the same integral, so a missing 1 / pi
    or Kd, or a direct term counted twice, shows as a factor. Measured on an MI355X: see DESIGN.md."""
    sc = scenes.cornell_box(W, H)
    white = sc.material(PM_MATTE, (0.75, 0.75, 0.75))
    sc.add_quads([[(0.0, 0.0, 0.0), (556.0, 0.0, 0.0), (556.0, 548.8, 0.0), (0.0, 548.8, 0.0)]], white)  # the front wall
    sc.camera = scenes.pinhole(W, H, eye=(278.0, 273.0, 20.0), look=(278.0, 273.0, 500.0), fov_deg=70.0)
    ctx = sc.load_into(hip.Context(0))
    try:
        p = params(paths_per_pass=65536, knn_lookup=50)
        fg, _ = ctx.render_final_gather(p, 64)
        recs = ctx.download_records()
        knn, _ = ctx.render(p)
        pix = ctx.record_pixels()
        ok = pix >= 0
        dl = np.zeros((W * H, 3), np.float32)
        dl[pix[ok]] = recs["dl"][ok]
        a = float((fg.reshape(-1, 3) - dl).mean())
        b = float((knn.reshape(-1, 3) - dl).mean())
        print(f"indirect mean: final-gathered {a:.6g}, plain kNN {b:.6g}, ratio {a / b:.4f}")
        assert b > 0 and 0.8 <= a / b <= 1.25
    finally:
        ctx.close()
