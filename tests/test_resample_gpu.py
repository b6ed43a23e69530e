"""Resampled renders on the GPU (pm_eye_resample, pm_render_resampled,
pm_camera_rays_pass). The yardstick is the existing stages: every pass of a
resampled context must leave the records that the existing eye pass (fed the
pass's rays as host rays), a numpy merge and the existing trace / build /
gather leave in plain contexts, bit for bit.
"""
import os
import subprocess

import numpy as np
import pytest

import ray_query_ref as Q
import resample_ref as X
from pmrender import hip, scenes
from pmrender.abi import (PM_ERR_INVALID, PM_ESTIMATOR_KNN, PM_MATTE, PM_REC_INVALID, RECORD_DTYPE, RenderParams)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_render_cli")
HOST = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_pbrt_host")
SCENES = os.path.join(ROOT, "cuda-raytrace_amd", "scenes")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_records_equal(got, ref, what):
    for name in RECORD_DTYPE.names:
        a, b = got[name], ref[name]
        if a.dtype.kind == "f":
            a, b = bits(a), bits(b)
        bad = np.nonzero((a != b).reshape(len(got), -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {name} differs in {bad.size} of {len(got)} records, first {bad[:8]}"


def params(**kw):
    """4,096 paths leave 0.009 photons per unit area on the box's walls: a radius of 50 (the default is 2)
    finds some 70 per record, so flux, radius2 and photon_count move in every pass"""
    return RenderParams.defaults(**{**dict(paths_per_pass=X.PATHS, passes=X.PASSES, initial_radius2=2500.0), **kw})


def cli_params():
    return RenderParams.defaults(paths_per_pass=X.PATHS, passes=X.PASSES)  # the front ends' own defaults


def photon_pass(ctx, p, k):
    ctx.trace_photons(p, k)
    ctx.build_photon_map(p)
    ctx.gather(p)


def composition(scene, passes, p=None):
    """Context A resamples; per pass the reference takes A's rays of that pass (camera_rays), runs the
    existing eye pass on them in a host-ray context B, merges in numpy (pos / ns / material / flags of the
    pass, dl the fp32 running sum, flux / radius2 / photon_count of the previous gather) and runs the
    existing trace / build / gather on the merged records in a plain pinhole context C. Returns A's
    records after every pass (all checked against C's)."""
    p = p or params()
    _, eye, fwd, right, up, w, h, kw = scene.camera
    n2d = sum(L[-1] for L in scene.lights if L[0] == "disk") + sum(L[4] for L in scene.lights if L[0] == "mesh")
    A = scene.load_into(hip.Context(0))
    plain = scenes.Scene(**{**scene.__dict__, "camera": ("pinhole", eye, fwd, right, up, w, h)})
    C = plain.load_into(hip.Context(0))
    B = None
    try:
        pix = A.record_pixels()
        ok = pix >= 0
        assert (~ok).any() and len(pix) % 64 == 0 and w % 8 and h % 8  # padding records, a ragged tile row
        dl_sum = np.zeros((w * h, 3), np.float32)
        prev, out = None, []
        for k in range(passes):
            rays, _ = A.camera_rays(pass_=k)
            rand2d = X.light_rand2d(w * h, n2d, p.light_rng_seed, k) if n2d else None
            if B is None:
                B = scenes.Scene(**{**scene.__dict__, "camera": ("rays", rays, rand2d, n2d)}).load_into(hip.Context(0))
            else:
                B.set_eye_rays(rays, rand2d, n2d)
            B.eye_pass(p)
            b = B.download_records()
            assert len(b) == w * h
            dl_sum = dl_sum + b["dl"]
            merged = np.zeros(len(pix), RECORD_DTYPE)
            merged["flags"] = PM_REC_INVALID  # padding: as pass 0 left it
            for f in ("pos", "flags", "ns", "material"):
                merged[f][ok] = b[f][pix[ok]]
            merged["dl"][ok] = dl_sum[pix[ok]]
            for f in ("flux", "radius2", "photon_count"):
                merged[f][ok] = b[f][pix[ok]] if prev is None else prev[f][ok]
            C.upload_records(merged)
            photon_pass(C, p, k)
            prev = C.download_records()
            A.eye_resample(p, k)
            photon_pass(A, p, k)
            got = A.download_records()
            assert_records_equal(got, prev, f"pass {k}")
            out.append(got)
        return out, A.scene_info()["mode"]
    finally:
        for c in (A, B, C):
            if c is not None:
                c.close()


# ------------------------------------------------------------------ composition
@pytest.mark.parametrize("light", ("point", "disk"))
def test_composition_bit_for_bit(light):
    """20 x 12 (padding records, a ragged tile row), a lens, 3 passes of 4,096 paths; with the disk light the
    reference's light samples are the numpy restatement of Philox (pixel, slot, 0, pass; light_rng_seed, 0)"""
    recs, _ = composition(X.composition_scene(light), X.PASSES)
    hit = [~X.inactive(r) for r in recs]
    valid = (recs[0]["flags"] & PM_REC_INVALID) == 0
    gathered = recs[-1]["photon_count"] > 0
    assert gathered.sum() > 50
    hit_then_miss = (hit[0] | hit[1]) & ~hit[2] & valid
    miss_then_hit = (~hit[0] | ~hit[1]) & hit[2] & valid
    print(f"{light}: {int(hit_then_miss.sum())} pixels hit earlier and miss in the last pass, "
          f"{int(miss_then_hit.sum())} the other way round")
    assert hit_then_miss.any() and miss_then_hit.any()
    # a record moved, its statistics did not restart: pass 0's hits keep gathering under later samples
    assert (recs[-1]["photon_count"][hit[0] & hit[2]] >= recs[0]["photon_count"][hit[0] & hit[2]]).all()


def padded(sc, pad):
    """`pad` tiny spheres parked below the floor (tests/ray_query_ref.py padding_spheres): they only raise the
    primitive count and the scene's size into the next traversal mode"""
    grey = sc.material(PM_MATTE, (0.5, 0.5, 0.5))
    for r, w2o in Q.padding_spheres(pad):
        o2w = np.eye(4, dtype=np.float32)
        o2w[:3, 3] = -w2o[:3, 3]
        sc.spheres.append((r, o2w.reshape(-1), w2o.reshape(-1), grey, -1))
    return sc


def instanced():
    sc = scenes.figure_scene(X.W, X.H, subdiv=2)  # killeroo-proxy at low resolution: two instances of one mesh
    sc.camera = scenes.device_camera(X.W, X.H, **X.CAMERA)
    return sc


@pytest.mark.parametrize("mode,make", [("brute", lambda: padded(X.composition_scene("point"), 0)),
                                       ("bvh-lds", lambda: padded(X.composition_scene("point"), 66)),
                                       ("bvh-instanced", instanced),
                                       ("bvh-hbm", lambda: padded(X.composition_scene("point"), 300))],
                         ids=("brute", "lds", "instanced", "hbm"))
def test_every_traversal_mode(mode, make):
    """passes 0 and 1 of the composition test on the scene sizes the existing tests use for each mode"""
    _, got = composition(make(), 2)
    assert got == mode


# ------------------------------------------------------------------ pass 0, final, degenerate case
def test_pass_zero_is_the_eye_pass():
    sc = X.composition_scene("disk")
    a, b = sc.load_into(hip.Context(0)), sc.load_into(hip.Context(0))
    try:
        p = params()
        a.eye_resample(p, 0)
        b.eye_pass(p)
        assert_records_equal(a.download_records(), b.download_records(), "eye_resample(0) vs eye_pass")
        ra, _ = a.camera_rays(pass_=0)
        rb, _ = b.camera_rays()
        assert np.array_equal(bits(ra), bits(rb))
        r1, _ = a.camera_rays(pass_=1)
        assert (bits(r1) != bits(ra)).any(axis=1).mean() > 0.99  # a fresh sample
    finally:
        a.close(); b.close()


def test_final_is_the_pinned_formula():
    """render_resampled == dl / n + flux (1 / pi) / (r^2 emitted) in fp32 in the header's order over the
    downloaded records, the pixels whose last sample missed included: they are not black"""
    sc = X.composition_scene("disk")
    ctx = sc.load_into(hip.Context(0))
    try:
        p = params()
        img, st = ctx.render_resampled(p)
        recs = ctx.download_records()
        assert st["paths_emitted"] == X.PATHS * X.PASSES and st["ms_eye"] > 0
        assert st["gather_points"] == int((~X.inactive(recs)).sum())
        ref = X.final_resampled32(recs, X.PASSES, X.PATHS * X.PASSES)
        pix = ctx.record_pixels()
        ok = pix >= 0
        want = np.zeros((X.W * X.H, 3), np.float32)
        want[pix[ok]] = ref[ok]
        assert img.shape == (X.H, X.W, 3)
        assert np.array_equal(bits(img).reshape(-1, 3), bits(want))
        kept = X.inactive(recs) & ok & ((recs["dl"] > 0).any(axis=1) | (recs["photon_count"] > 0))
        assert kept.sum() >= 3, "no pixel hit earlier and missed in the last pass"
        assert (img.reshape(-1, 3)[pix[kept]].sum(axis=1) > 0).all()
        # the stage call uses the context's count and the same kernel
        import torch
        d = torch.empty((len(recs), 3), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.final(X.PATHS * X.PASSES, 0, len(recs), d.data_ptr())
        ctx.synchronize()
        assert np.array_equal(bits(d.cpu().numpy())[ok], bits(ref)[ok])
    finally:
        ctx.close()


def test_degenerate_case_is_render():
    """jitter off, no lens, a point light, 2 passes: the rays repeat, x + x and / 2 are exact"""
    sc = X.composition_scene("point", lens_radius=0.0, focal_distance=0.0, jitter=False)
    a, b = sc.load_into(hip.Context(0)), sc.load_into(hip.Context(0))
    try:
        p = params(passes=2)
        got, _ = a.render_resampled(p)
        ref, _ = b.render(p)
        assert ref.max() > 0 and np.array_equal(bits(got), bits(ref))
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------ refusals
def refused(ctx, p, k, word):
    with pytest.raises(hip.PMError) as e:
        ctx.eye_resample(p, k)
    assert e.value.code == PM_ERR_INVALID and word in str(e.value), str(e.value)


def with_camera(sc, **kw):
    sc.camera = scenes.device_camera(X.W, X.H, **{**X.CAMERA, **kw})
    return sc


@pytest.mark.parametrize("name", ("knn", "textured", "specular", "xsamples", "filter", "group", "order", "pinhole"))
def test_refusals(name):
    p = params()
    word = {"knn": "PM_ESTIMATOR_PPM", "textured": "textured", "specular": "specular", "xsamples": "samples per pixel",
            "filter": "filter", "group": "multi-device", "order": "before any eye pass", "pinhole": "pm_set_camera"}[name]
    sc = X.composition_scene("point")
    devices = None
    if name == "knn":
        p.estimator = PM_ESTIMATOR_KNN
    elif name == "textured":
        sc = with_camera(scenes.cornell_textured(X.W, X.H))
    elif name == "specular":
        sc = with_camera(scenes.caustic_fresnel(X.W, X.H))
    elif name == "xsamples":
        sc = with_camera(sc, xsamples=2)
    elif name == "filter":
        sc = with_camera(sc, filter="box")
    elif name == "group":
        devices = [0, 0]
    elif name == "pinhole":
        sc.camera = scenes.pinhole(X.W, X.H)
    ctx = sc.load_into(hip.Context(0, devices=devices))
    try:
        refused(ctx, p, 1 if name == "order" else 0, word)
        if name not in ("group",):
            with pytest.raises(hip.PMError):
                ctx.render_resampled(p) if name != "order" else ctx.eye_resample(p, 2)
        if name == "order":  # an eye pass makes pass 1 legal; a new camera takes that back
            ctx.eye_pass(p)
            ctx.eye_resample(p, 1)
            with_camera(sc, sample_seed=9)
            ctx.set_camera(*sc.camera[1:7], **sc.camera[7])
            refused(ctx, p, 1, word)
    finally:
        ctx.close()


# ------------------------------------------------------------------ CLI and plugin
def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = (int(v) for v in f.readline().split())
        scale = float(f.readline())
        data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4").reshape(h, w, 3)
    return data[::-1].astype(np.float32)


def test_cli_renders_the_python_scene(tmp_path):
    """pm_render_cli --pbrt cornell-dof.pbrt (its Film made small, its passes few) == scenes.cornell_dof
    through Context.render_resampled, bit for bit"""
    text = open(os.path.join(SCENES, "cornell-dof.pbrt")).read()
    text = text.replace('"integer xresolution" [256] "integer yresolution" [256]',
                        f'"integer xresolution" [{X.W}] "integer yresolution" [{X.H}]')
    text = text.replace('Include "', 'Include "' + SCENES + "/")
    assert f"[{X.W}]" in text
    scene = tmp_path / "dof.pbrt"
    scene.write_text(text)
    out = tmp_path / "dof.pfm"
    r = subprocess.run([CLI, "--pbrt", str(scene), "--paths", str(X.PATHS), "--passes", str(X.PASSES), "--out", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    ctx = scenes.cornell_dof(X.W, X.H).load_into(hip.Context(0))
    try:
        ref, _ = ctx.render_resampled(cli_params())
    finally:
        ctx.close()
    assert ref.max() > 0 and np.array_equal(bits(read_pfm(out)), bits(ref))
    # a scene the C-ABI refuses under resampling fails with the library's message
    r = subprocess.run([CLI, "--pbrt", os.path.join(SCENES, "cornell-checker.pbrt"), "--resample", "--paths", "1024",
                        "--out", str(tmp_path / "no.pfm")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "pm_eye_resample" in r.stderr and "textured" in r.stderr, r.stderr


def test_plugin_renders_the_python_scene(tmp_path):
    """Renderer "cuda" "bool resample" through the pbrt-typed boundary (pm_pbrt_host --resample) ==
    scenes.cornell_dof's image, bit for bit. 20 x 12 is a size at which the basis the plugin recovers from
    three rays of the pbrt camera is scenes.pinhole's exactly (at others it is a few ulp off, see
    test_film_gpu.py::test_plugin_paramset_device_camera)."""
    out = tmp_path / "host.bin"
    r = subprocess.run([HOST, "--width", str(X.W), "--height", str(X.H), "--paths", str(X.PATHS), "--passes", str(X.PASSES),
                        "--out", str(out), "--resample", "--lensradius", "20", "--focaldistance", "970"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{X.W * X.H} samples added" in r.stdout
    got = np.fromfile(out, np.float32)[-X.W * X.H * 3:].reshape(X.H, X.W, 3)
    ctx = scenes.cornell_dof(X.W, X.H).load_into(hip.Context(0))
    try:
        ref, _ = ctx.render_resampled(cli_params())
    finally:
        ctx.close()
    diff = bits(got) != bits(ref)
    print(f"plugin: {int(diff.sum())} of {diff.size} values differ, max |d| {float(np.abs(got - ref).max()):.3e}")
    assert ref.max() > 0 and not diff.any()
