"""Resampled renders (a fresh eye sample every pass, pm_eye_resample /
pm_render_resampled), the parts that need no device: the scene-file key and
`pm_render_cli --resample` through `--dump`, the shipped cornell-dof.pbrt
against scenes.cornell_dof, the argument checks the C-ABI makes before it looks
at the context, and the composition scene of tests/test_resample_gpu.py: some of
its pixels hit in an earlier pass and miss in the last one, and some the other
way round, by the float64 ray query of tests/ray_query_ref.py.
"""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

import resample_ref as X
from pmrender import scenes
from pmrender.abi import PM_ERR_INVALID, RenderParams, Stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_render_cli")
SCENES = os.path.join(ROOT, "cuda-raytrace_amd", "scenes")


def f32(a):
    return np.asarray(a, np.float32)


def dump(path, *flags):
    r = subprocess.run([CLI, "--pbrt", str(path), "--dump", *flags], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout), r.stderr


def forced(cam):
    """the camera of a resampled render: the device camera, one stratum, no film, jitter on"""
    return (cam["device_camera"], cam["xsamples"], cam["ysamples"], cam["jitter"], cam["filter"]["type"]) == (1, 1, 1, 1, "none")


# ------------------------------------------------------------------ parser
def test_resample_key_of_the_shipped_scenes():
    d, err = dump(os.path.join(SCENES, "cornell-dof.pbrt"))
    assert d["resample"] == 1 and d["warnings"] == 0, err
    assert forced(d["camera"])
    assert (d["camera"]["lens_radius"], d["camera"]["focal_distance"]) == (20, 970)
    assert d["renderer"] == "photonmapping" and d["passes"] == 16
    d, _ = dump(os.path.join(SCENES, "cornell-box.pbrt"))
    assert d["resample"] == 0 and d["camera"]["device_camera"] == 0


def test_cornell_dof_pbrt_is_the_python_scene():
    """the same lights and shapes as scenes.cornell_dof, its camera and lens"""
    d, _ = dump(os.path.join(SCENES, "cornell-dof.pbrt"))
    sc = scenes.cornell_dof(256, 256)
    assert sc.resample
    shapes = [c for c in d["calls"] if c["call"] == "shape"]
    meshes = [c for c in shapes if c["name"] == "trianglemesh"]
    assert len(meshes) == len(sc.meshes) == 5
    for got, want in zip(meshes, sc.meshes):
        np.testing.assert_array_equal(f32(got["P"]), want["P"].reshape(-1))
        np.testing.assert_array_equal(np.int32(got["indices"]), want["idx"].reshape(-1))
        np.testing.assert_array_equal(f32(got["k"]), sc.materials[want["material"]][1])
        assert got["light"] == -1
    disks = [c for c in shapes if c["name"] == "disk"]
    assert len(disks) == len(sc.disks) == 1 and disks[0]["light"] == 0
    (L,) = d["lights"]
    assert len(sc.lights) == 1 and L["kind"] == "disk" and L["nsamples"] == 1
    m = f32(L["o2w"]).reshape(4, 4)
    r, h = L["radius_height_inner_phimax"][0], L["radius_height_inner_phimax"][1]
    _, o, p1, p2, n, Le, area, ns = sc.lights[0]
    np.testing.assert_array_equal((m @ f32([0, 0, h, 1]))[:3], o)
    np.testing.assert_array_equal((m[:3, :3] @ f32([r, 0, 0])), p1)
    np.testing.assert_array_equal((m[:3, :3] @ f32([0, r, 0])), p2)
    np.testing.assert_array_equal(f32(L["Le"]), Le)
    assert np.float32(L["radius_height_inner_phimax"][3]) == np.float32(2 * math.pi)
    _, eye, fwd, right, up, W, H, kw = sc.camera
    c = d["camera"]
    assert (c["width"], c["height"]) == (W, H)
    for k, v in (("eye", eye), ("fwd", fwd), ("right", right), ("up", up)):
        np.testing.assert_array_equal(f32(c[k]), f32(v), err_msg=k)
    assert (c["xsamples"], c["ysamples"], bool(c["jitter"]), c["sample_seed"]) == \
           (kw["xsamples"], kw["ysamples"], kw["jitter"], kw["sample_seed"])
    assert (np.float32(c["lens_radius"]), np.float32(c["focal_distance"])) == \
           (np.float32(kw["lens_radius"]), np.float32(kw["focal_distance"]))
    assert c["filter"]["type"] == kw["filter"] == "none"


def test_resample_overrides_sampler_and_filter_with_a_warning(tmp_path):
    text = open(os.path.join(SCENES, "cornell-dof.pbrt")).read()
    text = text.replace('Sampler "lowdiscrepancy" "integer pixelsamples" [1]',
                        'Sampler "stratified" "integer xsamples" [3] "integer ysamples" [2] "bool jitter" ["false"]\n'
                        'PixelFilter "gaussian" "float xwidth" [1.5]')
    assert "stratified" in text
    text = text.replace('Include "', 'Include "' + SCENES + "/")
    f = tmp_path / "over.pbrt"
    f.write_text(text)
    d, err = dump(f)
    assert d["resample"] == 1 and forced(d["camera"]) and d["camera"]["lens_radius"] == 20
    assert d["warnings"] == 2, err
    assert "Sampler" in err and "PixelFilter" in err and err.count("ignored") == 2
    # without the key the same file asks for the film: nothing is forced, nothing warned about
    g = tmp_path / "plain.pbrt"
    g.write_text(text.replace(' "bool resample" ["true"]', ""))
    d, err = dump(g)
    assert d["resample"] == 0 and d["warnings"] == 0, err
    assert (d["camera"]["xsamples"], d["camera"]["ysamples"], d["camera"]["jitter"]) == (3, 2, 0)
    assert d["camera"]["filter"]["type"] == "gaussian"


def test_cli_flag_resample():
    """--resample over a scene file without the key; --lens still sets the lens, --spp warns"""
    d, err = dump(os.path.join(SCENES, "cornell-box.pbrt"), "--resample", "--lens", "6:900")
    assert d["resample"] == 1 and forced(d["camera"]) and d["warnings"] == 0, err
    assert (d["camera"]["lens_radius"], d["camera"]["focal_distance"]) == (6, 900)
    d, err = dump(os.path.join(SCENES, "cornell-box.pbrt"), "--resample", "--spp", "2x2", "--filter", "box")
    assert d["resample"] == 1 and forced(d["camera"]) and d["warnings"] == 1 and "ignored" in err, err


# ------------------------------------------------------------------ C-ABI without a device
def test_argument_checks_without_a_context(hip_mod):
    """what the new calls check before they look at the context; a null context is an error, not a crash
    (the pattern of test_abi.py::test_create_reports_error_without_device)"""
    lib = hip_mod.load_library()
    p = RenderParams.defaults()
    assert lib.pm_eye_resample(None, ctypes.byref(p), -1, None) == PM_ERR_INVALID
    assert b"negative" in lib.pm_last_error(None)
    assert lib.pm_eye_resample(None, None, 0, None) == PM_ERR_INVALID
    assert b"null params" in lib.pm_last_error(None)
    assert lib.pm_eye_resample(None, ctypes.byref(p), 1, None) == PM_ERR_INVALID
    assert b"null context" in lib.pm_last_error(None)
    out = np.zeros(3, np.float32)
    st = Stats()
    assert lib.pm_render_resampled(None, ctypes.byref(p), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                   ctypes.byref(st)) == PM_ERR_INVALID
    assert b"null context" in lib.pm_last_error(None)
    assert lib.pm_camera_rays_pass(None, -3, 0, 1, None, None) == PM_ERR_INVALID
    assert b"negative" in lib.pm_last_error(None)
    assert lib.pm_camera_rays_pass(None, 2, 0, 1, None, None) == PM_ERR_INVALID
    assert b"null context" in lib.pm_last_error(None)


def test_python_front_end_has_the_calls(hip_mod):
    for name in ("eye_resample", "render_resampled", "camera_rays"):
        assert callable(getattr(hip_mod.Context, name))
    import inspect
    assert "pass_" in inspect.signature(hip_mod.Context.camera_rays).parameters


# ------------------------------------------------------------------ the composition scene
@pytest.mark.parametrize("light", ("point", "disk"))
def test_composition_scene_mixes_hits_and_misses(light, oracle_mod):
    """the inputs of test_resample_gpu.py's composition test: by the float64 rays and ray query, some pixels
    are a decided hit in pass 0 or 1 and a decided miss in pass 2, and some the other way round"""
    sc = X.composition_scene(light)
    hits = [X.pass_hits(sc, k) for k in range(X.PASSES)]
    assert all((h >= 0).mean() > 0.98 for h in hits)
    early_hit, early_miss = (hits[0] == 1) | (hits[1] == 1), (hits[0] == 0) | (hits[1] == 0)
    assert (early_hit & (hits[2] == 0)).sum() >= 3
    assert (early_miss & (hits[2] == 1)).sum() >= 3
