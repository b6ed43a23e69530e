"""CPU checks of the camera / film feature: the film's weight table
(pm_film_filter_table) against the float64 filters of film_ref.py, the .pbrt
directives (Camera lens, Sampler, PixelFilter) through pm_render_cli --dump,
and the ctypes mirrors of pm_filter / pm_camera. pm_set_camera's validation
needs a context, which needs a device: test_film_gpu.py holds it."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import film_ref as R
from pmrender.abi import (PM_FILTER_BOX, PM_FILTER_GAUSSIAN, PM_FILTER_MITCHELL, PM_FILTER_TRIANGLE, Camera, Filter)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_render_cli")
SCENES = os.path.join(ROOT, "cuda-raytrace_amd", "scenes")

TABLES = [(PM_FILTER_BOX, 0.5, 0.5, 0.0, 0.0), (PM_FILTER_TRIANGLE, 2.0, 2.0, 0.0, 0.0),
          (PM_FILTER_GAUSSIAN, 2.0, 2.0, 2.0, 0.0), (PM_FILTER_MITCHELL, 2.0, 2.0, 1.0 / 3.0, 1.0 / 3.0),
          (PM_FILTER_TRIANGLE, 1.3, 2.7, 0.0, 0.0), (PM_FILTER_GAUSSIAN, 1.3, 2.7, 0.7, 0.0),
          (PM_FILTER_MITCHELL, 1.3, 2.7, 0.5, 0.25), (PM_FILTER_BOX, 1.3, 2.7, 0.0, 0.0)]


@pytest.mark.parametrize("ftype,xw,yw,a,b", TABLES)
def test_filter_table(hip_mod, ftype, xw, yw, a, b):
    """each entry is one rounding of a double: <= 1 ulp from the float64 filter"""
    got = hip_mod.film_filter_table(Filter(ftype, xw, yw, a, b))
    want = R.filter_table64(ftype, xw, yw, a, b).astype(np.float32)
    assert got.shape == (16, 16)
    assert R.ulp_distance(got, want).max() <= 1
    assert np.any(got != 0)


def test_filter_table_rejects_bad_filters(hip_mod):
    for f in (Filter(0, 1.0, 1.0, 0, 0), Filter(5, 1.0, 1.0, 0, 0), Filter(PM_FILTER_BOX, 0.0, 1.0, 0, 0),
              Filter(PM_FILTER_BOX, 1.0, 4.5, 0, 0), Filter(PM_FILTER_BOX, float("nan"), 1.0, 0, 0)):
        with pytest.raises(ValueError):
            hip_mod.film_filter_table(f)


def test_struct_layouts(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pm_api.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu",'
                   'sizeof(pm_filter), sizeof(pm_camera), offsetof(pm_camera, width), offsetof(pm_camera, lens_radius),'
                   'offsetof(pm_camera, filter), offsetof(pm_camera, reserved)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(Filter), ctypes.sizeof(Camera), Camera.width.offset, Camera.lens_radius.offset,
                   Camera.filter.offset, Camera.reserved.offset]
    assert ctypes.sizeof(Filter) == 20 and ctypes.sizeof(Camera) == 116


# ---------------------------------------------------------------- parser
HEAD = 'LookAt 0 0 -5 0 0 0 0 1 0\n'
TAIL = 'Film "image" "integer xresolution" [8] "integer yresolution" [6]\nWorldBegin\nWorldEnd\n'


def dump_text(tmp_path, options, camera='Camera "perspective" "float fov" [40]\n'):
    p = tmp_path / "s.pbrt"
    p.write_text(HEAD + camera + options + TAIL)
    r = subprocess.run([CLI, "--pbrt", str(p), "--dump"], capture_output=True, text=True)
    return r, (json.loads(r.stdout) if r.returncode == 0 else None)


def test_parser_defaults_stay_pinhole(tmp_path):
    r, d = dump_text(tmp_path, "")
    c = d["camera"]
    assert d["warnings"] == 0 and c["device_camera"] == 0
    assert (c["xsamples"], c["ysamples"], c["lens_radius"], c["filter"]["type"]) == (1, 1, 0, "none")


@pytest.mark.parametrize("scene", ["cornell-box", "cornell-box-quad", "cornell-two-lights"])
def test_shipped_cornell_scenes_stay_pinhole(scene):
    r = subprocess.run([CLI, "--pbrt", os.path.join(SCENES, scene + ".pbrt"), "--dump"], capture_output=True, text=True, check=True)
    d = json.loads(r.stdout)
    assert d["warnings"] == 0 and d["camera"]["device_camera"] == 0 and r.stderr == ""


def test_parser_stratified_and_filters(tmp_path):
    _, d = dump_text(tmp_path, 'Sampler "stratified"\n')
    c = d["camera"]
    assert (c["device_camera"], c["xsamples"], c["ysamples"], c["jitter"]) == (1, 2, 2, 1)
    assert (c["filter"]["type"], c["filter"]["xwidth"], c["filter"]["ywidth"]) == ("box", 0.5, 0.5)  # no PixelFilter: box 0.5
    _, d = dump_text(tmp_path, 'Sampler "stratified" "integer xsamples" [3] "integer ysamples" [1] "bool jitter" ["false"]\n')
    c = d["camera"]
    assert (c["xsamples"], c["ysamples"], c["jitter"]) == (3, 1, 0)
    want = {"box": (0.5, 0.5, 0, 0), "triangle": (2, 2, 0, 0), "gaussian": (2, 2, 2, 0),
            "mitchell": (2, 2, np.float32(1 / 3), np.float32(1 / 3))}
    for name, (xw, yw, a, b) in want.items():
        _, d = dump_text(tmp_path, f'PixelFilter "{name}"\n')
        f = d["camera"]["filter"]
        assert d["camera"]["device_camera"] == 1 and d["warnings"] == 0
        assert (f["type"], f["xwidth"], f["ywidth"]) == (name, xw, yw)
        assert np.float32(f["a"]) == np.float32(a) and np.float32(f["b"]) == np.float32(b)
    _, d = dump_text(tmp_path, 'PixelFilter "mitchell" "float xwidth" [1.5] "float ywidth" [2.5] "float B" [0.25] "float C" [0.5]\n')
    f = d["camera"]["filter"]
    assert (f["xwidth"], f["ywidth"], f["a"], f["b"]) == (1.5, 2.5, 0.25, 0.5)
    _, d = dump_text(tmp_path, 'PixelFilter "gaussian" "float alpha" [0.75]\n')
    assert d["camera"]["filter"]["a"] == 0.75


@pytest.mark.parametrize("n,xs,ys", [(1, 1, 1), (2, 2, 1), (4, 2, 2), (5, 4, 2), (16, 4, 4), (100, 8, 8)])
@pytest.mark.parametrize("sampler", ["lowdiscrepancy", "bestcandidate", "random"])
def test_parser_pixelsamples(tmp_path, sampler, n, xs, ys):
    r, d = dump_text(tmp_path, f'Sampler "{sampler}" "integer pixelsamples" [{n}]\n')
    c = d["camera"]
    assert (c["xsamples"], c["ysamples"]) == (xs, ys)
    assert d["warnings"] == (1 if n > 1 else 0) and (("stratified" in r.stderr) == (n > 1))
    assert c["device_camera"] == (1 if n > 1 else 0)
    if n > 1:
        assert c["jitter"] == 1


def test_parser_lens_and_sinc(tmp_path):
    r, d = dump_text(tmp_path, "", 'Camera "perspective" "float fov" [40] "float lensradius" [0.5] "float focaldistance" [7]\n')
    c = d["camera"]
    assert (c["device_camera"], c["lens_radius"], c["focal_distance"], d["warnings"]) == (1, 0.5, 7, 0)
    assert "depth of field" not in r.stderr
    r, d = dump_text(tmp_path, "", 'Camera "perspective" "float fov" [40] "float lensradius" [0.5]\n')
    assert r.returncode != 0 and "focaldistance" in r.stderr
    r, d = dump_text(tmp_path, 'PixelFilter "sinc"\n')
    assert d["warnings"] == 1 and "sinc" in r.stderr and d["camera"]["filter"]["type"] == "mitchell"


# ---------------------------------------------------------------- pm_render_cli camera flags (parse only)
def cli_dump(path, *flags):
    r = subprocess.run([CLI, "--pbrt", str(path), "--dump", *flags], capture_output=True, text=True)
    return r, (json.loads(r.stdout)["camera"] if r.returncode == 0 else None)


def test_cli_flags_over_a_pinhole_scene():
    scene = os.path.join(SCENES, "cornell-box.pbrt")
    _, c = cli_dump(scene, "--spp", "2x3")
    assert (c["device_camera"], c["xsamples"], c["ysamples"], c["jitter"]) == (1, 2, 3, 1)
    assert (c["filter"]["type"], c["filter"]["xwidth"]) == ("box", 0.5)
    _, c = cli_dump(scene, "--spp", "2x3", "--no-jitter")
    assert (c["device_camera"], c["jitter"]) == (1, 0)
    _, c = cli_dump(scene, "--spp", "1x1")          # nothing asked for: today's pinhole
    assert (c["device_camera"], c["filter"]["type"]) == (0, "none")
    _, c = cli_dump(scene, "--filter", "gaussian:1.5:1.25:0.75")
    f = c["filter"]
    assert c["device_camera"] == 1 and (f["type"], f["xwidth"], f["ywidth"], f["a"]) == ("gaussian", 1.5, 1.25, 0.75)
    _, c = cli_dump(scene, "--filter", "mitchell:3")
    f = c["filter"]
    assert (f["type"], f["xwidth"], f["ywidth"]) == ("mitchell", 3, 3) and np.float32(f["a"]) == np.float32(1 / 3)
    _, c = cli_dump(scene, "--lens", "2.5:900")
    assert (c["device_camera"], c["lens_radius"], c["focal_distance"], c["filter"]["type"]) == (1, 2.5, 900, "box")


def test_cli_flags_keep_the_scenes_jitter(tmp_path):
    p = tmp_path / "s.pbrt"
    p.write_text(HEAD + 'Camera "perspective" "float fov" [40]\nSampler "stratified" "bool jitter" ["false"]\n' + TAIL)
    _, c = cli_dump(p, "--spp", "3x1")
    assert (c["xsamples"], c["ysamples"], c["jitter"]) == (3, 1, 0)
    _, c = cli_dump(p, "--lens", "1:10")
    assert (c["xsamples"], c["ysamples"], c["jitter"], c["lens_radius"]) == (2, 2, 0, 1)


@pytest.mark.parametrize("flags", [("--filter", "none"), ("--filter", "box:abc"), ("--filter", "box:0.5:x"),
                                   ("--filter", "box:9"), ("--filter", "sinc"), ("--filter", "box:1:1:1:1:1"),
                                   ("--spp", "9x1"), ("--spp", "2"), ("--spp", "2x2x"), ("--lens", "1"), ("--lens", "1:0"),
                                   ("--lens", "a:5"), ("--lens", "-1:5")])
def test_cli_flags_reject_bad_values(flags):
    r, _ = cli_dump(os.path.join(SCENES, "cornell-box.pbrt"), *flags)
    assert r.returncode == 1 and flags[0] in r.stderr


def test_cli_flags_need_a_scene_file():
    r = subprocess.run([CLI, "--spp", "2x2", "--out", "/dev/null"], capture_output=True, text=True)
    assert r.returncode == 2 and "--pbrt" in r.stderr
