"""Power-weighted light selection (PM_ALL_LIGHTS) without a device: the C-ABI
declares and exports it, pmrender mirrors the header, pm_light_selection_cdf
builds the table pm_api.h states (multi_light_ref restates it in float64), the
restated base-11 radical inverse is proved against the oracle on the other
bases, and the .pbrt front end carries "lightsource"."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import multi_light_ref as R
from pmrender import abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pm_api.h")
LIB = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "libpmhip.so")
CLI = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_render_cli")
SCENES = os.path.join(ROOT, "cuda-raytrace_amd", "scenes")
SETS = R.light_sets()


def header_source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_abi_declares_and_exports_the_selection(hip_mod):
    src = header_source()
    assert re.search(r"#define\s+PM_ALL_LIGHTS\s+\(-1\)\s*$", src, flags=re.M)
    assert re.search(r"#define\s+PM_SCENE_LIGHT_CDF\s+9\s*$", src, flags=re.M)
    assert abi.PM_ALL_LIGHTS == -1
    assert hip_mod.Context.SCENE_SECTIONS["light_cdf"] == (9, np.float32)
    decl = re.search(r"int\s+pm_light_selection_cdf\s*\(([^)]*)\)", src)
    assert decl, "pm_light_selection_cdf not declared"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert args == ["const int *types", "const float *le_rgb", "const float *areas", "int n", "float *cdf_out"]
    f = hip_mod.load_library().pm_light_selection_cdf
    assert f.restype is ctypes.c_int and len(f.argtypes) == len(args)
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T pm_light_selection_cdf$", out, flags=re.M)
    # the default stays the reference's single light
    assert abi.RenderParams.defaults().light_source_index == 0


@pytest.mark.parametrize("name", sorted(SETS))
def test_table_equals_the_reference(name, hip_mod):
    types, le, areas = SETS[name]
    got = hip_mod.light_selection_cdf(types, le, areas)
    ref = R.table_ref(types, le, areas)
    assert got.dtype == np.float32 and len(got) == len(types)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (got, ref)
    assert got[-1] == np.float32(1.0) and np.all(np.diff(got) >= 0)
    if name == "one":
        assert got.tolist() == [1.0]
    if name == "zero_second":
        assert got.tolist() == [1.0, 1.0]               # the dark light's bin is empty: never picked
        assert R.pmf_of(got).tolist() == [1.0, 0.0]
    if name == "mixed3":
        w = R.weights(types, le, areas)
        assert 900 < w.max() / w.min() < 1100           # the 1 : 1000 span
        assert np.all(R.pmf_of(got) > 0)


def test_negative_weight_counts_as_zero(hip_mod):
    types = [abi.PM_LIGHT_AREA_DISK, abi.PM_LIGHT_POINT, abi.PM_LIGHT_AREA_MESH]
    le = np.float32([[1, 1, 1], [-5, -5, -5], [1, 1, 1]])
    got = hip_mod.light_selection_cdf(types, le, np.float32([2.0, 0.0, 2.0]))
    assert got.tolist() == [0.5, 0.5, 1.0]
    assert np.array_equal(got, R.table_ref(types, le, np.float32([2.0, 0.0, 2.0])))


def test_table_errors(hip_mod):
    lib = hip_mod.load_library()
    t = (ctypes.c_int * 2)(abi.PM_LIGHT_POINT, abi.PM_LIGHT_AREA_DISK)
    le = (ctypes.c_float * 6)(1, 1, 1, 1, 1, 1)
    ar = (ctypes.c_float * 2)(0, 1)
    out = (ctypes.c_float * 2)()
    assert lib.pm_light_selection_cdf(t, le, ar, 2, out) == abi.PM_OK
    for n in (0, -3):
        assert lib.pm_light_selection_cdf(t, le, ar, n, out) == abi.PM_ERR_INVALID
    for args in ((None, le, ar, 2, out), (t, None, ar, 2, out), (t, le, None, 2, out), (t, le, ar, 2, None)):
        assert lib.pm_light_selection_cdf(*args) == abi.PM_ERR_INVALID
    zero = (ctypes.c_float * 6)()
    assert lib.pm_light_selection_cdf(t, zero, ar, 2, out) == abi.PM_ERR_INVALID          # total weight 0
    assert b"weight" in lib.pm_last_error(None)
    for bad in (float("inf"), float("nan")):                                             # total not finite
        le_bad = (ctypes.c_float * 6)(bad, bad, bad, 1, 1, 1)
        assert lib.pm_light_selection_cdf(t, le_bad, ar, 2, out) == abi.PM_ERR_INVALID
    ar_bad = (ctypes.c_float * 2)(0, float("inf"))
    assert lib.pm_light_selection_cdf(t, le, ar_bad, 2, out) == abi.PM_ERR_INVALID
    unknown = (ctypes.c_int * 2)(abi.PM_LIGHT_POINT, 2)
    assert lib.pm_light_selection_cdf(unknown, le, ar, 2, out) == abi.PM_ERR_INVALID
    with pytest.raises(ValueError):
        hip_mod.light_selection_cdf([abi.PM_LIGHT_POINT], np.zeros(3, np.float32), [0.0])


def test_restated_radical_inverse_is_the_oracles(oracle_mod):
    assert R.prove_restatement(0) >= 200
    assert R.prove_restatement(3) >= 200                 # another pass's permutation
    idx = R.edge_indices()
    assert all(e in idx for e in (0, 1, 12582911, 12582912, 12582914, (1 << 24) - 1, 1 << 24, (1 << 24) + 1))
    # base 11 itself: in [0, 1), index 0 gives 0, a one-digit index gives perm[digit] / 11
    perm = oracle_mod.halton_permutation(0)
    table = perm[17:28]
    assert sorted(table.tolist()) == list(range(11))
    u = R.radical_inverse_f32(np.arange(0, 11, dtype=np.uint32), 11, table)
    inv = np.float32(1.0) / np.float32(11.0)
    assert u[0] == 0 and np.array_equal(u[1:], (table[1:].astype(np.float32) * inv).astype(np.float32))
    u = R.u5(np.arange(4096))
    assert np.all((u >= 0) & (u < 1))
    # equidistributed enough to reach every light of the mixed scene (what the GPU replay relies on)
    assert len(np.unique(np.floor(u * 11))) == 11


def test_pick_convention():
    cdf = np.float32([0.25, 0.25, 0.75, 1.0, 1.0])
    u = np.float32([0.0, 0.2499, 0.25, 0.5, 0.75, 0.9999, 1.0])
    assert R.pick(cdf, u).tolist() == [0, 0, 2, 2, 3, 3, 3]   # empty bins (1, 4) are never picked, u = 1 held below 1


def dump(path):
    return subprocess.run([CLI, "--pbrt", str(path), "--dump"], capture_output=True, text=True, timeout=60)


def test_two_light_scene_file():
    r = dump(os.path.join(SCENES, "cornell-two-lights.pbrt"))
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["warnings"] == 0 and d["light_source_index"] == -1
    assert [L["kind"] for L in d["lights"]] == ["disk", "mesh"]
    sc = scenes.cornell_two_lights(256, 256)
    ref = R.table_ref(*R.scene_light_arrays(sc))
    assert np.array_equal(np.float32(d["light_cdf"]).view(np.uint32), ref.view(np.uint32))
    assert 0 < ref[0] < 1                                  # both lights can be picked
    L = d["lights"][1]
    np.testing.assert_array_equal(np.float32(L["P"]).reshape(-1, 3), np.float32(scenes.WALL_LIGHT))
    np.testing.assert_array_equal(np.float32(L["Le"]), np.float32(scenes.WALL_LIGHT_LE))
    # the quad faces into the box: cross(p1 - p0, p2 - p0) along +x
    P, idx = np.float32(L["P"]).reshape(-1, 3), np.int32(L["indices"]).reshape(-1, 3)
    n = np.cross(P[idx[:, 1]] - P[idx[:, 0]], P[idx[:, 2]] - P[idx[:, 0]])
    assert np.all(n[:, 0] > 0) and np.all(n[:, 1:] == 0)
    shapes = [c for c in d["calls"] if c["call"] == "shape"]
    assert [s["light"] for s in shapes if s["light"] >= 0] == [0, 1]


def test_default_scene_keeps_light_zero():
    r = dump(os.path.join(SCENES, "cornell-box.pbrt"))
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["light_source_index"] == 0 and d["light_cdf"] == [1.0]


TEXT = """
Camera "perspective" "float fov" [40]
Renderer "cuda" %s
WorldBegin
LightSource "point" "rgb I" [1 1 1] "point from" [0 1 0]
LightSource "point" "rgb I" [3 3 3] "point from" [0 2 0]
WorldEnd
"""


@pytest.mark.parametrize("param,index", [('"integer lightsource" [1]', 1), ('"integer lightsource" [-1]', -1),
                                         ('"string lightsource" "all"', -1), ("", 0)])
def test_parser_lightsource(tmp_path, param, index):
    f = tmp_path / "t.pbrt"
    f.write_text(TEXT % param)
    r = dump(f)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["light_source_index"] == index and d["light_cdf"] == [0.25, 1.0]


@pytest.mark.parametrize("param", ['"integer lightsource" [2]', '"integer lightsource" [-2]',
                                   '"string lightsource" "some"', '"integer lightsource" [7]'])
def test_parser_lightsource_out_of_range(tmp_path, param):
    f = tmp_path / "t.pbrt"
    f.write_text(TEXT % param)
    r = dump(f)
    assert r.returncode == 1 and "lightsource" in r.stderr, (r.returncode, r.stderr)
    assert r.stdout == ""


def test_null_context_is_an_error(hip_mod):
    """no device here: PM_ALL_LIGHTS on a null context fails cleanly"""
    lib = hip_mod.load_library()
    p = abi.RenderParams.defaults(light_source_index=abi.PM_ALL_LIGHTS)
    assert lib.pm_trace_photons(None, ctypes.byref(p), 0, 0, 64, 0, None) == abi.PM_ERR_INVALID
    n = ctypes.c_int64(-1)
    assert lib.pm_scene_section(None, 9, None, 0, ctypes.byref(n)) == abi.PM_ERR_INVALID
