"""Triangle-mesh area lights without a device: the C-ABI declares and exports
pm_add_light_mesh, pmrender/abi.py still mirrors include/pm_api.h, the .pbrt
front end turns AreaLightSource "diffuse" on a trianglemesh into one AreaMesh
light, and the Python scenes carry mesh lights (refused by the oracle API,
which has none)."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from pmrender import abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pm_api.h")
CLI = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_render_cli")
SCENES = os.path.join(ROOT, "cuda-raytrace_amd", "scenes")


def header_defines():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(PM_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+|\d+)u?\s*$",
                                                                 src, flags=re.M)}


def test_abi_declares_and_exports_the_mesh_light(hip_mod):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"int\s+pm_add_light_mesh\s*\(([^)]*)\)", src)
    assert decl, "pm_add_light_mesh not declared"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert args == ["void *ctx", "const float *P", "int nverts", "const int *indices", "int ntris",
                    "int reverse_orientation", "const float Le[3]", "int n_samples", "int *out_light"]
    lib = hip_mod.load_library()
    f = lib.pm_add_light_mesh
    assert f.restype is ctypes.c_int and len(f.argtypes) == len(args)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "cuda-raytrace_amd", "lib", "libpmhip.so")],
                         capture_output=True, text=True, check=True).stdout
    assert re.search(r" T pm_add_light_mesh$", out, flags=re.M)


def test_abi_constants_match_the_header():
    d = header_defines()
    assert d["PM_LIGHT_AREA_MESH"] == abi.PM_LIGHT_AREA_MESH == 4
    assert (d["PM_LIGHT_POINT"], d["PM_LIGHT_AREA_DISK"]) == (abi.PM_LIGHT_POINT, abi.PM_LIGHT_AREA_DISK) == (1, 3)
    assert d["PM_SCENE_LIGHT_TRIS"] == 8
    from pmrender import hip
    assert hip.Context.SCENE_SECTIONS["light_tris"] == (8, abi.LIGHT_TRI_DTYPE)
    assert abi.LIGHT_TRI_DTYPE.itemsize == 64 and abi.LIGHT_TRI_DTYPE.fields["cdf"][1] == 12


def test_null_context_is_an_error(hip_mod):
    """no device here: the call fails on the null context instead of crashing"""
    lib = hip_mod.load_library()
    out = ctypes.c_int(-1)
    P = (ctypes.c_float * 9)(0, 0, 0, 1, 0, 0, 0, 1, 0)
    idx = (ctypes.c_int * 3)(0, 1, 2)
    le = (ctypes.c_float * 3)(1, 1, 1)
    assert lib.pm_add_light_mesh(None, P, 3, idx, 1, 0, le, 1, ctypes.byref(out)) == abi.PM_ERR_INVALID


def dump(path):
    r = subprocess.run([CLI, "--pbrt", str(path), "--dump"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout), r.stderr


def test_quad_scene_file_is_cornell_quad():
    d, err = dump(os.path.join(SCENES, "cornell-box-quad.pbrt"))
    assert d["warnings"] == 0 and "UnImplemented" not in err
    assert len(d["lights"]) == 1
    L = d["lights"][0]
    sc = scenes.cornell_quad(256, 256)
    kind, P, idx, Le, ns, rev = sc.lights[0]
    assert L["kind"] == kind == "mesh" and L["nsamples"] == ns == 1 and L["reverse_orientation"] == 0 and not rev
    np.testing.assert_array_equal(np.float32(L["Le"]), Le)
    np.testing.assert_array_equal(np.float32(L["P"]).reshape(-1, 3), P)
    np.testing.assert_array_equal(np.int32(L["indices"]).reshape(-1, 3), idx)
    # it faces down: cross(p1 - p0, p2 - p0) along -y for both triangles
    n = np.cross(P[idx[:, 1]] - P[idx[:, 0]], P[idx[:, 2]] - P[idx[:, 0]])
    assert np.all(n[:, 1] < 0) and np.all(n[:, [0, 2]] == 0)
    assert abs(0.5 * np.linalg.norm(n, axis=1).sum() - 130.0 * 105.0) < 1e-3
    # the visible geometry: the same mesh, last, pointing at light 0; as in the Python scene
    shapes = [c for c in d["calls"] if c["call"] == "shape"]
    assert [s["light"] for s in shapes] == [-1] * (len(shapes) - 1) + [0]
    assert len(shapes) == len(sc.meshes)
    for s, m in zip(shapes, sc.meshes):
        np.testing.assert_array_equal(np.float32(s["P"]).reshape(-1, 3), m["P"])
        np.testing.assert_array_equal(np.int32(s["indices"]).reshape(-1, 3), m["idx"])
        assert s["light"] == m["light"]
    np.testing.assert_array_equal(np.float32(shapes[-1]["k"]), np.float32([0, 0, 0]))


WORLD = """
Camera "perspective" "float fov" [40]
WorldBegin
AttributeBegin
  %s
  AreaLightSource "diffuse" "rgb L" [2 3 4] "rgb scale" [2 2 2] "integer nsamples" [4]
  Shape "%s" %s
AttributeEnd
WorldEnd
"""
TRI = '"integer indices" [0 1 2] "point P" [0 0 0  1 0 0  0 1 0]'


def parse_text(tmp_path, text):
    f = tmp_path / "t.pbrt"
    f.write_text(text)
    return dump(f)


def test_parser_mesh_light_parameters(tmp_path):
    d, _ = parse_text(tmp_path, WORLD % ("Translate 1 2 3", "trianglemesh", TRI))
    (L,) = d["lights"]
    assert L["kind"] == "mesh" and L["nsamples"] == 4 and L["reverse_orientation"] == 0 and d["warnings"] == 0
    np.testing.assert_array_equal(np.float32(L["Le"]), np.float32([4, 6, 8]))
    np.testing.assert_array_equal(np.float32(L["P"]), np.float32([1, 2, 3, 2, 2, 3, 1, 3, 3]))   # world space
    assert [c["light"] for c in d["calls"]] == [0]


def test_parser_reverse_orientation_flips_the_light(tmp_path):
    d, _ = parse_text(tmp_path, WORLD % ("ReverseOrientation", "trianglemesh", TRI))
    assert d["lights"][0]["reverse_orientation"] == 1
    d, _ = parse_text(tmp_path, WORLD % ("ReverseOrientation ReverseOrientation", "trianglemesh", TRI))
    assert d["lights"][0]["reverse_orientation"] == 0


def test_parser_sphere_emitter_still_warns(tmp_path):
    d, err = parse_text(tmp_path, WORLD % ("", "sphere", '"float radius" [2]'))
    assert d["lights"] == [] and d["warnings"] == 1
    assert "UnImplemented Cuda Area Light Source: sphere" in err
    assert [c["light"] for c in d["calls"]] == [-1]


def test_parser_emitter_inside_object_still_warns(tmp_path):
    text = WORLD % ('ObjectBegin "o"', "trianglemesh", TRI + '\nObjectEnd')
    d, err = parse_text(tmp_path, text)
    assert d["lights"] == [] and "inside ObjectBegin" in err


class FakeApi:
    """records the scene calls of Scene.load_into (no device)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a):
            self.calls.append((name, a))
            return sum(1 for n, _ in self.calls if n.startswith("add_light")) - 1 if name.startswith("add_light") else 0
        return call


def test_scene_uploads_mesh_lights_and_the_oracle_refuses(oracle_mod):
    sc = scenes.cornell_quad(32, 24, nsamples=3)
    api = FakeApi()
    sc.load_into(api)
    (call,) = [a for n, a in api.calls if n == "add_light_mesh"]
    assert call[3] == 3 and call[4] is False and np.array_equal(call[0], np.float32(scenes.QUAD_LIGHT))
    tri = [a for n, a in api.calls if n == "add_trimesh"]
    assert tri[-1][5] == 0 and all(t[5] == -1 for t in tri[:-1])        # the quad is the light's geometry
    assert not [n for n, _ in api.calls if n in ("add_disk", "add_light_disk")]
    assert scenes.rays_from_pinhole(sc)[3] == 3                          # its 2-D light samples are counted
    # several mesh lights: each gets its own index, in the order of Scene.lights
    sc.add_mesh_light(np.float32(scenes.QUAD_LIGHT) - np.float32([0, 100, 0]), [(0, 1, 2)], (1, 1, 1), 2)
    api = FakeApi()
    sc.load_into(api)
    assert len([n for n, _ in api.calls if n == "add_light_mesh"]) == 2
    assert [a[5] for n, a in api.calls if n == "add_trimesh"][-2:] == [0, 1]
    assert scenes.rays_from_pinhole(sc)[3] == 5
    with pytest.raises(NotImplementedError, match="mesh"):
        sc.load_into(oracle_mod.Oracle(nthreads=1))
