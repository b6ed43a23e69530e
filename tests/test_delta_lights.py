"""The distant light without a device: the C ABI declares and exports
pm_add_light_distant and checks its parameters before it looks at the context,
pmrender/abi.py mirrors the header, the selection table knows the type (and
did not move for the old ones), the .pbrt front end parses LightSource
"distant", the Python scenes carry it (the oracle refuses), and the
stand-alone native check of the host-only scene unit (world sphere, the
light's record) builds and passes."""
import ctypes
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import delta_light_ref as R
import multi_light_ref as ML
from mesh_light_ref import ulp_distance
from pmrender import abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pm_api.h")
CSRC = os.path.join(ROOT, "cuda-raytrace_amd", "csrc")
CLI = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_render_cli")
SCENES = os.path.join(ROOT, "cuda-raytrace_amd", "scenes")


def header_source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_abi_declares_and_exports_the_distant_light(hip_mod):
    src = header_source()
    want = {"pm_add_light_distant": ["void *ctx", "const float to_light[3]", "const float L[3]", "int *out_light"]}
    lib = hip_mod.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "cuda-raytrace_amd", "lib", "libpmhip.so")],
                         capture_output=True, text=True, check=True).stdout
    for name, args in want.items():
        decl = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, src)
        assert decl, f"{name} not declared"
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == args
        f = getattr(lib, name)
        assert f.restype is ctypes.c_int and len(f.argtypes) == len(args)
        assert re.search(r" T %s$" % name, out, flags=re.M)


def test_abi_constants_match_the_header():
    d = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(PM_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+|\d+)u?\s*$",
                                                              header_source(), flags=re.M)}
    assert d["PM_LIGHT_DISTANT"] == abi.PM_LIGHT_DISTANT == 6
    assert d["PM_SCENE_WORLD_SPHERE"] == abi.PM_SCENE_WORLD_SPHERE == 10
    from pmrender import hip
    assert callable(hip.Context.world_sphere) and "world_sphere" not in hip.Context.SCENE_SECTIONS   # a host value
    # the older ones did not move
    assert (d["PM_LIGHT_POINT"], d["PM_LIGHT_AREA_DISK"], d["PM_LIGHT_AREA_MESH"]) == (1, 3, 4)


def f3(*v):
    return (ctypes.c_float * 3)(*v)


def test_null_context_and_invalid_parameters(hip_mod):
    """no device here: good parameters fail on the null context; bad ones are
    refused before the context is looked at, with a message that says why"""
    lib = hip_mod.load_library()
    out = ctypes.c_int(-1)
    o = ctypes.byref(out)
    err = lambda: lib.pm_last_error(None).decode()
    assert lib.pm_add_light_distant(None, f3(0, 1, 0), f3(1, 1, 1), o) == abi.PM_ERR_INVALID
    assert "null context" in err()
    nan = float("nan")
    for args, why in (((f3(0, 0, 0), f3(1, 1, 1), o), "zero direction"),
                      ((f3(0, nan, 0), f3(1, 1, 1), o), "not finite"),
                      ((f3(0, 1, 0), f3(1, float("inf"), 1), o), "not finite"),
                      ((f3(0, 1, 0), None, o), "null pointer")):
        assert lib.pm_add_light_distant(None, *args) == abi.PM_ERR_INVALID
        assert why in err() and "null context" not in err(), err()
    assert out.value == -1


def test_selection_table_with_the_distant_light(hip_mod):
    P, D, M, T = abi.PM_LIGHT_POINT, abi.PM_LIGHT_AREA_DISK, abi.PM_LIGHT_AREA_MESH, abi.PM_LIGHT_DISTANT
    rng = np.random.RandomState(5)
    sets = [([P, D, T], [[1, 1, 1], [3, 2, 1], [0.5, 0.4, 0.3]], [0.0, 57.0, 812.5]),
            ([T], [[1, 2, 3]], [1e6]),
            ([T, D], [[2, 2, 2], [0, 0, 0]], [1e6, 3.0]),
            ([(P, D, M, T)[i % 4] for i in range(17)], rng.uniform(0, 20, (17, 3)), rng.uniform(0.1, 500, 17))]
    for types, le, areas in sets:
        le, areas = np.asarray(le, np.float32), np.asarray(areas, np.float32)
        got = hip_mod.light_selection_cdf(types, le, areas)
        ref = R.power_table(types, le, areas)
        assert got[-1] == np.float32(1.0) and np.all(np.diff(got) >= 0)
        assert ulp_distance(got, ref).max() <= 1, (got, ref)
    # DistantLight::Power = L pi R^2 against PointLight::Power = 4 pi I
    y = R.luminance([40, 50, 60])
    got = hip_mod.light_selection_cdf([T, P], np.float32([[40, 50, 60], [40, 50, 60]]), np.float32([math.pi * 9.0, 0]))
    assert abs(float(got[0]) - 9.0 * math.pi / (9.0 * math.pi + 4.0 * math.pi)) < 2e-7 and y > 0
    # the spot light's number is kept, not taken
    for t in (5, 7):
        with pytest.raises(ValueError):
            hip_mod.light_selection_cdf([t], np.ones(3, np.float32), [1.0])


def test_selection_table_of_the_old_types_did_not_move(hip_mod):
    for name, (types, le, areas) in ML.light_sets().items():
        got = hip_mod.light_selection_cdf(types, le, areas)
        assert np.array_equal(got.view(np.uint32), ML.table_ref(types, le, areas).view(np.uint32)), name


# ------------------------------------------------------------------ parser
def dump(path):
    r = subprocess.run([CLI, "--pbrt", str(path), "--dump"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout), r.stderr


WORLD = """
Camera "perspective" "float fov" [40]
WorldBegin
AttributeBegin
  %s
AttributeEnd
Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0  1 0 0  0 1 0]
WorldEnd
"""
# a non-trivial CTM: x -> 2 y + 1, y -> -x + 2, z -> 3 z + 3 (a rotation about z, a scale, a translation)
CTM = "Translate 1 2 3 Rotate 90 0 0 1 Scale 1 2 3"


def ctm(p, w=1.0):
    x, y, z = p
    return np.array([-2.0 * y + 1.0 * w, 1.0 * x + 2.0 * w, 3.0 * z + 3.0 * w])


def parse_text(tmp_path, text):
    f = tmp_path / "t.pbrt"
    f.write_text(text)
    return dump(f)


def test_parser_distant(tmp_path):
    d, _ = parse_text(tmp_path, WORLD % (CTM + ' LightSource "distant"'))
    (L,) = d["lights"]
    assert L["kind"] == "distant" and d["warnings"] == 0
    np.testing.assert_allclose(L["to_light"], ctm((0, 0, -1), 0.0), atol=1e-5)    # from - to = (0, 0, -1)
    np.testing.assert_array_equal(np.float32(L["L"]), np.float32([1, 1, 1]))
    d, _ = parse_text(tmp_path, WORLD % (CTM + ' LightSource "distant" "rgb L" [1 2 3] "rgb scale" [3 3 3] "point from" [5 1 2] '
                                         '"point to" [1 1 4]'))
    (L,) = d["lights"]
    np.testing.assert_allclose(L["to_light"], ctm((4, 0, -2), 0.0), atol=1e-5)
    np.testing.assert_array_equal(np.float32(L["L"]), np.float32([3, 6, 9]))
    assert d["light_cdf"] == []            # its weight needs the commit's world sphere


def test_parser_unknown_light_still_warns(tmp_path):
    d, err = parse_text(tmp_path, WORLD % 'LightSource "goniometric" "rgb I" [1 1 1]')
    assert d["lights"] == [] and d["warnings"] == 1 and "UnImplemented Cuda Light Source: goniometric" in err


def test_scene_file_has_the_disk_and_one_distant_light():
    d, err = dump(os.path.join(SCENES, "cornell-sun.pbrt"))
    assert d["warnings"] == 0 and "UnImplemented" not in err
    assert [L["kind"] for L in d["lights"]] == ["disk", "distant"]
    sun = d["lights"][1]
    assert sun["to_light"][2] < 0 and sun["to_light"][1] > 0                            # in through the open front, from above
    assert d["light_source_index"] == -1 and d["light_cdf"] == []
    sc = scenes.cornell_sun(8, 8)                                                       # the Python scene: the same lights
    assert len([c for c in d["calls"] if c["call"] == "shape"]) == len(sc.meshes) + len(sc.disks)
    assert sc.lights[0][0] == "disk"
    _, w, L = sc.lights[1]
    np.testing.assert_array_equal(np.float32(sun["to_light"]), w)
    np.testing.assert_array_equal(np.float32(sun["L"]), L)


# ------------------------------------------------------------------ scenes
class FakeApi:
    """records the scene calls of Scene.load_into (no device)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a):
            self.calls.append((name, a))
            return sum(1 for n, _ in self.calls if n.startswith("add_light")) - 1 if name.startswith("add_light") else 0
        return call


def test_scene_uploads_the_distant_light_and_the_oracle_refuses(oracle_mod):
    sc = R.floor_scene(("point", (1, 2, 3)))
    sc.add_distant_light((1.0, 2.0, 3.0), (0.0, 0.0, 0.0), (4, 5, 6))
    api = FakeApi()
    sc.load_into(api)
    (sun,) = [a for n, a in api.calls if n == "add_light_distant"]
    np.testing.assert_array_equal(sun[0], np.float32([1, 2, 3]))
    np.testing.assert_array_equal(sun[1], np.float32([4, 5, 6]))
    assert [n for n, _ in api.calls if n.startswith("add_light")] == ["add_light_point", "add_light_distant"]
    with pytest.raises(NotImplementedError, match="distant"):
        sc.load_into(oracle_mod.Oracle(nthreads=1))


# ------------------------------------------------------------------ native
def test_native_delta_light_check(tmp_path):
    exe = tmp_path / "dcheck"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "delta_light_check.cpp"), os.path.join(CSRC, "pm_scene.cpp"),
                    os.path.join(CSRC, "pm_build.cpp"), "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "bad 0" in r.stdout, r.stdout + r.stderr
