"""Textures on the CPU: the C ABI's argument checks (they run before the
context is touched, so no device is needed), the host texture assembly through
tests/native/texture_check.cpp (plain and under the address and
undefined-behaviour sanitizers), texture_ref's own properties, and the Python
Scene's round trip of uvs and textures."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import texture_ref as T
from pmrender import hip, scenes
from pmrender.abi import PM_ERR_INVALID, PM_GLASS, PM_MATTE, PM_MIRROR, TEX_CHECKER, TEX_SCALE, TEX_SINGLE, f32, fptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-raytrace_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    return hip.load_library()


def _err(lib):
    return lib.pm_last_error(None).decode()


# ---- the ABI's argument checks, case by case (ctx = NULL: never reached) ----------
IMG = np.arange(18, dtype=np.float32).reshape(2, 3, 3) / 18
MAP, ONE = (1.0, 1.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def _image(lib, img=IMG, w=3, h=2, wrap=0, mapping=MAP, scale=ONE, out=True):
    o = ctypes.c_int(-7)
    return lib.pm_add_texture_image(None, fptr(f32(img)), w, h, wrap, fptr(f32(mapping)), fptr(f32(scale)),
                                    ctypes.byref(o) if out else None)


@pytest.mark.parametrize("kw", [dict(img=None), dict(mapping=None), dict(scale=None), dict(out=False), dict(w=0), dict(h=0),
                                dict(w=-3), dict(w=2 ** 31 - 1, h=2 ** 31 - 1), dict(w=65536, h=32768), dict(wrap=3),
                                dict(wrap=-1), dict(mapping=(1.0, float("nan"), 0.0, 0.0)), dict(scale=(1.0, float("inf"), 1.0)),
                                dict(img=np.where(np.arange(18).reshape(2, 3, 3) == 11, np.nan, IMG))],
                         ids=lambda kw: ",".join(kw))
def test_image_argument_checks(lib, kw):
    assert _image(lib, **kw) == PM_ERR_INVALID
    assert "pm_add_texture_image" in _err(lib)


def test_valid_image_reaches_the_context_check(lib):
    """valid arguments pass the checks and fail only on the null context"""
    assert _image(lib) == PM_ERR_INVALID and "null context" in _err(lib)


def _operands(lib, scale, mapping=MAP, t1=-1, c1=ONE, t2=-1, c2=ONE, out=True):
    o = ctypes.c_int(-7)
    op = ctypes.byref(o) if out else None
    if scale:
        return lib.pm_add_texture_scale(None, t1, fptr(f32(c1)), t2, fptr(f32(c2)), op)
    return lib.pm_add_texture_checker(None, fptr(f32(mapping)), t1, fptr(f32(c1)), t2, fptr(f32(c2)), op)


@pytest.mark.parametrize("scale", [False, True], ids=["checker", "scale"])
@pytest.mark.parametrize("kw", [dict(c1=None), dict(c2=None), dict(out=False), dict(c1=(0.0, float("nan"), 0.0)),
                                dict(c2=(float("-inf"), 0.0, 0.0))], ids=lambda kw: ",".join(kw))
def test_operand_argument_checks(lib, scale, kw):
    assert _operands(lib, scale, **kw) == PM_ERR_INVALID
    assert ("pm_add_texture_scale" if scale else "pm_add_texture_checker") in _err(lib)


def test_checker_mapping_checks(lib):
    assert _operands(lib, False, mapping=None) == PM_ERR_INVALID and "null pointer" in _err(lib)
    assert _operands(lib, False, mapping=(1.0, 1.0, float("inf"), 0.0)) == PM_ERR_INVALID and "not finite" in _err(lib)
    # an operand given by id needs no colour; with valid arguments only the context is missing
    assert _operands(lib, True, t1=0, c1=None, t2=1, c2=None) == PM_ERR_INVALID and "null context" in _err(lib)
    assert _operands(lib, False) == PM_ERR_INVALID and "null context" in _err(lib)


def test_textured_material_checks(lib):
    o = ctypes.c_int()
    for mtype in (PM_MIRROR, PM_GLASS, 17):
        assert lib.pm_add_material_textured(None, mtype, 0, ctypes.byref(o)) == PM_ERR_INVALID and "PM_MATTE" in _err(lib)
    assert lib.pm_add_material_textured(None, PM_MATTE, 0, None) == PM_ERR_INVALID and "null pointer" in _err(lib)
    assert lib.pm_add_material_textured(None, PM_MATTE, 0, ctypes.byref(o)) == PM_ERR_INVALID and "null context" in _err(lib)


# ---- the host assembly (native, sanitized) ----------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def native(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("texture_check")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    exe = str(d / "tcheck")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", *flags, "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "cuda-raytrace_amd", "adapter"),
                    os.path.join(ROOT, "cuda-raytrace_amd", "adapter", "pm_image.cpp"),
                    os.path.join(ROOT, "tests", "native", "texture_check.cpp"), os.path.join(CSRC, "pm_scene.cpp"),
                    os.path.join(CSRC, "pm_build.cpp"), "-lpthread", "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def _records(lines):
    recs = []
    for ln in lines:
        if not ln.startswith("tex "):
            continue
        head, *ops = ln.split(" op ")
        h = head.split()
        rec = dict(kind=int(h[3]), map=[float.fromhex(x) for x in h[5:9]], op=[])
        for o in ops:
            f = o.split()
            rec["op"].append(dict(rgb=[float.fromhex(x) for x in f[0:3]], texel0=int(f[3]), w=int(f[4]), h=int(f[5]),
                                  wrap=int(f[6]), map=[float.fromhex(x) for x in f[7:11]]))
        recs.append(rec)
    return recs


def test_host_texture_assembly(native):
    assert native[-1] == "bad 0", "\n".join(native)
    recs = _records(native)
    assert [r["kind"] for r in recs] == [TEX_SINGLE, TEX_SINGLE, TEX_CHECKER, TEX_SCALE, TEX_SCALE]
    f = lambda *v: [float(np.float32(x)) for x in v]
    img1 = dict(rgb=f(0.5, 2.0, 1.0), texel0=0, w=3, h=2, wrap=T.CLAMP, map=f(2.5, -1.5, 0.25, 0.75))
    img2 = dict(rgb=f(1, 1, 1), texel0=6, w=2, h=2, wrap=T.REPEAT, map=f(1, 1, 0, 0))
    const = lambda *c: dict(rgb=f(*c), texel0=-1, w=0, h=0, wrap=0, map=f(0, 0, 0, 0))
    assert recs[0]["op"][0] == img1 and recs[0]["op"][1]["texel0"] == -1
    assert recs[1]["op"][0] == img2
    # the checkerboard: its own mapping, operand 1 a copy of image 1's record, operand 2 a colour
    assert recs[2]["map"] == f(2.5, -1.5, 0.25, 0.75) and recs[2]["op"] == [img1, const(0.1, 0.2, 0.6)]
    assert recs[3]["op"] == [img1, img2]
    assert recs[4]["op"] == [const(0.8, 0.7, 0.2), const(0.1, 0.2, 0.6)]


# ---- texture_ref's own properties ---------------------------------------------------
def test_reference_bilinear_properties():
    rng = np.random.RandomState(3)
    u, v = rng.uniform(-2, 3, 500), rng.uniform(-2, 3, 500)
    c = np.float32([0.3, 0.6, 0.2])
    flat = np.broadcast_to(c, (5, 3, 3))
    for wrap in ("repeat", "clamp"):
        assert np.array_equal(T.image(flat, u, v, wrap, (2.7, -1.3, 0.21, 0.4)), np.broadcast_to(np.float64(c), (500, 3)))
    img = rng.uniform(0, 1, (4, 4, 3)).astype(np.float32)
    # texel centres return the texel: (i + 0.5) / w
    iy, ix = np.divmod(np.arange(16), 4)
    assert np.allclose(T.image(img, (ix + 0.5) / 4, (iy + 0.5) / 4), img.reshape(-1, 3), atol=1e-15)
    # repeat is periodic, black is 0 well outside, clamp continues the border
    assert np.allclose(T.image(img, u + 1, v - 2, "repeat"), T.image(img, u, v, "repeat"), atol=1e-12)
    assert np.all(T.image(img, np.float64([1.5, -0.5]), np.float64([0.5, 0.5]), "black") == 0)
    assert np.allclose(T.image(img, np.float64([7.0]), np.float64([0.125]), "clamp"), img[0, 3])
    # the checkerboard, C's % on negative sums included
    first = T.checker_first(np.float64([0.1, 1.1, -0.1, -0.1, 1.5]), np.float64([0.1, 0.1, 0.1, -0.1, 1.5]), MAP)
    assert first.tolist() == [True, False, False, True, True]
    sc = T.evaluate(("scale", ("const", (0.5, 2.0, 1.0)), ("image", img, "repeat", MAP, ONE)), u, v)
    assert np.allclose(sc, T.image(img, u, v) * [0.5, 2.0, 1.0])


def test_reference_checker_edges_stay_under_the_cap():
    """the GPU tests leave out records within 1e-3 of a checker edge and cap them at 5 %: on a 32 x 32
    grid of a wall's (u, v) the 4-square checkerboard's share of such points is far below that"""
    g = (np.arange(32) + 0.5) / 32
    u, v = [a.ravel() for a in np.meshgrid(g, g)]
    assert (T.checker_edge_distance(u, v, (4.0, 4.0, 0.0, 0.0)) < 1e-3).mean() <= 0.05


def test_reference_triangle_uv():
    P = np.float64([(0, 0, 0), (2, 0, 0), (2, 0, 3), (0, 0, 3)])
    idx = [(0, 1, 2), (0, 2, 3)]
    uv = [(0, 0), (1, 0), (1, 1), (0, 1)]
    p = np.float64([(0.5, 0, 0.75), (1.5, 0, 2.25), (0.2, 0, 2.9)])
    u, v, hit = T.mesh_uv(p, P, idx, uv)
    assert hit.all() and np.allclose(u, p[:, 0] / 2) and np.allclose(v, p[:, 2] / 3)
    u, v, hit = T.mesh_uv(np.float64([(1.5, 0, 0.75)]), P, idx, None)  # default corners on triangle (0, 1, 2)
    assert hit.all() and np.allclose([u[0], v[0]], [0.5, 0.25])
    assert not T.mesh_uv(np.float64([(3, 0, 1)]), P, idx, uv)[2].any()


# ---- the Python Scene -----------------------------------------------------------------
class Recorder:
    """the Scene.load_into protocol, recording the calls"""

    def __init__(self):
        self.calls, self.ids = [], {}

    def __getattr__(self, name):
        if not name.startswith(("add_", "set_", "commit")):
            raise AttributeError(name)
        kind = "texture" if name.startswith("add_texture") else "material" if name.startswith("add_material") else name

        def call(*a, **kw):
            self.calls.append((name, a))
            self.ids[kind] = self.ids.get(kind, -1) + 1  # ids count up per kind, as the C ABI's do
            return self.ids[kind]
        return call


def test_scene_round_trip_of_uvs_and_textures():
    s = scenes.Scene()
    img = s.texture_image(scenes.procedural_image(4, 2), wrap="black", mapping=(2, 2, 0, 0), scale=(1, 0.5, 1))
    chk = s.texture_checker(img, (0.1, 0.1, 0.1), mapping=(8, 8, 0, 0))
    scl = s.texture_scale(img, (0.5, 0.5, 0.5))
    m_img, m_plain, m_chk = s.material(PM_MATTE, img), s.material(PM_MATTE, (0.2, 0.3, 0.4)), s.material(PM_MATTE, chk)
    m_scl = s.material(PM_MATTE, scl)
    s.add_quads([scenes.FLOOR], m_chk, uvs=[scenes.QUAD_UV])
    s.add_quads([scenes.BACK], m_plain)
    with pytest.raises(ValueError):
        s.add_quads([scenes.FLOOR], m_chk, uvs=[scenes.QUAD_UV[:3]])
    obj = dict(P=np.float32([(0, 0, 0), (1, 0, 0), (0, 1, 0)]), idx=np.int32([(0, 1, 2)]), N=None,
               uv=np.float32([(0.25, 0.5), (1, 0), (0, 1)]), material=m_scl, light=-1)
    s.objects.append(obj)
    s.instances.append((0,) + scenes.translate(5, 6, 7))
    scenes._ceiling_light(s)
    s.camera = scenes.pinhole(8, 8)
    flat = s.flattened(0)
    assert np.array_equal(flat["uv"], obj["uv"]) and flat["material"] == m_scl
    assert np.array_equal(flat["P"], obj["P"] + np.float32([5, 6, 7]))
    for instancing in (True, False):
        r = Recorder()
        s.load_into(r, instancing=instancing)
        names = [c for c, _ in r.calls]
        assert names[:3] == ["add_texture_image", "add_texture_checker", "add_texture_scale"]
        _, (arr, wrap, mapping, scale) = r.calls[0]
        assert arr.shape == (2, 4, 3) and wrap == "black" and mapping.tolist() == [2, 2, 0, 0] and scale.tolist() == [1, 0.5, 1]
        assert r.calls[1][1][0] == 0 and np.allclose(r.calls[1][1][1], 0.1) and r.calls[1][1][2].tolist() == [8, 8, 0, 0]
        assert r.calls[2][1][0] == 0 and np.allclose(r.calls[2][1][1], 0.5)
        mats = [(c, a) for c, a in r.calls if c.startswith("add_material")]
        assert [c for c, _ in mats[:4]] == ["add_material_textured", "add_material", "add_material_textured", "add_material_textured"]
        assert [a[1] for c, a in mats if c == "add_material_textured"] == [0, 1, 2]
        meshes = [a for c, a in r.calls if c in ("add_trimesh", "add_object_mesh")]
        assert np.array_equal(meshes[0][3], np.float32(scenes.QUAD_UV)) and meshes[0][4] == m_chk
        assert meshes[1][3] is None
        assert np.array_equal(meshes[2][3], obj["uv"]) and meshes[2][4] == m_scl
        assert ("add_mesh_instance" in names) == instancing


def test_untextured_api_refuses_a_textured_scene():
    class Plain:
        def add_material(self, *a):
            return 0

    s = scenes.cornell_textured(8, 8)
    with pytest.raises(NotImplementedError, match="no textures"):
        s.load_into(Plain())


def test_cornell_textured_scene():
    s = scenes.cornell_textured(16, 16)
    kinds = [t[0] for t in s.textures]
    assert kinds == ["checker", "image"]
    img = s.textures[1][1]
    assert img.shape == (8, 8, 3) and img.dtype == np.float32 and 0.09 < img.min() and img.max() < 0.91
    textured = [m for m in s.meshes if isinstance(s.materials[m["material"]][1], scenes.Tex)]
    assert len(textured) == 2 and all(m["uv"] is not None for m in textured)
    assert s.num_triangles == scenes.cornell_box(16, 16).num_triangles


# ---- the .pbrt front end and the image readers -----------------------------------------
import json
import struct

CLI = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_render_cli")
HEAD = 'Camera "perspective"\nWorldBegin\nLightSource "point"\n'
QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [0 0 0 1 0 0 1 1 0 0 1 0] "float uv" [0 0 1 0 1 1 0 1]\n'


def dump(tmp_path, body, ok=True):
    f = tmp_path / "scene.pbrt"
    f.write_text(HEAD + body + QUAD + "WorldEnd\n")
    r = subprocess.run([CLI, "--pbrt", str(f), "--dump"], capture_output=True, text=True, timeout=60)
    if not ok:
        assert r.returncode != 0, r.stdout[-500:]
        return None, r.stderr
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    return d, r.stderr


def write_pfm(path, img, colour=True, little=True):
    """img (h, w, 3) with row 0 the bottom row, as a PFM stores it"""
    h, w = img.shape[:2]
    data = (img if colour else img[:, :, :1]).astype("<f4" if little else ">f4").tobytes()
    path.write_bytes(b"%s\n%d %d\n%s\n" % (b"PF" if colour else b"Pf", w, h, b"-1.0" if little else b"1.0") + data)


def write_tga(path, img8, bpp=24, top=False):
    """img8 (h, w, 3) uint8 with row 0 the bottom row; top: stored top row first (origin bit set)"""
    h, w = img8.shape[:2]
    rows = img8[::-1] if top else img8
    if bpp == 8:
        px, typ = rows[:, :, :1], 3
    else:
        px, typ = rows[:, :, ::-1], 2
        if bpp == 32:
            px = np.concatenate([px, np.full((h, w, 1), 200, np.uint8)], 2)
    hdr = struct.pack("<BBBHHBHHHHBB", 0, 0, typ, 0, 0, 0, 0, 0, w, h, bpp, (0x20 if top else 0) | (8 if bpp == 32 else 0))
    path.write_bytes(hdr + np.ascontiguousarray(px).tobytes())


IMG8 = (np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3) * 13 + 7)
IMGF = (np.arange(2 * 3 * 3, dtype=np.float32).reshape(2, 3, 3) * 0.25 - 1.0)


def kd_tex(d):
    shape = [c for c in d["calls"] if c["call"] == "shape"][-1]
    return shape.get("kd_tex"), shape


def test_pbrt_checkerboard_scale_and_constant(tmp_path):
    d, err = dump(tmp_path, 'Texture "c" "color" "constant" "color value" [0.1 0.2 0.3]\n'
                            'Texture "chk" "spectrum" "checkerboard" "float uscale" [8] "float vscale" [4] "float udelta" [0.5] '
                            '"float vdelta" [0.25] "string aamode" "none" "texture tex1" "c" "rgb tex2" [0.9 0.8 0.7]\n'
                            'Material "matte" "texture Kd" "chk"\n')
    t, shape = kd_tex(d)
    assert d["warnings"] == 0 and "Warning" not in err
    assert t["kind"] == 1 and t["map"] == [8, 4, 0.5, 0.25]
    assert [o["image"] for o in t["ops"]] == [0, 0]
    assert np.allclose(t["ops"][0]["rgb"], [0.1, 0.2, 0.3]) and np.allclose(t["ops"][1]["rgb"], [0.9, 0.8, 0.7])
    assert shape["material"] == 0 and np.allclose(shape["k"], [0.1, 0.2, 0.3])  # the stand-in at a default point: tex1
    # defaults: tex1 1, tex2 0, unit mapping; aamode closedform (pbrt's default) warns and uses none
    d, err = dump(tmp_path, 'Texture "chk" "color" "checkerboard"\nMaterial "matte" "texture Kd" "chk"\n')
    t, _ = kd_tex(d)
    assert d["warnings"] == 1 and "aamode" in err
    assert t["kind"] == 1 and t["map"] == [1, 1, 0, 0] and t["ops"][0]["rgb"] == [1, 1, 1] and t["ops"][1]["rgb"] == [0, 0, 0]
    d, err = dump(tmp_path, 'Texture "s" "color" "scale" "rgb tex1" [0.5 0.5 1] "rgb tex2" [0.2 0.4 0.6]\nMaterial "matte" "texture Kd" "s"\n')
    t, shape = kd_tex(d)
    assert d["warnings"] == 0 and t["kind"] == 2 and np.allclose(shape["k"], [0.1, 0.2, 0.6])
    # a constant texture keeps working as before: no texture description at all
    d, _ = dump(tmp_path, 'Texture "c" "color" "constant" "color value" [0.1 0.2 0.3]\nMaterial "matte" "texture Kd" "c"\n')
    t, shape = kd_tex(d)
    assert t is None and np.allclose(shape["k"], [0.1, 0.2, 0.3]) and d["warnings"] == 0


@pytest.mark.parametrize("body,word", [
    ('Texture "t" "color" "checkerboard" "integer dimension" [3]\n', "dimension"),
    ('Texture "t" "float" "checkerboard"\n', "color / spectrum"),
    ('Texture "t" "color" "checkerboard" "string aamode" "none" "string mapping" "spherical"\n', "mapping"),
    ('Texture "t" "color" "marble"\n', "not supported"),
    ('Texture "a" "color" "checkerboard" "string aamode" "none"\nTexture "t" "color" "scale" "texture tex1" "a"\n', "operand"),
    ('Texture "t" "color" "scale" "texture tex1" "nowhere"\n', "not defined"),
])
def test_pbrt_warned_forms_fall_back_to_the_default_kd(tmp_path, body, word):
    d, err = dump(tmp_path, body + 'Material "matte" "texture Kd" "t"\n')
    t, shape = kd_tex(d)
    assert word in err and t is None and shape["k"] == [0.5, 0.5, 0.5]
    assert d["warnings"] == 2  # the texture, and the material that finds none


def test_pbrt_textured_mirror_falls_back(tmp_path):
    d, err = dump(tmp_path, 'Texture "chk" "color" "checkerboard" "string aamode" "none"\nMaterial "mirror" "texture Kr" "chk"\n')
    t, shape = kd_tex(d)
    assert t is None and "constant" in err and np.allclose(shape["k"], [0.9, 0.9, 0.9])


@pytest.mark.parametrize("variant", ["pfm-colour-le", "pfm-colour-be", "pfm-grey-le", "pfm-grey-be", "tga24", "tga24-top", "tga32",
                                     "tga32-top", "tga8", "tga8-top"])
def test_pbrt_imagemap_readers(tmp_path, variant):
    """every supported file variant decodes to the same w x h RGB, row 0 the bottom row; paths resolve relative
    to the scene file"""
    (tmp_path / "tex").mkdir()
    if variant.startswith("pfm"):
        name, colour = "tex/img.pfm", "colour" in variant
        write_pfm(tmp_path / name, IMGF, colour, variant.endswith("le"))
        want = IMGF if colour else np.repeat(IMGF[:, :, :1], 3, 2)
    else:
        name, bpp = "tex/img.TGA", int(variant[3:].split("-")[0])
        write_tga(tmp_path / name, IMG8, bpp, variant.endswith("top"))
        want = (IMG8 if bpp != 8 else np.repeat(IMG8[:, :, :1], 3, 2)).astype(np.float32) / np.float32(255)
    d, err = dump(tmp_path, f'Texture "im" "color" "imagemap" "string filename" "{name}" "string wrap" "clamp" "float scale" [2] '
                            '"float uscale" [3] "float vdelta" [0.5]\nMaterial "matte" "texture Kd" "im"\n')
    t, _ = kd_tex(d)
    assert d["warnings"] == 0, err
    o = t["ops"][0]
    assert t["kind"] == 0 and o["image"] == 1 and (o["w"], o["h"], o["wrap"]) == (3, 2, 2)
    assert o["rgb"] == [2, 2, 2] and o["map"] == [3, 1, 0, 0.5]
    assert np.array_equal(np.float32(o["texels"]).reshape(2, 3, 3), want.astype(np.float32))


def test_pbrt_imagemap_as_operand_and_wraps(tmp_path):
    write_pfm(tmp_path / "a.pfm", IMGF)
    d, err = dump(tmp_path, 'Texture "im" "color" "imagemap" "string filename" "a.pfm" "string wrap" "black"\n'
                            'Texture "s" "color" "scale" "texture tex1" "im" "rgb tex2" [0.5 0.5 0.5]\nMaterial "matte" "texture Kd" "s"\n')
    t, _ = kd_tex(d)
    assert d["warnings"] == 0 and t["kind"] == 2 and t["ops"][0]["image"] == 1 and t["ops"][0]["wrap"] == 1 and t["ops"][1]["image"] == 0
    d, err = dump(tmp_path, 'Texture "im" "color" "imagemap" "string filename" "a.pfm" "string wrap" "mirror"\nMaterial "matte" "texture Kd" "im"\n')
    assert d["warnings"] == 1 and "wrap" in err and kd_tex(d)[0]["ops"][0]["wrap"] == 0


def _bad_files(tmp_path):
    good_pfm, good_tga = tmp_path / "g.pfm", tmp_path / "g.tga"
    write_pfm(good_pfm, IMGF)
    write_tga(good_tga, IMG8, 24)
    p, t = good_pfm.read_bytes(), good_tga.read_bytes()
    rle = bytearray(t); rle[2] = 10
    cmap = bytearray(t); cmap[1] = 1
    zero = bytearray(t); zero[12] = zero[13] = 0
    return {"short.pfm": p[:-5], "header.pfm": b"PF\n3", "huge.pfm": b"PF\n70000 70000\n-1.0\n" + p[14:],
            "overflow.pfm": b"PF\n99999999999999999999 2\n-1.0\n", "zero.pfm": b"PF\n0 2\n-1.0\n", "scale.pfm": b"PF\n3 2\n0\n" + p[14:],
            "magic.pfm": b"P6\n3 2\n255\n" + p[14:], "nan.pfm": p[:-4] + struct.pack("<f", float("nan")),
            "short.tga": t[:-1], "header.tga": t[:10], "rle.tga": bytes(rle), "cmap.tga": bytes(cmap), "zero.tga": bytes(zero),
            "idlen.tga": bytes([200]) + t[1:], "picture.png": b"\x89PNG\r\n", "missing.pfm": None}


@pytest.mark.parametrize("name", ["short.pfm", "header.pfm", "huge.pfm", "overflow.pfm", "zero.pfm", "scale.pfm", "magic.pfm", "nan.pfm",
                                  "short.tga", "header.tga", "rle.tga", "cmap.tga", "zero.tga", "idlen.tga", "picture.png", "missing.pfm"])
def test_pbrt_bad_image_files_are_parse_errors_that_name_the_file(tmp_path, name):
    data = _bad_files(tmp_path)[name]
    if data is not None:
        (tmp_path / name).write_bytes(data)
    _, err = dump(tmp_path, f'Texture "im" "color" "imagemap" "string filename" "{name}"\n', ok=False)
    assert name in err and "scene.pbrt:" in err
