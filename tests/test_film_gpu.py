"""The supersampled thin-lens camera and the on-device film (pm_set_camera,
pm_film, pm_camera_rays) on the GPU, against tests/film_ref.py: the film bit
for bit against its fp32 restatement in the pinned order and within the
sequential-sum bound of the float64 one; the camera tied to the pinhole and
host-ray paths the oracle suite already pins (bit for bit), and to its float64
formula. Images are 37 x 21 (no multiple of the film's tile or the records' 8).
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import film_ref as R
from pmrender import scenes
from pmrender.abi import (PM_ESTIMATOR_KNN, PM_ESTIMATOR_PPM, PM_MATTE, Filter, RenderParams)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_render_cli")

W, H = 37, 21
SPP = ((1, 1), (2, 2), (3, 1))
FILTERS = {"box": dict(filter="box", xwidth=0.5, ywidth=0.5), "triangle": dict(filter="triangle", xwidth=2.0, ywidth=2.0),
           "gaussian": dict(filter="gaussian", xwidth=2.0, ywidth=2.0, a=2.0),
           "mitchell": dict(filter="mitchell", xwidth=1.3, ywidth=2.7, a=1.0 / 3.0, b=1.0 / 3.0)}
SEED = 91
FLOOR_SCALE = 8.0  # test 4: the lens rays may deviate 8 x the unjittered pinhole's deviation from float64


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_filter(kw):
    kw = dict(kw)
    return Filter.make(kw.pop("filter"), **kw)


def camera_ctx(hip_mod, scene_fn, w, h, **cam):
    sc = scene_fn(w, h)
    sc.camera = scenes.device_camera(w, h, **cam)
    return sc.load_into(hip_mod.Context(0)), sc


@functools.lru_cache(maxsize=None)
def randoms(w, h, xs, ys, jitter, seed=SEED):
    return R.sample_randoms(w, h, xs, ys, jitter, seed)


@functools.lru_cache(maxsize=None)
def raster(w, h, xs, ys):
    """random non-negative radiance, a few exact zeros and one large value"""
    rng = np.random.RandomState(7 + xs * 10 + ys)
    L = rng.uniform(0.0, 4.0, size=(w * xs * h * ys, 3)).astype(np.float32)
    L[rng.randint(0, len(L), 40)] = 0.0
    L[len(L) // 3] = 1000.0
    return L


def film_on_device(ctx, samples, w, h):
    import torch
    d_s = torch.from_numpy(np.ascontiguousarray(samples, np.float32)).to("cuda:0")
    d_i = torch.full((h * w, 3), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.film(d_s.data_ptr(), d_i.data_ptr())
    ctx.synchronize()
    return d_i.cpu().numpy().reshape(h, w, 3)


def check_film(hip_mod, w, h, xs, ys, jitter, fkw):
    ctx, _ = camera_ctx(hip_mod, scenes.cornell_box, w, h, xsamples=xs, ysamples=ys, jitter=jitter, sample_seed=SEED,
                        filter=fkw["filter"], filter_kw={k: v for k, v in fkw.items() if k != "filter"})
    f = make_filter(fkw)
    table = hip_mod.film_filter_table(f)
    L = raster(w, h, xs, ys)
    fx, fy = R.film_positions32(w, h, xs, ys, randoms(w, h, xs, ys, jitter))
    got = film_on_device(ctx, L, w, h)
    ref32, _ = R.film32(L, fx, fy, w, h, table, f.xwidth, f.ywidth)
    assert np.array_equal(bits(got), bits(ref32)), f"film differs from the fp32 pinned-order reference in " \
        f"{int((bits(got) != bits(ref32)).sum())} values"
    ref64, sa, sw, saw, n = R.film64(L, fx, fy, w, h, table, f.xwidth, f.ywidth)
    ok = np.abs(sw) >= 1e-3 * saw
    ok &= saw > 0
    left_out = int(((~ok) & (saw > 0)).sum())
    assert left_out <= 0.01 * w * h, f"{left_out} ill-conditioned pixels: choose other inputs"
    with np.errstate(invalid="ignore", divide="ignore"):
        bound = (n + 4)[..., None] * 2.0 ** -23 * sa / np.abs(sw)[..., None]
    err = np.abs(got.astype(np.float64) - ref64)
    worst = float(np.max(np.where(ok[..., None], err / np.maximum(bound, 1e-300), 0.0)))
    print(f"film {fkw['filter']} {xs}x{ys} jitter={jitter}: max |err| / bound = {worst:.3f}, footprint <= {int(n.max())}, "
          f"left out {left_out}")
    assert np.all(err[ok] <= bound[ok])
    assert np.all(got[saw == 0] == 0)
    ctx.close()


# ---------------------------------------------------------------- 1. film alone
@pytest.mark.parametrize("jitter", (True, False))
@pytest.mark.parametrize("fname", list(FILTERS))
@pytest.mark.parametrize("spp", SPP)
def test_film_kernel(hip_mod, spp, fname, jitter):
    check_film(hip_mod, W, H, spp[0], spp[1], jitter, FILTERS[fname])


def test_film_largest_footprint(hip_mod):
    """8 x 8 samples, width 4, 16 x 16 pixels: the footprint that goes through LDS in several bands"""
    check_film(hip_mod, 16, 16, 8, 8, True, dict(filter="gaussian", xwidth=4.0, ywidth=4.0, a=0.5))


# ---------------------------------------------------------------- 2. centre sample = today
def test_centre_sample_equals_pinhole(hip_mod):
    p = RenderParams.defaults(paths_per_pass=4096)
    ref_ctx = scenes.cornell_box(W, H).load_into(hip_mod.Context(0))
    ref_img, _ = ref_ctx.render(p)
    ref_rec = ref_ctx.download_records()
    ctx, _ = camera_ctx(hip_mod, scenes.cornell_box, W, H, xsamples=1, ysamples=1, jitter=False, filter="box",
                        filter_kw=dict(xwidth=0.5, ywidth=0.5))
    img, _ = ctx.render(p)
    assert img.shape == (H, W, 3)
    assert np.array_equal(bits(img), bits(ref_img))
    assert ctx.download_records().tobytes() == ref_rec.tobytes()


# ---------------------------------------------------------------- 3. supersampling = larger pinhole
@pytest.mark.parametrize("estimator", (PM_ESTIMATOR_PPM, PM_ESTIMATOR_KNN))
def test_supersampling_equals_larger_pinhole(hip_mod, estimator):
    p = RenderParams.defaults(paths_per_pass=4096, passes=1, estimator=estimator)
    big = scenes.cornell_box(2 * W, 2 * H).load_into(hip_mod.Context(0))
    big_img, _ = big.render(p)
    big_rec = big.download_records()
    ctx, _ = camera_ctx(hip_mod, scenes.cornell_box, W, H, xsamples=2, ysamples=2, jitter=False, filter="none")
    img, _ = ctx.render(p)
    rec = ctx.download_records()
    assert img.shape == (2 * H, 2 * W, 3)
    assert np.array_equal(bits(rec["dl"]), bits(big_rec["dl"]))
    assert rec.tobytes() == big_rec.tobytes()
    assert np.array_equal(bits(img), bits(big_img))
    assert np.array_equal(ctx.record_pixels(), big.record_pixels())
    fkw = FILTERS["mitchell"]
    ctx2, _ = camera_ctx(hip_mod, scenes.cornell_box, W, H, xsamples=2, ysamples=2, jitter=False,
                         filter=fkw["filter"], filter_kw={k: v for k, v in fkw.items() if k != "filter"})
    filmed, _ = ctx2.render(p)
    f = make_filter(fkw)
    fx, fy = R.film_positions32(W, H, 2, 2, randoms(W, H, 2, 2, False))
    ref32, _ = R.film32(big_img.reshape(-1, 3), fx, fy, W, H, hip_mod.film_filter_table(f), f.xwidth, f.ywidth)
    assert filmed.shape == (H, W, 3)
    assert np.array_equal(bits(filmed), bits(ref32))


# ---------------------------------------------------------------- 4. rays
LENS = dict(lens_radius=12.5, focal_distance=1000.0)


def ray_floor(hip_mod, xs, ys, scene_fn=scenes.cornell_box, **view):
    """deviation of the unjittered pinhole rays (the rays of today's k_eye) of a camera from float64"""
    ctx, sc = camera_ctx(hip_mod, scene_fn, W, H, xsamples=xs, ysamples=ys, jitter=False, sample_seed=SEED, **view)
    rays, _ = ctx.camera_rays()
    _, eye, fwd, right, up = sc.camera[:5]
    o, d, _, _ = R.camera_rays64(eye, fwd, right, up, W, H, xs, ys, randoms(W, H, xs, ys, False))
    assert np.array_equal(rays[:, :3], np.broadcast_to(np.float32(eye), (len(rays), 3)))
    return float(np.max(np.abs(rays[:, 3:].astype(np.float64) - d)))


@pytest.mark.parametrize("spp", SPP)
def test_camera_rays(hip_mod, spp):
    xs, ys = spp
    floor = ray_floor(hip_mod, xs, ys)
    ctx, sc = camera_ctx(hip_mod, scenes.cornell_box, W, H, xsamples=xs, ysamples=ys, jitter=True, sample_seed=SEED, **LENS)
    rays, xy = ctx.camera_rays()
    _, eye, fwd, right, up = sc.camera[:5]
    u = randoms(W, H, xs, ys, True)
    o, d, fx, fy = R.camera_rays64(eye, fwd, right, up, W, H, xs, ys, u, **LENS)
    dev_d = float(np.max(np.abs(rays[:, 3:].astype(np.float64) - d)))
    scale = float(np.max(np.abs(np.float64(eye)))) + LENS["lens_radius"]
    dev_o = float(np.max(np.abs(rays[:, :3].astype(np.float64) - o))) / scale
    print(f"rays {xs}x{ys}: pinhole floor {floor:.3e}, lens direction {dev_d:.3e}, origin (relative) {dev_o:.3e}")
    assert floor > 0
    assert dev_d <= FLOOR_SCALE * floor and dev_o <= FLOOR_SCALE * floor
    assert R.ulp_distance(xy[:, 0], np.float32(fx)).max() <= 1 and R.ulp_distance(xy[:, 1], np.float32(fy)).max() <= 1
    # jitter stays inside its stratum (the closed one: the fp32 sum ix + ju may round up to the next)
    WS = W * xs
    iy, ix = np.divmod(np.arange(len(xy)), WS)
    assert np.all(xy[:, 0] * xs >= ix) and np.all(xy[:, 0] * xs <= ix + 1)
    assert np.all(xy[:, 1] * ys >= iy) and np.all(xy[:, 1] * ys <= iy + 1)
    assert np.ptp(xy[:, 0] * xs - ix) > 0.5
    # a sub-range equals the slice
    r2, xy2 = ctx.camera_rays(5, 40)
    assert np.array_equal(bits(r2), bits(rays[5:45])) and np.array_equal(bits(xy2), bits(xy[5:45]))
    other, _ = camera_ctx(hip_mod, scenes.cornell_box, W, H, xsamples=xs, ysamples=ys, jitter=True, sample_seed=SEED + 1, **LENS)
    rays_b, _ = other.camera_rays()
    assert np.mean(np.any(bits(rays_b) != bits(rays), axis=1)) > 0.99


# ---------------------------------------------------------------- 5. the eye pass uses those rays
def point_light_scene(w, h):
    sc = scenes.feature_scene(w, h)
    sc.lights = [L for L in sc.lights if L[0] == "point"]
    for m in sc.meshes:
        m["light"] = -1
    sc.disks = [d[:7] + (-1,) for d in sc.disks]
    return sc


@pytest.mark.parametrize("spp", SPP)
def test_eye_pass_uses_camera_rays(hip_mod, spp):
    xs, ys = spp
    p = RenderParams.defaults()
    ctx, sc = camera_ctx(hip_mod, point_light_scene, W, H, xsamples=xs, ysamples=ys, jitter=True, sample_seed=SEED, **LENS)
    ctx.eye_pass(p)
    ctx.synchronize()
    rec = ctx.download_records()
    pix = ctx.record_pixels()
    ok = pix >= 0
    by_q = np.zeros(W * xs * H * ys, dtype=rec.dtype)
    by_q[pix[ok]] = rec[ok]
    rays, _ = ctx.camera_rays()
    sc2 = point_light_scene(W, H)
    sc2.camera = ("rays", rays, None, 0)
    ctx2 = sc2.load_into(hip_mod.Context(0))
    ctx2.eye_pass(p)
    ctx2.synchronize()
    ref = ctx2.download_records()
    for k in ("pos", "ns", "flags", "material", "dl"):
        assert np.array_equal(by_q[k].view(np.uint32), ref[k].view(np.uint32)), k
    assert (ref["flags"] == 0).sum() > len(ref) // 2


# ---------------------------------------------------------------- 6. depth of field
FOCAL = 500.0


def wall_scene(distance):
    def make(w, h):
        s = scenes.Scene()
        m = s.material(PM_MATTE, (0.7, 0.7, 0.7))
        z, e = np.float32(distance), 4000.0
        s.add_quads([[(-e, -e, z), (e, -e, z), (e, e, z), (-e, e, z)]], m)
        s.lights.append(("point", np.float32([0, 0, 0]), np.float32([1e5, 1e5, 1e5])))
        s.camera = scenes.pinhole(w, h, eye=(0.0, 0.0, 0.0), look=(0.0, 0.0, 1.0), fov_deg=40.0)
        return s
    return make


def hits_by_sample(hip_mod, distance, xs, ys, **lens):
    ctx, sc = camera_ctx(hip_mod, wall_scene(distance), W, H, xsamples=xs, ysamples=ys, jitter=True, sample_seed=SEED,
                         eye=(0.0, 0.0, 0.0), look=(0.0, 0.0, 1.0), fov_deg=40.0, **lens)
    ctx.eye_pass(RenderParams.defaults())
    ctx.synchronize()
    rec, pix = ctx.download_records(), ctx.record_pixels()
    ok = pix >= 0
    assert np.all(rec["flags"][ok] & 0x7 == 0)
    pos = np.zeros((W * xs * H * ys, 3), np.float32)
    pos[pix[ok]] = rec["pos"][ok]
    return pos, sc


@pytest.mark.parametrize("spp", SPP)
def test_depth_of_field(hip_mod, spp):
    xs, ys = spp
    lens = dict(lens_radius=20.0, focal_distance=FOCAL)
    tol = FLOOR_SCALE * ray_floor(hip_mod, xs, ys, wall_scene(FOCAL), eye=(0.0, 0.0, 0.0), look=(0.0, 0.0, 1.0), fov_deg=40.0)
    # a wall at the focal distance: every lens sample lands on the pinhole sample's hit
    sharp, _ = hits_by_sample(hip_mod, FOCAL, xs, ys)
    lensed, _ = hits_by_sample(hip_mod, FOCAL, xs, ys, **lens)
    dist = np.linalg.norm(sharp.astype(np.float64), axis=1)
    dev = np.abs(lensed.astype(np.float64) - sharp).max(axis=1)
    print(f"dof {xs}x{ys}: in focus max |dp| / distance = {float((dev / dist).max()):.3e} (allowed {tol:.3e})")
    assert np.all(dev <= tol * dist)
    # at twice the focal distance the circle of confusion is the lens mirrored: hit - pinhole hit = eye - o'
    sharp2, sc = hits_by_sample(hip_mod, 2 * FOCAL, xs, ys)
    lensed2, _ = hits_by_sample(hip_mod, 2 * FOCAL, xs, ys, **lens)
    _, eye, fwd, right, up = sc.camera[:5]
    o, _, _, _ = R.camera_rays64(eye, fwd, right, up, W, H, xs, ys, randoms(W, H, xs, ys, True), **lens)
    want = np.float64(eye)[None] - o
    dist2 = np.linalg.norm(sharp2.astype(np.float64), axis=1)
    dev2 = np.abs((lensed2.astype(np.float64) - sharp2) - want).max(axis=1)
    print(f"dof {xs}x{ys}: at 2 f max |offset error| / distance = {float((dev2 / dist2).max()):.3e}")
    assert np.all(dev2 <= 2 * tol * dist2)  # two hit points, each within the tolerance
    assert np.abs(want).max() > 10.0


# ---------------------------------------------------------------- 7. multi-device context
def test_multi_device_context_films_the_same(hip_mod):
    p = RenderParams.defaults(paths_per_pass=4096)
    cam = dict(xsamples=2, ysamples=2, jitter=True, sample_seed=SEED, filter="gaussian", lens_radius=5.0, focal_distance=900.0)
    one, _ = camera_ctx(hip_mod, scenes.cornell_box, W, H, **cam)
    img, _ = one.render(p)
    sc = scenes.cornell_box(W, H)
    sc.camera = scenes.device_camera(W, H, **cam)
    two = sc.load_into(hip_mod.Context(devices=[0, 0]))
    img2, _ = two.render(p)
    assert img.shape == img2.shape == (H, W, 3)
    assert np.array_equal(bits(img), bits(img2))
    assert img.max() > 0


# ---------------------------------------------------------------- pm_set_camera's PM_ERR_INVALID cases
def test_set_camera_validation(hip_mod):
    ctx = hip_mod.Context(0)
    good = dict(eye=(0, 0, 0), fwd=(0, 0, 1), right=(1, 0, 0), up=(0, 1, 0), W=8, H=8)
    ctx.set_camera(**good, xsamples=8, ysamples=8, filter="mitchell", xwidth=4.0, ywidth=4.0)
    bad = [dict(xsamples=0), dict(ysamples=9), dict(lens_radius=-1.0), dict(lens_radius=1.0, focal_distance=0.0),
           dict(filter=7), dict(filter="box", xwidth=0.0), dict(filter="gaussian", xwidth=2.0, ywidth=4.5),
           dict(eye=(float("nan"), 0, 0)), dict(up=(0, float("inf"), 0)), dict(eye=(2.0 ** 20, 0, 0), lens_radius=1.0, focal_distance=5.0),
           dict(W=40000, H=40000, xsamples=2, ysamples=1), dict(W=0)]
    for kw in bad:
        with pytest.raises(hip_mod.PMError) as e:
            ctx.set_camera(**{**good, **kw})
        assert e.value.code == 1, kw
    assert ctx.lib.pm_set_camera(ctx.h, None) == 1
    with pytest.raises(hip_mod.PMError):  # no film without a filter
        ctx.set_camera(**good)
        ctx.film(1, 1)


# ---------------------------------------------------------------- 8. CLI
SCENES = os.path.join(ROOT, "cuda-raytrace_amd", "scenes")


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = (int(v) for v in f.readline().split())
        scale = float(f.readline())
        data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4").reshape(h, w, 3)
    return data[::-1].astype(np.float32)


def test_cli_writes_the_python_image(hip_mod, tmp_path):
    """the shipped Cornell scene (bit for bit scenes.cornell_box, tests/test_pbrt.py) with a stratified
    sampler, a gaussian filter and a lens, through pm_render_cli --pbrt and through Python"""
    text = open(os.path.join(SCENES, "cornell-box.pbrt")).read()
    text = text.replace('Camera "perspective" "float fov" [39.3]',
                        'Camera "perspective" "float fov" [39.3] "float lensradius" [6] "float focaldistance" [1000]')
    text = text.replace('Sampler "lowdiscrepancy" "integer pixelsamples" [1]',
                        'Sampler "stratified" "integer xsamples" [3] "integer ysamples" [2] "bool jitter" ["true"]\n'
                        'PixelFilter "gaussian" "float xwidth" [1.5] "float ywidth" [1.25] "float alpha" [1.5]')
    text = text.replace('"integer xresolution" [256] "integer yresolution" [256]',
                        f'"integer xresolution" [{W}] "integer yresolution" [{H}]')
    text = text.replace('Include "', f'Include "{SCENES}/')
    assert "stratified" in text and "lensradius" in text and f"[{W}]" in text
    scene = tmp_path / "dof.pbrt"
    scene.write_text(text)
    out = tmp_path / "dof.pfm"
    r = subprocess.run([CLI, "--pbrt", str(scene), "--paths", "4096", "--out", str(out)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    ctx, _ = camera_ctx(hip_mod, scenes.cornell_box, W, H, xsamples=3, ysamples=2, jitter=True, sample_seed=0,
                        lens_radius=6.0, focal_distance=1000.0, filter="gaussian",
                        filter_kw=dict(xwidth=1.5, ywidth=1.25, a=1.5))
    img, _ = ctx.render(RenderParams.defaults(paths_per_pass=4096))
    got = read_pfm(out)
    assert got.shape == img.shape == (H, W, 3)
    assert np.array_equal(bits(got), bits(img))


def test_cli_flags_write_the_python_image(hip_mod, tmp_path):
    """--spp / --filter / --lens / --no-jitter over the shipped one-sample Cornell scene"""
    out = tmp_path / "flags.pfm"
    r = subprocess.run([CLI, "--pbrt", os.path.join(SCENES, "cornell-box.pbrt"), "--paths", "4096", "--out", str(out),
                        "--spp", "2x2", "--filter", "mitchell:1.5:2", "--lens", "4:900", "--no-jitter"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    ctx, _ = camera_ctx(hip_mod, scenes.cornell_box, 256, 256, xsamples=2, ysamples=2, jitter=False, sample_seed=0,
                        lens_radius=4.0, focal_distance=900.0, filter="mitchell", filter_kw=dict(xwidth=1.5, ywidth=2.0))
    img, _ = ctx.render(RenderParams.defaults(paths_per_pass=4096))
    got = read_pfm(out)
    assert got.shape == img.shape == (256, 256, 3)
    assert np.array_equal(bits(got), bits(img))
    assert all(q.max() > 0 for q in (got[:128, :128], got[:128, 128:], got[128:, :128], got[128:, 128:]))  # every quadrant is written


# ---------------------------------------------------------------- the simple renderer through the camera
@pytest.mark.parametrize("scene_fn", (scenes.cornell_box, scenes.feature_scene), ids=("brute", "lds"))
def test_render_simple_through_the_camera(hip_mod, scene_fn):
    """k_simple's camera instantiation = the pinhole's at 2W x 2H, and pm_render_simple's film = film32"""
    p = RenderParams.simple_defaults()
    big = scene_fn(2 * W, 2 * H).load_into(hip_mod.Context(0))
    big_img, _ = big.render_simple(p)
    ctx, _ = camera_ctx(hip_mod, scene_fn, W, H, xsamples=2, ysamples=2, jitter=False, filter="none")
    assert ctx.scene_info()["mode"] == big.scene_info()["mode"]
    img, _ = ctx.render_simple(p)
    assert img.shape == (2 * H, 2 * W, 3) and img.max() > 0
    assert np.array_equal(bits(img), bits(big_img))
    fkw = FILTERS["mitchell"]
    ctx2, _ = camera_ctx(hip_mod, scene_fn, W, H, xsamples=2, ysamples=2, jitter=False,
                         filter=fkw["filter"], filter_kw={k: v for k, v in fkw.items() if k != "filter"})
    filmed, _ = ctx2.render_simple(p)
    f = make_filter(fkw)
    fx, fy = R.film_positions32(W, H, 2, 2, randoms(W, H, 2, 2, False))
    ref32, _ = R.film32(big_img.reshape(-1, 3), fx, fy, W, H, hip_mod.film_filter_table(f), f.xwidth, f.ywidth)
    assert filmed.shape == (H, W, 3)
    assert np.array_equal(bits(filmed), bits(ref32))
    # jittered lens samples: the simple renderer of the same rays fed back as host rays
    ctx3, _ = camera_ctx(hip_mod, point_light_scene, W, H, xsamples=2, ysamples=2, jitter=True, sample_seed=SEED,
                         filter="none", **LENS)
    a, _ = ctx3.render_simple(p)
    rays, _ = ctx3.camera_rays()
    sc = point_light_scene(W, H)
    sc.camera = ("rays", rays, None, 0)
    b, _ = sc.load_into(hip_mod.Context(0)).render_simple(p)
    assert np.array_equal(bits(a).reshape(-1, 3), bits(b).reshape(-1, 3))


# ---------------------------------------------------------------- the pbrt plugin's ParamSet keys
HOST = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_pbrt_host")


def test_plugin_paramset_device_camera(hip_mod, tmp_path):
    """Renderer "cuda" "integer devicecamera" [1] ...: the pbrt-typed boundary hands its camera to the
    device, and the pbrt Film gets one filmed value per pixel. The plugin recovers the camera's basis from
    three rays of the pbrt Camera (fp32, normalised), so the basis differs from scenes.pinhole's by a few
    ulp and every ray by ~1e-7 of its length: radiance is compared within 1e-4 (relative and absolute),
    and a sample that such a shift carries over a geometric edge may differ freely: at most 0.5 % of the
    values (3,108 samples, none within 1e-7 of an edge in expectation)."""
    out = tmp_path / "host.bin"
    r = subprocess.run([HOST, "--width", str(W), "--height", str(H), "--paths", "4096", "--out", str(out), "--devicecamera",
                        "--xsamples", "2", "--ysamples", "2", "--no-jitter", "--pixelfilter", "gaussian", "--filterwidth", "1.5",
                        "--lensradius", "3", "--focaldistance", "900"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{W * H} samples added" in r.stdout
    got = np.fromfile(out, np.float32)[-W * H * 3:].reshape(H, W, 3)
    ctx, _ = camera_ctx(hip_mod, scenes.cornell_box, W, H, xsamples=2, ysamples=2, jitter=False, lens_radius=3.0,
                        focal_distance=900.0, filter="gaussian", filter_kw=dict(xwidth=1.5, ywidth=1.5, a=2.0))
    ref, _ = ctx.render(RenderParams.defaults(paths_per_pass=4096))
    close = np.isclose(got, ref, rtol=1e-4, atol=1e-4)
    print(f"plugin device camera: {int((~close).sum())} of {close.size} values differ by more than 1e-4, max |d| "
          f"{float(np.abs(got - ref).max()):.3e}")
    assert ref.max() > 0 and close.mean() >= 0.995
