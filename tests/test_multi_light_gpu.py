"""Power-weighted light selection on the device (light_source_index =
PM_ALL_LIGHTS; pm_trace.hip emit_path<ALL>, pick_light): every path of an
all-lights trace is replayed against the trace of the light it picked, which
the existing tests pin to the oracle (point, disk) or to mesh_light_ref (mesh).
The pick itself is computed on the host from the device's own table
(PM_SCENE_LIGHT_CDF, held bit for bit to pm_light_selection_cdf) and the
base-11 radical inverse restated in multi_light_ref (proved there against the
oracle on bases 3, 5, 7).

Rounding count R behind the alpha tolerance (multi_light_ref.alpha_bound):
path_shade applies 3 float roundings to alpha per Lambert bounce (alpha * fr,
* |cos|, * 1/pdf; a specular continuation applies none) and the all-lights
emission 1 more (the division by pmf). Slot k of a path has seen at most k + 1
bounces (a path whose first hit is matte deposits only from its second hit
on, photontracing.cu's nI counter; one whose first hit is the mirror deposits
its emission weight unchanged into slot 0), so its alpha lies within
(1 + u)^(6 (k + 1) + 1) - 1 of alpha_k / pmf, u = 2^-24 / (1 - 2^-24).
"""
import os
import subprocess

import numpy as np
import pytest

import multi_light_ref as R
from mesh_light_ref import ulp_distance
from parity_util import assert_bitexact, u32
from pmrender import scenes
from pmrender.abi import (PM_ALL_LIGHTS, PM_ERR_INVALID, PM_ESTIMATOR_KNN, PM_ESTIMATOR_PPM, PM_GATHER_GRID,
                          PM_GATHER_KDTREE, PM_LIGHT_POINT, PM_MATTE, PM_REC_INACTIVE, RenderParams)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_render_cli")
HOST = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_pbrt_host")
SCENES = os.path.join(ROOT, "cuda-raytrace_amd", "scenes")

PATHS, W, H, MPC = 4096, 64, 48, 4
SETS = R.light_sets()


def params(light, **kw):
    return RenderParams.defaults(paths_per_pass=PATHS, light_source_index=light, **kw)


def trace(ctx, light, begin=0, count=PATHS):
    ctx.trace_photons(params(light), 0, begin, count, slot_path_base=begin)
    return ctx.download_slots(count * MPC)


# ------------------------------------------------------------------ 1. table
def set_scene(name):
    """a floor under the lights of a light set: a mesh light is a square of the set's area"""
    types, le, areas = SETS[name]
    s = scenes.Scene()
    grey = s.material(PM_MATTE, (0.5, 0.5, 0.5))
    s.add_quads([[(-300, 0, -300), (-300, 0, 300), (300, 0, 300), (300, 0, -300)]], grey)
    for i, (t, c, a) in enumerate(zip(types, le, areas)):
        x = np.float32(-200.0 + 12.0 * i)
        if t == PM_LIGHT_POINT:
            s.lights.append(("point", np.float32([x, 80, 0]), np.float32(c)))
        elif t == 3:
            r = np.float32(np.sqrt(a / np.pi))
            s.lights.append(("disk", np.float32([x, 100, 0]), np.float32([r, 0, 0]), np.float32([0, 0, r]),
                             np.float32([0, -1, 0]), np.float32(c), np.float32(a), 1))
        else:
            h = np.float32(np.sqrt(a) / 2)
            P = np.float32([[x - h, 100, -h], [x - h, 100, h], [x + h, 100, h], [x + h, 100, -h]])
            s.lights.append(("mesh", P, np.int32([[0, 1, 2], [0, 2, 3]]), np.float32(c), 1, False))
    s.camera = ("pinhole", np.float32([0, 40, 0]), np.float32([0, -1, 0]), np.float32([2.4, 0, 0]),
                np.float32([0, 0, 1.8]), 16, 8)
    return s


@pytest.mark.parametrize("name", sorted(SETS))
def test_device_table(name, hip_mod):
    sc = set_scene(name)
    arrays = R.scene_light_arrays(sc)
    ctx = sc.load_into(hip_mod.Context(0))
    try:
        cdf = ctx.scene_section("light_cdf")
    finally:
        ctx.close()
    host = hip_mod.light_selection_cdf(*arrays)
    assert cdf.dtype == np.float32 and len(cdf) == len(sc.lights)
    assert np.array_equal(cdf.view(np.uint32), host.view(np.uint32)), (cdf, host)
    assert np.array_equal(host.view(np.uint32), R.table_ref(*arrays).view(np.uint32))
    if name == "zero_second":
        assert cdf.tolist() == [1.0, 1.0]


# ------------------------------------------------------------------ 2. degenerate cases
@pytest.mark.parametrize("scene_fn", [R.one_light_scene, R.zero_second_scene])
def test_degenerate_selection_is_the_fixed_light(scene_fn, hip_mod):
    """pmf == 1: PM_ALL_LIGHTS is light_source_index = 0 bit for bit (slots, records, image)"""
    ctx = scene_fn(W, H).load_into(hip_mod.Context(0))
    try:
        assert R.pmf_of(ctx.scene_section("light_cdf"))[0] == np.float32(1.0)
        assert_bitexact(trace(ctx, PM_ALL_LIGHTS), trace(ctx, 0), "slots")
        for kw in (dict(estimator=PM_ESTIMATOR_PPM, gather_structure=PM_GATHER_GRID),
                   dict(estimator=PM_ESTIMATOR_PPM, gather_structure=PM_GATHER_KDTREE),
                   dict(estimator=PM_ESTIMATOR_KNN, gather_structure=PM_GATHER_GRID)):
            out = {}
            for light in (0, PM_ALL_LIGHTS):
                img, st = ctx.render(params(light, **kw))
                out[light] = (img, st["photons_valid"], ctx.download_records())
            assert out[0][1] == out[PM_ALL_LIGHTS][1] > 0
            assert np.array_equal(out[0][0].view(np.uint32), out[PM_ALL_LIGHTS][0].view(np.uint32)), kw
            assert_bitexact(out[PM_ALL_LIGHTS][2], out[0][2], f"records {kw}")
    finally:
        ctx.close()


# ------------------------------------------------------------------ 3 / 4. replay
def replay(ctx, begin, count):
    """all-lights slots of paths [begin, begin + count) against the slots of
    the same path traced from the light it picked; returns (pick, composed
    slots: the picked light's, alpha divided by pmf in float)"""
    cdf = ctx.scene_section("light_cdf")
    pmf = R.pmf_of(cdf)
    n_lights = len(cdf)
    pick = R.pick(cdf, R.u5(begin + np.arange(count, dtype=np.int64), MPC))
    per = np.stack([trace(ctx, k, begin, count).reshape(count, MPC) for k in range(n_lights)])
    ref = per[pick, np.arange(count)]
    got = trace(ctx, PM_ALL_LIGHTS, begin, count).reshape(count, MPC)
    for f in ("bits", "p", "wi"):
        bad = np.nonzero((u32(got[f].reshape(count, -1)) != u32(ref[f].reshape(count, -1))).any(axis=1))[0]
        assert bad.size == 0, f"{f}: {bad.size} paths differ from their light's trace, first path {begin + bad[0]} " \
                              f"(picked light {pick[bad[0]]})"
    p = pmf[pick]
    assert np.all(p > 0)
    comp = ref.copy()
    comp["alpha"] = (ref["alpha"] / p[:, None, None]).astype(np.float32)      # fl(alpha_k / pmf)
    want = ref["alpha"].astype(np.float64) / p.astype(np.float64)[:, None, None]
    valid = (ref["bits"] & 1) == 1
    worst = 0.0
    for k in range(MPC):
        g, w, v = got["alpha"][:, k].astype(np.float64), want[:, k], valid[:, k]
        assert np.all(g[~v] == 0)
        assert np.all(g[v][w[v] == 0] == 0)
        nz = v[:, None] & (w > 0)
        rel = np.abs(g[nz] - w[nz]) / w[nz]
        bound = float(R.alpha_bound(k + 1))
        if rel.size:
            worst = max(worst, float(rel.max()) / bound)
            assert rel.max() <= bound, f"slot {k}: alpha off by {rel.max():.3g} relative (bound {bound:.3g})"
    # slot 0 of a path that reached its first matte surface over the mirror
    # carries the emission weight itself: fl(alpha_k / pmf) exactly (the device
    # divides per component)
    exact = valid[:, 0] & (ulp_distance(got["alpha"][:, 0], comp["alpha"][:, 0]).max(axis=1) == 0)
    print(f"replay [{begin}, +{count}): picks {np.bincount(pick, minlength=n_lights).tolist()}, worst alpha "
          f"deviation {worst:.3g} of its bound, {int(exact.sum())} of {int(valid[:, 0].sum())} first deposits exact")
    return pick, comp.reshape(-1), exact


@pytest.fixture(scope="module")
def mixed_ctx(hip_mod):
    ctx = R.mixed_scene(W, H).load_into(hip_mod.Context(0))
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def mixed_replay(mixed_ctx):
    return replay(mixed_ctx, 0, PATHS)


def test_replay_against_each_lights_trace(mixed_ctx, mixed_replay):
    cdf = mixed_ctx.scene_section("light_cdf")
    arrays = R.scene_light_arrays(R.mixed_scene(W, H))
    assert np.array_equal(cdf.view(np.uint32), R.table_ref(*arrays).view(np.uint32))
    # the reference pick reaches every light (all three have weight): asserted on the reference first
    want = R.pick(R.table_ref(*arrays), R.u5(np.arange(PATHS), MPC))
    assert np.all(R.weights(*arrays) > 0) and np.all(np.bincount(want, minlength=3) > 0)
    pick, _, exact = mixed_replay
    assert np.array_equal(pick, want)
    assert np.all(np.bincount(pick, minlength=3) > 100)
    assert exact.sum() > 0, "no first deposit carried fl(alpha_k / pmf) exactly (paths over the mirror do)"


@pytest.mark.parametrize("begin", [3145728 - 32, 4194304 - 32])
def test_replay_at_large_indices(begin, mixed_ctx):
    """pm_index = 4 pid crosses 12,582,912 (the floor shortcut's limit) and 2^24"""
    idx = (begin + np.arange(64)) * MPC
    assert idx[0] < (12582912 if begin < 4000000 else 1 << 24) <= idx[-1]
    replay(mixed_ctx, begin, 64)


# ------------------------------------------------------------------ 5. modes
MODES = {0: "brute", 48: "bvh-lds", 300: "bvh-hbm", "inst": "bvh-instanced"}


def test_traversal_and_write_modes(hip_mod, mixed_replay, monkeypatch):
    """The mixed scene padded behind its back wall into each traversal mode,
    deposits held per path and written one by one: the same slots bit for bit."""
    base = None
    for hold in ("1", "0"):
        monkeypatch.setenv("PM_TRACE_HOLD", hold)
        for pad, mode in MODES.items():
            ctx = R.mixed_scene(W, H, pad=pad).load_into(hip_mod.Context(0))
            try:
                assert ctx.scene_info()["mode"] == mode
                slots = trace(ctx, PM_ALL_LIGHTS)
            finally:
                ctx.close()
            if base is None:
                base = slots
                assert (slots["bits"] & 1).sum() > PATHS
            assert_bitexact(slots, base, f"slots, {mode} hold={hold} vs brute held")


# ------------------------------------------------------------------ 6. sharding
@pytest.mark.parametrize("pad", [0, 300])
def test_sharded_trace_equals_one_call(pad, hip_mod):
    ctx = R.mixed_scene(W, H, pad=pad).load_into(hip_mod.Context(0))
    try:
        p = params(PM_ALL_LIGHTS)
        whole = trace(ctx, PM_ALL_LIGHTS)
        ctx.upload_slots(np.zeros(PATHS * MPC, whole.dtype))
        cut = 1000 + 37                                      # not a multiple of 64
        ctx.trace_photons(p, 0, 0, cut, slot_path_base=0)
        ctx.trace_photons(p, 0, cut, PATHS - cut, slot_path_base=0)
        assert_bitexact(ctx.download_slots(PATHS * MPC), whole, "two calls into one slot buffer")
    finally:
        ctx.close()


# ------------------------------------------------------------------ 7. end to end
def test_render_equals_composed_photons(mixed_ctx, mixed_replay):
    """pm_render(PM_ALL_LIGHTS) against build + gather over the slot buffer
    composed on the host from the per-light traces (alpha / pmf in float)."""
    ctx = mixed_ctx
    _, comp, _ = mixed_replay
    p = params(PM_ALL_LIGHTS, initial_radius2=2500.0)      # 4,096 paths in a 555-unit box: a radius that finds photons
    img, st = ctx.render(p)
    got = ctx.download_records()
    assert st["photons_valid"] == int((comp["bits"] & 1).sum()) > 0
    ctx.eye_pass(p)
    ctx.upload_slots(comp)
    ctx.build_photon_map(p, len(comp))
    ctx.gather(p)
    ref = ctx.download_records()
    act = (ref["flags"] & PM_REC_INACTIVE) == 0
    assert np.array_equal(got["flags"], ref["flags"]) and act.sum() > W * H // 2
    assert np.array_equal(got["photon_count"], ref["photon_count"]), "N' differs"
    assert np.array_equal(u32(got["radius2"]), u32(ref["radius2"])), "r^2 differs"
    assert (ref["photon_count"][act] > 0).sum() > act.sum() // 2
    # flux: a sum of non-negative terms linear in alpha. The composed alpha is
    # fl(alpha_k / pmf): one rounding more than the bound of the replay, taken
    # at the last slot (the most bounces). Each term is rounded to the gather's
    # fixed point (one unit per photon found, M = N' / ppm_alpha in the first
    # pass), and the update's float product adds a few ulps.
    u = R.U24 / (1 - R.U24)
    rel = (1.0 + float(R.alpha_bound(MPC))) * (1.0 + u) ** 5 - 1.0
    unit = R.ppm_fixed_unit(R.mixed_scene(W, H), ctx.scene_section("light_cdf"), MPC)
    found = ref["photon_count"].astype(np.float64) / 0.7 + 1.0
    g, r = got["flux"].astype(np.float64), ref["flux"].astype(np.float64)
    assert np.all(r[act] >= 0)
    tol = rel * np.maximum(g, r) + (found * unit)[:, None]
    dev = np.abs(g - r)
    print(f"flux: largest deviation {(dev[act] / np.maximum(tol[act], 1e-300)).max():.3g} of its tolerance "
          f"(relative part {rel:.3g}, unit {unit:.3g})")
    assert np.all(dev[act] <= tol[act])
    assert np.isfinite(img).all() and (img > 0).any()


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = (int(v) for v in f.readline().split())
        scale = float(f.readline())
        a = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4").reshape(h, w, 3)
    return np.ascontiguousarray(a[::-1]).astype(np.float32)


def test_two_light_scene_file_end_to_end(tmp_path, hip_mod):
    """cornell-two-lights.pbrt through the scene-file front end equals
    cornell_two_lights() through the Python driver; --light overrides the file."""
    paths = 16384
    ctx = scenes.cornell_two_lights(256, 256).load_into(hip_mod.Context(0))
    try:
        ref = {k: ctx.render(RenderParams.defaults(paths_per_pass=paths, light_source_index=k))[0]
               for k in (PM_ALL_LIGHTS, 0)}
    finally:
        ctx.close()
    assert not np.array_equal(ref[0], ref[PM_ALL_LIGHTS])            # the second light's photons show
    for k, extra in ((PM_ALL_LIGHTS, []), (0, ["--light", "0"])):
        out = tmp_path / f"img{k}.pfm"
        r = subprocess.run([CLI, "--pbrt", os.path.join(SCENES, "cornell-two-lights.pbrt"), "--paths", str(paths),
                            "--out", str(out)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(read_pfm(out).view(np.uint32), ref[k].view(np.uint32)), f".pbrt image differs (light {k})"
    r = subprocess.run([CLI, "--pbrt", os.path.join(SCENES, "cornell-two-lights.pbrt"), "--light", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "out of range" in r.stderr


def test_two_lights_through_pbrt_boundary(tmp_path, hip_mod):
    """pm_pbrt_host --two-lights --lightsource -1: the ParamSet key through
    cudaapi.cpp equals the stage driver on the host's rays and light randoms."""
    from test_pbrt_boundary import read_host_output
    out = tmp_path / "host.bin"
    r = subprocess.run([HOST, "--width", str(W), "--height", str(H), "--paths", "16384", "--nsamples", "2",
                        "--two-lights", "--lightsource", "-1", "--out", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rays, rand2d, n2d, written, img = read_host_output(out, W, H)
    assert written == 1 and n2d == 4
    sc = scenes.cornell_two_lights(W, H, nsamples=2)
    sc.camera = ("rays", rays.copy(), rand2d.copy(), n2d)
    ctx = sc.load_into(hip_mod.Context(0))
    try:
        ref, _ = ctx.render(RenderParams.defaults(paths_per_pass=16384, light_source_index=PM_ALL_LIGHTS))
        one, _ = ctx.render(RenderParams.defaults(paths_per_pass=16384))
    finally:
        ctx.close()
    assert (ref > 0).any() and not np.array_equal(ref, one)
    assert np.array_equal(img.view(np.uint32), ref.reshape(-1, 3).view(np.uint32))


# ------------------------------------------------------------------ 8. errors
def test_errors(hip_mod):
    sc = scenes.cornell_box(W, H)
    L = sc.lights[0]
    sc.lights[0] = L[:5] + (np.float32([0, 0, 0]),) + L[6:]           # the only light is dark
    ctx = sc.load_into(hip_mod.Context(0))
    try:
        assert ctx.scene_section("light_cdf").tolist() == [0.0]
        with pytest.raises(hip_mod.PMError, match="PM_ALL_LIGHTS.*weight") as e:
            ctx.trace_photons(params(PM_ALL_LIGHTS), 0, 0, 64)
        assert e.value.code == PM_ERR_INVALID
        with pytest.raises(hip_mod.PMError) as e:
            ctx.render(params(PM_ALL_LIGHTS))
        assert e.value.code == PM_ERR_INVALID
        ctx.trace_photons(params(0), 0, 0, 64)                         # a fixed light still traces (nothing)
    finally:
        ctx.close()
    ctx = R.mixed_scene(W, H).load_into(hip_mod.Context(0))
    try:
        for bad in (-2, 3, -100):
            with pytest.raises(hip_mod.PMError, match="out of range") as e:
                ctx.trace_photons(params(bad), 0, 0, 64)
            assert e.value.code == PM_ERR_INVALID
    finally:
        ctx.close()
