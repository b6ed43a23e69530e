"""Triangle-mesh area lights on the device (pm_add_light_mesh; pm_shade.h
sample_light_mesh, sample_le, sample_l_shading, light_le) against the float64
numpy restatement in mesh_light_ref.py, on four light meshes: (a) one
triangle, (b) a quad of two equal triangles, (c) a 7-triangle fan with areas
1 : 1000 and a zero-area triangle, (d) a 33-triangle strip.

Triangles are selected with the device's own cdf (PM_SCENE_LIGHT_TRIS), which
the table test holds to 1 ulp of the numpy one, so selection is reproducible
exactly and no path is left out. Positions, directions, alpha and direct
light are fp32 against float64: their tolerance is 8 x the deviation the
existing disk light (pinned to the oracle bit for bit) shows from the same
restatement of its formulas, on the same scenes and random numbers.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import mesh_light_ref as R
from parity_util import assert_bitexact
from pmrender import scenes
from pmrender.abi import (PM_ESTIMATOR_KNN, PM_GATHER_GRID, PM_REC_INACTIVE, RenderParams)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_render_cli")
HOST = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_pbrt_host")
SCENES = os.path.join(ROOT, "cuda-raytrace_amd", "scenes")

PATHS, W, H = 4096, 64, 48
MESHES = R.light_meshes()
DISK_RADIUS = 20.0
# The fp32 noise floor of this formula family: the largest relative deviation
# of the disk light from its float64 restatement, measured on the MI355X with
# these scenes and samples (test_disk_noise_floor prints the figures, here
# rounded up to three digits), per quantity: emission origin relative to the
# scene's extent 6.97e-8, direction 1.14e-6 (it is recovered from the deposit
# through the mirror's fp32 reflection), alpha 1.71e-7, direct light 5.25e-7
# (1 sample; 3.76e-7 with 16), simple renderer 2.55e-7.
DISK_FLOOR = {"position": 6.97e-8, "direction": 1.15e-6, "alpha": 1.71e-7, "dl": 5.25e-7, "simple": 2.56e-7}
# the mesh light adds the cdf remap, a square root and one more dot product:
# each quantity is allowed 8 x the disk's deviation in the same quantity
# (never more than 8 x the largest, 9.2e-6)
TOL = {k: 8 * v for k, v in DISK_FLOOR.items()}


@functools.lru_cache(maxsize=None)
def emission_samples():
    return R.emission_samples(PATHS)


@functools.lru_cache(maxsize=None)
def light_uv(slot):
    return R.philox_uv(range(W * H), slot, 2047)


def first_deposits(ctx, begin=0, count=PATHS, light=0):
    p = RenderParams.defaults(paths_per_pass=PATHS, light_source_index=light)
    ctx.trace_photons(p, 0, begin, count, slot_path_base=begin)
    return ctx.download_slots(count * 4)


def emission_deviation(first, org_ref, area):
    """largest deviations (origin / extent, direction, alpha relative) of the
    valid first deposits from the reference emission; the valid mask"""
    smp = emission_samples()
    ok = (first["bits"] & 1) == 1
    assert ok.sum() > PATHS // 2
    org, d = R.unfold(first[ok])
    d_ref = R.uniform_sphere(smp[:, 2], smp[:, 3], np.array([0.0, 0.0, 1.0]))[ok]
    a_ref = 2.0 * np.pi * area * np.float32(R.LE).astype(np.float64)[None, :] * np.abs(d_ref[:, 2:3])
    dev_p = np.abs(org - org_ref[ok]).max() / R.EXTENT
    dev_d = np.abs(d - d_ref).max()
    dev_a = (np.abs(first["alpha"][ok].astype(np.float64) - a_ref) / a_ref).max()
    return dev_p, dev_d, dev_a, ok, org


def disk_points(u1, u2, o, x, y):
    dx, dy = R.concentric_disk(np.asarray(u1, np.float32), np.asarray(u2, np.float32))
    return o[None, :] + dx[:, None] * x[None, :] + dy[:, None] * y[None, :]


def active_records(ctx):
    recs = ctx.download_records()
    act = (recs["flags"] & PM_REC_INACTIVE) == 0
    return recs, act, ctx.record_pixels()


def dl_reference(recs, act, pix, point_fn, normal_fn, area, nsamples, pdf_division=True, slot0=0):
    """slot0: the light's first 2-D sample slot (the samples of the lights before it)"""
    pts, nrm = [], []
    for s in range(nsamples):
        uv = light_uv(slot0 + s)[pix[act]]
        k_p = point_fn(uv[:, 0], uv[:, 1])
        pts.append(k_p[1])
        nrm.append(normal_fn(k_p[0]))
    return R.direct_light(recs["pos"][act], recs["ns"][act], pts, nrm, area, nsamples, pdf_division)


def rel_dev(got, ref):
    lit = ref > 0
    assert lit.any()
    assert np.all(got[~lit] == 0), "light where the reference has none"
    return float((np.abs(got[lit].astype(np.float64) - ref[lit]) / ref[lit]).max())


def mesh_sampler(name, cdf, height=None, shift=(0.0, 0.0, 0.0)):
    P, idx = MESHES[name]
    Pw = P if height is None else R.to_floor(P, height) + np.float32(shift)
    _, _, n = R.table_ref(Pw, idx)
    return (lambda u1, u2: R.mesh_points(Pw, idx, cdf, u1, u2)), (lambda k: n[k])


def test_disk_noise_floor(hip_mod):
    """The disk light against the same float64 restatement: the noise floor
    DISK_FLOOR was read from. The restatement is right if the disk stays
    under it."""
    r = np.float64(np.float32(DISK_RADIUS))
    area = float(np.float32(np.float32(2.0 * np.pi) * np.float32(0.5) * np.float32(DISK_RADIUS * DISK_RADIUS)))
    ctx = R.mirror_scene(("disk", DISK_RADIUS)).load_into(hip_mod.Context(0))
    try:
        smp = emission_samples()
        org_ref = disk_points(smp[:, 0], smp[:, 1], np.zeros(3), np.array([r, 0, 0]), np.array([0, r, 0]))
        dev_p, dev_d, dev_a, _, _ = emission_deviation(first_deposits(ctx)[0::4], org_ref, area)
    finally:
        ctx.close()
    devs = {"position": dev_p, "direction": dev_d, "alpha": dev_a, "dl": 0.0}
    o, x, y = np.array([0.0, 100.0, 0.0]), np.array([r, 0, 0]), np.array([0, 0, r])
    nrm = np.array([0.0, -1.0, 0.0])
    for ns in (1, 16):
        ctx = R.floor_scene(("disk", DISK_RADIUS), ns).load_into(hip_mod.Context(0))
        try:
            ctx.eye_pass(RenderParams.defaults())
            recs, act, pix = active_records(ctx)
            pf = lambda u1, u2: (np.zeros(len(u1), np.int64), disk_points(u1, u2, o, x, y))
            ref = dl_reference(recs, act, pix, pf, lambda k: nrm[None, :], area, ns)
            devs["dl"] = max(devs["dl"], rel_dev(recs["dl"][act], ref))
            if ns == 1:
                img, _ = ctx.render_simple(RenderParams.simple_defaults())
                ref = dl_reference(recs, act, pix, pf, lambda k: nrm[None, :], area, 1, pdf_division=False)
                devs["simple"] = rel_dev(img.reshape(-1, 3)[pix[act]], ref)
        finally:
            ctx.close()
    print("disk noise floor:", {k: f"{v:.3g}" for k, v in devs.items()})
    assert all(devs[k] <= DISK_FLOOR[k] for k in DISK_FLOOR), devs


@pytest.fixture(scope="module", params=sorted(MESHES))
def mesh_ctx(request, hip_mod):
    name = request.param
    P, idx = MESHES[name]
    ctx = R.mirror_scene(("mesh", P, idx)).load_into(hip_mod.Context(0))
    yield name, ctx
    ctx.close()


def test_table(mesh_ctx):
    name, ctx = mesh_ctx
    P, idx = MESHES[name]
    t = ctx.scene_section("light_tris")
    cdf, area, n = R.table_ref(P, idx)
    assert len(t) == len(idx)
    assert np.all(np.diff(t["cdf"]) >= 0) and t["cdf"][-1] == np.float32(1.0)
    assert R.ulp_distance(t["cdf"], cdf).max() <= 1
    if name == "c":
        assert t["cdf"][3] == t["cdf"][2]                # the zero-area triangle's bin is empty
    if name == "b":
        assert t["cdf"][0] == np.float32(0.5)
    np.testing.assert_array_equal(t["p0"], P[idx[:, 0]])
    np.testing.assert_array_equal(t["e1"][:, :3], P[idx[:, 1]] - P[idx[:, 0]])
    np.testing.assert_array_equal(t["e2"][:, :3], P[idx[:, 2]] - P[idx[:, 0]])
    np.testing.assert_allclose(t["n"][:, :3], n, atol=1e-7)


def check_emission(name, ctx, first, entry0=0):
    """test 2's checks on the first deposits of paths [0, PATHS); entry0: the
    light's first entry in the table (the triangles of the lights before it)"""
    P, idx = MESHES[name]
    cdf = ctx.scene_section("light_tris")["cdf"][entry0:entry0 + len(idx)]
    _, area, _ = R.table_ref(P, idx)
    smp = emission_samples()
    k, org_ref = R.mesh_points(P, idx, cdf, smp[:, 0], smp[:, 1])
    dev_p, dev_d, dev_a, ok, org = emission_deviation(first, org_ref, area)
    print(f"mesh {name}: position {dev_p:.3g} direction {dev_d:.3g} alpha {dev_a:.3g} ({ok.sum()} paths)")
    assert dev_p <= TOL["position"] and dev_d <= TOL["direction"] and dev_a <= TOL["alpha"], (dev_p, dev_d, dev_a)
    # every origin lies on the triangle the reference chose (barycentrics of
    # the recovered origin within the position tolerance): with that, the
    # counts per triangle are the reference's, and nothing more is compared
    Pd = P.astype(np.float64)
    p0, e1, e2 = Pd[idx[k[ok], 0]], Pd[idx[k[ok], 1]] - Pd[idx[k[ok], 0]], Pd[idx[k[ok], 2]] - Pd[idx[k[ok], 0]]
    v = org - p0
    det = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    assert np.all(det > 0), "a zero-area triangle was chosen"
    b1 = (v[:, 0] * e2[:, 1] - v[:, 1] * e2[:, 0]) / det
    b2 = (e1[:, 0] * v[:, 1] - e1[:, 1] * v[:, 0]) / det
    margin = TOL["position"] * R.EXTENT / np.sqrt(det)
    on = (b1 >= -margin) & (b2 >= -margin) & (b1 + b2 <= 1 + 2 * margin) & (np.abs(org[:, 2]) <= TOL["position"] * R.EXTENT)
    assert on.all(), f"{(~on).sum()} origins off the reference's triangle"
    if name == "c":
        assert not np.any(k == 3)                        # the zero-area triangle: chosen by no path
    return ok


def test_emission_through_mirror(mesh_ctx):
    name, ctx = mesh_ctx
    check_emission(name, ctx, first_deposits(ctx)[0::4])


@pytest.mark.parametrize("name", sorted(MESHES))
def test_direct_light(name, hip_mod):
    P, idx = MESHES[name]
    _, area, _ = R.table_ref(R.to_floor(P), idx)
    for ns in (1, 16):
        ctx = R.floor_scene(("mesh", P, idx), ns).load_into(hip_mod.Context(0))
        try:
            ctx.eye_pass(RenderParams.defaults())
            recs, act, pix = active_records(ctx)
            pf, nf = mesh_sampler(name, ctx.scene_section("light_tris")["cdf"], 100.0)
            dev = rel_dev(recs["dl"][act], dl_reference(recs, act, pix, pf, nf, area, ns))
            print(f"mesh {name}: dl with {ns} samples {dev:.3g}")
            assert dev <= TOL["dl"]
            if ns == 1:  # the simple renderer: sample 0 only, no pdf division
                img, _ = ctx.render_simple(RenderParams.simple_defaults())
                ref = dl_reference(recs, act, pix, pf, nf, area, 1, pdf_division=False)
                dev = rel_dev(img.reshape(-1, 3)[pix[act]], ref)
                print(f"mesh {name}: simple renderer {dev:.3g}")
                assert dev <= TOL["simple"]
        finally:
            ctx.close()
    # an opaque slab under the whole light: nothing below it is lit
    ctx = R.floor_scene(("mesh", P, idx), 16, slab=True).load_into(hip_mod.Context(0))
    try:
        ctx.eye_pass(RenderParams.defaults())
        recs, act, _ = active_records(ctx)
        below = act & (recs["pos"][:, 1] < 1.0)
        assert below.sum() > W * H // 2 and np.all(recs["dl"][below] == 0)
    finally:
        ctx.close()
    # looking up at the light: its front emits (dl >= Le), its back does not;
    # reverse_orientation swaps the two
    for reverse in (False, True):
        ctx = R.floor_scene(("mesh", P, idx), 1, reverse=reverse, look_up=True).load_into(hip_mod.Context(0))
        try:
            ctx.eye_pass(RenderParams.defaults())
            recs, act, _ = active_records(ctx)
            on_light = act & (recs["pos"][:, 1] > 99.0)
            assert on_light.sum() > 8
            if reverse:
                assert np.all(recs["dl"][on_light] == 0)
            else:
                assert np.all(recs["dl"][on_light] >= np.float32(R.LE)[None, :])
        finally:
            ctx.close()


def test_two_mesh_lights(hip_mod):
    """Two mesh lights in one scene: the second one's triangles start past the
    first one's in the table, its 2-D samples past the first one's slots."""
    (Pc, ic), (Pd, idd) = MESHES["c"], MESHES["d"]
    shift = (50.0, 0.0, 40.0)
    sc = R.floor_scene(("mesh", Pc, ic), 2)
    sc.add_mesh_light(R.to_floor(Pd) + np.float32(shift), idd, R.LE, 3)
    ctx = sc.load_into(hip_mod.Context(0))
    try:
        t = ctx.scene_section("light_tris")
        assert len(t) == len(ic) + len(idd)
        for (P, idx, sh), part in (((Pc, ic, (0, 0, 0)), t[:len(ic)]), ((Pd, idd, shift), t[len(ic):])):
            Pw = R.to_floor(P) + np.float32(sh)
            cdf, _, n = R.table_ref(Pw, idx)
            assert R.ulp_distance(part["cdf"], cdf).max() <= 1 and part["cdf"][-1] == np.float32(1.0)
            np.testing.assert_array_equal(part["p0"], Pw[idx[:, 0]])
            np.testing.assert_allclose(part["n"][:, :3], n, atol=1e-7)
        ctx.eye_pass(RenderParams.defaults())
        recs, act, pix = active_records(ctx)
        ref = 0.0
        for name, sh, part, ns, slot0 in (("c", (0, 0, 0), t[:len(ic)], 2, 0), ("d", shift, t[len(ic):], 3, 2)):
            pf, nf = mesh_sampler(name, part["cdf"], 100.0, sh)
            _, area, _ = R.table_ref(R.to_floor(MESHES[name][0]), MESHES[name][1])
            ref = ref + dl_reference(recs, act, pix, pf, nf, area, ns, slot0=slot0)
        dev = rel_dev(recs["dl"][act], ref)
        print(f"two mesh lights: dl {dev:.3g}")
        assert dev <= TOL["dl"]
    finally:
        ctx.close()
    # emission from the second light (light_source_index 1)
    (Pa, ia) = MESHES["a"]
    sc = R.mirror_scene(("mesh", Pa, ia))
    sc.lights.append(("mesh", Pc, ic, np.float32(R.LE), 1, False))
    ctx = sc.load_into(hip_mod.Context(0))
    try:
        check_emission("c", ctx, first_deposits(ctx, light=1)[0::4], entry0=len(ia))
    finally:
        ctx.close()


def test_light_sample_of_exactly_one(hip_mod):
    """Host rays may carry a 2-D sample of 1.0: held below 1, it lands in the
    last non-empty bin even when the mesh ends on a zero-area triangle."""
    P, idx = MESHES["b"]
    idx = np.int32(list(idx) + [(0, 3, 3)])
    sc = R.floor_scene(("mesh", P, idx), 1)
    kind, rays, rand2d, n2d = scenes.rays_from_pinhole(sc)
    rand2d[:] = 1.0
    sc.camera = (kind, rays, rand2d, n2d)
    ctx = sc.load_into(hip_mod.Context(0))
    try:
        cdf = ctx.scene_section("light_tris")["cdf"]
        assert cdf[1] == cdf[2] == np.float32(1.0)
        ctx.eye_pass(RenderParams.defaults())
        recs, act, _ = active_records(ctx)
        assert np.isfinite(recs["dl"]).all()
        Pw = R.to_floor(P)
        _, area, n = R.table_ref(Pw, idx)
        one = np.ones(int(act.sum()), np.float32)
        k, pts = R.mesh_points(Pw, idx, cdf, one, one)
        assert np.all(k == 1)
        ref = R.direct_light(recs["pos"][act], recs["ns"][act], [pts], [n[k]], area, 1)
        assert rel_dev(recs["dl"][act], ref) <= TOL["dl"]
    finally:
        ctx.close()


MODES = {0: "brute", 66: "bvh-lds", 300: "bvh-hbm", "inst": "bvh-instanced"}


@pytest.mark.parametrize("name", ["c", "d"])
def test_traversal_and_write_modes(name, hip_mod):
    """The mirror scene padded out of every path's reach into each traversal
    mode: the slots satisfy the emission test and equal each other bit for
    bit; a trace sharded by path_begin equals the whole one."""
    P, idx = MESHES[name]
    slots = {}
    for pad, mode in MODES.items():
        ctx = R.mirror_scene(("mesh", P, idx), pad).load_into(hip_mod.Context(0))
        try:
            assert ctx.scene_info()["mode"] == mode
            slots[mode] = first_deposits(ctx)
            check_emission(name, ctx, slots[mode][0::4])
            if mode in ("brute", "bvh-hbm"):
                half = PATHS // 2
                a = first_deposits(ctx, 0, half)
                b = first_deposits(ctx, half, PATHS - half)
                assert_bitexact(np.concatenate([a, b]), slots[mode], f"{mode}: sharded trace")
        finally:
            ctx.close()
    for mode in MODES.values():
        assert_bitexact(slots[mode], slots["brute"], f"slots, {mode} vs brute")


def test_disk_light_unchanged(hip_mod, oracle_mod):
    """the Cornell box with its disk light: the same bits as the oracle"""
    sc = scenes.cornell_box(W, H)
    ctx, orc = sc.load_into(hip_mod.Context(0)), sc.load_into(oracle_mod.Oracle())
    try:
        p = RenderParams.defaults(paths_per_pass=PATHS)
        ctx.trace_photons(p, 0, 0, PATHS)
        assert_bitexact(ctx.download_slots(PATHS * 4), orc.trace_photons(p), "photon slots")
    finally:
        ctx.close()


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = (int(v) for v in f.readline().split())
        scale = float(f.readline())
        a = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4").reshape(h, w, 3)
    return np.ascontiguousarray(a[::-1]).astype(np.float32)


def test_quad_light_end_to_end(tmp_path, hip_mod):
    """cornell-box-quad.pbrt through the scene-file front end equals
    cornell_quad() through the Python driver; both estimators render."""
    paths = 16384
    out = tmp_path / "img.pfm"
    r = subprocess.run([CLI, "--pbrt", os.path.join(SCENES, "cornell-box-quad.pbrt"), "--paths", str(paths),
                        "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = read_pfm(out)
    ctx = scenes.cornell_quad(256, 256).load_into(hip_mod.Context(0))
    try:
        p = RenderParams.defaults(paths_per_pass=paths, gather_structure=PM_GATHER_GRID)
        ref, st = ctx.render(p)
        assert st["photons_valid"] > 0
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), ".pbrt image differs from cornell_quad()"
        assert np.isfinite(ref).all()
        recs, act, pix = active_records(ctx)
        floor = act & (recs["pos"][:, 1] < 0.5)
        lum = ref.reshape(-1, 3)[pix[floor]] @ np.float32([0.212671, 0.715160, 0.072169])
        assert floor.sum() > 1000 and lum.mean() > 0
        # the ceiling (y = 548.8) lies above the light, which faces down: no direct light
        ceil = act & (recs["pos"][:, 1] > 548.75) & (np.abs(recs["ns"][:, 1]) > 0.99)
        assert ceil.sum() > 100 and np.all(recs["dl"][ceil] == 0)
        knn, _ = ctx.render(RenderParams.defaults(paths_per_pass=paths, estimator=PM_ESTIMATOR_KNN))
        assert np.isfinite(knn).all() and knn.reshape(-1, 3)[pix[floor]].mean() > 0
    finally:
        ctx.close()


def test_quad_light_through_pbrt_boundary(tmp_path, hip_mod):
    """pm_pbrt_host --quad-light: a TriangleMesh in a DiffuseAreaLight's shape
    set through cudaapi.cpp equals the stage driver on the host's rays and
    light randoms."""
    from test_pbrt_boundary import read_host_output
    out = tmp_path / "host.bin"
    r = subprocess.run([HOST, "--width", str(W), "--height", str(H), "--paths", "16384", "--nsamples", "2",
                        "--quad-light", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rays, rand2d, n2d, written, img = read_host_output(out, W, H)
    assert written == 1 and n2d == 2
    sc = scenes.cornell_quad(W, H, nsamples=2)
    sc.camera = ("rays", rays.copy(), rand2d.copy(), n2d)
    ctx = sc.load_into(hip_mod.Context(0))
    try:
        ref, _ = ctx.render(RenderParams.defaults(paths_per_pass=16384))
    finally:
        ctx.close()
    assert (ref > 0).any()
    assert np.array_equal(img.view(np.uint32), ref.reshape(-1, 3).view(np.uint32))
