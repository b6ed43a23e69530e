"""Textures on matte triangle meshes on the device (pm_add_texture_*,
csrc/pm_texture.h): exact equivalences with the constant-colour path the
oracle covers, and the texel lookups against the float64 restatement in
texture_ref.py.

Every scene is the open Cornell box without blocks at 32 x 32, 4,096 paths of
4 photons, one pass.

Tolerance of the lookups against float64 (test_record_albedo...), by the
convention of test_delta_lights_gpu.py: the floor is measured first, with the
walls' textures replaced by a probe whose value is (u, v) itself (a 2 x 2 ramp
image read between its texel centres: bilinear interpolation of a ramp is the
ramp; a one-colour image would return its colour whatever (u, v) is and show
nothing). The probe's largest deviation from the float64 (u, v) of the
record's fp32 position is the (u, v) error of fp32 position against float64,
the floor. It is measured in the run that uses it (uv_floor(), once per
process), so a compiler that moves a rounding moves floor and tolerance
together; test_uv_floor only holds it within 4 x the values recorded on the
MI355X (UV_FLOOR), against a gross regression. A bilinear image changes by at
most (largest texel difference) x w x su per unit of u, so a lookup is allowed
8 x that slope x the floor. Left out, and at most 5 % of the active records in
each case: records within EDGE = 1e-3 (in checker squares) of a checker edge;
within EDGE (as a barycentric) of a quad's diagonal on a mesh without uvs (its
default corners jump there); within EDGE radians of the phi = 0 seam of a
sphere or disk; within POLE = 0.05 radians of a sphere's poles (u = phi / 2 pi
loses its meaning there: its error grows as 1 / sin theta); within EDGE of a
disk's centre (v > 1 - EDGE).
"""
import functools
import os

import numpy as np
import pytest

import ray_query_ref as Q
import texture_ref as T
from parity_util import assert_bitexact
from pmrender import hip, scenes
from pmrender.abi import (PM_ESTIMATOR_KNN, PM_ESTIMATOR_PPM, PM_GATHER_GRID, PM_GATHER_KDTREE, PM_MATTE, PM_REC_INACTIVE,
                          RenderParams)

pytestmark = pytest.mark.gpu

PATHS, W, H, MPC = 4096, 32, 32, 4
EDGE, POLE = 1e-3, 0.05
# recorded on the MI355X (test_uv_floor and test_sphere_and_disk print the run's own): the largest
# |(u, v) - float64| of the ramp probe on the box's walls (5.65e-7), and on the sphere and the disk (1.32e-7)
UV_FLOOR = {"walls": 5.7e-7, "quadrics": 1.4e-7}
RIGHT = [(0, 0, 559.2), (0, 0, 0), (0, 548.8, 0), (0, 548.8, 559.2)]
LEFT = [(552.8, 0, 0), (549.6, 0, 559.2), (556.0, 548.8, 559.2), (556.0, 548.8, 0)]
IMG44 = (np.arange(48, dtype=np.float32).reshape(4, 4, 3) * 0.017 + 0.1).astype(np.float32)  # 48 distinct values in [0.1, 0.9]
CHECK_MAP = (4.0, 4.0, 0.0, 0.0)
C1, C2 = (0.8, 0.7, 0.2), (0.1, 0.2, 0.6)


def box(floor, back, right, uv=True):
    """The open box; floor / back / right: a colour or a function of the Scene returning a Tex."""
    s = scenes.Scene()
    mat = lambda m: s.material(PM_MATTE, m(s) if callable(m) else m)
    uvs = [scenes.QUAD_UV] if uv else None
    s.add_quads([scenes.FLOOR], mat(floor), uvs=uvs)
    s.add_quads([scenes.CEILING], mat(scenes.WHITE))
    s.add_quads([scenes.BACK], mat(back), uvs=uvs)
    s.add_quads([RIGHT], mat(right), uvs=uvs)
    s.add_quads([LEFT], mat(scenes.RED))
    scenes._ceiling_light(s)
    s.camera = scenes.pinhole(W, H)
    return s


def params(**kw):
    return RenderParams.defaults(paths_per_pass=PATHS, max_photon_count=MPC, passes=1, **kw)


def stages(sc, p, ctx=None, instancing=True):
    """eye pass, trace, map, gather on a fresh context: (ctx, records, slots)"""
    ctx = ctx or sc.load_into(hip.Context(0), instancing=instancing)
    ctx.eye_pass(p)
    ctx.trace_photons(p, 0, 0, PATHS)
    slots = ctx.download_slots(PATHS * MPC)
    ctx.build_photon_map(p)
    ctx.gather(p)
    return ctx, ctx.download_records(), slots


VARIANTS = {"ppm": dict(estimator=PM_ESTIMATOR_PPM, gather_structure=PM_GATHER_GRID),
            "knn": dict(estimator=PM_ESTIMATOR_KNN, gather_structure=PM_GATHER_GRID, knn_lookup=8),
            "kdtree": dict(estimator=PM_ESTIMATOR_PPM, gather_structure=PM_GATHER_KDTREE)}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_white_texture_is_the_constant_white_material_bit_for_bit(variant):
    """a floor whose Kd is a 2 x 2 all-ones image against Scene.material(PM_MATTE, (1, 1, 1)):
    slots, records and the pm_render image are identical"""
    p = params(**VARIANTS[variant])
    white = lambda s: s.texture_image(np.ones((2, 2, 3), np.float32))
    a = box(white, scenes.WHITE, scenes.GREEN)
    b = box((1.0, 1.0, 1.0), scenes.WHITE, scenes.GREEN)
    ca, ra, sa = stages(a, p)
    cb, rb, sb = stages(b, p)
    assert ((ra["flags"] & PM_REC_INACTIVE) == 0).sum() > W * H // 2
    assert (sa["bits"] & 1).sum() > PATHS
    assert sa.tobytes() == sb.tobytes(), "photon slots differ"
    assert ra.tobytes() == rb.tobytes(), "records differ"
    ia, _ = ca.render(p)
    ib, _ = cb.render(p)
    assert_bitexact(ia, ib, "pm_render image")
    assert ia.max() > 0


def final_ref(recs, kd, emitted, knn, mats=None):
    """pm_final's arithmetic in fp32 numpy from the downloaded records and albedo factors"""
    f = np.float32
    flux, r2, dl = recs["flux"].astype(f), recs["radius2"].astype(f), recs["dl"].astype(f)
    inv_pi = f(0.31830988618379067154)
    if knn:
        ind = (flux * (f(1.0) / f(emitted))) * ((mats * inv_pi) * kd)
    else:
        ind = ((kd * flux) * inv_pi) * (f(1.0) / (r2 * f(emitted)))[:, None]
        ind[recs["photon_count"] == 0] = 0
    out = dl + ind
    out[(recs["flags"] & PM_REC_INACTIVE) != 0] = 0
    return out


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_uniform_colour_image_equals_the_constant_colour():
    """a 3 x 5 image of one colour with repeat and a non-trivial mapping against the constant: slots and
    direct light bit for bit (the lerp form returns the texel exactly); the image to the 4 ulp of
    test_final_radiance (Kd multiplies the sum instead of every term, and the sums are exact fixed point:
    they differ only by their roundings)"""
    c = (0.3, 0.6, 0.2)
    p = params()
    img = np.broadcast_to(np.float32(c), (5, 3, 3)).copy()
    a = box(lambda s: s.texture_image(img, wrap="repeat", mapping=(2.7, -1.3, 0.21, 0.4)), scenes.WHITE, scenes.GREEN)
    b = box(c, scenes.WHITE, scenes.GREEN)
    ca, ra, sa = stages(a, p)
    cb, rb, sb = stages(b, p)
    assert sa.tobytes() == sb.tobytes(), "photon slots differ"
    assert_bitexact(ra["dl"], rb["dl"], "direct light")
    assert_bitexact(ra["pos"], rb["pos"], "record positions")
    floor = (ra["material"] == 0) & ((ra["flags"] & PM_REC_INACTIVE) == 0)
    assert floor.sum() > 50
    kd = ca.record_albedo()
    assert_bitexact(kd[floor], np.broadcast_to(np.float32(c), (floor.sum(), 3)), "floor albedo")
    ia, ib = ca.final_image(PATHS), cb.final_image(PATHS)
    # flux of the textured floor is the sum with Kd = 1: c x it must give the constant's flux to fp32 rounding
    u = ulps(ia, ib)
    print("uniform colour: largest image difference", u.max(), "ulp")
    assert u.max() <= 4


def textured_scene(wrap="repeat", mapping=(1.0, 1.0, 0.0, 0.0), uv=True):
    """a 4 x 4 image of distinct texels on the floor, a 4 x 4-square checkerboard on the back wall, a
    scale of both on the right wall; its textures for texture_ref.evaluate per material id"""
    holder = {}

    def floor(s):
        holder["img"] = s.texture_image(IMG44, wrap=wrap, mapping=mapping, scale=(0.9, 1.0, 0.8))
        return holder["img"]

    sc = box(floor, lambda s: s.texture_checker(C1, C2, mapping=CHECK_MAP),
             lambda s: s.texture_scale(holder["img"], (0.5, 0.9, 1.0)), uv=uv)
    image = ("image", IMG44, wrap, mapping, (0.9, 1.0, 0.8))
    ref = {0: image, 2: ("checker", ("const", C1), ("const", C2), CHECK_MAP), 3: ("scale", image, ("const", (0.5, 0.9, 1.0)))}
    return sc, ref


def expected_albedo(sc, ref, pos, material):
    """(kd (n, 3) float64, near_edge (n,)) of surface points by material id; untextured: factor 1"""
    kd, near = np.ones((len(pos), 3)), np.zeros(len(pos), bool)
    for m, tex in ref.items():
        sel = np.nonzero(material == m)[0]
        mesh = next(x for x in sc.meshes if x["material"] == m)
        u, v, hit, margin = T.mesh_uv(pos[sel], mesh["P"], mesh["idx"], mesh["uv"], with_margin=True)
        assert hit.all(), f"material {m}: a point lies on none of its triangles"
        kd[sel] = T.evaluate(tex, u, v)
        if tex[0] == "checker":
            near[sel] = T.checker_edge_distance(u, v, tex[3]) < EDGE
        if mesh["uv"] is None:  # default corners per triangle: (u, v) jumps across the quad's diagonal
            near[sel] |= margin < EDGE
    return kd, near


def albedo_tolerance(mapping):
    slope = float(IMG44.max() - IMG44.min()) * 4 * max(abs(mapping[0]), abs(mapping[1]))
    return 8 * slope * uv_floor()


@pytest.mark.parametrize("wrap,mapping,uv", [("repeat", (1.0, 1.0, 0.0, 0.0), True), ("black", (1.6, 1.4, -0.3, -0.2), True),
                                             ("clamp", (1.6, 1.4, -0.3, -0.2), True), ("repeat", (2.0, 3.0, 0.25, 0.5), False)])
def test_record_albedo_against_float64(wrap, mapping, uv):
    """every active record's albedo factor against texture_ref at the record's position; the last case has
    no uvs on the meshes: the default corners (0,0) (1,0) (0,1) per triangle"""
    sc, ref = textured_scene(wrap, mapping, uv)
    p = params()
    ctx = sc.load_into(hip.Context(0))
    ctx.eye_pass(p)
    recs = ctx.download_records()
    act = (recs["flags"] & PM_REC_INACTIVE) == 0
    got = ctx.record_albedo()
    assert np.all(got[~act] == 0)
    want, near = expected_albedo(sc, ref, recs["pos"][act].astype(np.float64), recs["material"][act])
    for m in ref:
        assert (recs["material"][act] == m).sum() > 20, f"material {m} is hardly seen"
    assert near.sum() <= 0.05 * act.sum(), (near.sum(), act.sum())
    err = np.abs(got[act][~near] - want[~near]).max()
    print(f"albedo {wrap} {mapping} uv={uv}: largest error {err:.3e}, tolerance {albedo_tolerance(mapping):.3e}, "
          f"{near.sum()} of {act.sum()} records near a checker edge")
    assert err <= albedo_tolerance(mapping)
    if wrap == "black":  # the mapping leaves [0, 1]: some floor records must be black, some not
        floor = got[act][recs["material"][act] == 0]
        assert (floor.max(axis=1) == 0).any() and (floor.max(axis=1) > 0).any()


def bounce_deviation(sc, ref, slots):
    """largest |alpha[k+1] / alpha[k] - Kd(p[k])| over consecutive valid slots of a path (flat walls with
    geometric normals: the Lambert weight is Kd up to rounding); ref: textures by material, constants else"""
    s = slots.reshape(PATHS, MPC)
    valid = (s["bits"] & 1) == 1
    pair = valid[:, :-1] & valid[:, 1:]
    # A few paths are emitted with weight exactly (0, 0, 0): their Halton direction sample is exactly 0, which
    # puts the direction in the light's plane (|cos| = 0). The CPU oracle deposits the same all-zero photons for
    # the same path ids; such a path gives no ratio. Any other zero channel is an error.
    dark = (s["alpha"] == 0).all(axis=2)
    assert not ((s["alpha"] == 0).any(axis=2) & ~dark & valid).any(), "a deposit has a zero channel"
    dead = (dark & valid).any(axis=1)
    assert np.array_equal((dark | ~valid).all(axis=1), dead | ~valid.any(axis=1)), "a path's weight became zero on the way"
    assert dead.sum() <= 4, np.flatnonzero(dead)
    pair &= ~dead[:, None]
    p = s["p"][:, :-1][pair].astype(np.float64)
    ratio = s["alpha"][:, 1:][pair].astype(np.float64) / s["alpha"][:, :-1][pair]
    kd, near, best = np.zeros((len(p), 3)), np.zeros(len(p), bool), np.full(len(p), np.inf)
    for mesh in sc.meshes:  # a point belongs to the wall whose plane is nearest
        u, v, hit, dist = T.mesh_uv(p, mesh["P"], mesh["idx"], mesh["uv"], with_distance=True)
        hit &= dist < best
        best[hit] = dist[hit]
        m = mesh["material"]
        near[hit] = False
        if m in ref:
            kd[hit] = T.evaluate(ref[m], u[hit], v[hit])
            if ref[m][0] == "checker":
                near[hit] = T.checker_edge_distance(u[hit], v[hit], ref[m][3]) < EDGE
        else:
            kd[hit] = np.float64(np.float32(sc.materials[m][1]))
    # deposits on the light's disk (black matte) end the path: no pair starts there
    assert np.isfinite(best).all(), "a deposit lies on no wall"
    assert len(p) > PATHS // 2 and near.sum() <= 0.05 * len(p)
    return float(np.abs(ratio - kd)[~near].max()), int(len(p))


def test_photon_bounce_carries_the_texel():
    """tolerance: 8 x the largest deviation of the same ratio test on the all-constant box, measured in this
    run on code the oracle pins (MI355X: 2.1e-7 constant, 4.7e-7 textured)"""
    p = params()
    const = box((0.3, 0.6, 0.2), scenes.WHITE, scenes.GREEN)
    _, _, s0 = stages(const, p)
    floor_dev, n0 = bounce_deviation(const, {}, s0)
    sc, ref = textured_scene()
    _, _, s1 = stages(sc, p)
    dev, n1 = bounce_deviation(sc, ref, s1)
    tol = 8 * floor_dev
    print(f"bounce: constant box {floor_dev:.3e} over {n0} pairs; textured {dev:.3e} over {n1} pairs, tolerance {tol:.3e}")
    assert floor_dev < 1e-5
    assert dev <= tol


@pytest.mark.parametrize("variant", ["ppm", "knn"])
def test_final_radiance_from_records_and_albedo(variant):
    """pm_final equals its fp32 restatement from the downloaded records and albedo factors to 4 ulp per
    channel; after an upload of all-zero factors the image is the direct light"""
    p = params(**VARIANTS[variant])
    sc, _ = textured_scene()
    ctx, recs, _ = stages(sc, p)
    kd = ctx.record_albedo()
    mats = np.stack([np.ones(3, np.float32) if isinstance(rgb, scenes.Tex) else np.float32(rgb) for _, rgb in sc.materials])
    act = (recs["flags"] & PM_REC_INACTIVE) == 0
    want = final_ref(recs, kd, PATHS, variant == "knn", mats[np.clip(recs["material"], 0, len(mats) - 1)])
    pix = ctx.record_pixels()
    img = ctx.final_image(PATHS).reshape(-1, 3)
    got = img[pix[pix >= 0]]
    want = want[pix >= 0]
    textured = act[pix >= 0] & np.isin(recs["material"][pix >= 0], (0, 2, 3))
    assert textured.sum() > 100 and (np.abs(got[textured] - recs["dl"][pix >= 0][textured]) > 0).any(), "no indirect light"
    u = ulps(got, want)
    print(f"final {variant}: largest difference {u.max()} ulp")
    assert u.max() <= 4
    ctx.upload_record_albedo(np.zeros((len(recs), 3), np.float32))
    dark = ctx.final_image(PATHS).reshape(-1, 3)[pix[pix >= 0]]
    dl = recs["dl"][pix >= 0].copy()
    dl[~act[pix >= 0]] = 0
    assert_bitexact(dark, dl, "image with zero albedo")


def test_textured_instance_equals_its_flattened_copy():
    """a textured instanced mesh (with uvs) against the same scene flattened: records, albedo, slots"""
    sc, _ = textured_scene()
    tex = sc.texture_image(scenes.procedural_image(5, 3), wrap="repeat", mapping=(3.0, 2.0, 0.1, 0.2))
    mat = sc.material(PM_MATTE, tex)
    P = np.float32([(-60, 0, -40), (60, 0, -40), (60, 0, 40), (-60, 0, 40), (0, 90, 0)])
    idx = np.int32([(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4), (0, 2, 1), (0, 3, 2)])
    uv = np.float32([(0, 0), (1, 0), (1, 1), (0, 1), (0.5, 0.5)])
    sc.objects.append(dict(P=P, idx=idx, N=None, uv=uv, material=mat, light=-1))
    for yaw, t in ((20.0, (180.0, 0.5, 200.0)), (-35.0, (380.0, 0.5, 300.0))):
        o2w, w2o = scenes.affine(yaw_deg=yaw, scale=(1.0, 1.5, 1.0), t=t)
        sc.instances.append((0, o2w, w2o))
    p = params()
    ca, ra, sa = stages(sc, p, instancing=True)
    cb, rb, sb = stages(sc, p, instancing=False)
    assert ca.scene_info()["mode"] == "bvh-instanced" and cb.scene_info()["mode"] != "bvh-instanced"
    assert ((ra["material"] == mat) & ((ra["flags"] & PM_REC_INACTIVE) == 0)).sum() > 10, "the instances are not seen"
    assert sa.tobytes() == sb.tobytes(), "photon slots differ"
    assert ra.tobytes() == rb.tobytes(), "records differ"
    assert_bitexact(ca.record_albedo(), cb.record_albedo(), "albedo factors")


def test_simple_renderer_uses_the_texel():
    """pm_render_simple on the textured box: per pixel direct light = texel x the same box rendered with
    Kd = 1 on the textured walls (f is linear in Kd; one product per channel). This is not the float32
    restatement of the light sampling from records and albedo: it checks the texel's use against the
    untextured simple renderer, which the oracle pins, to 4 ulp per pixel and channel."""
    sc, _ = textured_scene()
    ones = box((1.0, 1.0, 1.0), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0))
    p = RenderParams.simple_defaults()
    ctx = sc.load_into(hip.Context(0))
    img, _ = ctx.render_simple(p)
    base, _ = ones.load_into(hip.Context(0)).render_simple(p)
    ctx.eye_pass(params(scene_epsilon=p.scene_epsilon))
    recs, kd, pix = ctx.download_records(), ctx.record_albedo(), ctx.record_pixels()
    ok = (pix >= 0) & ((recs["flags"] & PM_REC_INACTIVE) == 0) & np.isin(recs["material"], (0, 2, 3))
    got, want = img.reshape(-1, 3)[pix[ok]], base.reshape(-1, 3)[pix[ok]] * kd[ok]
    assert ok.sum() > 100 and want.max() > 0
    # one light, one sample: L = (att |cos|) * (kd / pi) * li against ((att |cos|) * (1 / pi) * li) * kd, a few
    # roundings apart in every pixel and channel, dark ones included
    u = ulps(got, want)
    print("simple renderer: largest difference", u.max(), "ulp")
    assert u.max() <= 4


def test_untextured_scene_refuses_the_albedo_calls():
    ctx = scenes.cornell_box(W, H, blocks=False).load_into(hip.Context(0))
    ctx.eye_pass(params())
    with pytest.raises(hip.PMError):
        ctx.record_albedo()
    with pytest.raises(hip.PMError):
        ctx.upload_record_albedo(np.zeros((ctx.num_records(), 3), np.float32))


def test_cornell_textured_renders():
    """scenes.cornell_textured: the floor shows the checker (two distinct albedo factors on it)"""
    sc = scenes.cornell_textured(W, H)
    ctx = sc.load_into(hip.Context(0))
    img, st = ctx.render(params())
    assert st["photons_valid"] > 0 and np.isfinite(img).all() and img.max() > 0
    ctx.eye_pass(params())
    recs, kd = ctx.download_records(), ctx.record_albedo()
    floor = kd[(recs["material"] == 3) & ((recs["flags"] & PM_REC_INACTIVE) == 0)]
    assert len(np.unique(floor.round(4), axis=0)) == 2
    # the committed tables as the kernels read them
    assert ctx.scene_section("mat_tex").tolist() == [-1, -1, -1, 0, 1, -1]
    tex = ctx.scene_section("textures")
    assert tex["kind"].tolist() == [1, 0] and tex["map"][0].tolist() == [8.0, 8.0, 0.0, 0.0]
    assert tex["op"][1][0]["w"] == 8 and tex["op"][1][0]["h"] == 8 and tex["op"][1][0]["texel0"] == 0
    plain = scenes.cornell_box(W, H, blocks=False).load_into(hip.Context(0))
    assert plain.scene_section("textures").size == 0 and plain.scene_section("mat_tex").size == 0


# ---- the (u, v) floor ------------------------------------------------------------------
RAMP = np.float32([[(0, 0, 0), (1, 0, 0)], [(0, 1, 0), (1, 1, 0)]])  # texel (x, y) = (x, y, 0)
RAMP_MAP = (0.5, 0.5, 0.25, 0.25)  # (u, v) in [0, 1] -> between the texel centres: the lookup returns (u, v, 0)


def probe(s):
    return s.texture_image(RAMP, wrap="clamp", mapping=RAMP_MAP)


@functools.lru_cache(maxsize=None)
def uv_floor():
    """the ramp probe on the three walls: albedo (r, g) against the float64 (u, v) of the record's position"""
    sc = box(probe, probe, probe)
    ctx = sc.load_into(hip.Context(0))
    ctx.eye_pass(params())
    recs, got = ctx.download_records(), ctx.record_albedo()
    worst = 0.0
    for m in (0, 2, 3):
        sel = (recs["material"] == m) & ((recs["flags"] & PM_REC_INACTIVE) == 0)
        mesh = next(x for x in sc.meshes if x["material"] == m)
        u, v, hit = T.mesh_uv(recs["pos"][sel].astype(np.float64), mesh["P"], mesh["idx"], mesh["uv"])
        assert hit.all() and sel.sum() > 20
        worst = max(worst, np.abs(got[sel][:, 0] - u).max(), np.abs(got[sel][:, 1] - v).max())
    return float(worst)


def test_uv_floor():
    worst = uv_floor()
    print(f"uv floor, walls: {worst:.3e} (recorded {UV_FLOOR['walls']:.3e})")
    assert 0 < worst <= 4 * UV_FLOOR["walls"]


# ---- every traversal mode ----------------------------------------------------------------
def padded(pad, **kw):
    """textured_scene() with `pad` tiny spheres parked below the floor, outside every ray: they only raise
    the primitive count and the scene's size into the next traversal mode (test_ray_query_gpu.py's knob)"""
    sc, ref = textured_scene(**kw)
    grey = sc.material(PM_MATTE, (0.5, 0.5, 0.5))
    for r, w2o in Q.padding_spheres(pad):
        o2w = np.eye(4, dtype=np.float32)
        o2w[:3, 3] = -w2o[:3, 3]
        sc.spheres.append((r, o2w.reshape(-1), w2o.reshape(-1), grey, -1))
    return sc


def mode_result(sc, mode, instancing=True):
    p = params()
    ctx = sc.load_into(hip.Context(0), instancing=instancing)
    assert ctx.scene_info()["mode"] == mode, (ctx.scene_info(), mode)
    ctx.eye_pass(p)
    ctx.trace_photons(p, 0, 0, PATHS)
    return ctx.download_records(), ctx.record_albedo(), ctx.download_slots(PATHS * MPC)


def test_every_traversal_mode_gives_the_same_records_albedo_and_slots(monkeypatch):
    for k in ("PM_BVH8", "PM_BVH_BUILD", "PM_TRACE_POOL", "PM_TRACE_HOLD", "PM_BVH_GPU_MIN"):
        monkeypatch.delenv(k, raising=False)
    want = mode_result(padded(0), "brute")
    assert ((want[0]["flags"] & PM_REC_INACTIVE) == 0).sum() > W * H // 2 and (want[2]["bits"] & 1).sum() > PATHS
    inst, _ = textured_scene()  # the walls as object meshes under the identity: the two-level walk
    ident = np.eye(4, dtype=np.float32).reshape(-1)
    for m in inst.meshes:
        inst.objects.append(m)
        inst.instances.append((len(inst.objects) - 1, ident, ident))
    inst.meshes = []
    cases = [("bvh-lds", padded(60), {}), ("bvh-hbm", padded(300), {}),           # pooled 4-wide trace
             ("bvh-hbm", padded(300), {"PM_TRACE_POOL": "0"}),                     # per-lane trace from HBM
             ("bvh-hbm", padded(300), {"PM_BVH_BUILD": "gpu"}),                    # device-built tree: uvs in its order
             ("bvh-hbm", padded(300), {"PM_BVH8": "1"}), ("bvh-instanced", inst, {})]
    for mode, sc, env in cases:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got = mode_result(sc, mode)
        for k in env:
            monkeypatch.delenv(k)
        for a, b, what in zip(got, want, ("records", "albedo", "slots")):
            if what == "records":  # the padding's material shifts no id: materials are appended last
                a, b = a.copy(), b.copy()
            assert a.tobytes() == b.tobytes(), f"{mode} {env}: {what} differ from the brute-force scene's"


@pytest.mark.parametrize("bvh8", ["0", "1"])
def test_pool_stack_spill_leaves_the_slots_unchanged(monkeypatch, bvh8):
    """The pooled trace keeps PM_POOL_STACK traversal-stack entries per lane in LDS and spills deeper ones to
    global memory (pm_trav_step.h SpillStack; sized by pm_plan.cpp plan_trace). PM_POOL_STACK=0 reserves the tree's
    exact bound: no spill. PM_POOL_STACK=1 is the smallest cap SpillStack supports by its code (entry i < cap in
    LDS, every other one in the spill area; a cap of 0 means `the exact bound` to plan_trace), and it is below
    every tree's bound: fill_scene_dev sets S.stack_depth = max(2, the wide tree's stack bound + 1), and the
    tree here is at least three levels deep (scene_info), so a ray that hits two children of a node on two
    levels in a row holds a second entry. Same paths, same traversal order: the slots must not differ by a bit."""
    for k in ("PM_BVH8", "PM_BVH_BUILD", "PM_TRACE_POOL", "PM_TRACE_HOLD", "PM_BVH_GPU_MIN", "PM_POOL_STACK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PM_BVH8", bvh8)
    sc = padded(300)
    info = sc.load_into(hip.Context(0)).scene_info()
    assert info["mode"] == "bvh-hbm" and info["bvh_depth"] >= 3, info
    slots = {}
    for cap in ("0", "1"):
        monkeypatch.setenv("PM_POOL_STACK", cap)
        slots[cap] = mode_result(sc, "bvh-hbm")[2]
    assert (slots["0"]["bits"] & 1).sum() > PATHS
    assert slots["1"].tobytes() == slots["0"].tobytes(), f"bvh8={bvh8}: the spilled stack changed the photon slots"


# ---- sphere and disk ---------------------------------------------------------------------------
SPH_C, SPH_R = (150.0, 90.0, 220.0), 80.0
DISK_O, DISK_R = (400.0, 150.0, 500.0), 110.0  # upright, facing the camera


def quadric_scene(sphere_tex, disk_tex):
    sc = box(scenes.WHITE, scenes.WHITE, scenes.GREEN)
    ms, md = sc.material(PM_MATTE, sphere_tex(sc)), sc.material(PM_MATTE, disk_tex(sc))
    o2w, w2o = scenes.translate(*SPH_C)
    sc.spheres.append((np.float32(SPH_R), o2w, w2o, ms, -1))
    sc.disks.append((np.float32(DISK_O), np.float32([DISK_R, 0, 0]), np.float32([0, -DISK_R, 0]), np.float32([0, 0, -1]),
                     np.float32(0.0), np.float32(2.0 * np.pi), md, -1))
    return sc, ms, md, w2o


def quadric_uv(recs, ms, md, w2o):
    """(sel, u, v, left_out) for the sphere's and the disk's active records"""
    act = (recs["flags"] & PM_REC_INACTIVE) == 0
    out = {}
    pos = recs["pos"].astype(np.float64)
    sel = act & (recs["material"] == ms)
    u, v, phi, theta = T.sphere_uv(pos[sel], w2o)
    out["sphere"] = (sel, u, v, (np.minimum(phi, 2 * np.pi - phi) < EDGE) | (np.minimum(theta, np.pi - theta) < POLE))
    sel = act & (recs["material"] == md)
    u, v, phi = T.disk_uv(pos[sel], DISK_O, (DISK_R, 0, 0), (0, -DISK_R, 0))
    out["disk"] = (sel, u, v, (np.minimum(phi, 2 * np.pi - phi) < EDGE) | (v > 1 - EDGE))
    return out


def test_sphere_and_disk():
    """a checkerboard on a sphere and an image on a disk: record albedo against texture_ref at pbrt-v2's
    (u, v); first the ramp probe on both for the floor, then 8 x slope x floor as on the walls"""
    p = params()
    sc, ms, md, w2o = quadric_scene(probe, probe)
    ctx = sc.load_into(hip.Context(0))
    ctx.eye_pass(p)
    recs, got = ctx.download_records(), ctx.record_albedo()
    worst = 0.0
    for name, (sel, u, v, out) in quadric_uv(recs, ms, md, w2o).items():
        assert sel.sum() > 30 and out.sum() <= 0.05 * sel.sum(), (name, sel.sum(), out.sum())
        worst = max(worst, np.abs(got[sel][~out][:, 0] - u[~out]).max(), np.abs(got[sel][~out][:, 1] - v[~out]).max())
    print(f"uv floor, sphere and disk: {worst:.3e} (recorded {UV_FLOOR['quadrics']:.3e})")
    assert 0 < worst <= 4 * UV_FLOOR["quadrics"]
    cmap, imap = (8.0, 6.0, 0.0, 0.0), (1.0, 1.0, 0.0, 0.0)
    sc, ms, md, w2o = quadric_scene(lambda s: s.texture_checker(C1, C2, mapping=cmap),
                                    lambda s: s.texture_image(IMG44, wrap="clamp", mapping=imap))
    ctx = sc.load_into(hip.Context(0))
    ctx.eye_pass(p)
    recs, got = ctx.download_records(), ctx.record_albedo()
    q = quadric_uv(recs, ms, md, w2o)
    sel, u, v, out = q["sphere"]
    out = out | (T.checker_edge_distance(u, v, cmap) < EDGE)
    assert out.sum() <= 0.05 * sel.sum(), (out.sum(), sel.sum())
    want = T.evaluate(("checker", ("const", C1), ("const", C2), cmap), u, v)
    assert np.abs(got[sel][~out] - want[~out]).max() <= 2.0 ** -24, "sphere checker"
    assert len(np.unique(got[sel].round(4), axis=0)) == 2
    sel, u, v, out = q["disk"]
    want = T.evaluate(("image", IMG44, "clamp", imap, (1.0, 1.0, 1.0)), u, v)
    err = np.abs(got[sel][~out] - want[~out]).max()
    tol = 8 * float(IMG44.max() - IMG44.min()) * 4 * float(worst)
    print(f"disk image: largest error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol


# ---- multi-device context ------------------------------------------------------------------------
def _n_gpus():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:
        return 1


def _group_render(devices):
    ctx = scenes.cornell_textured(40, 32).load_into(hip.Context(0, devices=devices))
    try:
        p = RenderParams.defaults(paths_per_pass=8192, initial_radius2=25.0)
        return ctx.render(p)[0], ctx.render_simple(RenderParams.simple_defaults())[0]
    finally:
        ctx.close()


@pytest.mark.parametrize("devices", [[0], [0, 0]])
def test_group_context_equals_the_plain_context(devices):
    """cornell_textured through the group path (the forwarded texture calls, k_final's factor per band)"""
    want, want_simple = _group_render(None)
    got, got_simple = _group_render(devices)
    assert (want > 0).any()
    assert_bitexact(got, want, f"group {devices} image")
    assert_bitexact(got_simple, want_simple, f"group {devices} simple image")


@pytest.mark.skipif(_n_gpus() < 2, reason="needs two GPUs")
def test_two_device_group_equals_the_plain_context():
    want, _ = _group_render(None)
    got, _ = _group_render([0, 1])
    assert_bitexact(got, want, "two-device image")


# ---- front ends ---------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_render_cli")
HOST = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_pbrt_host")
SCENES = os.path.join(ROOT, "cuda-raytrace_amd", "scenes")


def test_checker_scene_through_every_front_end(tmp_path):
    """cornell-checker.pbrt through pm_render_cli, the same box built through the pbrt plugin
    (pm_pbrt_host --checker) and scenes.cornell_checker() through the Python driver: the same image bit for
    bit; the floor shows the checker"""
    import subprocess
    from test_delta_lights_gpu import read_pfm
    from test_pbrt_boundary import read_host_output
    paths = 16384
    out = tmp_path / "checker.pfm"
    r = subprocess.run([CLI, "--pbrt", os.path.join(SCENES, "cornell-checker.pbrt"), "--paths", str(paths), "--out", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Warning" not in r.stderr, r.stderr
    cli = read_pfm(out)
    ctx = scenes.cornell_checker(256, 256).load_into(hip.Context(0))
    p = RenderParams.defaults(paths_per_pass=paths)
    ref, st = ctx.render(p)
    assert st["photons_valid"] > 0
    assert_bitexact(cli, ref, "pm_render_cli image against the Python driver")
    # the floor shows the checker: both colours among its records' albedo factors, and the image differs
    # from the plain Cornell box on the floor
    ctx.eye_pass(p)
    recs, kd = ctx.download_records(), ctx.record_albedo()
    floor = kd[(recs["material"] == 0) & ((recs["flags"] & PM_REC_INACTIVE) == 0)]
    assert len(floor) > 5000 and len(np.unique(floor.round(4), axis=0)) == 2
    plain, _ = scenes.cornell_box(256, 256).load_into(hip.Context(0)).render(p)
    assert np.abs(plain - ref).max() > 0.05
    # the plugin path, on the host's rays and light randoms
    w, h = 64, 48
    hout = tmp_path / "host.bin"
    r = subprocess.run([HOST, "--width", str(w), "--height", str(h), "--paths", str(paths), "--checker", "--out", str(hout)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rays, rand2d, n2d, written, img = read_host_output(hout, w, h)
    sc = scenes.cornell_checker(w, h)
    sc.camera = ("rays", rays.copy(), rand2d.copy(), n2d)
    ref2, _ = sc.load_into(hip.Context(0)).render(p)
    assert (ref2 > 0).any()
    assert_bitexact(img, ref2.reshape(-1, 3), "pm_pbrt_host --checker image against the Python driver")
    r = subprocess.run([HOST, "--width", str(w), "--height", str(h), "--paths", str(paths), "--out", str(hout)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not np.array_equal(read_host_output(hout, w, h)[4], img)
