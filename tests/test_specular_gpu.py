"""The physical specular model (pm_add_material_specular) on the device,
against the reference's materials where the two must agree bit for bit and
against the float64 restatement in specular_ref.py elsewhere.

The directed scenes are z-up, as mesh_light_ref.mirror_scene: the light at the
origin, a specular quad (or a slab of two) above it at z = 50, a matte catcher
above that at z = 100 and one below at z = -50; 4,096 paths of 4 photons, one
pass. Slot 4 pid is path pid's first deposit. Each is repeated in every
traversal mode by padding the scene out of reach (MODES); with "inst" the
specular quads are an instanced object mesh.

Tolerances against float64 come from floors measured in the run, by the
convention of test_texture_gpu.py: for a weight, the distance between the
float32 and the float64 evaluation of the same Fresnel expression on the
test's own inputs (specular_ref.fresnel with dtype float32); for positions,
directions and direct light, the error of the same float64 formula on the
reference glass (always transmitting, index 1.5) run next to the scene under
test. A check allows FLOOR_X = 4 times its floor plus 4 float32 ulps of the
value. The lobe choice compares u with F: paths with |u - F| below
specular_ref.MARGIN_ULPS = 8 float32 ulps of F are left out, at most 1 % of
them (tests/test_specular.py confirms the reference alone leaves out none for
this seed and count). Measured on the MI355X: see each test's print.

The pbrt plugin host renders on its own rays (one per pixel centre, packed as
the reference's camera does), so its leg of the whole-render equality compares
against the Python scene on those rays; the plugin's device camera recovers
its basis from three pbrt rays and is only close to scenes.pinhole's
(tests/test_film_gpu.py), which rules out bit equality with strata there.
"""
import os
import subprocess

import numpy as np
import pytest

import delta_light_ref as D
import mesh_light_ref as M
import specular_ref as R
from parity_util import assert_bitexact
from pmrender import hip, scenes
from pmrender.abi import (PM_ESTIMATOR_KNN, PM_GATHER_GRID, PM_GLASS, PM_MATTE, PM_MIRROR, PM_REC_EXCEPTION,
                          PM_REC_INACTIVE, RenderParams)

pytestmark = pytest.mark.gpu

PATHS, MPC = 4096, 4
MODES = {0: "brute", 66: "bvh-lds", 300: "bvh-hbm", "inst": "bvh-instanced"}
Z_SPEC, Z_TOP, Z_BOT, HALF = 50.0, 100.0, -50.0, 2000.0
FLOOR_X = 4.0


def bound(floor, value=1.0):
    return FLOOR_X * floor + 4.0 * float(np.max(R.ulp32(value)))


ONE, BLACK = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)


def at(p, z):
    """deposits on the plane z (a position is o + t d in fp32: a few ulp of 100 off it)"""
    return np.abs(p[:, 2] - np.float32(z)) < 1e-3


def quad(z, up):
    q = [(-HALF, -HALF, z), (HALF, -HALF, z), (HALF, HALF, z), (-HALF, HALF, z)]
    return q if up else q[::-1]


def directed(make_spec, faces, pad, light="disk", bottom=True, top=True, textured_top=False, top_half=None, far=False):
    """faces: [(z, normal up?)] of the specular quads; make_spec(scene) -> material id"""
    s = scenes.Scene()
    spec = make_spec(s)
    grey = s.material(PM_MATTE, (0.5, 0.5, 0.5))
    quads = [quad(z, up) for z, up in faces]
    if pad == "inst":
        P, idx = [], []
        for q in quads:
            b = len(P)
            P.extend(q)
            idx += [(b, b + 1, b + 2), (b, b + 2, b + 3)]
        s.objects.append(dict(P=np.float32(P), idx=np.int32(idx), N=None, uv=None, material=spec, light=-1))
        s.instances.append((0, *scenes.translate(0.0, 0.0, 0.0)))
        s.objects.append(dict(P=np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), idx=np.int32([[0, 1, 2]]), N=None, uv=None,
                              material=grey, light=-1))
        s.instances.append((1, *scenes.translate(0.0, 0.0, -200.0)))
    else:
        s.add_quads(quads, spec)
        for i in range(int(pad)):
            o2w, w2o = scenes.translate(-300.0 + 30.0 * (i % 20), -300.0 + 30.0 * (i // 20), -200.0)
            s.spheres.append((np.float32(5.0), o2w, w2o, grey, -1))
    c = top_half or M.EXTENT / 2
    if top:
        if textured_top:
            tex = s.texture_image(np.broadcast_to(np.float32([0.25, 0.5, 0.75]), (2, 2, 3)).copy())
            s.add_quads([[(-c, -c, Z_TOP), (-c, c, Z_TOP), (c, c, Z_TOP), (c, -c, Z_TOP)]], s.material(PM_MATTE, tex),
                        uvs=[scenes.QUAD_UV])
        else:
            s.add_quads([[(-c, -c, Z_TOP), (-c, c, Z_TOP), (c, c, Z_TOP), (c, -c, Z_TOP)]], grey)
    c = M.EXTENT / 2
    if far:  # a speck far along +x: it moves the world sphere, and with it a distant light's disk
        s.add_quads([[(6000, 0, 75), (6001, 0, 75), (6001, 1, 75), (6000, 1, 75)]], grey)
    if bottom:
        s.add_quads([[(-c, -c, Z_BOT), (c, -c, Z_BOT), (c, c, Z_BOT), (-c, c, Z_BOT)]], grey)
    if light == "disk":
        r = np.float32(10.0)
        area = np.float32(np.float32(2.0 * np.pi) * np.float32(0.5) * np.float32(r * r))
        s.lights.append(("disk", np.float32([0, 0, 0]), np.float32([r, 0, 0]), np.float32([0, r, 0]),
                         np.float32([0, 0, 1]), np.float32(M.LE), area, 1))
    elif light == "distant":  # travelling along (0.6, 0, 0.8): every path meets the quad at cos 0.8
        s.add_distant_light((0.0, 0.0, 0.0), (0.6, 0.0, 0.8), (3.0, 3.0, 3.0))
    else:  # "point": at the origin; "above": between the slab and the top catcher, which it lights
        s.lights.append(("point", np.float32([0, 0, 80.0 if light == "above" else 0.0]), np.float32([100.0, 100.0, 100.0])))
    s.camera = scenes.pinhole(32, 32, eye=(0.0, 0.0, 10.0), look=(30.0, 0.0, 100.0), up=(0.0, 1.0, 0.0), fov_deg=60.0)
    return s


def params(**kw):
    return RenderParams.defaults(paths_per_pass=PATHS, max_photon_count=MPC, passes=1, scene_epsilon=1e-2, **kw)


def run(sc, pad, p=None, eye=True):
    p = p or params()
    ctx = sc.load_into(hip.Context(0))
    assert ctx.scene_info()["mode"] == MODES[pad]
    recs = None
    if eye:
        ctx.eye_pass(p)
        recs = ctx.download_records()
    ctx.trace_photons(p, 0, 0, PATHS)
    return ctx, recs, ctx.download_slots(PATHS * MPC)


old = lambda t, rgb=ONE: (lambda s: s.material(t, rgb))
new = lambda t, kr, kt=ONE, index=1.5: (lambda s: s.material_specular(t, kr, kt, index))
MIRROR_FACE, SLAB = [(Z_SPEC, False)], [(Z_SPEC, False), (Z_SPEC + 10.0, True)]


@pytest.mark.parametrize("pad", MODES, ids=lambda p: MODES[p])
def test_white_mirror_equals_the_reference_mirror_bit_for_bit(pad):
    p = params()
    ca, ra, sa = run(directed(new(PM_MIRROR, ONE), MIRROR_FACE, pad), pad)
    cb, rb, sb = run(directed(old(PM_MIRROR), MIRROR_FACE, pad), pad)
    assert (sa["bits"] & 1).sum() > PATHS // 2
    assert sa.tobytes() == sb.tobytes(), "photon slots differ"
    assert ra.tobytes() == rb.tobytes(), "records differ"
    assert ((ra["flags"] & PM_REC_INACTIVE) == 0).sum() > 100
    kd = ca.record_albedo()[(ra["flags"] & PM_REC_INACTIVE) == 0]
    assert_bitexact(kd, np.ones_like(kd), "albedo factor")
    ia, _ = ca.render(p)
    ib, _ = cb.render(p)
    assert_bitexact(ia, ib, "pm_render image")


@pytest.mark.parametrize("pad", MODES, ids=lambda p: MODES[p])
def test_coloured_mirror_scales_the_flux_once_per_hit(pad):
    kr = (0.9, 0.5, 0.25)
    _, ra, sa = run(directed(new(PM_MIRROR, kr), MIRROR_FACE, pad), pad)
    _, rb, sb = run(directed(old(PM_MIRROR), MIRROR_FACE, pad), pad)
    fa, fb = sa[::MPC], sb[::MPC]
    assert np.array_equal(fa["bits"], fb["bits"]) and (fa["bits"] & 1).sum() > PATHS // 2
    v = (fa["bits"] & 1) != 0
    assert np.all(at(fa["p"][v], Z_BOT))      # one mirror hit, then the catcher below
    assert_bitexact(fa["p"], fb["p"], "first deposit positions")
    assert_bitexact(fa["alpha"][v], R.mirror_weight_chain(fb["alpha"][v], kr, 1), "alpha after one mirror hit")
    # the eye sees the top catcher in the mirror: dl and the factor carry Kr
    act = (ra["flags"] & PM_REC_INACTIVE) == 0
    assert np.array_equal(act, (rb["flags"] & PM_REC_INACTIVE) == 0) and act.sum() > 100
    assert_bitexact(ra["dl"][act], (np.float32(kr) * rb["dl"][act]).astype(np.float32), "dl = Kr L")


def test_coloured_mirror_chain_of_several_hits():
    """a second, small mirror under the light sends some paths back up: the first deposit after k = 1, 3, 5
    mirror hits carries fl(alpha Kr) applied k times; k from the path's float64 emission (disk light:
    concentric disk point, hemisphere direction)"""
    kr = (0.9, 0.5, 0.25)
    faces, zb, hb = [(Z_SPEC, False), (-40.0, True)], -40.0, HALF
    def scene(make):
        s = directed(make, [(Z_SPEC, False)], 0)
        q = [(-100.0, -100.0, zb), (100.0, -100.0, zb), (100.0, 100.0, zb), (-100.0, 100.0, zb)]
        s.add_quads([q], 0)                      # material 0: the specular one
        return s
    _, _, sa = run(scene(new(PM_MIRROR, kr)), 0, eye=False)
    _, _, sb = run(scene(old(PM_MIRROR)), 0, eye=False)
    fa, fb = sa[::MPC], sb[::MPC]
    assert np.array_equal(fa["bits"], fb["bits"])
    assert_bitexact(fa["p"], fb["p"], "first deposit positions")
    smp = M.emission_samples(PATHS, MPC).astype(np.float64)
    x, y = M.concentric_disk(smp[:, 0], smp[:, 1])
    pos = np.stack([10.0 * x, 10.0 * y], 1)
    d = M.uniform_sphere(smp[:, 2], smp[:, 3], np.array([[0.0, 0.0, 1.0]]))
    slope = d[:, :2] / d[:, 2:3]
    pos = pos + slope * Z_SPEC                   # at the upper mirror
    k = np.ones(PATHS, int)
    clear = np.ones(PATHS, bool)
    live = np.ones(PATHS, bool)
    for _ in range(4):
        at_b = pos + slope * (Z_SPEC - zb)
        edge = np.abs(np.abs(at_b).max(axis=1) - 100.0) < 1.0
        inside = live & (np.abs(at_b).max(axis=1) < 100.0)
        clear &= ~(live & edge)
        k[inside] += 2
        pos[inside] = at_b[inside] + slope[inside] * (Z_SPEC - zb)
        live = inside
    v = ((fa["bits"] & 1) != 0) & clear & ~live & at(fa["p"], Z_BOT)
    assert v.sum() > PATHS // 2 and (k[v] == 3).sum() > 20 and (k[v] >= 5).sum() > 0
    for kk in np.unique(k[v]):
        m = v & (k == kk)
        assert_bitexact(fa["alpha"][m], R.mirror_weight_chain(fb["alpha"][m], kr, int(kk)), f"alpha after {kk} mirror hits")


def test_facing_mirrors_end_as_exceptions():
    s = directed(new(PM_MIRROR, (0.9, 0.5, 0.25)), [(Z_SPEC, False), (Z_BOT + 10.0, True)], 0, top=False, bottom=False)
    s.camera = scenes.pinhole(16, 16, eye=(0.0, 0.0, 10.0), look=(0.0, 0.0, 50.0), up=(0.0, 1.0, 0.0), fov_deg=30.0)
    ctx = s.load_into(hip.Context(0))
    ctx.eye_pass(params(max_specular_depth=6))
    recs = ctx.download_records()
    assert np.all((recs["flags"] & PM_REC_EXCEPTION) != 0)
    assert not ctx.record_albedo().any() and not recs["dl"].any()


def slab_factor(wi_first, index=1.5):
    """(1 - F)^2 of a path through the parallel slab from its first deposit's direction"""
    F = R.fresnel(np.abs(wi_first[:, 2].astype(np.float64)), index)[0]
    return (1.0 - F) ** 2


@pytest.mark.parametrize("pad", MODES, ids=lambda p: MODES[p])
def test_transmitting_glass_keeps_the_reference_geometry(pad):
    """Kr = 0, Kt = 1, index 1.5: every slot's p and wi are the reference glass's bit for bit; alpha is the
    reference's times (1 - F)^2 through the slab (paths steeper than cos 0.2: 1 - F loses its relative
    precision towards grazing)"""
    _, ra, sa = run(directed(new(PM_GLASS, BLACK, ONE, 1.5), SLAB, pad), pad)
    _, rb, sb = run(directed(old(PM_GLASS), SLAB, pad), pad)
    assert np.array_equal(sa["bits"], sb["bits"]) and (sa["bits"] & 1).sum() > PATHS
    assert_bitexact(sa["p"], sb["p"], "deposit positions")
    assert_bitexact(sa["wi"], sb["wi"], "deposit directions")
    fa, fb = sa[::MPC], sb[::MPC]
    v = ((fa["bits"] & 1) != 0) & (np.abs(fa["wi"][:, 2]) > 0.2)
    assert v.sum() > PATHS // 2 and np.all(at(fa["p"][v], Z_TOP))
    want = fb["alpha"][v].astype(np.float64) * slab_factor(fa["wi"][v])[:, None]
    err = np.abs(fa["alpha"][v] / want - 1.0).max()
    cosv = np.abs(fa["wi"][v][:, 2])
    # the floor: the chain as the device runs it in float32 (F at the entry, then F at the exit from the
    # float32 cost). Added to it, an allowance that is chosen, not measured: the reference reads its
    # cosine from the deposit's direction, which went through two refractions and four frame changes in
    # float32, so the float64 factor is also taken with that cosine moved by 8 float32 ulps
    F1, _, cost1 = R.fresnel(cosv, 1.5, np.float32)
    F2 = R.fresnel(-cost1, 1.5, np.float32)[0]
    f32 = ((np.float32(1.0) - F1) * (np.float32(1.0) - F2)).astype(np.float64)
    f64 = slab_factor(fa["wi"][v])
    moved = fa["wi"][v].astype(np.float64) * (1.0 + 8.0 * 2.0 ** -24)
    floor = np.abs(f32 / f64 - 1.0).max() + np.abs(slab_factor(moved) / f64 - 1.0).max()
    print(f"alpha against (1 - F)^2: largest relative error {err:.3g}, fp32 floor {floor:.3g}")
    assert err <= bound(floor)
    # the eye through the slab: the same records
    act = (ra["flags"] & PM_REC_INACTIVE) == 0
    assert np.array_equal(ra["flags"], rb["flags"]) and act.sum() > 100
    assert_bitexact(ra["pos"], rb["pos"], "record positions")


@pytest.mark.parametrize("pad", MODES, ids=lambda p: MODES[p])
def test_white_glass_conserves_energy_and_reflects(pad):
    """Kr = Kt = 1: every weight is exactly 1, so a first deposit carries its path's emission weight, which
    the reference glass's first deposit of the same path carries too; some paths are reflected to the lower
    catcher, which no path of the reference glass reaches first"""
    _, _, sa = run(directed(new(PM_GLASS, ONE, ONE, 1.5), SLAB, pad), pad, eye=False)
    _, _, sb = run(directed(old(PM_GLASS), SLAB, pad), pad, eye=False)
    fa, fb = sa[::MPC], sb[::MPC]
    both = ((fa["bits"] & 1) != 0) & ((fb["bits"] & 1) != 0)
    assert both.sum() > PATHS // 2
    assert_bitexact(fa["alpha"][both], fb["alpha"][both], "first deposits' alpha")
    below = ((fa["bits"] & 1) != 0) & at(fa["p"], Z_BOT)
    print(f"{below.sum()} of {PATHS} first deposits below the slab")
    assert below.sum() > PATHS // 100
    assert not (((fb["bits"] & 1) != 0) & at(fb["p"], Z_BOT)).any()


def first_deposits(d, refl, eta, cost):
    """where a point light's path d lands after the quad at Z_SPEC, and its direction there, float64"""
    hit = d * (Z_SPEC / d[:, 2])[:, None]
    out = np.where(refl[:, None], d * np.array([1.0, 1.0, -1.0]), np.stack([eta * d[:, 0], eta * d[:, 1], cost], 1))
    dist = np.where(refl, (Z_BOT - Z_SPEC) / out[:, 2], (Z_TOP - Z_SPEC) / out[:, 2])
    return hit + out * dist[:, None], out


def deposit_errors(first, ids, want_p, want_d):
    got = first[ids]
    return np.abs(got["p"] - want_p).max() / M.EXTENT, np.abs(got["wi"] + want_d).max()


@pytest.mark.parametrize("pad", MODES, ids=lambda p: MODES[p])
def test_lobe_choice_follows_the_draw(pad):
    """one glass quad, index 1.33, over a point light: per upward path the branch is the reference's for the
    same Philox draw, and the first deposit lies where the reference puts it. Floor: the reference glass
    (index 1.5, every path transmitted) under the same light against the same formula."""
    p = params()
    index = 1.33
    _, _, sl = run(directed(new(PM_GLASS, ONE, ONE, index), MIRROR_FACE, pad, light="point"), pad, p, eye=False)
    _, _, so = run(directed(old(PM_GLASS), MIRROR_FACE, pad, light="point"), pad, p, eye=False)
    up, d, F, eta, cost, u, sure = R.point_light_choice(PATHS, index, p.rng_seed, MPC)
    assert (~sure).sum() <= len(up) // 100
    up, d, F, eta, cost, u = up[sure], d[sure], F[sure], eta[sure], cost[sure], u[sure]
    refl = u < F
    assert 20 < refl.sum() < len(up) // 2
    got = sl[::MPC][up]
    assert np.all((got["bits"] & 1) != 0)
    assert np.array_equal(at(got["p"], Z_BOT), refl), "branch taken"
    assert np.array_equal(at(got["p"], Z_TOP), ~refl)
    _, eta_o, cost_o = R.fresnel(d[:, 2], 1.5)
    fp, fd = deposit_errors(so[::MPC], up, *first_deposits(d, np.zeros(len(up), bool), eta_o, cost_o))
    ep, ed = deposit_errors(sl[::MPC], up, *first_deposits(d, refl, eta, cost))
    print(f"{len(up)} paths, {refl.sum()} reflected; position error {ep:.3g} of the extent (floor {fp:.3g}), "
          f"direction error {ed:.3g} (floor {fd:.3g})")
    assert ep <= bound(fp) and ed <= bound(fd)


@pytest.mark.parametrize("pad", MODES, ids=lambda p: MODES[p])
def test_lobe_choice_under_a_distant_light(pad):
    """a distant light travelling along (0.6, 0, 0.8) under the glass quad (index 1.33) and a catcher above
    it, nothing below: every path meets the quad at one cosine, so u is compared with a single F. A path that
    crosses the quad and would land on the catcher deposits there iff u >= F; a reflected one leaves the
    scene. Origins: the float64 distant emission (delta_light_ref) on the commit's world sphere. Left out:
    paths within 1 unit of an edge of the quad or the catcher, and those that pass the padding at z = -200.
    Floor: the reference glass (index 1.5) through the same formula."""
    p = params()
    index, top_half = 1.33, 1900.0
    kw = dict(light="distant", bottom=False, top_half=top_half, far=True)
    ctx, _, sl = run(directed(new(PM_GLASS, ONE, ONE, index), MIRROR_FACE, pad, **kw), pad, p, eye=False)
    _, _, so = run(directed(old(PM_GLASS), MIRROR_FACE, pad, **kw), pad, p, eye=False)
    ws = ctx.world_sphere().astype(np.float64)
    smp = M.emission_samples(PATHS, MPC)
    to_light = np.float32([0.0, 0.0, 0.0]) - np.float32([0.6, 0.0, 0.8])
    org, d, _ = D.distant_emission(to_light, (3.0, 3.0, 3.0), ws[:3], ws[3], smp[:, 0], smp[:, 1])
    d = np.array(d[0])
    hit = org + d * ((Z_SPEC - org[:, 2]) / d[2])[:, None]
    low = org + d * ((-200.0 - org[:, 2]) / d[2])[:, None]

    def landing(ix):
        F, eta, cost = (float(v) for v in R.fresnel(d[2], ix))
        out = np.array([eta * d[0], eta * d[1], cost])
        return F, hit + out * ((Z_TOP - Z_SPEC) / cost), out

    def inside(q, half):
        m = np.abs(q[:, :2]).max(axis=1)
        return m < half - 1.0, np.abs(m - half) <= 1.0

    F, land, out = landing(index)
    _, land_o, out_o = landing(1.5)
    in_q, edge_q = inside(hit, HALF)
    in_t, edge_t = inside(land, top_half)
    in_to, edge_to = inside(land_o, top_half)
    padded = np.abs(low[:, :2]).max(axis=1) < 340.0
    u = np.array([R.photon_u(pid, 1, 0, 1, p.rng_seed, MPC) for pid in range(PATHS)], np.float64)
    sure = np.abs(u - F) >= R.MARGIN_ULPS * R.ulp32(F)
    clear = in_q & ~edge_t & ~edge_to & ~padded
    assert (clear & ~sure).sum() <= max(1, clear.sum() // 100)
    clear &= sure
    want = clear & in_t & (u >= F)
    first, first_o = sl[::MPC], so[::MPC]
    got = (first["bits"] & 1) != 0
    assert clear.sum() > 100 and 10 < (clear & in_t & (u < F)).sum() and want.sum() > 50
    assert np.array_equal(got[clear], want[clear]), "lobe taken"
    ref = clear & in_to
    assert np.all((first_o["bits"][ref] & 1) != 0)
    fp = np.abs(first_o["p"][ref] - land_o[ref]).max() / M.EXTENT
    fd = np.abs(first_o["wi"][ref] + out_o).max()
    ep = np.abs(first["p"][want] - land[want]).max() / M.EXTENT
    ed = np.abs(first["wi"][want] + out).max()
    print(f"F = {F:.6f}; {clear.sum()} paths cross the quad, {want.sum()} transmitted onto the catcher, "
          f"{(clear & in_t & (u < F)).sum()} reflected; position {ep:.3g} (floor {fp:.3g}), direction {ed:.3g} (floor {fd:.3g})")
    assert ep <= bound(fp) and ed <= bound(fd)


def pixel_dirs(rr):
    """float64 pinhole ray of record rr of directed()'s camera (records lie in 8 x 8 tiles), and its pixel index"""
    _, eye, fwd, right, upv, Wc, Hc = scenes.pinhole(32, 32, eye=(0.0, 0.0, 10.0), look=(30.0, 0.0, 100.0),
                                                     up=(0.0, 1.0, 0.0), fov_deg=60.0)
    tile, lane = rr >> 6, rr & 63
    px, py = (tile % (Wc // 8)) * 8 + (lane & 7), (tile // (Wc // 8)) * 8 + (lane >> 3)
    sx = (2.0 * (px.astype(np.float32) + np.float32(0.5))) / np.float32(Wc) - np.float32(1.0)
    sy = np.float32(1.0) - (2.0 * (py.astype(np.float32) + np.float32(0.5))) / np.float32(Hc)
    d = fwd.astype(np.float64) + sx.astype(np.float64)[:, None] * right + sy.astype(np.float64)[:, None] * upv
    return d / np.linalg.norm(d, axis=1)[:, None], py * Wc + px


@pytest.mark.parametrize("pad", MODES, ids=lambda p: MODES[p])
@pytest.mark.parametrize("textured", [False, True], ids=["plain", "textured"])
def test_eye_chain_through_the_slab(textured, pad):
    """the camera looks up through the slab at the matte top, lit by a point light above the slab: per record the factor is
    the product of the weights and of eta^2 (which cancels through the slab) times the texel, dl is T L"""
    p = params()
    kr, kt = (0.0, 0.0, 0.0), (0.9, 0.8, 0.7)
    ca, ra, _ = run(directed(new(PM_GLASS, kr, kt, 1.5), SLAB, pad, light="above", textured_top=textured), pad, p)
    cb, rb, _ = run(directed(old(PM_GLASS), SLAB, pad, light="above", textured_top=textured), pad, p)
    act = (ra["flags"] & PM_REC_INACTIVE) == 0
    assert np.array_equal(ra["flags"], rb["flags"]) and act.sum() > 100
    assert_bitexact(ra["pos"], rb["pos"], "record positions")
    # the chain's direction in the air on both sides of the parallel slab: the pinhole ray of the record's pixel
    cos = np.abs(pixel_dirs(np.nonzero(act)[0])[0][:, 2])
    F = R.fresnel(cos, 1.5)[0]
    T = ((1.0 - F) ** 2)[:, None] * (np.float64(np.float32(kt)) ** 2)[None, :]
    base = cb.record_albedo()[act].astype(np.float64) if textured else np.ones((act.sum(), 3))
    if textured:
        assert np.allclose(base, [0.25, 0.5, 0.75])
    got = ca.record_albedo()[act].astype(np.float64)
    err = np.abs(got / (T * base) - 1.0).max()
    kt32 = np.float32(kt)
    t32 = ((np.float32(1.0) - R.fresnel(cos, 1.5, np.float32)[0]) ** 2)[:, None] * (kt32 * kt32)[None, :]
    floor = np.abs(t32.astype(np.float64) / T - 1.0).max()
    print(f"factor against (1 - F)^2 Kt^2 texel: largest relative error {err:.3g}, fp32 floor {floor:.3g}")
    assert err <= bound(floor)
    lit = act & (rb["dl"].max(axis=1) > 0)
    assert lit.sum() > 50
    ratio = ra["dl"][lit].astype(np.float64) / rb["dl"][lit].astype(np.float64)
    fac = got[lit[act]] / base[lit[act]]
    assert np.abs(ratio[rb["dl"][lit] > 0] / fac[rb["dl"][lit] > 0] - 1.0).max() <= bound(0.0), "dl = T L"


def eye_reference(recs, d, refl, eta, cost):
    """position and direct light (point light at z = 80 over the grey top, nothing lit below) per record"""
    eye = np.float64([0.0, 0.0, 10.0])
    hit = eye + d * ((Z_SPEC - 10.0) / d[:, 2])[:, None]
    out = np.where(refl[:, None], d * np.array([1.0, 1.0, -1.0]), np.stack([eta * d[:, 0], eta * d[:, 1], cost], 1))
    dist = np.where(refl, (Z_BOT - Z_SPEC) / out[:, 2], (Z_TOP - Z_SPEC) / out[:, 2])
    pos = hit + out * dist[:, None]
    to = np.float64([0.0, 0.0, 80.0]) - pos
    d2 = np.sum(to * to, 1)
    L = (np.abs(to[:, 2]) / np.sqrt(d2)) * (0.5 / np.pi) * 100.0 / d2
    return pos, np.where(refl, 0.0, L)      # the glass shadows the lower catcher


@pytest.mark.parametrize("pad", MODES, ids=lambda p: MODES[p])
def test_eye_chain_at_an_oblique_interface(pad):
    """the camera looks obliquely at one glass interface (Kr = Kt = 1, index 1.33: both lobes live, eta^2
    does not cancel): per record the lobe is the reference's for the eye draw of its pixel at depth 1, the
    factor is 1 (reflected) or eta^2 (transmitted), and position and dl = T L are the reference's. Floor:
    the reference glass (index 1.5, T = 1) through the same formulas."""
    p = params()
    index = 1.33
    ca, ra, _ = run(directed(new(PM_GLASS, ONE, ONE, index), MIRROR_FACE, pad, light="above"), pad, p)
    _, rb, _ = run(directed(old(PM_GLASS), MIRROR_FACE, pad, light="above"), pad, p)
    rr = np.arange(len(ra))
    d, q = pixel_dirs(rr)
    F, eta, cost = R.fresnel(d[:, 2], index)
    u = np.array([R.eye_u(k, 1, p.light_rng_seed) for k in q], np.float64)
    sure = np.abs(u - F) >= R.MARGIN_ULPS * R.ulp32(F)
    assert (~sure).sum() <= len(rr) // 100
    refl = u < F
    assert 10 < refl[sure].sum() < sure.sum() // 2
    assert np.all((ra["flags"] & PM_REC_INACTIVE) == 0) and np.all((rb["flags"] & PM_REC_INACTIVE) == 0)
    assert np.array_equal(at(ra["pos"], Z_BOT)[sure], refl[sure]), "lobe taken"
    assert np.array_equal(at(ra["pos"], Z_TOP)[sure], ~refl[sure])
    # floors from the reference glass
    _, eta_o, cost_o = R.fresnel(d[:, 2], 1.5)
    pos_o, L_o = eye_reference(rb, d, np.zeros(len(rr), bool), eta_o, cost_o)
    fpos = np.abs(rb["pos"] - pos_o).max() / M.EXTENT
    fL = np.abs(rb["dl"][:, 0] / L_o - 1.0).max()
    pos, L = eye_reference(ra, d, refl, eta, cost)
    T = np.where(refl, 1.0, eta * eta)
    epos = np.abs(ra["pos"] - pos)[sure].max() / M.EXTENT
    kd = ca.record_albedo().astype(np.float64)
    eT = np.abs(kd / T[:, None] - 1.0)[sure].max()
    fT = np.abs((R.fresnel(d[:, 2], index, np.float32)[1].astype(np.float64) ** 2) / (eta * eta) - 1.0).max()
    tr = sure & ~refl
    eL = np.abs(ra["dl"][tr] / (T[tr] * L[tr])[:, None] - 1.0).max()
    print(f"{sure.sum()} records, {refl[sure].sum()} reflected; position {epos:.3g} (floor {fpos:.3g}), "
          f"factor {eT:.3g} (floor {fT:.3g}), dl {eL:.3g} (floor {fL:.3g})")
    assert epos <= bound(fpos) and eT <= bound(fT) and eL <= bound(fL + fT)
    assert not ra["dl"][sure & refl].any()


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_render_cli")
SCENES = os.path.join(ROOT, "cuda-raytrace_amd", "scenes")


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = (int(v) for v in f.readline().split())
        scale = float(f.readline())
        data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4").reshape(h, w, 3)
    return data[::-1].astype(np.float32)


def test_scene_file_renders_the_python_scene(tmp_path):
    """caustic-fresnel.pbrt at 32 x 32 with 4 x 4 strata and 4,096 paths through pm_render_cli: bit for bit
    scenes.caustic_fresnel; with --specular reference bit for bit scenes.caustic_scene, and another image"""
    W = 32
    text = open(os.path.join(SCENES, "caustic-fresnel.pbrt")).read()
    text = text.replace('"integer xresolution" [256] "integer yresolution" [256]',
                        f'"integer xresolution" [{W}] "integer yresolution" [{W}]').replace('Include "', f'Include "{SCENES}/')
    assert f"[{W}]" in text and '"string specular" "pbrt"' in text
    scene = tmp_path / "cf.pbrt"
    scene.write_text(text)
    cam = dict(xsamples=4, ysamples=4, jitter=False, sample_seed=0, filter="box", filter_kw=dict(xwidth=0.5, ywidth=0.5))
    p = RenderParams.defaults(paths_per_pass=PATHS, passes=1)
    imgs = {}
    for mode, fn in (("pbrt", scenes.caustic_fresnel), ("reference", scenes.caustic_scene)):
        out = tmp_path / f"{mode}.pfm"
        flags = [] if mode == "pbrt" else ["--specular", "reference"]
        r = subprocess.run([CLI, "--pbrt", str(scene), "--paths", str(PATHS), "--passes", "1", "--spp", "4x4", "--no-jitter",
                            "--out", str(out), *flags], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        sc = fn(W, W)
        sc.camera = scenes.device_camera(W, W, **cam)
        img, _ = sc.load_into(hip.Context(0)).render(p)
        imgs[mode] = read_pfm(out)
        assert_bitexact(imgs[mode], img, f"pm_render_cli ({mode}) against the Python scene")
        assert np.isfinite(img).all() and (img >= 0).all() and img.max() > 0
    assert not np.array_equal(imgs["pbrt"], imgs["reference"])


HOST = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_pbrt_host")


def test_plugin_renders_the_python_scene(tmp_path):
    """the same scene built from pbrt objects (pm_pbrt_host --caustic: GlassMaterial, MirrorMaterial, two
    Spheres) with Renderer "cuda" "string specular" "pbrt": bit for bit scenes.caustic_fresnel on the host's
    own rays and light randoms; with "reference", or without the key, bit for bit scenes.caustic_scene"""
    from test_pbrt_boundary import read_host_output
    w = h = 32
    p = RenderParams.defaults(paths_per_pass=PATHS)
    imgs = {}
    for mode, flags, fn in (("pbrt", ["--specular", "pbrt"], scenes.caustic_fresnel),
                            ("reference", ["--specular", "reference"], scenes.caustic_scene),
                            ("absent", [], scenes.caustic_scene)):
        hout = tmp_path / f"{mode}.bin"
        r = subprocess.run([HOST, "--width", str(w), "--height", str(h), "--paths", str(PATHS), "--caustic", *flags,
                            "--out", str(hout)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        rays, rand2d, n2d, written, img = read_host_output(hout, w, h)
        sc = fn(w, h)
        sc.camera = ("rays", rays.copy(), rand2d.copy(), n2d)
        ref, _ = sc.load_into(hip.Context(0)).render(p)
        assert (ref > 0).any() and np.isfinite(ref).all()
        assert_bitexact(img, ref.reshape(-1, 3), f"pm_pbrt_host --caustic ({mode}) against the Python scene")
        imgs[mode] = img
    assert not np.array_equal(imgs["pbrt"], imgs["reference"]) and np.array_equal(imgs["reference"], imgs["absent"])


def test_caustic_fresnel_renders():
    p = RenderParams.defaults(paths_per_pass=PATHS, passes=1)
    W = 32
    new_s, old_s = scenes.caustic_fresnel(W, W), scenes.caustic_scene(W, W)
    ctx = new_s.load_into(hip.Context(0))
    img, st = ctx.render(p)
    ref, _ = old_s.load_into(hip.Context(0)).render(p)
    assert np.isfinite(img).all() and (img >= 0).all() and img.max() > 0
    assert not np.array_equal(img, ref)
    spec = ctx.scene_section("mat_spec").reshape(-1, 8)
    rows = spec[spec.view(np.int32)[:, 7] == 1]
    assert_bitexact(rows[:, :7], np.float32([[1, 1, 1, 1.5, 1, 1, 1], [0.9, 0.9, 0.9, 0, 0, 0, 0]]), "PM_SCENE_MAT_SPEC")
    knn, _ = ctx.render(RenderParams.defaults(paths_per_pass=PATHS, passes=1, estimator=PM_ESTIMATOR_KNN,
                                              gather_structure=PM_GATHER_GRID, knn_lookup=8))
    assert np.isfinite(knn).all() and (knn >= 0).all() and knn.max() > 0
    multi, _ = new_s.load_into(hip.Context(devices=[0])).render(p)
    assert_bitexact(multi, img, "one-context multi-device render on one device")
