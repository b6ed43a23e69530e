"""The caustic map of final gathering on the GPU (pm_set_caustic_map, pm_build_caustic_map, pm_caustic_gather,
the resolve with Lc). The yardsticks are independent of the marking code:

 - marking: the twin scene with every matte Kd = 0, where a path ends at its first diffuse hit, so the valid
   slots of its plain trace are exactly the L S+ D deposits (emission and the specular chain read no Kd);
 - the map: numpy's cell keys of the marked slots on tests/pass_plan_ref.py's grid;
 - the lookup: the ordinary bucket build and kNN gather of a second context over the marked slots alone;
 - the resolve: the numpy float32 restatement of the formula in pm_api.h.

Small shapes: 32 x 32 records, 4,096 paths of at most 4 photons, 8 photons looked up, 4 gather rays, two passes.
"""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import fgather_ref as G
import pass_plan_ref as PP
import ray_query_ref as Q
from pmrender import hip, scenes
from pmrender.abi import PM_ERR_INVALID, PM_ESTIMATOR_KNN, PM_GATHER_KDTREE, PM_GLASS, PM_MATTE, RenderParams

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
W = H = 32
PATHS, MPC, KNN, NG, PASSES = 4096, 4, 8, 4, 2
NSLOTS = PATHS * MPC
INV_PI = F32(0.31830988618379067154)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def params(**kw):
    return RenderParams.defaults(**{**dict(paths_per_pass=PATHS, passes=PASSES, max_photon_count=MPC, knn_lookup=KNN,
                                           initial_radius2=2500.0, estimator=PM_ESTIMATOR_KNN), **kw})


def scene_c(pad=0):
    """C: the caustic scene — a glass and a mirror sphere over the matte floor of the Cornell box, disk light —
    padded with small grey spheres outside the view to reach the LDS and HBM traversal modes"""
    s = scenes.caustic_scene(W, H)
    s.camera = scenes.pinhole(W, H)
    grey = s.material(PM_MATTE, (0.5, 0.5, 0.5))
    for r, w2o in Q.padding_spheres(pad):
        o2w = np.eye(4, dtype=np.float32)
        o2w[:3, 3] = -w2o[:3, 3]
        s.spheres.append((r, o2w.reshape(-1), w2o.reshape(-1), grey, -1))
    return s


def instanced_c():
    """the instanced test scene (a mirror figure among matte ones) at this file's shape"""
    s = scenes.instanced_scene(W, H, subdiv=2)
    s.camera = scenes.pinhole(W, H)
    return s


def black_twin(s):
    """C0: the same scene with every matte Kd = 0"""
    mats = [(t, np.zeros(3, np.float32) if t == PM_MATTE else rgb) for t, rgb in s.materials]
    return dataclasses.replace(s, materials=mats)


def open_ctx(scene, caustic=False, instancing=True):
    ctx = scene.load_into(hip.Context(0), instancing=instancing)
    if caustic:
        ctx.set_caustic_map(True)
    return ctx


def traced(scene, p, pass_=0, caustic=False, instancing=True):
    ctx = open_ctx(scene, caustic, instancing)
    try:
        ctx.trace_photons(p, pass_)
        return ctx.download_slots(NSLOTS), ctx.scene_info()["mode"]
    finally:
        ctx.close()


def same_photons(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("p", "alpha", "wi"))


# ------------------------------------------------------------------ 1. marking against the independent twin
def check_marking(scene, p, want_mode, instancing=True, twin_instancing=True):
    c, mode = traced(scene, p, caustic=True, instancing=instancing)
    c0, _ = traced(black_twin(scene), p, instancing=twin_instancing)
    assert mode == want_mode
    assert set(np.unique(c["bits"])) <= {0, 1, 3} and set(np.unique(c0["bits"])) <= {0, 1}
    marked, twin = (c["bits"] & 2) != 0, (c0["bits"] & 1) != 0
    slot0 = (np.arange(NSLOTS) % MPC) == 0
    unmarked_slot0 = slot0 & ((c["bits"] & 1) != 0) & ~marked
    print(f"{want_mode}: {int(marked.sum())} marked, {int(unmarked_slot0.sum())} unmarked slot-0 deposits")
    assert marked.any() and unmarked_slot0.any(), "the scene and seed must give both"
    bad = np.nonzero(marked != twin)[0]
    assert bad.size == 0, f"{bad.size} slots differ, first {bad[:8]}"
    assert same_photons(c[marked], c0[twin])
    return c


def test_marking_brute_and_the_oracle_condition(oracle_mod):
    """the brute-force scene; and, on the CPU oracle, that scene and seed give both kinds of slot-0 deposit"""
    p = params()
    sc = scene_c()
    orc = sc.load_into(oracle_mod.Oracle(nthreads=4)).trace_photons(p, 0)
    orc0 = black_twin(sc).load_into(oracle_mod.Oracle(nthreads=4)).trace_photons(p, 0)
    twin = (orc0["bits"] & 1) != 0
    slot0 = (np.arange(NSLOTS) % MPC) == 0
    assert twin.any() and not twin[~slot0].any(), "C0's deposits are slot-0 deposits"
    assert (slot0 & ((orc["bits"] & 1) != 0) & ~twin).any(), "C has slot-0 deposits that are no caustic photons (L D D)"
    c = check_marking(sc, p, "brute")
    # the device's marked set is the oracle's twin set, photon for photon
    assert np.array_equal((c["bits"] & 2) != 0, twin) and same_photons(c[twin], orc0[twin])


@pytest.mark.parametrize("mode,pad", [("bvh-lds", 66), ("bvh-hbm", 300)], ids=("lds", "hbm"))
def test_marking_traversal_modes(mode, pad):
    check_marking(scene_c(pad), params(), mode)


def test_marking_per_lane_on_the_wide_tree(monkeypatch):
    """PM_TRACE_POOL=0: the HBM scene through the per-lane kernel instead of the pooled one"""
    monkeypatch.setenv("PM_TRACE_POOL", "0")
    check_marking(scene_c(300), params(), "bvh-hbm")


def test_marking_on_the_eight_wide_tree(monkeypatch):
    """PM_BVH8=1: the HBM scene over the 8-wide tree (k_trace_pool8's marked twin)"""
    monkeypatch.setenv("PM_BVH8", "1")
    check_marking(scene_c(300), params(), "bvh-hbm")


def test_marking_instanced_against_its_flattened_twin():
    sc, p = instanced_c(), params()
    a = check_marking(sc, p, "bvh-instanced", twin_instancing=False)
    flat, mode = traced(sc, p, caustic=True, instancing=False)
    assert mode != "bvh-instanced" and a.tobytes() == flat.tobytes()


def test_marking_every_light():
    """PM_ALL_LIGHTS (the ALL instantiations): a point light beside the disk"""
    sc = scene_c()
    sc.lights.append(("point", np.float32([150.0, 400.0, 200.0]), np.float32([60000.0, 60000.0, 60000.0])))
    check_marking(sc, params(light_source_index=-1), "brute")


# ------------------------------------------------------------------ 2. marking on against off
def full_map_state(scene, p, caustic):
    ctx = open_ctx(scene, caustic)
    try:
        ctx.eye_pass(p)
        ctx.trace_photons(p, 0)
        ctx.build_photon_map(p)
        ctx.gather(p)
        return ctx.download_slots(NSLOTS), ctx.map_info(), ctx.download_records()
    finally:
        ctx.close()


@pytest.mark.parametrize("pad", (0, 300), ids=("brute", "hbm"))
def test_marking_changes_nothing_else(pad):
    """Slots equal after clearing bit 1. The full map's keys and cell_start are functions of the slots' positions
    and the grid, so they follow (the counts are compared through pm_map_info); its ranks are atomic arrival order
    within a cell, which differs from run to run on any build. What the ranks must keep — every cell holding its
    own photons — is held through the device: the kNN gather over the full map gives the same records, bit for bit."""
    p, sc = params(), scene_c(pad)
    on, info_on, recs_on = full_map_state(sc, p, True)
    off, info_off, recs_off = full_map_state(sc, p, False)
    assert (on["bits"] & 2).any() and not (off["bits"] & 2).any()
    cleared = on.copy()
    cleared["bits"] &= ~np.uint32(2)
    assert cleared.tobytes() == off.tobytes()
    assert info_on == info_off and info_on["valid"] == int((off["bits"] & 1).sum())
    assert (recs_on["photon_count"] > 0).any() and recs_on.tobytes() == recs_off.tobytes()


def test_no_specular_material_marks_nothing():
    sc = scenes.cornell_box(W, H)
    slots, _ = traced(sc, params(), caustic=True)
    assert (slots["bits"] & 1).any() and not (slots["bits"] & 2).any()
    plain, _ = traced(sc, params())
    assert slots.tobytes() == plain.tobytes()


# ------------------------------------------------------------------ 3. the map
def cell_keys(scene, p, pos):
    lo, hi = PP.scene_bbox(scene)
    dx, dy, dz, ncells, inv_bits = PP.make_grid(lo, hi, PM_ESTIMATOR_KNN, 2, p.initial_radius2)
    inv = PP.from_bits(inv_bits)
    c = [np.clip(np.floor((pos[:, a].astype(F32) - F32(lo[a])) * inv).astype(np.int64), 0, d - 1)
         for a, d in enumerate((dx, dy, dz))]
    return (c[2] * dy + c[1]) * dx + c[0], ncells


def test_map_is_the_marked_slots_cell_by_cell():
    p, sc = params(), scene_c()
    ctx = open_ctx(sc, True)
    try:
        ctx.trace_photons(p, 0)
        ctx.build_photon_map(p)
        ctx.build_caustic_map()
        slots = ctx.download_slots(NSLOTS)
        marked = np.nonzero(slots["bits"] & 2)[0]
        assert ctx.caustic_map_count() == marked.size > 0
        order, cs = ctx.caustic_slots(), ctx.caustic_cell_start()
        assert np.array_equal(np.sort(order), marked), "a permutation of the marked slots"
        keys, ncells = cell_keys(sc, p, slots["p"][order])
        assert len(cs) == ncells + 1 == ctx.map_info()["cells"] + 1 and cs[-1] == marked.size
        want = np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=ncells))])
        assert np.array_equal(cs, want), "cell_start is the scan of the marked slots' cell counts"
        assert (np.diff(keys) >= 0).all(), "cell-contiguous: entry i lies in the cell whose range holds i"
        # a second build: the same set per cell (the order inside a cell is atomic arrival order)
        ctx.build_caustic_map()
        again, cs2 = ctx.caustic_slots(), ctx.caustic_cell_start()
        assert np.array_equal(cs, cs2)
        assert all(np.array_equal(np.sort(order[a:b]), np.sort(again[a:b])) for a, b in zip(cs[:-1], cs[1:]) if b > a)
        # and the full map still holds every valid photon
        assert ctx.map_info()["valid"] == int((slots["bits"] & 1).sum()) > marked.size
    finally:
        ctx.close()


# ------------------------------------------------------------------ 4. the lookup
def test_lookup_equals_the_ordinary_gather_over_the_marked_slots():
    p, sc = params(), scene_c()
    A, B = open_ctx(sc, True), open_ctx(sc)
    try:
        A.eye_pass(p)
        B.eye_pass(p)
        for k in range(PASSES):
            A.trace_photons(p, k)
            A.build_photon_map(p)
            A.build_caustic_map()
            A.caustic_gather(p, k)
            slots = A.download_slots(NSLOTS)
            only = slots.copy()
            only[(slots["bits"] & 2) == 0] = 0
            B.upload_slots(only)
            B.build_photon_map(p)
            B.gather(p)
            a, b = A.download_records(), B.download_records()
            assert (a["photon_count"] > 0).any(), k
            for f in ("flux", "radius2", "photon_count"):
                assert np.array_equal(bits(a[f]), bits(b[f])), (k, f)
            assert a.tobytes() == b.tobytes()
    finally:
        A.close(); B.close()


# ------------------------------------------------------------------ 5. the resolve
def kd_of(scene, recs):
    kd = np.zeros((len(recs), 3), np.float32)
    for i, r in enumerate(recs):
        if not (r["flags"] & G.INACTIVE):
            t, rgb = scene.materials[int(r["material"])]
            kd[i] = rgb if t == PM_MATTE else 0
    return kd


def caustic_radiance32(recs, kd, emitted):
    """Lc_r = (flux_r * (1 / emitted)) * (Kd_r * (1 / pi)) per channel in float32; 0 for an inactive record"""
    inv = F32(1.0) / F32(emitted)
    with np.errstate(all="ignore"):
        lc = ((recs["flux"].astype(F32) * inv).astype(F32) * (kd * INV_PI).astype(F32)).astype(F32)
    lc[(recs["flags"] & G.INACTIVE) != 0] = 0
    return lc


def resolve_caustic32(recs, kd, lc, acc, n, passes):
    """out_r = (dl_r + Lc_r) + Kd_r x (A_r / (float)(N P)), sanitised; inactive records black"""
    with np.errstate(all="ignore"):
        out = ((recs["dl"].astype(F32) + lc).astype(F32) + (kd * (np.asarray(acc, F32) / F32(n * passes))).astype(F32)).astype(F32)
    out = G.sanitize32(out)
    out[(recs["flags"] & G.INACTIVE) != 0] = 0
    return out


def raster(ctx, per_record):
    pix = ctx.record_pixels()
    ok = pix >= 0
    img = np.zeros((W * H, 3), np.float32)
    img[pix[ok]] = per_record[ok]
    return img.reshape(H, W, 3)


def staged(scene, p, caustic):
    """the stage calls of pm_render_final_gather: (context, image, records, A, Lc or None)"""
    ctx = open_ctx(scene, caustic)
    ctx.eye_pass(p)
    for k in range(p.passes):
        ctx.trace_photons(p, k)
        ctx.build_photon_map(p)
        ctx.final_gather_pass(p, NG, k)
        if caustic:
            ctx.build_caustic_map()
            ctx.caustic_gather(p, k)
    img = ctx.final_gather_resolve()
    return ctx, img, ctx.download_records(), ctx.gather_sum(), (ctx.caustic_radiance() if caustic else None)


@pytest.fixture(scope="module")
def rendered():
    """scene C through the stage calls with the switch on and off, shared by the resolve and the feature tests"""
    p, sc = params(), scene_c()
    on = staged(sc, p, True)
    off = staged(sc, p, False)
    yield p, sc, on, off
    on[0].close(); off[0].close()


def test_resolve_is_the_formula(rendered):
    p, sc, (ctx, img, recs, acc, lc), _ = rendered
    kd = kd_of(sc, recs)
    want_lc = caustic_radiance32(recs, kd, PASSES * PATHS)
    assert np.array_equal(bits(lc), bits(want_lc)) and (lc > 0).any()
    want = raster(ctx, resolve_caustic32(recs, kd, want_lc, acc, NG, PASSES))
    assert np.array_equal(bits(img), bits(want))
    whole, st = ctx.render_final_gather(p, NG)
    assert np.array_equal(bits(whole), bits(img)) and st["ms_gather"] > 0
    assert ctx.timing_total("caustic")[0] >= 2 * PASSES, "the render reports its two stages per pass as \"caustic\""


def test_switch_off_is_the_parent_image(rendered):
    """pm_render_final_gather with the switch off (never set, and set then cleared) equals the image of the stage
    calls as they were before the caustic map existed, restated in numpy from their sums"""
    p, sc, _, (ctx, img, recs, acc, _) = rendered
    want = raster(ctx, G.resolve32(recs, kd_of(sc, recs), acc, NG, PASSES))
    assert np.array_equal(bits(img), bits(want))
    whole, _ = ctx.render_final_gather(p, NG)
    assert np.array_equal(bits(whole), bits(img))
    ctx.set_caustic_map(True)
    ctx.set_caustic_map(False)
    again, _ = ctx.render_final_gather(p, NG)
    assert np.array_equal(bits(again), bits(img))
    slots = ctx.download_slots(NSLOTS)
    assert not (slots["bits"] & 2).any()


def test_secondary_hits_keep_the_full_map(rendered):
    """the gather rays' sums A do not depend on the switch: L S+ D D E stays indirect light"""
    _, _, on, off = rendered
    assert np.array_equal(bits(on[3]), bits(off[3])) and (on[3] > 0).any()


# ------------------------------------------------------------------ 6. the feature shows
def test_the_caustic_shows_under_the_glass(rendered):
    p, sc, (ctx, img_on, recs, _, lc), (_, img_off, *_) = rendered
    glass = next(s for s in sc.spheres if sc.materials[s[3]][0] == PM_GLASS)
    centre = -np.asarray(glass[2], np.float64).reshape(4, 4)[:3, 3]
    pos = recs["pos"].astype(np.float64)
    active = (recs["flags"] & G.INACTIVE) == 0
    matte = np.array([sc.materials[int(m)][0] == PM_MATTE for m in recs["material"]])
    floor = active & matte & (np.abs(pos[:, 1]) < 1.0) & (np.hypot(pos[:, 0] - centre[0], pos[:, 2] - centre[2]) < 2.0 * float(glass[0]))
    assert floor.sum() >= 8, "the floor under the glass sphere is in view"
    mean_lc = float(lc[floor].mean())
    pix = ctx.record_pixels()[floor]
    on_mean = float(img_on.reshape(-1, 3)[pix].mean())
    off_mean = float(img_off.reshape(-1, 3)[pix].mean())
    print(f"{int(floor.sum())} floor records under the glass: mean Lc {mean_lc:.5g}, image {off_mean:.5g} -> {on_mean:.5g}")
    assert mean_lc > 0 and on_mean > off_mean


# ------------------------------------------------------------------ 7. refusals
@pytest.mark.parametrize("name", ("group", "kdtree", "textured", "specular", "textured trace", "build off", "build no map",
                                  "gather off", "gather no map", "gather other radius", "gather continues",
                                  "gather no eye pass", "resolve passes"))
def test_refusals(name):
    word = {"group": "multi-device", "kdtree": "PM_GATHER_KDTREE", "textured": "textured", "specular": "specular",
            "textured trace": "textured", "build off": "is off", "build no map": "no photon map", "gather off": "is off",
            "gather no map": "no caustic map", "gather other radius": "initial_radius2", "gather continues": "continues",
            "gather no eye pass": "pm_eye_pass", "resolve passes": "1 of the 2"}[name]
    p = params()
    sc = scene_c()
    if name in ("textured", "textured trace"):
        sc = scenes.cornell_textured(W, H)
    elif name == "specular":
        sc = scenes.caustic_fresnel(W, H)
    ctx = hip.Context(0, devices=[0, 0] if name == "group" else None)
    try:
        if name == "textured trace":
            ctx.set_caustic_map(True)  # before the commit: the trace refuses
        sc.load_into(ctx)
        with pytest.raises(hip.PMError) as e:
            if name in ("group", "textured", "specular"):
                ctx.set_caustic_map(True)
            elif name == "textured trace":
                ctx.trace_photons(p, 0)
            elif name == "kdtree":
                ctx.set_caustic_map(True)
                ctx.trace_photons(params(gather_structure=PM_GATHER_KDTREE, estimator=0), 0)
            elif name == "build off":
                ctx.trace_photons(p, 0)
                ctx.build_photon_map(p)
                ctx.build_caustic_map()
            elif name == "build no map":
                ctx.set_caustic_map(True)
                ctx.trace_photons(p, 0)
                ctx.build_caustic_map()
            else:
                if name != "gather no eye pass":
                    ctx.eye_pass(p)
                ctx.set_caustic_map(name != "gather off")
                ctx.trace_photons(p, 0)
                ctx.build_photon_map(p)
                if name not in ("gather off", "gather no map"):
                    ctx.build_caustic_map()
                if name == "gather other radius":
                    ctx.caustic_gather(params(initial_radius2=100.0), 0)
                elif name == "gather continues":
                    ctx.caustic_gather(p, 1)
                elif name == "resolve passes":
                    ctx.final_gather_pass(p, NG, 0)
                    ctx.caustic_gather(p, 0)
                    ctx.final_gather_pass(p, NG, 1)
                    ctx.final_gather_resolve()
                else:
                    ctx.caustic_gather(p, 0)
        assert e.value.code == PM_ERR_INVALID and word in str(e.value), str(e.value)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 8. front ends
CLI = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_render_cli")
HOST = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_pbrt_host")
SCENES = os.path.join(ROOT, "cuda-raytrace_amd", "scenes")


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = (int(v) for v in f.readline().split())
        scale = float(f.readline())
        data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4").reshape(h, w, 3)
    return data[::-1].astype(np.float32)


def test_front_ends_switch_it_on(tmp_path):
    """pm_render_cli on caustic-glass.pbrt at 32 x 32 with --final-gather 4: --caustic-map and the Renderer key give
    one image, which differs from the image without them; pm_pbrt_host --caustic-map changes its image too"""
    text = open(os.path.join(SCENES, "caustic-glass.pbrt")).read()
    text = text.replace('Include "', f'Include "{SCENES}/')
    import re
    text, n = re.subn(r'"integer xresolution" \[\d+\] "integer yresolution" \[\d+\]',
                      f'"integer xresolution" [{W}] "integer yresolution" [{H}]', text)
    assert n == 1
    keyed, n = re.subn(r'(Renderer "cuda"[^\n]*)', r'\1 "integer finalgathersamples" [4] "bool causticmap" ["true"]', text, count=1)
    assert n == 1
    (tmp_path / "plain.pbrt").write_text(text)
    (tmp_path / "key.pbrt").write_text(keyed)
    imgs = {}
    for name, scene, extra in (("off", "plain", ["--final-gather", "4"]), ("flag", "plain", ["--final-gather", "4", "--caustic-map"]),
                               ("key", "key", [])):
        out = tmp_path / f"{name}.pfm"
        r = subprocess.run([CLI, "--pbrt", str(tmp_path / f"{scene}.pbrt"), "--paths", str(PATHS), "--out", str(out), *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        imgs[name] = read_pfm(out)
    assert np.array_equal(bits(imgs["flag"]), bits(imgs["key"])) and imgs["off"].max() > 0
    assert not np.array_equal(bits(imgs["flag"]), bits(imgs["off"])) and imgs["flag"].sum() > imgs["off"].sum()
    host = {}
    for name, extra in (("off", []), ("on", ["--caustic-map"])):
        out = tmp_path / f"host_{name}.bin"
        r = subprocess.run([HOST, "--width", str(W), "--height", str(H), "--paths", str(PATHS), "--out", str(out),
                            "--final-gather", "4", "--caustic", *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        host[name] = open(out, "rb").read()
    # the same rays and samples in front, another image behind them
    assert len(host["on"]) == len(host["off"]) and host["on"] != host["off"]
    n = W * H * 3 * 4
    assert host["on"][:-n] == host["off"][:-n]
