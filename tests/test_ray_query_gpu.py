"""Directed ray-query tests: every traversal mode (brute pair loop, binary LDS
tree, quantized 4-wide tree, 8-wide tree, two-level instance walk, the pooled
resumable walk of the photon trace) on rays aimed where they can part company,
against brute force bit for bit and against the float64 reference of
ray_query_ref.py.

The probe: Context.set_eye_rays + eye_pass + download_records is a closest-hit
query (every test triangle is its own mesh with its own matte material, so the
record's material index names the primitive hit, its position gives t), and
with one point light dl != 0 exactly when the shadow ray from the recorded
point found no occluder, an any-hit query. trace_photons + download_slots is
the photon side.

Every case asserts scene_info()["mode"], so none can pass in the wrong mode.
"""
import functools

import numpy as np
import pytest

import mesh_light_ref as R
import ray_query_ref as Q
from pmrender import scenes
from pmrender.abi import PM_MATTE, PM_REC_EXCEPTION, PM_REC_INVALID, PM_REC_MISS, RenderParams

pytestmark = pytest.mark.gpu

HBM_PAD = 300          # padding spheres that push any case past the LDS budget
PATHS = 2048


def lds_pad(case):
    """padding that makes the primitive count 65, the first past BRUTE_MAX_PRIMS"""
    return max(0, 65 - case.n_prims())


def build(case, order=None, pad=0, inst=None, obj_tris=None, normals=None):
    """The case as a Scene: material k belongs to primitive k (triangles in
    canonical order, then disks, then spheres), whatever `order` the triangle
    meshes are inserted in; the padding shares one more material. inst: (o2w,
    w2o) — every triangle becomes an object mesh of its own (obj_tris: their
    object-space vertices) under that transform."""
    s = scenes.Scene()
    n = case.n_prims()
    for _ in range(n + 1):
        s.material(PM_MATTE, (0.5, 0.5, 0.5))
    nt = len(case.tris)
    for k in (range(nt) if order is None else order):
        P = case.tris[k] if obj_tris is None else obj_tris[k]
        N = None if normals is None else np.ascontiguousarray(normals[k], np.float32)
        mesh = dict(P=np.ascontiguousarray(P, np.float32), idx=np.int32([[0, 1, 2]]), N=N, uv=None, material=int(k), light=-1)
        if inst is None:
            s.meshes.append(mesh)
        else:
            s.objects.append(mesh)
            s.instances.append((len(s.objects) - 1, *inst))
    for j, d in enumerate(case.disks):
        s.disks.append((*d, nt + j, -1))
    spheres = [(sp, nt + len(case.disks) + j) for j, sp in enumerate(case.spheres)] + [(sp, n) for sp in Q.padding_spheres(pad)]
    for (r, w2o), mat in spheres:
        o2w = np.eye(4, dtype=np.float32)
        o2w[:3, 3] = -np.asarray(w2o, np.float32).reshape(4, 4)[:3, 3]
        s.spheres.append((np.float32(r), o2w.reshape(-1), np.asarray(w2o, np.float32).reshape(-1), mat, -1))
    s.lights.append(("point", case.light, np.float32([1.0, 1.0, 1.0])))
    s.camera = ("rays", case.rays, None, 0)
    return s


def params(**kw):
    return RenderParams.defaults(scene_epsilon=Q.EPS, **kw)


def eye_records(hip_mod, scene, mode, instancing=True):
    ctx = scene.load_into(hip_mod.Context(0), instancing=instancing)
    try:
        assert ctx.scene_info()["mode"] == mode, (ctx.scene_info(), mode)
        ctx.eye_pass(params())
        return ctx.download_records()
    finally:
        ctx.close()


def first_deposits(hip_mod, scene, mode):
    ctx = scene.load_into(hip_mod.Context(0))
    try:
        assert ctx.scene_info()["mode"] == mode, (ctx.scene_info(), mode)
        ctx.trace_photons(params(paths_per_pass=PATHS), 0, 0, PATHS)
        return ctx.download_slots(PATHS * 4)
    finally:
        ctx.close()


def assert_same_bits(a, b, what):
    a8 = np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)
    b8 = np.ascontiguousarray(b).view(np.uint8).reshape(len(b), -1)
    bad = np.flatnonzero((a8 != b8).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(a)} differ, first at {bad[:8]}"


def mode_records(hip_mod, monkeypatch, case, order=None, want=("brute", "bvh-lds", "bvh-hbm", "bvh8", "bvh-instanced"),
                 normals=None):
    """records of the case in each traversal mode it can be built in"""
    out = {}
    build = functools.partial(globals()["build"], normals=normals)
    monkeypatch.delenv("PM_BVH8", raising=False)
    if "brute" in want and case.n_prims() <= 64:
        out["brute"] = eye_records(hip_mod, build(case, order), "brute")
    if "bvh-lds" in want:
        out["bvh-lds"] = eye_records(hip_mod, build(case, order, lds_pad(case)), "bvh-lds")
    if "bvh-hbm" in want:
        out["bvh-hbm"] = eye_records(hip_mod, build(case, order, HBM_PAD), "bvh-hbm")
    if "bvh-instanced" in want and not case.disks and not case.spheres:
        ident = (np.eye(4, dtype=np.float32).reshape(-1), np.eye(4, dtype=np.float32).reshape(-1))
        out["bvh-instanced"] = eye_records(hip_mod, build(case, order, inst=ident), "bvh-instanced")
    if "bvh8" in want:
        monkeypatch.setenv("PM_BVH8", "1")
        out["bvh8"] = eye_records(hip_mod, build(case, order, HBM_PAD), "bvh-hbm")
        monkeypatch.delenv("PM_BVH8")
    return out


@functools.lru_cache(maxsize=None)
def answer(make, *args):
    """(case, its reference answer with the largest padding in the scene)"""
    case = make(*args)
    ans = Q.query(case.prims(HBM_PAD), case.rays, Q.EPS, Q.TMAX)
    npr = case.n_prims()
    assert not (ans.state[:, npr:] != Q.SURE_MISS).any(), "a ray reaches the padding"
    return case, ans


def hit_ids(case, recs):
    flags = recs["flags"]
    assert not (flags & (PM_REC_EXCEPTION | PM_REC_INVALID)).any()
    miss = (flags & PM_REC_MISS) != 0
    got = np.where(miss, Q.MISS, recs["material"])
    assert got.max() < case.n_prims(), "a ray hit the padding"
    return got


def check_reference(case, ans, recs, label):
    """the assertions every record gets against the float64 reference"""
    n, npr = len(case.rays), case.n_prims()
    got = hit_ids(case, recs)
    col = np.where(got < 0, ans.cand.shape[1] - 1, got)
    in_set = ans.cand[np.arange(n), col]
    assert in_set.all(), f"{label}: {(~in_set).sum()} answers outside the candidate set, first {np.flatnonzero(~in_set)[:8]}"
    dec = ans.decided
    wrong = dec & (got != ans.hit)
    assert not wrong.any(), f"{label}: {wrong.sum()} decided rays differ from the reference, first {np.flatnonzero(wrong)[:8]}"
    hit = dec & (got >= 0)
    o, d = case.rays[:, :3].astype(np.float64), case.rays[:, 3:].astype(np.float64)
    pos = recs["pos"].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t_rec = np.sum((pos - o) * d, axis=1) / np.sum(d * d, axis=1)
        off = np.abs(t_rec - ans.t_hit)
        late = hit & ~(off <= ans.mt_hit)
    assert not late.any(), f"{label}: t off by up to {off[late].max():.3g} (bound {ans.mt_hit[late].min():.3g})"
    if not case.shadow:
        return
    # the shadow ray of every hit record, from the recorded fp32 point
    h = np.flatnonzero(got >= 0)
    p32 = recs["pos"][h]
    sray = np.concatenate([p32, case.light[None, :] - p32], axis=1).astype(np.float32)
    sh = Q.query(case.prims(0), sray, float(np.float32(0.001)), float(np.float32(1.0) - np.float32(0.001)))
    lit = (recs["dl"][h] != 0).any(axis=1)
    bad = (sh.occluded_sure & lit) | (sh.clear_sure & ~lit)
    assert not bad.any(), (f"{label}: {bad.sum()} shadow answers differ from the reference "
                           f"({(sh.occluded_sure | sh.clear_sure).sum()} decided), first records {h[bad][:8]}")


def check_modes(case, ans, recs, base=None):
    base = base or ("brute" if "brute" in recs else sorted(recs)[0])
    for mode, r in recs.items():
        assert_same_bits(r, recs[base], f"{case.name}: records, {mode} vs {base}")
    check_reference(case, ans, recs[base], f"{case.name} ({base})")


# ------------------------------------------------------------------ group 1
def test_control_every_mode(hip_mod, monkeypatch):
    case, ans = answer(Q.control_case)
    assert 1.0 - ans.decided.mean() <= case.cap
    recs = mode_records(hip_mod, monkeypatch, case)
    assert set(recs) == {"brute", "bvh-lds", "bvh-hbm", "bvh8", "bvh-instanced"}
    check_modes(case, ans, recs)


def test_instances_rotated_and_scaled(hip_mod):
    """one object per triangle under a rotated, non-uniformly scaled transform:
    the two-level walk equals the flattened scene's records bit for bit, and
    the reference on the flattened world-space triangles"""
    obj = Q.grid_triangles(seed=13)
    xf = scenes.affine(30.0, 20.0, (1.3, 0.7, 1.1), (0.2, -0.1, 0.3))
    shell = Q.Case("shell", obj, np.zeros((1, 6)))
    s = build(shell, inst=xf, obj_tris=obj)
    world = np.stack([s.flattened(k)["P"] for k in range(len(obj))])
    case = Q.Case("instanced", world, Q.mixed_rays(world, 3072, 17, lo=-0.4, size=2.2))
    ans = Q.query(case.prims(), case.rays, Q.EPS, Q.TMAX)
    s = build(case, inst=xf, obj_tris=obj)
    two_level = eye_records(hip_mod, s, "bvh-instanced")
    flat = eye_records(hip_mod, s, "brute", instancing=False)
    assert_same_bits(two_level, flat, "two-level vs flattened")
    check_reference(case, ans, flat, "instanced (flattened)")


# ------------------------------------------------------------------ group 2
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64])
def test_brute_counts_and_pair_positions(n, hip_mod):
    """odd / even counts, the scalar tail and the BRUTE_MAX_PRIMS boundary;
    every storage order gives the same record bits (no equal-t ties here, so
    the insertion order cannot matter)"""
    case, ans = answer(Q.count_case, n)
    base = eye_records(hip_mod, build(case), "brute")
    check_reference(case, ans, base, case.name)
    for order in storage_orders(n)[1:]:
        r = eye_records(hip_mod, build(case, order), "brute")
        assert_same_bits(r, base, f"{case.name}: storage order {order[:4]}...")


def storage_orders(n):
    """every rotation for an odd count (each triangle is lane x, lane y and
    the scalar tail in turn); for an even one the identity, one rotation and
    the reverse (each triangle is lane x and lane y)"""
    ident = list(range(n))
    if n % 2:
        return [ident[r:] + ident[:r] for r in range(n)]
    return [ident, ident[1:] + ident[:1], ident[::-1]]


@pytest.mark.parametrize("name", ["count3", "count63", "control"])
def test_shading_normals_follow_barycentrics(name, hip_mod, monkeypatch):
    """Distinct per-vertex normals: the recorded shading normal (and with it
    dl) depends on beta and gamma of the winning lane or tail. Bit-equal
    across storage orders and modes, and the float64 interpolation of the
    same normals within the reference's own barycentric margin."""
    case, ans = answer(Q.control_case) if name == "control" else answer(Q.count_case, int(name[5:]))
    N = Q.vertex_normals(case.tris)
    if name == "control":
        recs = mode_records(hip_mod, monkeypatch, case, normals=N)
        assert len(recs) == 5
    else:
        orders = storage_orders(len(case.tris))
        orders = orders if len(orders) <= 3 else orders[:2] + orders[len(orders) // 2:len(orders) // 2 + 2] + orders[-1:]
        recs = {f"order {o[:3]}": eye_records(hip_mod, build(case, o, normals=N), "brute") for o in orders}
    base = recs[sorted(recs)[0]] if "brute" not in recs else recs["brute"]
    for k, r in recs.items():
        assert_same_bits(r, base, f"{case.name} with vertex normals: {k}")
    got = hit_ids(case, base)
    hit = np.flatnonzero(ans.decided & (got >= 0) & (got == ans.hit))
    assert hit.size > len(case.rays) // 4
    P = case.tris.astype(np.float64)[got[hit]]
    L = np.maximum(np.maximum(np.linalg.norm(P[:, 1] - P[:, 0], axis=1), np.linalg.norm(P[:, 2] - P[:, 0], axis=1)),
                   np.linalg.norm(P[:, 2] - P[:, 1], axis=1))
    m = ans.mt_hit[hit] * np.linalg.norm(case.rays[hit, 3:].astype(np.float64), axis=1) / L   # >= the barycentric margin
    # each weight is off by <= 2 m, the three normals are unit vectors and their sum is longer than 1/2
    tol = 32.0 * m + 16 * Q.U
    ns_ref = Q.shading_normal(case.tris, N, case.rays[hit], got[hit])
    dev = np.abs(base["ns"][hit].astype(np.float64) - ns_ref).max(axis=1)
    tight = tol < 0.02          # the vertex normals of a triangle differ by ~0.5: grazing hits with a wider bound say nothing
    assert tight.sum() > hit.size // 2
    bad = tight & ~(dev <= tol)
    assert not bad.any(), f"{case.name}: {bad.sum()} shading normals off by up to {dev[bad].max():.3g} (bound {tol[bad].min():.3g})"


@pytest.mark.parametrize("n", [65, 66])
def test_first_counts_past_brute(n, hip_mod, monkeypatch):
    case, ans = answer(Q.count_case, n)
    recs = mode_records(hip_mod, monkeypatch, case, want=("bvh-lds", "bvh-hbm", "bvh8"))
    assert lds_pad(case) == 0 and set(recs) == {"bvh-lds", "bvh-hbm", "bvh8"}
    check_modes(case, ans, recs, base="bvh-lds")


# ------------------------------------------------------------------ group 3
def test_pair_slow_path_small(hip_mod, monkeypatch):
    """a triangle whose normal underflows 2^-125 as lane x, lane y and the
    scalar tail, a zero-area triangle beside it: the ordinary triangles return
    the bits they return without them, and neither is ever hit"""
    case, ans = answer(Q.slow_small_case)
    assert 1.0 - ans.decided.mean() <= case.cap
    n = len(case.tris)                       # 7: five ordinary, TINY (5), FLAT (6)
    plain = Q.Case("plain", case.tris[:5], case.rays)
    ref_bits = eye_records(hip_mod, build(plain), "brute")
    for order in ([5, 0, 1, 2, 3, 4, 6], [0, 5, 1, 2, 3, 4, 6], [0, 1, 2, 3, 6, 4, 5], [6, 5, 0, 1, 2, 3, 4], [0, 1, 5, 6, 2, 3, 4]):
        r = eye_records(hip_mod, build(case, order), "brute")
        got = hit_ids(case, r)
        assert not np.isin(got, (5, 6)).any(), "a degenerate triangle was hit"
        assert_same_bits(r, ref_bits, f"slow path, order {order}")
    check_modes(case, ans, mode_records(hip_mod, monkeypatch, case))


def test_pair_slow_path_huge(hip_mod):
    """normals above 2^125: the divide fallback keeps these hits (1 / den is
    subnormal there)"""
    case, ans = answer(Q.slow_huge_case)
    assert 1.0 - ans.decided.mean() <= case.cap
    base = eye_records(hip_mod, build(case), "brute")
    check_reference(case, ans, base, case.name)
    for order in ([1, 2, 0], [2, 0, 1]):
        assert_same_bits(eye_records(hip_mod, build(case, order), "brute"), base, f"huge, order {order}")


# ------------------------------------------------------------------ group 4
@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0), (1, 2, 0)])
def test_ties_lowest_id_wins(order, hip_mod, monkeypatch):
    case, ans = answer(Q.tie_case)
    recs = mode_records(hip_mod, monkeypatch, case, order)
    assert set(recs) == {"brute", "bvh-lds", "bvh-hbm", "bvh8"}
    check_modes(case, ans, recs)
    want = Q.tie_expected(case, order)
    for mode, r in recs.items():
        got = hit_ids(case, r)[:len(want)]
        bad = got != want
        assert not bad.any(), f"{mode}, order {order}: {bad.sum()} ties not won by the lowest id, first {np.flatnonzero(bad)[:8]}"


# ------------------------------------------------------------ groups 5 and 7
@pytest.mark.parametrize("make", [Q.axis_case, Q.grazing_case], ids=["axis", "grazing"])
def test_adversarial_rays(make, hip_mod, monkeypatch):
    case, ans = answer(make)
    recs = mode_records(hip_mod, monkeypatch, case)
    assert len(recs) == 5
    check_modes(case, ans, recs)


# ------------------------------------------------------------------ group 6
@pytest.mark.parametrize("dist", Q.FAR_DISTANCES)
def test_far_origins(dist, hip_mod, monkeypatch):
    case, ans = answer(Q.far_case, dist)
    recs = mode_records(hip_mod, monkeypatch, case)
    for mode, r in recs.items():
        diff = (r.view(np.uint8).reshape(len(r), -1) != recs["brute"].view(np.uint8).reshape(len(r), -1)).any(axis=1)
        print(f"far origins {dist:g}: {mode} differs from brute on {diff.sum()} of {len(r)} rays")
    assert len(recs) == 5
    check_modes(case, ans, recs)


def test_origin_domain(hip_mod, monkeypatch):
    """the modes agree up to the documented origin bound (2^20: the rays come
    from 2^19 away); origins beyond it and non-finite rays are rejected"""
    tris = Q.grid_triangles()
    case = Q.Case("far2^19", tris, Q.far_rays(tris, 512, 2.0 ** 19, 113))
    assert np.abs(case.rays[:, :3]).max() <= 2.0 ** 20
    ans = Q.query(case.prims(HBM_PAD), case.rays, Q.EPS, Q.TMAX)
    check_modes(case, ans, mode_records(hip_mod, monkeypatch, case))
    ctx = hip_mod.Context(0)
    try:
        for bad in (2.0 ** 20 + 1, np.inf, np.nan):
            rays = case.rays[:4].copy()
            rays[2, 1] = bad
            with pytest.raises(hip_mod.PMError):
                ctx.set_eye_rays(rays)
            with pytest.raises(hip_mod.PMError):
                ctx.set_pinhole(np.float32([0, bad, 0]), np.float32([0, 0, 1]), np.float32([1, 0, 0]), np.float32([0, 1, 0]), 8, 8)
        rays = case.rays[:4].copy()
        rays[1, 4] = np.nan
        with pytest.raises(hip_mod.PMError):
            ctx.set_eye_rays(rays)
    finally:
        ctx.close()


def test_far_coordinates_near_origin(hip_mod, monkeypatch):
    case, ans = answer(Q.shifted_case)
    recs = mode_records(hip_mod, monkeypatch, case)
    assert len(recs) == 5
    check_modes(case, ans, recs)


# ------------------------------------------------------- the commit pad
def leaf_boxes(ctx):
    """{global triangle id: (lo, hi)} — the box of the leaf holding each
    triangle, decoded from the committed quantized 4-wide nodes exactly as
    the kernels decode them (o + q 2^e, one rounding)"""
    w = ctx.scene_section("bvh4").reshape(-1, 16)
    refs, tri_id = ctx.scene_section("refs"), ctx.scene_section("tri_id")
    out = {}
    for nd in w:
        o = nd[0:3].view(np.float32).astype(np.float64)
        step = np.array([(((int(nd[3]) >> (8 * a)) & 0xff) - 1) << 23 for a in range(3)], np.uint32).view(np.float32).astype(np.float64)
        cnt = np.array([nd[10] & 0xffff, nd[10] >> 16, nd[11] & 0xffff, nd[11] >> 16], np.uint16).view(np.int16)
        for k in range(4):
            if cnt[k] <= 0:
                continue
            q = lambda word: float((int(nd[word]) >> (8 * k)) & 0xff)
            lo = np.float32([o[a] + q(4 + a) * step[a] for a in range(3)])
            hi = np.float32([o[0] + q(7) * step[0], o[1] + q(8) * step[1], o[2] + q(9) * step[2]])
            start = ~int(nd[12 + k]) & 0xffffffff
            if cnt[k] & 0x4000:
                slots = range(start, start + (int(cnt[k]) & 0x3fff))
            else:
                slots = [int(r) & 0x3fffffff for r in refs[start:start + int(cnt[k])] if (int(r) >> 30) == 0]
            for s in slots:
                out[int(tri_id[s])] = (lo, hi)
    return out


def test_commit_pad_reaches_the_tree(hip_mod, monkeypatch):
    """The bound test of test_ray_query.py holds for boxes padded as
    ray_query_ref.padded_box pads them; this holds the product to it: the
    leaf box the kernels decode for every triangle contains the triangle's
    box widened by that pad (the quantizer only ever rounds outwards)."""
    monkeypatch.delenv("PM_BVH8", raising=False)
    for case in (Q.control_case(), Q.shifted_case()):
        ctx = build(case, pad=HBM_PAD).load_into(hip_mod.Context(0))
        try:
            assert ctx.scene_info()["mode"] == "bvh-hbm"
            boxes = leaf_boxes(ctx)
        finally:
            ctx.close()
        assert set(range(len(case.tris))) <= set(boxes)
        for k, tri in enumerate(case.tris):
            lo, hi = Q.padded_box(tri.min(axis=0), tri.max(axis=0))
            assert (boxes[k][0] <= lo).all() and (boxes[k][1] >= hi).all(), (case.name, k, boxes[k], lo, hi)


# ------------------------------------------------------------------ group 8
def photon_case(name):
    if name == "control":
        return Q.control_case()
    # (path pid takes Halton index 4 pid, whose base-2 digit sum keeps u1 < 1/4:
    # every photon leaves a point light upwards, z >= 1/2)
    if name == "ties":
        t = Q.tie_case()                      # lit from below the plane of the coplanar triangles and the disk
        return Q.Case("ties-from-below", t.tris, t.rays, t.disks, t.spheres, light=(0.31, 0.40, -0.4))
    # "far": the light 1e4 above two large sheets 5e-4 apart. Their padded
    # boxes (thin in z, the axis the light is far along) do not overlap, and
    # an ulp of the origin is 1e-3: with the upper sheet's box culled or its
    # t interval misplaced by that much, the lower sheet wins. A third sheet
    # above the light takes every photon's first hit; its bounce comes down
    # from 3e4 and deposits on one of the two sheets, which the bits show.
    c = Q.control_case()
    e = 2.0e4
    zs = (1.125, 1.1255, 3.0e4)
    sheets = [[[-e, -e, z], [e, -e, z], [e, e, z]] for z in zs] + [[[-e, -e, z], [e, e, z], [-e, e, z]] for z in zs]
    return Q.Case("far-light", np.concatenate([c.tris, np.float32(sheets)]), c.rays, light=(0.41, 0.52, 1.0e4))


@functools.lru_cache(maxsize=None)
def emitted_directions():
    """direction of path pid from the point light: the Halton stream of
    mesh_light_ref and its uniform_sphere (whose flip to +z is undone)"""
    smp = R.emission_samples(PATHS)
    d = R.uniform_sphere(smp[:, 0], smp[:, 1], np.array([0.0, 0.0, 1.0]))
    z = 1.0 - 2.0 * smp[:, 0].astype(np.float64)
    return np.where((z < 0)[:, None], -d, d)


DIR_ERR = 16 * Q.U    # the fp32 sincos / sqrt of uniform_sample_sphere against float64: 16 ulps


@pytest.mark.parametrize("name", ["control", "ties", "far"])
def test_photon_first_deposits(name, hip_mod, monkeypatch):
    case = photon_case(name)
    for v in ("PM_BVH8", "PM_TRACE_POOL", "PM_TRACE_HOLD"):
        monkeypatch.delenv(v, raising=False)
    runs = {}
    if case.n_prims() <= 64:
        runs["brute"] = first_deposits(hip_mod, build(case), "brute")
    runs["bvh-lds"] = first_deposits(hip_mod, build(case, pad=lds_pad(case)), "bvh-lds")
    if not case.disks and not case.spheres:
        ident = (np.eye(4, dtype=np.float32).reshape(-1), np.eye(4, dtype=np.float32).reshape(-1))
        runs["bvh-instanced"] = first_deposits(hip_mod, build(case, inst=ident), "bvh-instanced")
    for bvh8 in ("0", "1"):
        for pool in ("0", "1"):
            for hold in ("0", "1"):
                monkeypatch.setenv("PM_BVH8", bvh8)
                monkeypatch.setenv("PM_TRACE_POOL", pool)
                monkeypatch.setenv("PM_TRACE_HOLD", hold)
                runs[f"hbm bvh8={bvh8} pool={pool} hold={hold}"] = first_deposits(hip_mod, build(case, pad=HBM_PAD), "bvh-hbm")
    for v in ("PM_BVH8", "PM_TRACE_POOL", "PM_TRACE_HOLD"):
        monkeypatch.delenv(v)
    base = "brute" if "brute" in runs else "bvh-lds"
    for k, s in runs.items():
        assert_same_bits(s[0::4], runs[base][0::4], f"{case.name}: first deposits, {k} vs {base}")
    # against the reference: the first segment, light -> first hit
    slots = runs[base]
    d = emitted_directions()
    rays = np.concatenate([np.tile(case.light, (PATHS, 1)), d.astype(np.float32)], axis=1)
    ans = Q.query(case.prims(), rays, Q.EPS, Q.TMAX, dir_err=DIR_ERR)
    any_slot = (slots["bits"].reshape(PATHS, 4) & 1).any(axis=1)
    gone = ans.decided & (ans.hit == Q.MISS)
    assert not (gone & any_slot).any(), "a path the reference sends past everything deposited"
    first = slots[0::4]
    ok = ans.decided & (ans.hit >= 0) & ((first["bits"] & 1) == 1)
    print(f"{case.name}: {ok.sum()} first deposits on decided paths, {gone.sum()} decided misses")
    assert name != "far" or ok.sum() > PATHS // 8
    x1 = case.light.astype(np.float64)[None, :] + d * ans.t_hit[:, None]
    p, wi = first["p"].astype(np.float64), first["wi"].astype(np.float64)
    v = x1 - p
    dist = np.linalg.norm(np.cross(v, wi), axis=1) / np.linalg.norm(wi, axis=1)
    tol = ans.mt_hit * 1.0 + DIR_ERR * np.abs(ans.t_hit) + 4 * Q.U * (np.linalg.norm(x1, axis=1) + np.linalg.norm(p, axis=1))
    bad = ok & ~(dist <= tol)
    assert not bad.any(), f"{case.name}: {bad.sum()} first deposits do not start at the reference's first hit"
