"""GPU parity tests: the HIP path (through the C-ABI) against the CPU oracle
on the same seeded inputs.

Bars:
  * eye records, photon slots, kd-tree nodes: bit-exact;
  * kd-tree gather (reference layout, same visiting order): bit-exact;
  * photon-bucket gather: per-record photon count / radius exact, flux
    within 2e-5 relative (fp32 summation order);
  * final radiance: per-pixel RMSE < 1e-3 (north_star), in practice ~1e-7.
"""
import numpy as np
import pytest

from parity_util import assert_bitexact, compare_gathered_records, rmse
from pmrender import scenes
from pmrender.abi import PM_GATHER_GRID, PM_GATHER_KDTREE, PM_REC_INVALID, RenderParams

pytestmark = pytest.mark.gpu


def make_pair(scene, oracle_mod, hip_mod):
    ctx = scene.load_into(hip_mod.Context(0))
    orc = scene.load_into(oracle_mod.Oracle())
    return ctx, orc


@pytest.fixture(scope="module")
def cornell(oracle_mod, hip_mod):
    return make_pair(scenes.cornell_box(64, 64), oracle_mod, hip_mod)


def test_eye_pass_bitexact(cornell):
    ctx, orc = cornell
    p = RenderParams.defaults()
    ctx.eye_pass(p)
    assert_bitexact(ctx.download_records(), orc.eye_pass(p), "eye records")


@pytest.mark.parametrize("paths,pass_index", [(4096, 0), (65536, 2)])
def test_photon_trace_bitexact(cornell, paths, pass_index):
    ctx, orc = cornell
    p = RenderParams.defaults(paths_per_pass=paths)
    ctx.trace_photons(p, pass_index, 0, paths)
    gpu = ctx.download_slots(paths * 4)
    ref = orc.trace_photons(p, pass_index, 0, paths)
    assert (ref["bits"] & 1).sum() > 0.3 * len(ref)
    assert_bitexact(gpu, ref, "photon slots")


@pytest.mark.parametrize("hold", ["0", "1"])
@pytest.mark.parametrize("scene", ["cornell", "soup"])
def test_photon_trace_write_modes_bitexact(hold, scene, oracle_mod, hip_mod, monkeypatch):
    """Slots and the fused bucket counts are the same whether a path's
    deposits are written as they happen (PM_TRACE_HOLD=0) or held and written
    once per path with 16-B stores: brute-force and BVH scenes, every slot
    bit-exact vs the oracle, map photons == valid slots."""
    monkeypatch.setenv("PM_TRACE_HOLD", hold)
    sc = scenes.cornell_box(32, 32) if scene == "cornell" else scenes.triangle_soup(20000, 32, 32)
    ctx, orc = make_pair(sc, oracle_mod, hip_mod)
    try:
        paths = 32768
        p = RenderParams.defaults(paths_per_pass=paths)
        ctx.trace_photons(p, 1, 0, paths)
        gpu = ctx.download_slots(paths * 4)
        ref = orc.trace_photons(p, 1, 0, paths)
        assert_bitexact(gpu, ref, f"slots (hold={hold}, {scene})")
        ctx.build_photon_map(p, paths * 4)
        assert ctx.map_info()["valid"] == int((ref["bits"] & 1).sum()) > paths // 2
    finally:
        ctx.close()


def test_pooled_trace_spheres_bitexact(oracle_mod, hip_mod):
    """The pooled BVH trace (4-wide quantized BVH in HBM, lanes refilled as
    paths end) on a 20K-triangle soup with a glass and a mirror sphere
    (specular chains): every slot bit-exact vs the oracle, also for a shard
    traced at a global path offset; map photons == valid slots. (The
    wavefront variant with per-bounce ray reordering this test also covered
    was measured slower and removed)"""
    sc = scenes.triangle_soup(20000, 32, 32)
    glass = sc.material(scenes.PM_GLASS, (1.0, 1.0, 1.0))
    mirror = sc.material(scenes.PM_MIRROR, (0.9, 0.9, 0.9))
    for (x, y, z), r, m in (((370.0, 100.0, 250.0), 100.0, glass), ((150.0, 90.0, 380.0), 90.0, mirror)):
        o2w, w2o = scenes.translate(x, y, z)
        sc.spheres.append((np.float32(r), o2w, w2o, m, -1))
    ctx, orc = make_pair(sc, oracle_mod, hip_mod)
    try:
        paths = 32768
        p = RenderParams.defaults(paths_per_pass=paths)
        ref = orc.trace_photons(p, 1, 0, paths)
        ctx.trace_photons(p, 1, 0, paths)
        assert_bitexact(ctx.download_slots(paths * 4), ref, "pooled-trace slots")
        ctx.build_photon_map(p, paths * 4)
        assert ctx.map_info()["valid"] == int((ref["bits"] & 1).sum()) > paths // 4
        half = paths // 2
        ctx.trace_photons(p, 1, half, half, slot_path_base=half)
        assert_bitexact(ctx.download_slots(half * 4), ref[half * 4:], "pooled-trace shard")
    finally:
        ctx.close()


def test_photon_trace_sharded_equals_whole(cornell):
    """Global path ids: two shards traced separately == one launch (owner-writes)."""
    ctx, orc = cornell
    p = RenderParams.defaults(paths_per_pass=8192)
    ref = orc.trace_photons(p, 0, 0, 8192)
    ctx.trace_photons(p, 0, 4096, 4096, slot_path_base=4096)
    hi = ctx.download_slots(4096 * 4)
    ctx.trace_photons(p, 0, 0, 4096, slot_path_base=0)
    lo = ctx.download_slots(4096 * 4)
    assert_bitexact(np.concatenate([lo, hi]), ref, "sharded photon slots")


def test_photon_trace_overwrites_stale_slots(cornell):
    """The trace kernel writes every slot of its paths: unused ones become zero
    even over garbage left by an earlier pass (no separate memset)."""
    from pmrender.abi import PHOTON_DTYPE
    ctx, orc = cornell
    p = RenderParams.defaults(paths_per_pass=4096)
    ctx.upload_slots(np.frombuffer(b"\xa5" * (4096 * 4 * PHOTON_DTYPE.itemsize), PHOTON_DTYPE))
    ctx.trace_photons(p, 1, 0, 4096)
    assert_bitexact(ctx.download_slots(4096 * 4), orc.trace_photons(p, 1, 0, 4096), "photon slots over garbage")


def test_trace_census(cornell):
    """Counting launch: same slots; census consistent with the deposits."""
    ctx, orc = cornell
    p = RenderParams.defaults(paths_per_pass=16384)
    ctx.trace_photons(p, 0, 0, 16384)
    plain = ctx.download_slots(16384 * 4)
    ctx.set_counting(True)
    try:
        ctx.trace_photons(p, 0, 0, 16384)
        rays, nodes, prims, deposits = ctx.trace_counters()
    finally:
        ctx.set_counting(False)
    counted = ctx.download_slots(16384 * 4)
    assert_bitexact(counted, plain, "slots of a counting launch")
    assert deposits == int((plain["bits"] & 1).sum())
    assert 16384 <= rays <= 16384 * (4 + 1 + 10)
    assert nodes >= rays and prims >= deposits


def test_scene_info(cornell, hip_mod):
    """Traversal mode chosen per scene: the Cornell box (30 triangles + the
    disk light) is brute-forced; a few thousand triangles get a BVH."""
    ctx, _ = cornell
    info = ctx.scene_info()
    assert info["mode"] == "brute" and info["triangles"] == 30 and info["disks"] == 1
    big = scenes.triangle_soup(3000, 32, 24).load_into(hip_mod.Context(0))
    try:
        bi = big.scene_info()
        assert bi["mode"] in ("bvh-hbm", "bvh-lds") and bi["triangles"] >= 3000 and bi["bvh_nodes"] > 1
    finally:
        big.close()


@pytest.mark.parametrize("structure", [PM_GATHER_GRID, PM_GATHER_KDTREE])
def test_deferred_reset(cornell, structure):
    """pm_reset_records is deferred: a fused full gather consumes it (same
    records as a gather right after the eye pass); any other reader sees the
    reset applied first."""
    ctx, _ = cornell
    p = RenderParams.defaults(paths_per_pass=16384, initial_radius2=25.0, gather_structure=structure)
    ctx.eye_pass(p)
    eye = ctx.download_records()
    ctx.trace_photons(p, 0, 0, 16384)
    ctx.build_photon_map(p, 16384 * 4)
    ctx.gather(p)
    first = ctx.download_records()
    assert (first["photon_count"] > 0).sum() > 100
    for _ in range(2):
        ctx.reset_records(p)
        ctx.gather(p)
        assert_bitexact(ctx.download_records(), first, "gather after deferred reset")
    ctx.reset_records(p)
    assert_bitexact(ctx.download_records(), eye, "reset records read back")


def _gather_inputs(orc, paths=16384, radius2=25.0):
    p = RenderParams.defaults(paths_per_pass=paths, initial_radius2=radius2)
    recs = orc.eye_pass(p)
    slots = orc.trace_photons(p, 0, 0, paths)
    return p, recs, slots


def test_kdtree_gather_bitexact(cornell, oracle_mod):
    ctx, orc = cornell
    p, recs, slots = _gather_inputs(orc)
    p.gather_structure = PM_GATHER_KDTREE
    ctx.upload_records(recs)
    ctx.upload_slots(slots)
    ctx.build_photon_map(p, len(slots))
    nodes_ref = oracle_mod.Oracle.build_kdtree(slots)
    assert_bitexact(ctx.download_kdtree(), nodes_ref, "kd-tree nodes")
    ctx.set_counting(True)
    ctx.gather(p)
    vis, hits = ctx.gather_counters()
    ctx.set_counting(False)
    ref = recs.copy()
    vis_ref, hits_ref = orc.gather(nodes_ref, ref, p)
    assert (vis, hits) == (vis_ref, hits_ref)
    assert_bitexact(ctx.download_records(), ref, "kd gathered records")


@pytest.mark.parametrize("radius2", [4.0, 25.0, 0.3])
def test_grid_gather_parity(cornell, radius2):
    ctx, orc = cornell
    p, recs, slots = _gather_inputs(orc, radius2=radius2)
    ctx.upload_records(recs)
    ctx.upload_slots(slots)
    p.gather_structure = PM_GATHER_GRID
    ctx.build_photon_map(p, len(slots))
    ctx.set_counting(True)
    ctx.gather(p)
    vis, hits = ctx.gather_counters()
    ctx.set_counting(False)
    ref = recs.copy()
    _, hits_ref = orc.gather(orc.build_kdtree(slots), ref, p)
    assert hits == hits_ref
    assert vis >= hits
    compare_gathered_records(ctx.download_records(), ref)


@pytest.mark.parametrize("radius2", [4.0, 25.0, 400.0])
@pytest.mark.parametrize("W,H,paths", [(64, 48, 16384), (320, 180, 131072)])
def test_bucket_gather_kernels_agree(radius2, W, H, paths, oracle_mod, hip_mod, monkeypatch):
    """The bucket gather kernels find the same photons: the LDS-staged tile
    kernel (default) and the per-lane kernel give bit-identical fused records
    and split partials. radius2 25 makes the unions of a tile exceed one LDS
    window (several windows); 400 exceeds the grid's design radius for
    uploaded records -> the per-lane fallbacks. PM_CELL_SPAN 3..5: finer
    bucket cells (edge 2 r / (span - 1)), the tile kernel's lanes reading
    span z-runs of span rows each."""
    torch = pytest.importorskip("torch")
    sc = scenes.cornell_box(W, H)
    orc = sc.load_into(oracle_mod.Oracle())
    p, recs, slots = _gather_inputs(orc, radius2=radius2, paths=paths)
    p.gather_structure = PM_GATHER_GRID
    outs = {}
    for name, env in (("lane", {"PM_GATHER_KERNEL": "lane"}), ("tile", {"PM_GATHER_KERNEL": "tile"}),
                      ("tile_span3", {"PM_GATHER_KERNEL": "tile", "PM_CELL_SPAN": "3"}),
                      ("tile_span4", {"PM_GATHER_KERNEL": "tile", "PM_CELL_SPAN": "4"}),
                      ("tile_span5", {"PM_GATHER_KERNEL": "tile", "PM_CELL_SPAN": "5"}),
                      ("lane_span3", {"PM_GATHER_KERNEL": "lane", "PM_CELL_SPAN": "3"})):
        for k in ("PM_GATHER_KERNEL", "PM_CELL_SPAN"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = sc.load_into(hip_mod.Context(0))
        try:
            ctx.upload_records(recs)
            ctx.upload_slots(slots)
            ctx.build_photon_map(p, len(slots))
            part = torch.zeros((len(recs), 4), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ctx.gather_partial(p, part.data_ptr())
            ctx.synchronize()
            ctx.gather(p)
            outs[name] = (ctx.download_records(), part.cpu().numpy())
        finally:
            ctx.close()
    ref_rec, ref_part = outs["lane"]
    assert (ref_part[:, 0] > 0).sum() > 100
    for name in ("tile", "tile_span3", "tile_span4", "tile_span5", "lane_span3"):
        assert np.array_equal(outs[name][1], ref_part), name
        assert_bitexact(outs[name][0], ref_rec, f"{name} vs per-lane gather")


def test_tile_gather_nan_photons(oracle_mod, hip_mod, monkeypatch):
    """Uploaded slots whose positions hold NaNs of either sign (and infinities):
    the tile kernel reads d2 < r^2 off the sign of min(d2, FLT_MAX) - r^2,
    exact for finite d2, with a NaN d2 (of either sign) clamped first.
    Partials and records equal the per-lane kernel's float comparisons bit
    for bit."""
    torch = pytest.importorskip("torch")
    sc = scenes.cornell_box(64, 48)
    orc = sc.load_into(oracle_mod.Oracle())
    p, recs, slots = _gather_inputs(orc, radius2=25.0, paths=16384)
    p.gather_structure = PM_GATHER_GRID
    slots = slots.copy()
    valid = np.flatnonzero(slots["bits"] & 1)
    rng = np.random.RandomState(3)
    pick = rng.choice(valid, size=len(valid) // 20, replace=False)
    pos = slots["p"].view(np.uint32)
    for k, idx in enumerate(np.array_split(pick, 4)):
        axis = k % 3
        pos[idx, axis] = (0x7fc00000, 0xffc00000, 0x7f800000, 0xff800001)[k]
    outs = {}
    for name in ("lane", "tile"):
        monkeypatch.setenv("PM_GATHER_KERNEL", name)
        ctx = sc.load_into(hip_mod.Context(0))
        try:
            ctx.upload_records(recs)
            ctx.upload_slots(slots)
            ctx.build_photon_map(p, len(slots))
            part = torch.zeros((len(recs), 4), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ctx.gather_partial(p, part.data_ptr())
            ctx.synchronize()
            ctx.gather(p)
            outs[name] = (ctx.download_records(), part.cpu().numpy())
        finally:
            ctx.close()
    assert (outs["lane"][1][:, 0] > 0).sum() > 100
    assert np.array_equal(outs["tile"][1], outs["lane"][1])
    assert_bitexact(outs["tile"][0], outs["lane"][0], "tile vs per-lane gather with NaN photons")


@pytest.mark.parametrize("scene", ["cornell", "caustic", "soup"])
def test_fresh_gather_tile_vs_lane(scene, oracle_mod, hip_mod, monkeypatch):
    """Fresh gathers (after pm_reset_records: every radius the initial one,
    read from the gather's parameters, not memory): the tile kernel — groups,
    and on the soup the wave-cooperative scan of a tile's few direct lanes —
    equals the per-lane kernel bit for bit, also with a few records at
    non-finite or far-away positions, over two reset + gather rounds; the
    fresh pass matches the oracle's single pass."""
    sc = {"cornell": lambda: scenes.cornell_box(96, 72), "caustic": lambda: scenes.caustic_scene(96, 72),
          "soup": lambda: scenes.triangle_soup(20000, 64, 48)}[scene]()
    orc = sc.load_into(oracle_mod.Oracle())
    p, recs, slots = _gather_inputs(orc, radius2=16.0, paths=32768)
    odd = recs.copy()
    act = np.nonzero((odd["flags"] & 7) == 0)[0]
    odd["pos"][act[7]] = (np.nan, 1.0, 2.0)
    odd["pos"][act[300]] = (np.inf, 0.0, 0.0)
    odd["pos"][act[1000]] = odd["pos"][act[1000]] + np.float32(5000.0)
    outs = {}
    for name in ("tile", "lane"):
        monkeypatch.setenv("PM_GATHER_KERNEL", name)
        ctx = sc.load_into(hip_mod.Context(0))
        try:
            ctx.upload_slots(slots)
            ctx.build_photon_map(p, len(slots))
            got = []
            for rr in (recs, odd):
                ctx.upload_records(rr)
                for _ in range(2):
                    ctx.reset_records(p)
                    ctx.gather(p)
                got.append(ctx.download_records())
            outs[name] = got
        finally:
            ctx.close()
    for i in range(2):
        assert_bitexact(outs["tile"][i], outs["lane"][i], f"fresh tile vs per-lane gather ({scene}, set {i})")
    ref = recs.copy()
    orc.gather(orc.build_kdtree(slots), ref, p)
    assert (ref["photon_count"] > 0).sum() > 500
    compare_gathered_records(outs["tile"][0], ref)


def test_adaptive_grid_radius_progressive(oracle_mod, hip_mod, monkeypatch):
    """Progressive passes size the photon grid from the records' current
    radii (a histogram binned by the fused gather, PM_GRID_QUANTILE; records
    above the grid's radius scan their own cells): 8 passes with the grid
    fixed at the initial radius (0), the default quantile and an aggressive
    one (0.5: half the records scan per lane) give identical records, and
    match the oracle's kd-tree passes (N', r^2 exact)."""
    sc = scenes.caustic_scene(96, 72)
    orc = sc.load_into(oracle_mod.Oracle())
    p = RenderParams.defaults(paths_per_pass=32768, initial_radius2=25.0)
    outs = {}
    for q in ("0", "0.99", "0.5"):
        monkeypatch.setenv("PM_GRID_QUANTILE", q)
        ctx = sc.load_into(hip_mod.Context(0))
        try:
            ctx.eye_pass(p)
            for k in range(8):
                ctx.trace_photons(p, k, 0, p.paths_per_pass)
                ctx.build_photon_map(p, p.paths_per_pass * 4)
                ctx.gather(p)
                ctx.synchronize()  # lets each histogram land before the next pass picks its grid
            outs[q] = (ctx.download_records(), ctx.map_info())
        finally:
            ctx.close()
    ref = orc.eye_pass(p)
    for k in range(8):
        orc.gather(orc.build_kdtree(orc.trace_photons(p, k, 0, p.paths_per_pass)), ref, p)
    assert (ref["photon_count"] > 0).sum() > 1000
    for q in ("0.99", "0.5"):
        assert_bitexact(outs[q][0], outs["0"][0], f"records, grid quantile {q} vs fixed grid")
    assert outs["0.5"][1]["cells"] > outs["0"][1]["cells"], "the grid did not follow the shrinking radii"
    compare_gathered_records(outs["0"][0], ref, flux_rtol=5e-5)


def test_lazy_zero_fill_of_unused_slots(oracle_mod, hip_mod, monkeypatch):
    """A fused-count trace leaves a path's unused slots stale (their keys mark
    them invalid; PM_LAZY_ZERO) and the context zeroes them before any other
    reader: slots read back, a kd-tree build, a smaller trace over part of the
    range and a recount all see the eager trace's slots, bit for bit, and the
    oracle's."""
    sc = scenes.cornell_box(48, 32)
    p = RenderParams.defaults(paths_per_pass=20000)
    pk = RenderParams.defaults(paths_per_pass=20000, gather_structure=PM_GATHER_KDTREE)
    out = {}
    for lazy in ("0", "1"):
        monkeypatch.setenv("PM_LAZY_ZERO", lazy)
        ctx = sc.load_into(hip_mod.Context(0))
        try:
            ctx.eye_pass(p)
            got = []
            ctx.trace_photons(p, 1, 0, 20000)            # fused: slots [0, 80000) lazily zeroed
            ctx.build_photon_map(p, 80000)
            ctx.gather(p)
            got.append(ctx.download_slots(80000))
            ctx.trace_photons(p, 2, 0, 20000)
            ctx.build_photon_map(pk, 80000)             # kd build reads every slot
            got.append(ctx.download_slots(80000))
            ctx.trace_photons(p, 3, 0, 20000)
            ctx.trace_photons(p, 4, 0, 5000)             # covers a quarter: the stale tail is zeroed first
            got.append(ctx.download_slots(80000))
            ctx.trace_photons(p, 5, 0, 20000)
            ctx.trace_photons(p, 6, 5000, 15000, slot_path_base=0)  # not fused: zeroes pass 5's stale slots first
            ctx.build_photon_map(p, 80000)              # recount reads every slot's valid bit
            ctx.gather(p)
            got.append(ctx.download_slots(80000))
            out[lazy] = (got, ctx.download_records())
        finally:
            ctx.close()
    orc = sc.load_into(oracle_mod.Oracle())
    ref = [orc.trace_photons(p, k, 0, 20000) for k in (1, 2)]
    tail = orc.trace_photons(p, 3, 0, 20000)
    head = orc.trace_photons(p, 4, 0, 5000)
    ref.append(np.concatenate([head, tail[20000:]]))
    ref.append(np.concatenate([orc.trace_photons(p, 5, 0, 20000)[:20000], orc.trace_photons(p, 6, 5000, 15000)]))
    for k in range(4):
        assert_bitexact(out["1"][0][k], out["0"][0][k], f"slots, step {k}: lazy vs eager zero fill")
        assert_bitexact(out["1"][0][k], ref[k], f"slots, step {k}: vs oracle")
    assert_bitexact(out["1"][1], out["0"][1], "records: lazy vs eager zero fill")


def test_adaptive_grid_radius_from_bands(hip_mod):
    """Band gathers (an all-gather rank's or a group device's record ranges)
    bin their radii into one histogram per pass, summed once at the next
    pass: a context that gathers every band of 4 ranks in turn
    picks the same grid as full-range gathers, pass for pass, with the same
    records; one rank's interleaved bands pick a grid within one histogram
    bin of it."""
    from pmrender.dist import HipEngine, _bands  # noqa: F401
    sc = scenes.caustic_scene(96, 72)
    p = RenderParams.defaults(paths_per_pass=32768, initial_radius2=25.0)
    runs = {}
    for mode in ("full", "all_bands", "rank0"):
        ctx = sc.load_into(hip_mod.Context(0))
        try:
            ctx.eye_pass(p)
            unit = ((ctx.width + 7) // 8) * 64 if ctx.pinhole else 512
            bands = _bands(ctx.num_records(), unit, 4)
            ranges = {"full": [(0, ctx.num_records())], "all_bands": [r for b in bands for r in b],
                      "rank0": bands[0]}[mode]
            cells = []
            for k in range(8):
                ctx.trace_photons(p, k, 0, p.paths_per_pass)
                ctx.build_photon_map(p, p.paths_per_pass * 4)
                cells.append(ctx.map_info()["cells"])
                for b, c in ranges:
                    ctx.gather_range(p, b, c)
                ctx.synchronize()  # each histogram lands before the pass after next picks its grid
            runs[mode] = (cells, ctx.download_records())
        finally:
            ctx.close()
    assert runs["full"][0][-1] > runs["full"][0][0], "the grid did not follow the shrinking radii"
    assert runs["all_bands"][0] == runs["full"][0], (runs["all_bands"][0], runs["full"][0])
    assert_bitexact(runs["all_bands"][1], runs["full"][1], "records, band gathers vs full-range gathers")
    # one bin of the histogram is 2^(1/8) in r^2: cells scale with r^-3 (1.30x per bin)
    for a, b in zip(runs["rank0"][0], runs["full"][0]):
        assert b / 1.31 <= a <= b * 1.31, (runs["rank0"][0], runs["full"][0])


def test_soup_tile_gather(oracle_mod, hip_mod):
    """Incoherent tiles (a triangle soup: neighbouring pixels on unrelated
    triangles: leader groups and per-lane scans): two fused passes match the
    oracle (M -> N', r^2 exact). (Waves over the records in cell order, the
    variant this test also covered, were measured slower and removed.)"""
    sc = scenes.triangle_soup(50000, 160, 120)
    ctx, orc = make_pair(sc, oracle_mod, hip_mod)
    try:
        p = RenderParams.defaults(paths_per_pass=65536, initial_radius2=25.0)
        recs = orc.eye_pass(p)
        slots = orc.trace_photons(p, 0, 0, 65536)
        ctx.eye_pass(p)
        ctx.trace_photons(p, 0, 0, 65536)
        ctx.build_photon_map(p, 65536 * 4)
        ctx.gather(p)
        ctx.gather(p)  # a second pass over the same map: PPM state carried
        got = ctx.download_records()
        ref = recs.copy()
        nodes = orc.build_kdtree(slots)
        orc.gather(nodes, ref, p)
        orc.gather(nodes, ref, p)
        assert (ref["photon_count"] > 0).sum() > 1000
        compare_gathered_records(got, ref)
    finally:
        ctx.close()


def test_partial_plus_update_equals_fused(cornell):
    torch = pytest.importorskip("torch")
    ctx, orc = cornell
    p, recs, slots = _gather_inputs(orc)
    ctx.upload_slots(slots)
    ctx.build_photon_map(p, len(slots))
    ctx.upload_records(recs)
    ctx.gather(p)
    fused = ctx.download_records()
    ctx.upload_records(recs)
    part = torch.zeros((len(recs), 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.gather_partial(p, part.data_ptr())
    ctx.synchronize()
    ref_part = orc.gather_partial(orc.build_kdtree(slots), recs)
    gp = part.cpu().numpy()
    assert np.array_equal(gp[:, 0], ref_part[:, 0].astype(np.int64))
    half = len(recs) // 2
    ctx.ppm_update(p, part.data_ptr(), 0, half)
    ctx.ppm_update(p, part[half:].data_ptr(), half, len(recs) - half)
    assert_bitexact(ctx.download_records(), fused, "partial+update vs fused")


@pytest.mark.parametrize("view", [False, True])
def test_deferred_reset_before_partial_gather(cornell, view):
    """A deferred pm_reset_records is applied before a partial gather (which
    does not consume it), with and without the active-record view (where the
    launch covers only the tiles holding active records): the partials equal
    those of a gather over freshly uploaded records."""
    torch = pytest.importorskip("torch")
    ctx, orc = cornell
    p, recs, slots = _gather_inputs(orc)
    ctx.upload_slots(slots)
    ctx.build_photon_map(p, len(slots))
    ctx.upload_records(recs)
    n = ctx.set_record_view(True) if view else len(recs)
    try:
        ref = torch.zeros((len(recs), 4), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.gather_partial(p, ref.data_ptr())
        ctx.synchronize()
        ctx.gather(p)                       # PPM state moves away from the initial one
        ctx.reset_records(p)                # deferred
        got = torch.zeros((len(recs), 4), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.gather_partial(p, got.data_ptr())
        ctx.synchronize()
        assert np.array_equal(got.cpu().numpy()[:n], ref.cpu().numpy()[:n])
        assert (ref.cpu().numpy()[:n, 0] > 0).sum() > 100
    finally:
        if view:
            ctx.set_record_view(False)


def test_sharded_reduce_exchange_bitexact(oracle_mod, hip_mod):
    """The multi-GPU "reduce" exchange emulated on one device: two contexts
    each trace half of the global paths, gather all records against their
    own photon buckets, the int64 partials are summed (what RCCL
    reduce_scatter does), owners update, radii are exchanged. The records
    must equal a single context over all paths bit for bit."""
    torch = pytest.importorskip("torch")
    sc = scenes.cornell_box(64, 48)
    paths = 8192
    p = RenderParams.defaults(paths_per_pass=paths)
    ref = sc.load_into(hip_mod.Context(0))
    pr = RenderParams.defaults(paths_per_pass=2 * paths)
    ref.eye_pass(pr)
    shards = [sc.load_into(hip_mod.Context(0)) for _ in range(2)]
    for c in shards:
        c.eye_pass(p)
    n = ref.num_records()
    half = n // 2
    for pass_index in range(3):
        ref.trace_photons(pr, pass_index, 0, 2 * paths)
        ref.build_photon_map(pr)
        ref.gather(pr)
        parts = []
        for rank, c in enumerate(shards):
            c.trace_photons(p, pass_index, rank * paths, paths, rank * paths)
            c.build_photon_map(p, paths * 4)
            t = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            c.gather_partial(p, t.data_ptr())
            c.synchronize()
            parts.append(t)
        total = parts[0] + parts[1]
        torch.cuda.synchronize()
        r2 = torch.zeros(n, dtype=torch.float32, device="cuda")
        for rank, c in enumerate(shards):
            b, cnt = (0, half) if rank == 0 else (half, n - half)
            c.ppm_update(p, total[b:].data_ptr(), b, cnt)
            c.get_radius2(b, cnt, r2[b:].data_ptr())
            c.synchronize()
        for c in shards:
            c.set_radius2(r2.data_ptr(), 0, n)
            c.synchronize()
    got = np.concatenate([shards[0].download_records()[:half], shards[1].download_records()[half:]])
    assert_bitexact(got, ref.download_records(), "2-shard reduce exchange vs 1 context")


def test_sharded_reduce_exchange_active_view(oracle_mod, hip_mod):
    """Same emulated exchange over the active-record view (what PassRunner
    moves across GPUs), ownership in view chunks, final radiance gathered per
    view chunk and scattered through the view list: bit-identical records and
    image to one context over all paths."""
    torch = pytest.importorskip("torch")
    sc = scenes.cornell_box(64, 48)
    paths = 8192
    p = RenderParams.defaults(paths_per_pass=paths)
    pr = RenderParams.defaults(paths_per_pass=2 * paths)
    ref = sc.load_into(hip_mod.Context(0))
    ref.eye_pass(pr)
    shards = [sc.load_into(hip_mod.Context(0)) for _ in range(2)]
    for c in shards:
        c.eye_pass(p)
    nv = [c.set_record_view(True) for c in shards][0]
    recs0 = ref.download_records()
    active = np.nonzero((recs0["flags"] & 7) == 0)[0]
    assert nv == len(active) and 0 < nv < len(recs0)
    vl = torch.zeros(nv, dtype=torch.int32, device="cuda")
    shards[0].record_view_list(vl.data_ptr())
    shards[0].synchronize()
    assert np.array_equal(vl.cpu().numpy(), active)
    half = nv // 2
    for pass_index in range(3):
        ref.trace_photons(pr, pass_index, 0, 2 * paths)
        ref.build_photon_map(pr)
        ref.gather(pr)
        parts = []
        for rank, c in enumerate(shards):
            c.trace_photons(p, pass_index, rank * paths, paths, rank * paths)
            c.build_photon_map(p, paths * 4)
            t = torch.zeros((nv, 4), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            c.gather_partial(p, t.data_ptr())
            c.synchronize()
            parts.append(t)
        total = parts[0] + parts[1]
        torch.cuda.synchronize()
        r2 = torch.zeros(nv, dtype=torch.float32, device="cuda")
        for rank, c in enumerate(shards):
            b, cnt = (0, half) if rank == 0 else (half, nv - half)
            c.ppm_update(p, total[b:].data_ptr(), b, cnt)
            c.get_radius2(b, cnt, r2[b:].data_ptr())
            c.synchronize()
        for c in shards:
            c.set_radius2(r2.data_ptr(), 0, nv)
            c.synchronize()
    want = ref.download_records()
    got0, got1 = shards[0].download_records(), shards[1].download_records()
    assert_bitexact(got0[active[:half]], want[active[:half]], "owned view chunk 0")
    assert_bitexact(got1[active[half:]], want[active[half:]], "owned view chunk 1")
    emitted = float(2 * paths * 3)
    img = torch.zeros((nv, 3), dtype=torch.float32, device="cuda")
    for rank, c in enumerate(shards):
        b, cnt = (0, half) if rank == 0 else (half, nv - half)
        c.final_view(emitted, b, cnt, img[b:].data_ptr())
        c.synchronize()
    full = torch.zeros((len(want), 3), dtype=torch.float32, device="cuda")
    ref.final(emitted, 0, len(want), full.data_ptr())
    ref.synchronize()
    full = full.cpu().numpy()
    assert np.array_equal(img.cpu().numpy().view(np.uint32), full[active].view(np.uint32))
    inactive = np.setdiff1d(np.arange(len(want)), active)
    assert not full[inactive].any()          # records outside the view are black


@pytest.mark.parametrize("structure", [PM_GATHER_KDTREE, PM_GATHER_GRID])
def test_render_parity_cornell(cornell, structure):
    ctx, orc = cornell
    p = RenderParams.defaults(paths_per_pass=32768, passes=2, gather_structure=structure)
    img, st = ctx.render(p)
    ref, st_ref = orc.render(p)
    assert st["photons_valid"] == st_ref["photons_valid"]
    assert st["gather_points"] == st_ref["gather_points"]
    if structure == PM_GATHER_KDTREE:
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert rmse(img, ref) < 1e-3
    assert np.abs(img - ref).max() <= 1e-4 * max(1.0, float(ref.max()))


def test_render_deterministic(cornell):
    """Bucket order comes from atomic arrival order; the fixed-point gather
    makes the image independent of it."""
    ctx, _ = cornell
    p = RenderParams.defaults(paths_per_pass=65536, passes=2)
    a, _ = ctx.render(p)
    for _ in range(3):
        b, _ = ctx.render(p)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_grid_gather_independent_of_photon_order(cornell):
    """Permuting the slot array (hence every bucket's order) changes no bit."""
    ctx, orc = cornell
    p, recs, slots = _gather_inputs(orc)
    outs = []
    for perm in (np.arange(len(slots)), np.random.RandomState(4).permutation(len(slots))):
        ctx.upload_records(recs)
        ctx.upload_slots(slots[perm])
        ctx.build_photon_map(p, len(slots))
        ctx.gather(p)
        outs.append(ctx.download_records())
    assert_bitexact(outs[0], outs[1], "records after permuted-photon gather")


@pytest.mark.parametrize("builder", ["caustic", "feature", "soup", "figure"])
def test_scene_parity(builder, oracle_mod, hip_mod):
    if builder == "caustic":
        sc = scenes.caustic_scene(96, 64)
    elif builder == "feature":
        sc = scenes.feature_scene(72, 40)
    elif builder == "figure":   # killeroo substitute: instanced 5,120-triangle mesh, 4-wide BVH + pooled trace
        sc = scenes.figure_scene(80, 64)
    else:
        sc = scenes.triangle_soup(20000, 80, 48)
    ctx, orc = make_pair(sc, oracle_mod, hip_mod)
    p = RenderParams.defaults(paths_per_pass=16384)
    ctx.eye_pass(p)
    recs = ctx.download_records()
    assert_bitexact(recs, orc.eye_pass(p), f"{builder} eye records")
    if builder == "feature":
        assert (recs["flags"] & PM_REC_INVALID).sum() == ctx.num_records() - 72 * 40
    ctx.trace_photons(p, 1, 0, 16384)
    assert_bitexact(ctx.download_slots(16384 * 4), orc.trace_photons(p, 1, 0, 16384), f"{builder} slots")
    p.gather_structure = PM_GATHER_KDTREE
    img, _ = ctx.render(p)
    ref, _ = orc.render(p)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))


def test_two_level_instances(oracle_mod, hip_mod):
    """Object instances through pm_add_object_mesh / pm_add_mesh_instance
    (each mesh once, its own 4-wide tree, hits rebuilt in world space) give
    the flattened scene's bits: eye records and slots vs the oracle (which
    flattens), kd render vs the oracle, grid render vs the flattened GPU
    context. Rotations, non-uniform scales, shading normals, uvs, a mirror."""
    sc = scenes.instanced_scene(80, 64)
    two = sc.load_into(hip_mod.Context(0))
    flat = sc.load_into(hip_mod.Context(0), instancing=False)
    orc = sc.load_into(oracle_mod.Oracle())
    info = two.scene_info()
    assert info["mode"] == "bvh-instanced"
    assert info["triangles"] == flat.scene_info()["triangles"] == sc.num_triangles
    n_obj_tris = sum(len(o["idx"]) for o in sc.objects)
    assert len(two.scene_section("obj_tris")) == 12 * n_obj_tris
    assert len(two.scene_section("instances")) == 32 * len(sc.instances)
    p = RenderParams.defaults(paths_per_pass=16384)
    two.eye_pass(p)
    assert_bitexact(two.download_records(), orc.eye_pass(p), "instanced eye records")
    two.trace_photons(p, 1, 0, 16384)
    assert_bitexact(two.download_slots(16384 * 4), orc.trace_photons(p, 1, 0, 16384), "instanced slots")
    p.gather_structure = PM_GATHER_KDTREE
    img, _ = two.render(p)
    ref, _ = orc.render(p)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    p.gather_structure = PM_GATHER_GRID
    img, _ = two.render(p)
    ref, _ = flat.render(p)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))


def test_many_instances(hip_mod):
    """48 instances of a 320-triangle object under random rotations, scales
    and translations (a top tree of many instance boxes, overlapping object
    trees): slots and grid renders of the two-level scene equal the flattened
    scene's bit for bit."""
    rng = np.random.RandomState(7)
    sc = scenes.cornell_box(48, 40, blocks=False)
    mat = sc.material(scenes.PM_MATTE, (0.6, 0.5, 0.4))
    P, idx = scenes.figure_mesh(2)
    sc.objects.append(dict(P=P, idx=idx, N=None, uv=None, material=mat, light=-1))
    for _ in range(48):
        s = rng.uniform(0.2, 0.45, 3)
        t = rng.uniform([60, 0, 60], [480, 350, 480])
        sc.instances.append((0, *scenes.affine(rng.uniform(-180, 180), rng.uniform(-40, 40), s, t)))
    two = sc.load_into(hip_mod.Context(0))
    flat = sc.load_into(hip_mod.Context(0), instancing=False)
    try:
        assert two.scene_info()["mode"] == "bvh-instanced"
        p = RenderParams.defaults(paths_per_pass=32768)
        for ctx in (two, flat):
            ctx.trace_photons(p, 2, 0, 32768)
        assert_bitexact(two.download_slots(32768 * 4), flat.download_slots(32768 * 4), "many-instance slots")
        p.gather_structure = PM_GATHER_GRID
        a, _ = two.render(p)
        b, _ = flat.render(p)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        two.close()
        flat.close()


def test_instance_arguments(hip_mod):
    """pm_add_mesh_instance refuses an unknown object and a projective
    transform (the two-level path handles affine ones only); pm_add_object_mesh
    refuses out-of-range indices."""
    ctx = hip_mod.Context(0)
    mat = ctx.add_material(0, (0.5, 0.5, 0.5))
    P = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    with pytest.raises(hip_mod.PMError):
        ctx.add_object_mesh(P, np.int32([[0, 1, 3]]), None, None, mat, -1)
    obj = ctx.add_object_mesh(P, np.int32([[0, 1, 2]]), None, None, mat, -1)
    o2w, w2o = scenes.translate(1.0, 2.0, 3.0)
    with pytest.raises(hip_mod.PMError):
        ctx.add_mesh_instance(obj + 1, o2w, w2o)
    proj = np.array(o2w, np.float32).copy()
    proj[14] = 0.5  # last row (0, 0, 0.5, 1): not affine
    with pytest.raises(hip_mod.PMError):
        ctx.add_mesh_instance(obj, proj, w2o)
    ctx.add_mesh_instance(obj, o2w, w2o)
    ctx.close()


def test_eye_rays_mode(oracle_mod, hip_mod):
    sc = scenes.cornell_box(40, 24, nsamples=3)
    sc.camera = scenes.rays_from_pinhole(sc)
    ctx, orc = make_pair(sc, oracle_mod, hip_mod)
    p = RenderParams.defaults(paths_per_pass=8192, gather_structure=PM_GATHER_KDTREE)
    img, _ = ctx.render(p)
    ref, _ = orc.render(p)
    assert img.shape == (40 * 24, 3)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))


def test_no_photons_raises(hip_mod):
    sc = scenes.cornell_box(16, 16)
    o, x, y, n, Le, area, ns = sc.lights[0][1:]
    sc.lights[0] = ("disk", o, x, y, n, np.float32([0, 0, 0]), area, ns)  # black light: every path returns early
    ctx = sc.load_into(hip_mod.Context(0))
    with pytest.raises(hip_mod.NoPhotonsError):
        ctx.render(RenderParams.defaults(paths_per_pass=1024))


def test_invalid_arguments(hip_mod):
    ctx = hip_mod.Context(0)
    with pytest.raises(hip_mod.PMError):
        ctx.commit()  # no lights / shapes
    with pytest.raises(hip_mod.PMError):
        ctx.add_trimesh(np.zeros((3, 3)), np.int32([[0, 1, 5]]), material=0)  # no material 0, bad index


def test_full_size_c2_parity(oracle_mod, hip_mod):
    """BASELINE config 2 at full size (1920x1080, 262,144 paths = 1M slots):
    slots bit-exact, photon counts exact, radiance RMSE < 1e-3."""
    sc = scenes.cornell_box(1920, 1080)
    ctx, orc = make_pair(sc, oracle_mod, hip_mod)
    p = RenderParams.defaults()
    img, st = ctx.render(p)
    slots = ctx.download_slots(262144 * 4)
    ref_slots = orc.trace_photons(p, 0, 0, 262144)
    assert_bitexact(slots, ref_slots, "C2 slots")
    ref, st_ref = orc.render(p)
    assert st["photons_valid"] == st_ref["photons_valid"]
    assert rmse(img, ref) < 1e-3


# ---- kNN estimator (pbrt-v2 LPhoton, PM_ESTIMATOR_KNN) ----------------------
@pytest.mark.parametrize("K,radius2", [(50, 900.0), (16, 400.0), (64, 2500.0), (1, 25.0)])
def test_knn_gather_parity(cornell, K, radius2):
    """k_gather_knn over the photon buckets vs the oracle's pbrt kd-tree
    lookup (shrinking radius, PhotonProcess heap): photons found and r_k^2
    bit-exact, flux to fp32 summation order; two passes accumulate."""
    from parity_util import compare_knn_records, knn_term_floor
    from pmrender.abi import PM_ESTIMATOR_KNN
    ctx, orc = cornell
    p = RenderParams.defaults(paths_per_pass=16384, initial_radius2=radius2, estimator=PM_ESTIMATOR_KNN,
                              knn_lookup=K)
    recs = orc.eye_pass(p)
    ref = recs.copy()
    ctx.upload_records(recs)
    floor = np.zeros(len(recs))
    for pass_index in range(2):
        slots = orc.trace_photons(p, pass_index, 0, 16384)
        ctx.upload_slots(slots)
        ctx.build_photon_map(p, len(slots))
        ctx.gather(p)
        orc.gather(orc.build_kdtree(slots), ref, p)
        floor += knn_term_floor(scenes.cornell_box(), ref["photon_count"], ref["radius2"])
    got = ctx.download_records()
    act = (ref["flags"] & 7) == 0
    assert (ref["photon_count"][act] == K).mean() > 0.2 and (ref["photon_count"][act] < K).any()
    compare_knn_records(got, ref["photon_count"].astype(np.int64), ref["radius2"], ref["flux"], floor=floor)


def test_knn_render_parity(cornell):
    """Whole render with the kNN estimator: image RMSE < 1e-3 vs the oracle,
    deterministic run to run."""
    from pmrender.abi import PM_ESTIMATOR_KNN
    ctx, orc = cornell
    p = RenderParams.defaults(paths_per_pass=32768, passes=2, initial_radius2=400.0, estimator=PM_ESTIMATOR_KNN)
    img, st = ctx.render(p)
    ref, st_ref = orc.render(p)
    assert st["photons_valid"] == st_ref["photons_valid"]
    assert rmse(img, ref) < 1e-3
    assert np.abs(img - ref).max() <= 1e-4 * max(1.0, float(ref.max()))
    again, _ = ctx.render(p)
    assert np.array_equal(img.view(np.uint32), again.view(np.uint32))


@pytest.mark.parametrize("scene,W,H,paths,K,radius2", [
    ("cornell", 160, 120, 16384, 50, 900.0),
    ("cornell", 160, 120, 16384, 64, 2500.0),
    ("cornell", 160, 120, 16384, 1, 25.0),
    ("caustic", 128, 128, 65536, 64, 400.0),      # dense caustic: deeper re-binning
    ("soup", 128, 96, 16384, 16, 100.0),          # incoherent tiles: per-lane passes
    ("cornell", 32, 24, 40000, 8, 1.0e7),         # >= 2^16 photons inside maxD: minimum extraction
])
def test_knn_kernels_agree(scene, W, H, paths, K, radius2, oracle_mod, hip_mod, monkeypatch):
    """The kNN tile kernels (k_gather_knn_tile: LDS-staged tile unions;
    k_gather_knn_ss: scalar-streamed photon pairs, bit-pattern histograms)
    and the per-lane heap kernel give bit-identical records: same found
    count, r_k^2 and fixed-point flux, over two accumulating passes."""
    from pmrender.abi import PM_ESTIMATOR_KNN
    sc = {"cornell": lambda: scenes.cornell_box(W, H), "caustic": lambda: scenes.caustic_scene(W, H),
          "soup": lambda: scenes.triangle_soup(20000, W, H)}[scene]()
    orc = sc.load_into(oracle_mod.Oracle())
    p = RenderParams.defaults(paths_per_pass=paths, initial_radius2=radius2, estimator=PM_ESTIMATOR_KNN,
                              knn_lookup=K)
    recs = orc.eye_pass(p)
    slots = [orc.trace_photons(p, i, 0, paths) for i in range(2)]
    outs = {}
    for name in ("lane", "tile", "ss"):
        monkeypatch.setenv("PM_GATHER_KERNEL", "lane" if name == "lane" else "tile")
        monkeypatch.setenv("PM_KNN_SS", "1" if name == "ss" else "0")
        ctx = sc.load_into(hip_mod.Context(0))
        try:
            ctx.upload_records(recs)
            for s in slots:
                ctx.upload_slots(s)
                ctx.build_photon_map(p, len(s))
                ctx.gather(p)
            outs[name] = ctx.download_records()
        finally:
            ctx.close()
    act = (recs["flags"] & 7) == 0
    n = outs["lane"]["photon_count"][act]
    assert (n > 0).mean() > 0.5
    if radius2 < 1e6:
        assert (n == K).any() and (n < K).any()   # both full and partial lookups occur
    else:
        assert (n == K).all() and (slots[1]["bits"] & 1).sum() >= 65536
    assert_bitexact(outs["tile"], outs["lane"], f"kNN tile vs per-lane ({scene}, K={K})")
    assert_bitexact(outs["ss"], outs["lane"], f"kNN scalar-stream vs per-lane ({scene}, K={K})")


def test_knn_rejects_partial_gathers(cornell, hip_mod):
    torch = pytest.importorskip("torch")
    from pmrender.abi import PM_ESTIMATOR_KNN
    ctx, orc = cornell
    p = RenderParams.defaults(paths_per_pass=4096, estimator=PM_ESTIMATOR_KNN)
    ctx.eye_pass(p)
    ctx.trace_photons(p, 0, 0, 4096)
    ctx.build_photon_map(p, 4096 * 4)
    part = torch.zeros((ctx.num_records(), 4), dtype=torch.int64, device="cuda")
    with pytest.raises(hip_mod.PMError):
        ctx.gather_partial(p, part.data_ptr())
    with pytest.raises(hip_mod.PMError):
        ctx.gather(RenderParams.defaults(paths_per_pass=4096, estimator=PM_ESTIMATOR_KNN,
                                         gather_structure=PM_GATHER_KDTREE))


def test_kd_gather_reports_stack_overflow(oracle_mod, hip_mod, monkeypatch):
    """k_gather_kd drops no subtree silently: with a 2-entry traversal stack
    (PM_KD_STACK, test knob) the gather fails with PM_ERR_INVALID; with the
    default stack the same gather succeeds and matches the oracle."""
    sc = scenes.cornell_box(32, 32)
    orc = sc.load_into(oracle_mod.Oracle())
    p, recs, slots = _gather_inputs(orc)
    p.gather_structure = PM_GATHER_KDTREE
    for stack, ok in (("2", False), ("32", True)):
        monkeypatch.setenv("PM_KD_STACK", stack)
        ctx = sc.load_into(hip_mod.Context(0))
        try:
            ctx.upload_records(recs)
            ctx.upload_slots(slots)
            ctx.build_photon_map(p, len(slots))
            if ok:
                ctx.gather(p)
                ref = recs.copy()
                orc.gather(oracle_mod.Oracle.build_kdtree(slots), ref, p)
                assert_bitexact(ctx.download_records(), ref, "kd gather, default stack")
            else:
                with pytest.raises(hip_mod.PMError, match="stack"):
                    ctx.gather(p)
        finally:
            ctx.close()


@pytest.mark.parametrize("n_tris", [20_000, 300_000])
def test_bvh8_equals_bvh4(n_tris, oracle_mod, hip_mod, monkeypatch):
    """The 8-wide quantized tree (PM_BVH8=1: pm_build.h collapse_bvh8 /
    quantize_bvh8, pm_traverse.h traverse8 and the pooled kernel's
    k_trace_pool8 with pm_trav_step.h trav_step) against the 4-wide one on the same soup: eye records,
    every photon slot and the grid render bit for bit (closest hits do not
    depend on the tree; ties resolve to the lowest global id), and the slots
    equal the oracle's."""
    sc = scenes.triangle_soup(n_tris, 96, 64)
    paths = 65_536
    p = RenderParams.defaults(paths_per_pass=paths)
    out = {}
    for w in ("4", "8"):
        monkeypatch.setenv("PM_BVH8", "1" if w == "8" else "0")
        ctx = sc.load_into(hip_mod.Context(0))
        try:
            info = ctx.scene_info()
            assert info["mode"] == "bvh-hbm"
            node_bytes = ctx.scene_section("bvh4").nbytes // max(info["bvh_nodes"], 1)
            assert node_bytes == (128 if w == "8" else 64), (w, node_bytes)
            ctx.eye_pass(p)
            recs = ctx.download_records()
            ctx.trace_photons(p, 0, 0, paths)
            slots = ctx.download_slots(paths * 4)
            img, st = ctx.render(p)
            out[w] = (recs, slots, img, info["bvh_nodes"])
        finally:
            ctx.close()
    assert out["8"][3] < out["4"][3]
    assert_bitexact(out["8"][0], out["4"][0], "eye records, 8-wide vs 4-wide")
    assert_bitexact(out["8"][1], out["4"][1], "photon slots, 8-wide vs 4-wide")
    assert np.array_equal(out["8"][2].view(np.uint32), out["4"][2].view(np.uint32)), "render, 8-wide vs 4-wide"
    orc = sc.load_into(oracle_mod.Oracle())
    assert_bitexact(out["8"][1], orc.trace_photons(p, 0, 0, paths), "photon slots, 8-wide vs oracle")
