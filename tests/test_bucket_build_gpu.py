"""The index structures the gather kernels read, against bucket_ref.py's numpy
references, bit for bit (test_bucket_build.py certifies the cases and the
checkers on the CPU): the bucket map of pm_build_photon_map (cell_start, ph_a,
ph_b) over the scan's size edges, slot counts, photon distributions, rebuilds
and every variant of the trace's fused counting; the bucket counters, all zero
after every build; the record view list; the tile list and its cost sort.

Before anything else each build's grid (pm_map_info's cells, pm_map_grid) is
held against the reference's. Only a valid photon with a NaN or inf position
is exempt from the cell check (it must still appear once, bit-equal, in some
cell). Unreachable, by make_grid's two cells per axis: N = cells + 1 < 8 (the
smallest is 9), and N = 2048 exactly (2047 = 23 * 89 has no third factor)."""
import numpy as np
import pytest

import bucket_ref as B
import gather_ref as G
import pass_plan_ref
from parity_util import assert_bitexact
from pmrender import scenes
from pmrender.abi import PM_ESTIMATOR_KNN, PM_GATHER_GRID, RenderParams

pytestmark = pytest.mark.gpu

ENV_KEYS = ("PM_GATHER_KERNEL", "PM_CELL_SPAN", "PM_KNN_SS", "PM_TILE_SORT", "PM_LAZY_ZERO", "PM_TRACE_HOLD",
            "PM_TRACE_POOL", "PM_GRID_QUANTILE", "PM_POOL_STACK")


@pytest.fixture
def context(hip_mod, monkeypatch):
    made = []

    def make(scene, **env):
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        made.append(scene.load_into(hip_mod.Context(0)))
        return made[-1]
    yield make
    for c in made:
        c.close()


def check_build(ctx, scene, p, slots, span=2, grid_params=None):
    """the map the context holds is a correct build of `slots` on the grid of grid_params (default p)"""
    g = G.Grid(scene, grid_params or p, span)
    info, mg = ctx.map_info(), ctx.map_grid()
    assert info["structure"] == PM_GATHER_GRID and info["cells"] == g.ncells and info["slots"] == len(slots), (info, g.ncells)
    assert mg["dims"] == g.dims and mg["inv_cs_bits"] == pass_plan_ref.bits(g.inv_cs), (mg, g.dims)
    assert np.array_equal(B.u32(mg["origin"]), B.u32(g.lo))
    cs, a, b = ctx.photon_map()
    assert info["valid"] == int(B.valid_mask(slots).sum()) == int(cs[-1])
    B.assert_map(cs, a, b, slots, g)
    cnt = ctx.map_counters()
    assert len(cnt) == g.ncells + 1
    assert not cnt.any(), f"{int((cnt != 0).sum())} counters left nonzero, first at cell {int(np.flatnonzero(cnt)[0])}"
    return cs, a, b


def canonical(cs, a, b):
    """the map with each cell's photons in slot order: equal for any two correct builds of the same slots"""
    order = np.lexsort((B.u32(b)[:, 1, 1], B.cell_of(cs, np.arange(len(a)))))
    return cs, B.u32(a)[order], B.u32(b)[order]


def same_map(m1, m2):
    return all(np.array_equal(x, y) for x, y in zip(canonical(*m1), canonical(*m2)))


# ---- scan sizes, slot counts, distributions -------------------------------------------
@pytest.mark.parametrize("name", sorted(B.CASES))
def test_uploaded_case(name, context):
    c = B.case(name)
    ctx = context(c.scene)
    ctx.upload_slots(c.slots)
    ctx.build_photon_map(c.params, len(c.slots))
    cs, a, b = check_build(ctx, c.scene, c.params, c.slots)
    if name == "all_invalid":
        assert not cs.any() and len(a) == 0 and ctx.map_info()["valid"] == 0
    if name == "one_cell":  # the ranks are a permutation of 0 .. n - 1
        assert sorted(B.u32(b)[:, 1, 1].tolist()) == list(range(500)) and cs[1234] == 0 and cs[1235] == 500


# ---- reuse ------------------------------------------------------------------------------
def test_build_twice_and_regrow(context):
    c = B.reuse_case()
    ctx = context(c.scene)
    ctx.upload_slots(c.slots)
    ctx.build_photon_map(c.params, len(c.slots))
    first = check_build(ctx, c.scene, c.params, c.slots)
    ctx.build_photon_map(c.params, len(c.slots))
    again = check_build(ctx, c.scene, c.params, c.slots)
    assert np.array_equal(first[0], again[0]) and same_map(first, again), "the same slots built twice"
    # a coarser grid, a finer one (the buffers regrow), the first again
    for r2 in (9.0, 0.09, c.params.initial_radius2):
        p = RenderParams.from_buffer_copy(c.params)
        p.initial_radius2 = r2
        ctx.build_photon_map(p, len(c.slots))
        m = check_build(ctx, c.scene, p, c.slots)
    assert same_map(first, m)
    # fewer slots after more, then more again: what the shorter upload left behind stays out
    rng = np.random.RandomState(3)
    few = B.make_slots(B.uniform_points(c.grid, 257, rng), rng)
    ctx.upload_slots(few)
    ctx.build_photon_map(c.params, len(few))
    check_build(ctx, c.scene, c.params, few)
    ctx.build_photon_map(c.params, 100)
    check_build(ctx, c.scene, c.params, few[:100])
    ctx.upload_slots(c.slots)
    ctx.build_photon_map(c.params, 0)  # 0: every uploaded slot
    assert same_map(first, check_build(ctx, c.scene, c.params, c.slots))


@pytest.mark.parametrize("estimator,span", [(0, 3), (PM_ESTIMATOR_KNN, 2)], ids=["span3", "knn"])
def test_build_on_other_grids(estimator, span, context):
    """PM_CELL_SPAN=3's coarser PPM cells and the kNN estimator's finer ones"""
    c = B.reuse_case(estimator, span)
    ctx = context(c.scene, PM_CELL_SPAN=span)
    ctx.upload_slots(c.slots)
    for _ in range(2):
        ctx.build_photon_map(c.params, len(c.slots))
        check_build(ctx, c.scene, c.params, c.slots, span)


# ---- the trace's fused counting ---------------------------------------------------------------
PATHS = 1000  # no multiple of 256
R2 = 64.0


def _fused_params(**kw):
    return RenderParams.defaults(paths_per_pass=PATHS, initial_radius2=R2, gather_structure=PM_GATHER_GRID, **kw)


def _trace_build_check(ctx, sc, p, paths=PATHS, begin=0, base=0, build_params=None, grid_params=None, n_slots=None):
    ctx.trace_photons(p, 0, begin, paths, slot_path_base=base)
    n = (begin + paths - base) * p.max_photon_count if n_slots is None else n_slots
    bp = build_params or p
    ctx.build_photon_map(bp, n)
    slots = ctx.download_slots(n)
    assert 0 < B.valid_mask(slots).sum() < n
    assert not B.exempt_mask(slots).any()
    return slots, check_build(ctx, sc, bp, slots, grid_params=grid_params)


@pytest.mark.parametrize("hold", [0, 1])
@pytest.mark.parametrize("mpc", [3, 4, 5])
def test_fused_count_cornell(hold, mpc, context):
    """slot-major held key quads (hold 1, mpc 4), plane-major keys (hold 0), deferred ranks, mpc != HOLD_MPC"""
    sc = scenes.cornell_box(16, 16)
    ctx = context(sc, PM_TRACE_HOLD=hold)
    _trace_build_check(ctx, sc, _fused_params(max_photon_count=mpc))


def test_fused_count_lazy_zero(context):
    sc = scenes.cornell_box(16, 16)
    ctx = context(sc, PM_TRACE_HOLD=0, PM_LAZY_ZERO=1)
    slots, _ = _trace_build_check(ctx, sc, _fused_params())
    dead = slots[~B.valid_mask(slots)]
    assert len(dead) and not dead.view(np.uint32).any(), "the downloaded invalid slots are zero"
    slots2, _ = _trace_build_check(ctx, sc, _fused_params())  # and again over the lazily filled buffer
    assert np.array_equal(slots.view(np.uint32), slots2.view(np.uint32))


def test_fused_count_pooled_soup(context):
    sc = scenes.triangle_soup(20000, 32, 32)
    ctx = context(sc)
    assert ctx.scene_info()["mode"] == "bvh-hbm"
    _trace_build_check(ctx, sc, _fused_params())


def test_fused_count_shards(context):
    sc = scenes.cornell_box(16, 16)
    p = _fused_params()
    ctx = context(sc)
    # a shard whose slots start at its first path: fused
    _trace_build_check(ctx, sc, p, begin=512, base=512)
    # a second call that continues the buffer: not fused, the build counts again over the counters the first dirtied
    ctx.trace_photons(p, 0, 0, 600, slot_path_base=0)
    slots, _ = _trace_build_check(ctx, sc, p, paths=400, begin=600, base=0)
    assert B.valid_mask(slots[:2400]).any() and B.valid_mask(slots[2400:]).any()
    # a smaller fused trace after a larger one: over its own slots, then over every slot the buffer holds
    small, _ = _trace_build_check(ctx, sc, p, paths=300)
    assert len(small) == 1200
    ctx.build_photon_map(p, 0)
    everything = ctx.download_slots(4000)
    assert np.array_equal(everything[:1200].view(np.uint32), small.view(np.uint32))
    assert B.valid_mask(everything[1200:]).any()
    check_build(ctx, sc, p, everything)


def test_fused_count_then_another_grid(context):
    sc = scenes.cornell_box(16, 16)
    p = _fused_params()
    ctx = context(sc)
    # another radius: the build keeps the grid the trace counted on (the two of one pass agree), no recount
    p2 = _fused_params()
    p2.initial_radius2 = 16.0
    _trace_build_check(ctx, sc, p, build_params=p2, grid_params=p)
    # another estimator: its cells are four times finer, so the grids differ and the build counts again over
    # the counters the trace dirtied
    pk = _fused_params(estimator=PM_ESTIMATOR_KNN)
    assert G.Grid(sc, pk).ncells > 8 * G.Grid(sc, p).ncells
    _trace_build_check(ctx, sc, p, build_params=pk)
    # and back, fused again
    _trace_build_check(ctx, sc, p)


# ---- the record view -------------------------------------------------------------------------------
@pytest.mark.parametrize("image", sorted(B.VIEW_IMAGES))
def test_record_view_list(image, context):
    torch = pytest.importorskip("torch")
    sc, p = B.box_scene((2, 2, 2), *B.VIEW_IMAGES[image])
    n = G.num_records(sc)
    ctx = context(sc)
    assert ctx.num_records() == n
    ctx.upload_records(B.blank_records(sc, np.ones(n, bool)))
    assert ctx.set_record_view(True) == n
    pats = B.view_patterns(n)
    rng = np.random.RandomState(n)
    pats["random"] = rng.uniform(size=n) < 0.4
    for name, on in pats.items():
        recs = B.blank_records(sc, on)
        ctx.upload_records(recs)  # rebuilds the view
        want = B.view_ref(recs)
        assert ctx.record_view_size() == len(want), name
        d = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.record_view_list(d.data_ptr())
        ctx.synchronize()
        got = d.cpu().numpy()
        assert np.array_equal(got[:len(want)].astype(np.uint32), want), name
        assert (got[len(want):] == -1).all(), f"{name}: written beyond the view's length"
        assert ctx.set_record_view(True) == len(want)


# ---- the tile list ------------------------------------------------------------------------------------
def _tile_context(context, nt, **env):
    sc, p = B.box_scene((4, 4, 4), *B.TILE_IMAGES[nt])
    ctx = context(sc, PM_GATHER_KERNEL="tile", **env)
    assert ctx.num_records() == nt * 64
    g = G.Grid(sc, p)
    rng = np.random.RandomState(nt)
    slots = B.make_slots(B.uniform_points(g, 600, rng), rng)
    ctx.upload_slots(slots)
    ctx.build_photon_map(p, len(slots))
    return sc, p, ctx, rng, slots


@pytest.mark.parametrize("nt", sorted(B.TILE_IMAGES))
def test_tile_list_and_sort(nt, context):
    sc, p, ctx, rng, slots = _tile_context(context, nt)
    found = False
    for name, tile_on in B.tile_patterns(nt).items():
        recs = B.tile_records(sc, tile_on, rng)
        want = B.tile_list_ref(recs)
        assert np.array_equal(want, np.flatnonzero(tile_on)), name
        ctx.upload_records(recs)
        compact, is_sorted = ctx.tile_list()
        assert not is_sorted and np.array_equal(compact, want), f"{name}: the compact list"
        ctx.gather(p)
        first = ctx.download_records()
        after, is_sorted = ctx.tile_list()
        assert is_sorted, name
        B.assert_sorted(compact, after)
        if len(compact) < 8:
            assert np.array_equal(after, compact), f"{name}: fewer than 8 tiles, nothing to reorder"
        live = np.flatnonzero(B.active(recs))[:512]  # the gathers below compare something: photons were found
        # N' = int(0.7 M) is positive from two photons on
        near = any((G.d2_f32(recs["pos"][i], slots["p"]) < recs["radius2"][i]).sum() >= 2 for i in live)
        assert (first["photon_count"][live] > 0).any() == near, name
        found |= near
        # the same gather over the sorted list, from the initial state
        ctx.reset_records(p)
        ctx.gather(p)
        assert_bitexact(ctx.download_records(), first, f"{name}: the gather over the sorted list")
        assert np.array_equal(ctx.tile_list()[0], after), "sorted once"
        # and from re-uploaded records (a new compact list)
        ctx.upload_records(recs)
        again, is_sorted = ctx.tile_list()
        assert not is_sorted and np.array_equal(again, want)
        ctx.gather(p)
        assert_bitexact(ctx.download_records(), first, f"{name}: the gather from re-uploaded records")
    assert found or nt == 1, "no pattern's records lie near a photon: the gathers compared nothing"


@pytest.mark.parametrize("nt", [9, 65, 1025])
def test_tile_list_unsorted(nt, context):
    sc, p, ctx, rng, _ = _tile_context(context, nt, PM_TILE_SORT=0)
    recs = B.tile_records(sc, B.tile_patterns(nt)["sparse"], rng)
    ctx.upload_records(recs)
    want = B.tile_list_ref(recs)
    ctx.gather(p)
    got, is_sorted = ctx.tile_list()
    assert not is_sorted and np.array_equal(got, want), "PM_TILE_SORT=0 keeps the compact list"
