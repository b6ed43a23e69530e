"""What a correct photon-map build is, independent of any gather (numpy only),
for test_bucket_build.py (CPU) and test_bucket_build_gpu.py.

expected_map / assert_map: the bucket map (cell_start, ph_a, ph_b) of a slot
array on a grid (gather_ref.Grid over pass_plan_ref.make_grid). tile_list_ref /
assert_sorted: the compact tile list and what the cost sort may do to it.
view_ref: the record view list.

The cases are tiny scenes, two triangles that span a box, whose box and
initial_radius2 are steered until make_grid gives the wanted cells per axis
(box_scene). make_grid gives every axis at least two cells, so the smallest
grid has 8 cells and N = cells + 1 = 9 counters: N < 8 cannot be reached; and
N = 2048 would need three factors >= 2 of 2047 = 23 * 89.

The scan (pm_bucket.hip) gives each thread SCAN_ITEMS = 8 counters and each
block SCAN_TILE = 2048; a tile's offset is a sum over the earlier tiles'
sums, 256 per trip."""
import numpy as np

import gather_ref as G
import pass_plan_ref
from pmrender import scenes
from pmrender.abi import (PHOTON_DTYPE, PM_ESTIMATOR_KNN, PM_ESTIMATOR_PPM, PM_GATHER_GRID, PM_MATTE, PM_REC_INACTIVE,
                          PM_REC_MISS, RECORD_DTYPE, RenderParams)

f32 = np.float32
SCAN_ITEMS, SCAN_BLOCK = 8, 256
SCAN_TILE = SCAN_ITEMS * SCAN_BLOCK


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- scenes whose grid is chosen ----------------------------------------------
def box_scene(dims, W=8, H=8, estimator=PM_ESTIMATOR_PPM, cell_span=2, r2=1.0, lo=(-3.25, 10.5, 2.0), **kw):
    """(scene, params): two triangles spanning a box whose grid for params is dims = (dx, dy, dz), each >= 2"""
    lo = np.asarray(lo, f32)
    rq = np.sqrt(f32(r2)) * f32(1.0001) + f32(1e-4)
    f = f32(0.5) if estimator == PM_ESTIMATOR_KNN else f32(2.0) / f32(cell_span - 1)
    cs = float((f * rq) * f32(1.001))
    assert all(d >= 2 for d in dims)
    ext = np.array([(d - 1.5) * cs for d in dims])  # ceil(ext / cs) + 1 = d
    hi = (lo + ext).astype(f32)
    sc = scenes.Scene()
    white = sc.material(PM_MATTE, (0.5, 0.5, 0.5))
    sc.add_quads([[(lo[0], lo[1], lo[2]), (hi[0], lo[1], lo[2]), (hi[0], hi[1], hi[2]), (lo[0], hi[1], hi[2])]], white)
    sc.lights.append(("point", (lo + f32(0.5) * (hi - lo) + f32([0.0, 0.0, -5.0])).astype(f32), f32([100.0, 100.0, 100.0])))
    sc.camera = scenes.pinhole(W, H, eye=tuple(lo - f32([0.0, 0.0, 50.0])), look=tuple(lo + f32(0.5) * (hi - lo)))
    p = RenderParams.defaults(initial_radius2=r2, gather_structure=PM_GATHER_GRID, estimator=estimator, **kw)
    g = G.Grid(sc, p, cell_span)
    assert g.dims == tuple(dims), (g.dims, dims)
    return sc, p


# ---- the bucket map -------------------------------------------------------------
def valid_mask(slots):
    return (slots["bits"] & 1) != 0


def exempt_mask(slots):
    """valid slots whose position has a NaN or inf coordinate: their cell is the build's choice"""
    return valid_mask(slots) & ~np.isfinite(slots["p"]).all(axis=1)


def keys(slots, g):
    """per slot the cell key (cz dy + cy) dx + cx; -1 for an invalid slot, -2 for an exempt one"""
    dx, dy, dz = g.dims
    k = np.full(len(slots), -1, np.int64)
    ok = valid_mask(slots) & ~exempt_mask(slots)
    c = g.cells(slots["p"][ok])
    k[ok] = (c[:, 2] * dy + c[:, 1]) * dx + c[:, 0]
    k[exempt_mask(slots)] = -2
    return k


def cell_start_of(cell_keys, ncells):
    """exclusive cumsum of the bincount: ncells + 1 entries, the last one the photon count"""
    cnt = np.bincount(np.asarray(cell_keys, np.int64), minlength=ncells)
    assert len(cnt) == ncells
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)


def rows_of(slots, idx):
    """(ph_a [n, 4], ph_b [n, 2, 4]) as uint32, the rows of the slots idx"""
    idx = np.asarray(idx, np.int64)
    s = slots[idx]
    a = np.concatenate([u32(s["p"]).reshape(-1, 3), u32(s["wi"][:, 0]).reshape(-1, 1)], axis=1)
    b0 = np.concatenate([u32(s["alpha"]).reshape(-1, 3), u32(s["wi"][:, 1]).reshape(-1, 1)], axis=1)
    b1 = np.stack([u32(s["wi"][:, 2]), idx.astype(np.uint32), np.zeros(len(idx), np.uint32), np.zeros(len(idx), np.uint32)], 1)
    return a, np.stack([b0, b1], axis=1)


def expected_map(slots, g):
    """One correct map (cell_start, ph_a, ph_b as float32): slot order inside a cell; an exempt slot in cell 0"""
    k = keys(slots, g)
    k[k == -2] = 0
    idx = np.flatnonzero(k >= 0)
    order = idx[np.argsort(k[idx], kind="stable")]
    a, b = rows_of(slots, order)
    return cell_start_of(k[idx], g.ncells), a.view(f32), b.view(f32)


def cell_of(cell_start, j):
    """the cell photon j lies in by a nondecreasing cell_start: the k with cell_start[k] <= j < cell_start[k + 1]"""
    return np.searchsorted(np.asarray(cell_start[1:], np.int64), np.asarray(j, np.int64), side="right")


def assert_map(cell_start, ph_a, ph_b, slots, g):
    """The map is a correct build of `slots` on grid g; the order inside a cell is free."""
    k = keys(slots, g)
    valid = np.flatnonzero(k != -1)
    n, ncells = len(valid), g.ncells
    cell_start = np.asarray(cell_start)
    assert cell_start.dtype == np.uint32 and cell_start.shape == (ncells + 1,), (cell_start.dtype, cell_start.shape, ncells)
    assert int(cell_start[-1]) == n, f"cell_start[ncells] = {int(cell_start[-1])} photons, {n} valid slots"
    A, B = u32(np.asarray(ph_a, f32)).reshape(-1, 4), u32(np.asarray(ph_b, f32)).reshape(-1, 2, 4)
    assert len(A) == n and len(B) == n, f"{len(A)} / {len(B)} rows for {n} valid slots"
    cs = cell_start.astype(np.int64)
    down = np.flatnonzero(np.diff(cs) < 0)
    assert down.size == 0, f"cell_start decreases after cell {int(down[0])}: {int(cs[down[0]])} -> {int(cs[down[0] + 1])}"
    assert cs[0] == 0, f"cell_start[0] = {int(cs[0])}"
    if n == 0:
        assert not cs.any(), "no valid slot, but cell_start is not all zero"
        return
    cell = cell_of(cs, np.arange(n))
    idx = B[:, 1, 1].astype(np.int64)
    # the slot indices are a permutation of the valid slots
    bad = np.flatnonzero((idx >= len(slots)) | (k[np.minimum(idx, len(slots) - 1)] == -1))
    assert bad.size == 0, (f"photon {int(bad[0])} (cell {int(cell[bad[0]])}) carries slot index {int(idx[bad[0]])}: "
                           f"no valid slot ({bad.size} such photons)")
    seen = np.bincount(idx, minlength=len(slots))
    dup = np.flatnonzero(seen > 1)
    if dup.size:
        js = np.flatnonzero(idx == dup[0])
        raise AssertionError(f"slot {int(dup[0])} appears {int(seen[dup[0]])} times: photons {js.tolist()} in cells "
                             f"{cell[js].tolist()}, expected cell {int(k[dup[0]])}")
    miss = np.flatnonzero((seen == 0) & (k != -1))
    assert miss.size == 0, f"valid slot {int(miss[0])} (expected cell {int(k[miss[0]])}) is in no photon ({miss.size} missing)"
    # every row bit-equal to its slot's fields, both pad words 0
    ea, eb = rows_of(slots, idx)
    bad = np.flatnonzero((A != ea).any(axis=1) | (B != eb).any(axis=(1, 2)))
    if bad.size:
        j = int(bad[0])
        raise AssertionError(f"photon {j} (slot {int(idx[j])}, expected cell {int(k[idx[j]])}, actual cell {int(cell[j])}): rows "
                             f"ph_a {A[j].tolist()} ph_b {B[j].ravel().tolist()} differ from the slot's "
                             f"{ea[j].tolist()} {eb[j].ravel().tolist()} ({bad.size} such photons)")
    # the cell each photon lies in is its slot's key (an exempt slot: any cell in range)
    want = k[idx]
    bad = np.flatnonzero((want >= 0) & (want != cell))
    if bad.size:
        j = int(bad[0])
        raise AssertionError(f"photon {j} (slot {int(idx[j])}): expected cell {int(want[j])}, actual cell {int(cell[j])} "
                             f"({bad.size} photons in a wrong cell)")
    assert ((cell >= 0) & (cell < ncells)).all(), f"photon {int(np.argmax(cell >= ncells))} lies beyond the last cell"
    # cell_start exactly: the keys, with the exempt photons counted where the build put them
    ref = cell_start_of(np.where(want >= 0, want, cell), ncells)
    bad = np.flatnonzero(ref != cell_start)
    assert bad.size == 0, (f"cell_start differs from cell {int(bad[0])} on: {int(cell_start[bad[0]])}, expected "
                           f"{int(ref[bad[0]])} ({bad.size} entries)")


# ---- the tile list and the record view -----------------------------------------
def active(recs):
    return (recs["flags"] & PM_REC_INACTIVE) == 0


def view_ref(recs):
    return np.flatnonzero(active(recs)).astype(np.uint32)


def tile_list_ref(recs):
    """ascending ids of the 64-record tiles with at least one record without PM_REC_INACTIVE"""
    a = active(recs)
    pad = (-len(a)) % 64
    a = np.concatenate([a, np.zeros(pad, bool)]).reshape(-1, 64)
    return np.flatnonzero(a.any(axis=1)).astype(np.uint32)


def assert_sorted(unsorted, sorted_):
    """sorted_ is unsorted with its aligned groups of 8 entries reordered whole; the n % 8 tail stays in place"""
    unsorted, sorted_ = np.asarray(unsorted, np.uint32), np.asarray(sorted_, np.uint32)
    n = len(unsorted)
    assert len(sorted_) == n, f"the sorted list has {len(sorted_)} entries, the compact one {n}"
    S = n // 8
    assert np.array_equal(sorted_[8 * S:], unsorted[8 * S:]), \
        f"the last {n % 8} entries moved: {sorted_[8 * S:].tolist()} vs {unsorted[8 * S:].tolist()}"
    src = {tuple(gr): i for i, gr in enumerate(unsorted[:8 * S].reshape(S, 8).tolist())}
    assert len(src) == S, "the compact list repeats a group: not a list of distinct tiles"
    used = set()
    for o, gr in enumerate(sorted_[:8 * S].reshape(S, 8).tolist()):
        i = src.get(tuple(gr))
        assert i is not None, f"entries {8 * o}..{8 * o + 7} of the sorted list {gr} are no aligned group of the compact list"
        assert i not in used, f"group {i} of the compact list appears twice in the sorted list"
        used.add(i)


def blank_records(scene, pattern, r2=1.0, seed=0):
    """records of scene's raster, live where pattern (a bool per record) says, each MISS elsewhere; the live ones in the
    initial state (flux 0, N 0, r2) inside the scene box"""
    n = G.num_records(scene)
    pattern = np.asarray(pattern, bool)
    assert pattern.shape == (n,)
    rng = np.random.RandomState(seed)
    lo, hi = pass_plan_ref.scene_bbox(scene)
    recs = np.zeros(n, RECORD_DTYPE)
    recs["flags"] = np.where(pattern, 0, PM_REC_MISS)
    recs["pos"] = (lo + rng.uniform(0.0, 1.0, size=(n, 3)) * (hi - lo)).astype(f32)
    recs["ns"] = (0.0, 0.0, -1.0)
    recs["radius2"] = r2
    return recs


# ---- slots ------------------------------------------------------------------------
def make_slots(p, rng, bits=1):
    p = np.asarray(p, f32).reshape(-1, 3)
    s = np.zeros(len(p), PHOTON_DTYPE)
    s["bits"] = bits
    s["p"] = p
    s["alpha"] = rng.uniform(1.0, 64.0, size=(len(p), 3)).astype(f32)
    v = rng.normal(size=(len(p), 3))
    s["wi"] = (v / np.linalg.norm(v, axis=1)[:, None]).astype(f32)
    return s


def garbage_slots(n, rng, bits=None):
    """invalid slots with garbage in every field: random words (NaNs, infs and huge values among them), bit 0 clear"""
    w = rng.randint(0, 2 ** 32, size=(n, 10), dtype=np.uint64).astype(np.uint32)
    w[::5, 1] = 0x7fc00000  # NaN x
    w[1::5, 2] = 0x7f800000  # +inf y
    w[:, 0] &= 0xfffffffe
    if bits is not None:
        w[:, 0] = bits
    return np.ascontiguousarray(w).view(PHOTON_DTYPE).reshape(n)


def interleave(valid, invalid, rng):
    out = np.concatenate([valid, invalid])
    return out[rng.permutation(len(out))]


def cell_centre(g, key):
    key = np.asarray(key, np.int64)
    dx, dy, dz = g.dims
    c = np.stack([key % dx, (key // dx) % dy, key // (dx * dy)], axis=-1)
    return (g.lo.astype(np.float64) + (c + 0.5) * g.cs).astype(f32)


def in_cells(g, key, rng):
    """one point per key, anywhere in the middle 80 % of its cell"""
    key = np.asarray(key, np.int64).ravel()
    return (cell_centre(g, key).astype(np.float64) + rng.uniform(-0.4, 0.4, size=(len(key), 3)) * g.cs).astype(f32)


def uniform_points(g, n, rng):
    ext = np.asarray(g.dims) * g.cs
    return (g.lo.astype(np.float64) + rng.uniform(0.0, 1.0, size=(n, 3)) * ext).astype(f32)


# ---- the cases ----------------------------------------------------------------------
class Case:
    def __init__(self, name, scene, params, slots, cell_span=2, **edges):
        self.name, self.scene, self.params, self.slots, self.cell_span = name, scene, params, slots, cell_span
        self.edges = edges  # what test_bucket_build.py asserts the case reaches
        self.grid = G.Grid(scene, params, cell_span)

    @property
    def N(self):
        return self.grid.ncells + 1


# scan sizes: dims -> N = cells + 1
SCAN_DIMS = {
    "n9": (2, 2, 2),            # the smallest grid: one full 8-word thread and a 1-word tail
    "n64": (3, 3, 7),           # N % 8 == 0: vector path only
    "n2047": (2, 3, 341),       # one word short of a scan tile
    "n2049": (2, 2, 512),       # one word into the second tile (2048 itself cannot be reached)
    "n4095": (2, 23, 89),
    "n4096": (5, 7, 117),       # exactly two tiles
    "n4097": (2, 2, 1024),
    "n720001": (2, 600, 600),   # 352 scan tiles: the offset loop's second trip
}


def scan_case(name):
    sc, p = box_scene(SCAN_DIMS[name])
    g = G.Grid(sc, p)
    rng = np.random.RandomState(len(name) + g.ncells % 97)
    n = g.ncells
    if name == "n720001":
        # the first tile, tiles beyond the 256th, the last cell, and a spread over everything
        key = np.concatenate([rng.randint(0, SCAN_TILE, 700), rng.randint(256 * SCAN_TILE, n, 900), np.full(40, n - 1),
                              [256 * SCAN_TILE - 1, 256 * SCAN_TILE, 257 * SCAN_TILE - 1, 257 * SCAN_TILE],
                              rng.randint(0, n, 1500)])
        pts = in_cells(g, key, rng)
    else:
        key = np.concatenate([[0, 0, n - 1, n - 1, n - 1], rng.randint(0, n, 400)])
        pts = np.concatenate([in_cells(g, key, rng), uniform_points(g, 200, rng)])
    slots = interleave(make_slots(pts, rng), garbage_slots(len(pts) // 9 + 1, rng), rng)
    return Case(name, sc, p, slots, N=SCAN_DIMS[name][0] * SCAN_DIMS[name][1] * SCAN_DIMS[name][2] + 1)


COUNT_DIMS = (3, 3, 7)
SLOT_COUNTS = (1, 255, 256, 257, 3000)


def count_case(n):
    sc, p = box_scene(COUNT_DIMS)
    g = G.Grid(sc, p)
    rng = np.random.RandomState(1000 + n)
    return Case(f"slots{n}", sc, p, make_slots(uniform_points(g, n, rng), rng), count=n)


def all_invalid_case():
    sc, p = box_scene(COUNT_DIMS)
    return Case("all_invalid", sc, p, garbage_slots(300, np.random.RandomState(5)), count=300, valid=0)


DIST_DIMS = (6, 5, 70)  # 2100 cells: cell 2048 starts the second scan tile


def _dist(name, build, **edges):
    sc, p = box_scene(DIST_DIMS)
    g = G.Grid(sc, p)
    rng = np.random.RandomState(sum(map(ord, name)))
    return Case(name, sc, p, build(g, rng), **edges)


def _one_cell(g, rng):
    return make_slots(in_cells(g, np.full(500, 1234), rng), rng)


def _tile_run(g, rng):
    return make_slots(in_cells(g, np.arange(SCAN_TILE - 8, SCAN_TILE + 13), rng), rng)


def _ends_only(g, rng):
    return make_slots(in_cells(g, np.concatenate([np.zeros(37, int), np.full(91, g.ncells - 1)]), rng), rng)


def _outside(g, rng):
    pts = []
    ext = np.asarray(g.dims) * g.cs
    for a in range(3):
        for d in (0.1, 3.0, 50.0):
            for side in (0, 1):
                q = g.lo.astype(np.float64) + rng.uniform(0.05, 0.95, size=(6, 3)) * (ext - g.cs)
                q[:, a] = g.lo[a] - d * g.cs if side == 0 else g.lo[a] + (g.dims[a] + d) * g.cs
                pts.append(q)
    # and beyond three faces at once
    pts.append(g.lo.astype(np.float64) - np.array([[50.0, 3.0, 0.1]]) * g.cs)
    pts.append(g.lo.astype(np.float64) + (np.asarray(g.dims) + np.array([[0.1, 50.0, 3.0]])) * g.cs)
    return make_slots(np.concatenate(pts), rng)


def _ulp_planes(g, rng):
    pts = []
    for a in range(3):
        for k in sorted({1, 2, g.dims[a] // 2, g.dims[a] - 1}):
            for v in g.first_in_cell(k, a):
                q = uniform_points(g, 3, rng)
                q[:, a] = v
                pts.append(q)
    return make_slots(np.concatenate(pts), rng)


def _invalid_mix(g, rng):
    return interleave(make_slots(uniform_points(g, 700, rng), rng), garbage_slots(500, rng), rng)


def _caustic_bits(g, rng):
    pts = uniform_points(g, 600, rng)
    s = make_slots(pts, rng, bits=np.where(np.arange(600) % 2 == 0, 3, 1))
    bad = make_slots(pts[:300], rng, bits=2)  # the caustic bit without the valid bit, on top of valid photons
    return interleave(s, bad, rng)


def _nonfinite(g, rng):
    s = make_slots(uniform_points(g, 800, rng), rng)
    s["p"][100] = (np.nan, s["p"][100][1], s["p"][100][2])
    s["p"][300] = (np.inf, -np.inf, np.nan)
    s["p"][500][2] = np.inf
    s["p"][700][1] = -np.inf
    return s


DIST_CASES = {
    "one_cell": lambda: _dist("one_cell", _one_cell),
    "tile_run": lambda: _dist("tile_run", _tile_run),
    "ends_only": lambda: _dist("ends_only", _ends_only),
    "outside": lambda: _dist("outside", _outside),
    "ulp_planes": lambda: _dist("ulp_planes", _ulp_planes),
    "invalid_mix": lambda: _dist("invalid_mix", _invalid_mix),
    "caustic_bits": lambda: _dist("caustic_bits", _caustic_bits),
    "nonfinite": lambda: _dist("nonfinite", _nonfinite),
}

CASES = {**{n: (lambda n=n: scan_case(n)) for n in SCAN_DIMS},
         **{f"slots{n}": (lambda n=n: count_case(n)) for n in SLOT_COUNTS},
         "all_invalid": all_invalid_case, **DIST_CASES}

_cache = {}


def case(name):
    """the case, built once (its arrays are shared: leave them unchanged)"""
    if name not in _cache:
        _cache[name] = CASES[name]()
        _cache[name].slots.setflags(write=False)
    return _cache[name]


# reuse: grids of one box at three radii (coarser, finer, back), and fewer slots after more
def reuse_case(estimator=PM_ESTIMATOR_PPM, cell_span=2):
    sc, p = box_scene((9, 11, 13), estimator=estimator, cell_span=cell_span)
    rng = np.random.RandomState(77 + estimator + cell_span)
    g = G.Grid(sc, p, cell_span)
    slots = interleave(make_slots(np.concatenate([uniform_points(g, 1500, rng), in_cells(g, [0, g.ncells - 1], rng)]), rng),
                       garbage_slots(200, rng), rng)
    return Case(f"reuse[{estimator},{cell_span}]", sc, p, slots, cell_span)


# ---- tile-list and view cases ------------------------------------------------------
TILE_IMAGES = {1: (8, 8), 7: (56, 8), 8: (64, 8), 9: (72, 8), 63: (504, 8), 64: (512, 8), 65: (520, 8),
               1023: (264, 248), 1024: (256, 256), 1025: (328, 200), 2049: (24, 5464)}


def tile_patterns(nt):
    """name -> per-tile bool (tile holds an active record): tiles left empty at the start and the end, around the
    wave boundaries (multiples of 64) and the step boundaries (multiples of 1024) of k_tile_compact"""
    t = np.arange(nt)
    full = np.ones(nt, bool)
    ends = full.copy()
    ends[[0, nt - 1]] = False
    edges = full.copy()
    for m in range(64, nt + 1, 64):
        edges[[m - 1] + ([m] if m < nt else [])] = (m // 64) % 2 == 0  # empty on either side of every other boundary
    for m in range(1024, nt + 1, 1024):
        edges[max(m - 2, 0):min(m + 2, nt)] = False
    sparse = (t * 2654435761 % 7) < 3
    sparse[nt - 1] = True
    return {"full": full, "ends": ends, "edges": edges, "sparse": sparse}


def tile_records(scene, tile_on, rng):
    """records whose tile t holds active records iff tile_on[t]: a random few of the 64, sometimes only the last"""
    nt = len(tile_on)
    lane_on = rng.uniform(size=(nt, 64)) < 0.3
    lane_on[::3] = False
    lane_on[::3, 63] = True
    lane_on[np.arange(nt), rng.randint(0, 64, nt)] = True
    lane_on &= np.asarray(tile_on, bool)[:, None]
    return blank_records(scene, lane_on.ravel(), seed=nt)


VIEW_IMAGES = {"2049": (64, 32), "1985": (248, 8), "ragged": (13, 9)}


def view_patterns(n):
    r = np.arange(n)
    last = np.zeros(n, bool)
    last[-1] = True
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alternating": r % 2 == 0, "last": last}
