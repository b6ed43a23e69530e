"""CPU tests of the photon-map build cases and checkers (bucket_ref.py): every
case reaches the edge of the scan, the fill or the tile kernels it was built
for; assert_map rejects each way a bucket map can be wrong and assert_sorted
each way a cost sort can; and the argument checks the new read-only hooks of
the C-ABI make without a device. No kernel runs here, and no mutated kernel
runs anywhere: the checkers' sensitivity is shown on corrupted references."""
import ctypes

import numpy as np
import pytest

import bucket_ref as B
import gather_ref as G
from pmrender import hip
from pmrender.abi import PM_ERR_INVALID, PM_ESTIMATOR_KNN

TILE, ITEMS = B.SCAN_TILE, B.SCAN_ITEMS


# ---- the cases reach their edges ------------------------------------------------
def test_scan_sizes_straddle_the_edges():
    N = {n: B.case(n).N for n in B.SCAN_DIMS}
    assert N == {"n9": 9, "n64": 64, "n2047": 2047, "n2049": 2049, "n4095": 4095, "n4096": 4096, "n4097": 4097,
                 "n720001": 720001}
    for n, c in ((n, B.case(n)) for n in B.SCAN_DIMS):
        assert c.edges["N"] == c.N == c.grid.ncells + 1
    assert min(N.values()) == 9, "make_grid gives every axis two cells: N < 8 cannot be reached"
    assert N["n64"] % ITEMS == 0 and N["n4096"] % ITEMS == 0 and N["n9"] % ITEMS != 0 and N["n2047"] % ITEMS != 0
    # either side of one and of two scan tiles; 2048 itself would need dx dy dz = 2047 = 23 * 89
    assert N["n2047"] == TILE - 1 and N["n2049"] == TILE + 1
    assert (N["n4095"], N["n4096"], N["n4097"]) == (2 * TILE - 1, 2 * TILE, 2 * TILE + 1)
    assert not [d for d in np.ndindex(24, 90, 2048) if min(d) >= 2 and d[0] * d[1] * d[2] == 2047][:1]
    # the tile offset's strided loop makes a second trip from the 257th tile on
    tiles = -(-N["n720001"] // TILE)
    assert N["n720001"] > B.SCAN_BLOCK * TILE and tiles == 352 > B.SCAN_BLOCK + 1
    c = B.case("n720001")
    k = B.keys(c.slots, c.grid)
    k = k[k >= 0]
    assert (k < TILE).sum() >= 500 and (k >= 256 * TILE).sum() >= 500 and (k == c.grid.ncells - 1).sum() >= 40
    assert {256 * TILE - 1, 256 * TILE, 257 * TILE - 1, 257 * TILE} <= set(k.tolist())
    assert 2000 < len(k) < 5000, "a few thousand photons"
    for n in B.SCAN_DIMS:
        c = B.case(n)
        k = B.keys(c.slots, c.grid)
        assert (k == 0).any() and (k == c.grid.ncells - 1).any() and (k == -1).any(), n


def test_slot_counts_straddle_a_block():
    assert B.SLOT_COUNTS == (1, 255, 256, 257, 3000)
    for n in B.SLOT_COUNTS:
        c = B.case(f"slots{n}")
        assert len(c.slots) == n == c.edges["count"] and B.valid_mask(c.slots).all()
    c = B.case("all_invalid")
    assert len(c.slots) == 300 and not B.valid_mask(c.slots).any()
    cs, a, b = B.expected_map(c.slots, c.grid)
    assert not cs.any() and len(a) == 0 and len(b) == 0
    B.assert_map(cs, a, b, c.slots, c.grid)
    w = B.u32(c.slots.view(np.uint32).reshape(-1, 10))
    assert (w != 0).mean() > 0.9 and np.isnan(c.slots["p"]).any() and np.isinf(c.slots["p"]).any(), "garbage in every field"


def test_distributions_reach_their_edges():
    g = B.case("one_cell").grid
    assert g.dims == B.DIST_DIMS and g.ncells == 2100 > TILE + 13
    k = B.keys(B.case("one_cell").slots, g)
    assert len(k) == 500 and (k == 1234).all()
    k = B.keys(B.case("tile_run").slots, g)
    assert sorted(k.tolist()) == list(range(TILE - 8, TILE + 13)), "one photon per cell across the scan-tile boundary"
    k = B.keys(B.case("ends_only").slots, g)
    assert set(k.tolist()) == {0, g.ncells - 1} and (k == 0).sum() == 37
    # outside: 0.1, 3 and 50 cells beyond each face, clamped to the border cells
    s = B.case("outside").slots
    c = g.cells(s["p"])
    for a in range(3):
        below = (g.lo[a] - s["p"][:, a].astype(np.float64)) / g.cs
        above = (s["p"][:, a].astype(np.float64) - (g.lo[a] + g.dims[a] * g.cs)) / g.cs
        for d, border in ((below, 0), (above, g.dims[a] - 1)):
            for lo, hi in ((0.05, 0.15), (2.9, 3.1), (49.0, 51.0)):
                m = (d > lo) & (d < hi)
                assert m.sum() >= 6 and (c[m, a] == border).all(), (a, lo)
    out = ((s["p"] < g.lo) | (s["p"] > g.lo + np.asarray(g.dims) * g.cs)).any(axis=1)
    assert out.all()
    # ulp_planes: every photon is the float32 neighbour of a cell plane, on either side, first and last plane included
    s = B.case("ulp_planes").slots
    c = g.cells(s["p"])
    up = g.cells(np.nextafter(s["p"], np.float32(np.inf)))
    down = g.cells(np.nextafter(s["p"], np.float32(-np.inf)))
    assert ((up != c) | (down != c)).any(axis=1).all()
    for a in range(3):
        assert ((up[:, a] != c[:, a]) & (c[:, a] == 0)).any() and ((down[:, a] != c[:, a]) & (c[:, a] == g.dims[a] - 1)).any()
        assert (up[:, a] != c[:, a]).sum() >= 6 and (down[:, a] != c[:, a]).sum() >= 6
    s = B.case("invalid_mix").slots
    v = B.valid_mask(s)
    assert v.sum() == 700 and (~v).sum() == 500 and (np.diff(v.astype(int)) != 0).sum() > 300, "interleaved"
    assert (s["bits"][~v] != 0).any() and np.isnan(s["p"][~v]).any() and np.isinf(s["p"][~v]).any()
    s = B.case("caustic_bits").slots
    assert sorted(set(s["bits"].tolist())) == [1, 2, 3] and (s["bits"] == 2).sum() == 300 and (s["bits"] == 3).sum() == 300
    assert B.valid_mask(s).sum() == 600


def test_exempt_photons_are_under_one_percent():
    """only valid slots with a NaN or inf coordinate are exempt from the cell check, and only `nonfinite` has any"""
    for name in B.CASES:
        c = B.case(name)
        ex, valid = int(B.exempt_mask(c.slots).sum()), int(B.valid_mask(c.slots).sum())
        assert ex == (4 if name == "nonfinite" else 0), name
        assert ex * 100 < max(valid, 1), name
        assert (B.keys(c.slots, c.grid) == -2).sum() == ex
    for est, span in ((0, 2), (0, 3), (PM_ESTIMATOR_KNN, 2)):
        assert not B.exempt_mask(B.reuse_case(est, span).slots).any()
    s = B.case("nonfinite").slots
    assert np.isnan(s["p"]).any() and (s["p"] == np.inf).any() and (s["p"] == -np.inf).any()


def test_reuse_grids():
    a, b, c = B.reuse_case(), B.reuse_case(cell_span=3), B.reuse_case(PM_ESTIMATOR_KNN)
    assert a.grid.dims == b.grid.dims == c.grid.dims == (9, 11, 13), "each steered for its own estimator and span"
    assert a.grid.inv_cs != b.grid.inv_cs != c.grid.inv_cs
    # the same box at other radii: a coarser and a finer grid, the finer one beyond the first one's buffers + 50 %
    from pmrender.abi import RenderParams
    coarse = G.Grid(a.scene, RenderParams.from_buffer_copy(a.params), 2)
    pc, pf = RenderParams.from_buffer_copy(a.params), RenderParams.from_buffer_copy(a.params)
    pc.initial_radius2, pf.initial_radius2 = 9.0, 0.09
    coarse, fine = G.Grid(a.scene, pc), G.Grid(a.scene, pf)
    assert coarse.ncells < a.grid.ncells and fine.ncells + 1 > (a.grid.ncells + 1) * 3 // 2


def test_tile_and_view_sizes():
    assert sorted(B.TILE_IMAGES) == [1, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 2049]
    for nt, (W, H) in B.TILE_IMAGES.items():
        assert ((W + 7) // 8) * ((H + 7) // 8) == nt
        pats = B.tile_patterns(nt)
        assert pats["full"].all() and not pats["ends"][0] and not pats["ends"][-1]
        e = pats["edges"]
        for m in range(64, nt, 128):
            assert not e[m - 1] and not e[m], "empty tiles on either side of a wave boundary"
        for m in range(1024, nt, 1024):
            assert not e[m - 2:m + 2].any(), "empty tiles on either side of a step boundary"
        if nt > 64:
            assert e.any() and not e.all()
    # the sort's S = n / 8 groups and n % 8 tail, on the lists the patterns give
    lens = {nt: {k: int(v.sum()) for k, v in B.tile_patterns(nt).items()} for nt in B.TILE_IMAGES}
    assert lens[7]["full"] == 7 and lens[8]["full"] == 8 and lens[9]["full"] == 9 and lens[1]["ends"] == 0
    assert {n % 8 for d in lens.values() for n in d.values()} == set(range(8))
    assert G.num_records(B.box_scene((2, 2, 2), 64, 32)[0]) + 1 == 2049
    assert G.num_records(B.box_scene((2, 2, 2), 248, 8)[0]) + 1 == 1985
    assert G.num_records(B.box_scene((2, 2, 2), 13, 9)[0]) == 256
    rng = np.random.RandomState(0)
    sc = B.box_scene((2, 2, 2), 72, 8)[0]
    on = np.array([0, 1, 1, 0, 1, 0, 0, 1, 1], bool)
    recs = B.tile_records(sc, on, rng)
    assert B.tile_list_ref(recs).tolist() == [1, 2, 4, 7, 8]
    assert (B.active(recs).reshape(-1, 64).sum(axis=1)[on] >= 1).all()
    assert B.view_ref(recs).tolist() == np.flatnonzero(B.active(recs)).tolist()
    p = B.view_patterns(256)
    assert p["all"].all() and not p["none"].any() and p["alternating"].sum() == 128 and np.flatnonzero(p["last"]).tolist() == [255]


# ---- assert_map rejects what is wrong ---------------------------------------------
@pytest.fixture(scope="module")
def good():
    c = B.case("invalid_mix")
    cs, a, b = B.expected_map(c.slots, c.grid)
    B.assert_map(cs, a, b, c.slots, c.grid)
    return c, cs, a, b


def _busy_cell(cs, least=2):
    """a cell with >= least photons whose neighbour also has one"""
    cnt = np.diff(cs.astype(np.int64))
    return int(np.flatnonzero((cnt[:-1] >= least) & (cnt[1:] >= 1))[0])


def test_checker_accepts_any_order_inside_a_cell(good):
    c, cs, a, b = good
    k = _busy_cell(cs)
    a2, b2 = a.copy(), b.copy()
    j = int(cs[k])
    a2[[j, j + 1]], b2[[j, j + 1]] = a[[j + 1, j]], b[[j + 1, j]]
    B.assert_map(cs, a2, b2, c.slots, c.grid)
    for name in B.CASES:  # and the reference map of every case
        cc = B.case(name)
        B.assert_map(*B.expected_map(cc.slots, cc.grid), cc.slots, cc.grid)


def test_checker_rejects_a_photon_in_the_neighbouring_cell(good):
    """the last photon of cell k handed to cell k + 1: rows untouched, one boundary moved"""
    c, cs, a, b = good
    k = _busy_cell(cs)
    cs2 = cs.copy()
    cs2[k + 1] -= 1
    j = int(cs2[k + 1])
    slot = int(B.u32(b)[j, 1, 1])
    with pytest.raises(AssertionError, match=rf"photon {j} \(slot {slot}\): expected cell {k}, actual cell {k + 1}"):
        B.assert_map(cs2, a, b, c.slots, c.grid)


def test_checker_rejects_rows_swapped_across_cells(good):
    c, cs, a, b = good
    k = _busy_cell(cs)
    j, j2 = int(cs[k]), int(cs[k + 1])
    a2, b2 = a.copy(), b.copy()
    a2[[j, j2]], b2[[j, j2]] = a[[j2, j]], b[[j2, j]]
    with pytest.raises(AssertionError, match=rf"photon {j} \(slot \d+\): expected cell {k + 1}, actual cell {k}"):
        B.assert_map(cs, a2, b2, c.slots, c.grid)


def test_checker_rejects_a_dropped_photon(good):
    c, cs, a, b = good
    k = _busy_cell(cs)
    j = int(cs[k])
    cs2 = cs.copy()
    cs2[k + 1:] -= 1
    with pytest.raises(AssertionError, match="photons, 700 valid slots"):
        B.assert_map(cs2, np.delete(a, j, 0), np.delete(b, j, 0), c.slots, c.grid)
    # the count kept, the photon's place taken by a shifted tail: a slot is missing and another doubled
    a2, b2 = a.copy(), b.copy()
    a2[j:-1], b2[j:-1] = a[j + 1:], b[j + 1:]
    with pytest.raises(AssertionError, match=r"slot \d+ appears 2 times"):
        B.assert_map(cs, a2, b2, c.slots, c.grid)


def test_checker_rejects_a_duplicated_photon(good):
    c, cs, a, b = good
    k = _busy_cell(cs)
    j = int(cs[k])
    a2, b2 = a.copy(), b.copy()
    a2[j + 1], b2[j + 1] = a[j], b[j]
    slot = int(B.u32(b)[j, 1, 1])
    with pytest.raises(AssertionError, match=rf"slot {slot} appears 2 times: photons \[{j}, {j + 1}\]"):
        B.assert_map(cs, a2, b2, c.slots, c.grid)


@pytest.mark.parametrize("word", [2, 3])
def test_checker_rejects_a_nonzero_pad_word(good, word):
    c, cs, a, b = good
    b2 = b.copy()
    B.u32(b2)[311, 1, word] = 1
    with pytest.raises(AssertionError, match=r"photon 311 \(slot \d+, expected cell \d+, actual cell \d+\): rows"):
        B.assert_map(cs, a, b2, c.slots, c.grid)
    b2 = b.copy()
    B.u32(b2)[311, 1, word] = 0x80000000  # -0.0 is not 0
    with pytest.raises(AssertionError, match="photon 311"):
        B.assert_map(cs, a, b2, c.slots, c.grid)


def test_checker_rejects_a_wrong_slot_index(good):
    c, cs, a, b = good
    invalid = int(np.flatnonzero(~B.valid_mask(c.slots))[0])
    other = int(B.u32(b)[12, 1, 1])
    for j, wrong, msg in ((40, invalid, "no valid slot"), (40, len(c.slots), "no valid slot"),
                          (40, other, rf"slot {other} appears 2 times")):
        b2 = b.copy()
        B.u32(b2)[j, 1, 1] = wrong
        with pytest.raises(AssertionError, match=msg):
            B.assert_map(cs, a, b2, c.slots, c.grid)


def test_checker_rejects_every_single_bit_of_a_row(good):
    c, cs, a, b = good
    for w in range(4):
        a2 = a.copy()
        B.u32(a2)[5, w] ^= 1
        with pytest.raises(AssertionError, match="photon 5"):
            B.assert_map(cs, a2, b, c.slots, c.grid)
    for h, w in ((0, 0), (0, 1), (0, 2), (0, 3), (1, 0)):
        b2 = b.copy()
        B.u32(b2)[5, h, w] ^= 1
        with pytest.raises(AssertionError, match="photon 5"):
            B.assert_map(cs, a, b2, c.slots, c.grid)


def test_checker_rejects_cell_start_off_by_one_from_a_cell_on(good):
    c, cs, a, b = good
    empty = int(np.flatnonzero(np.diff(cs.astype(np.int64)) == 0)[3])
    for k, d in ((_busy_cell(cs) + 1, 1), (empty + 1, 1), (_busy_cell(cs) + 1, -1)):
        cs2 = cs.copy()
        cs2[k:] = (cs2[k:].astype(np.int64) + d).astype(np.uint32)
        with pytest.raises(AssertionError):
            B.assert_map(cs2, a, b, c.slots, c.grid)
    # the total kept, every boundary from k on but the last moved
    k = _busy_cell(cs) + 1
    cs2 = cs.copy()
    cs2[k:-1] -= 1
    with pytest.raises(AssertionError, match=r"expected cell \d+, actual cell \d+"):
        B.assert_map(cs2, a, b, c.slots, c.grid)
    with pytest.raises(AssertionError):
        B.assert_map(cs[:-1], a, b, c.slots, c.grid)


def test_checker_places_exempt_photons_anywhere_but_once(good):
    c = B.case("nonfinite")
    cs, a, b = B.expected_map(c.slots, c.grid)
    B.assert_map(cs, a, b, c.slots, c.grid)
    # the exempt photons in the last cell instead of the first: still a correct map
    ex = np.flatnonzero(B.exempt_mask(c.slots))
    idx = B.u32(b)[:, 1, 1]
    mine = np.isin(idx, ex)
    assert mine.sum() == 4 and (B.cell_of(cs, np.flatnonzero(mine)) == 0).all()
    order = np.concatenate([np.flatnonzero(~mine), np.flatnonzero(mine)])
    cs2 = cs.copy()
    cs2[1:-1] -= 4
    B.assert_map(cs2, a[order], b[order], c.slots, c.grid)
    # one of them dropped, or its row altered
    a3, b3, cs3 = a[order][:-1], b[order][:-1], cs2.copy()
    cs3[-1] -= 1
    with pytest.raises(AssertionError, match="valid slots"):
        B.assert_map(cs3, a3, b3, c.slots, c.grid)
    a4 = a[order].copy()
    B.u32(a4)[-1, 3] ^= 1
    with pytest.raises(AssertionError, match=f"photon {len(a4) - 1}"):
        B.assert_map(cs2, a4, b[order], c.slots, c.grid)


# ---- assert_sorted ---------------------------------------------------------------------
def _lists(n, seed=3):
    rng = np.random.RandomState(seed)
    un = np.sort(rng.choice(4 * n + 8, n, replace=False)).astype(np.uint32)
    S = n // 8
    order = rng.permutation(S)
    so = np.concatenate([un[:8 * S].reshape(S, 8)[order].ravel(), un[8 * S:]]).astype(np.uint32)
    return un, so


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65, 1023, 1025])
def test_assert_sorted_accepts_whole_groups_in_any_order(n):
    un, so = _lists(n)
    B.assert_sorted(un, so)
    B.assert_sorted(un, un)
    if n >= 16:
        assert not np.array_equal(un, so)


def test_assert_sorted_rejects_a_dropped_group():
    un, so = _lists(67)
    with pytest.raises(AssertionError, match="59 entries, the compact one 67"):
        B.assert_sorted(un, np.concatenate([so[:8], so[16:]]))
    lost = so.copy()
    lost[8:16] = so[0:8]  # its place taken by a copy of another group
    with pytest.raises(AssertionError, match="appears twice"):
        B.assert_sorted(un, lost)


def test_assert_sorted_rejects_entries_exchanged_between_groups():
    un, so = _lists(67)
    bad = so.copy()
    bad[[3, 5, 19, 22]] = so[[19, 22, 3, 5]]
    with pytest.raises(AssertionError, match="no aligned group"):
        B.assert_sorted(un, bad)
    bad = so.copy()
    bad[[1, 2]] = so[[2, 1]]  # a group must stay intact in its order too
    with pytest.raises(AssertionError, match="no aligned group"):
        B.assert_sorted(un, bad)


def test_assert_sorted_rejects_a_moved_tail():
    un, so = _lists(67)
    bad = np.concatenate([so[64:], so[:64]])
    with pytest.raises(AssertionError):
        B.assert_sorted(un, bad)
    bad = so.copy()
    bad[[64, 66]] = so[[66, 64]]
    with pytest.raises(AssertionError, match="last 3 entries moved"):
        B.assert_sorted(un, bad)
    un7, so7 = _lists(7)
    with pytest.raises(AssertionError, match="last 7 entries moved"):
        B.assert_sorted(un7, so7[::-1])


# ---- the hooks' argument checks, no device ---------------------------------------------
def test_argument_checks_of_the_hooks():
    lib = hip.load_library()
    err = lambda: lib.pm_last_error(None)
    u = (ctypes.c_uint32 * 4)()
    f = (ctypes.c_float * 8)()
    i3, i64, ci = (ctypes.c_int32 * 3)(), ctypes.c_int64(), ctypes.c_int()
    for fn in (lib.pm_download_map_cell_start, lib.pm_download_map_counters):
        name = fn.__name__.encode()
        assert fn(None, u, 1) == PM_ERR_INVALID and name + b": null context" in err()
        assert fn(None, None, 1) == PM_ERR_INVALID and name + b": null pointer" in err()
        assert fn(None, u, -1) == PM_ERR_INVALID and name + b": negative size" in err()
    fn = lib.pm_download_map_photons
    assert fn(None, f, f, 1) == PM_ERR_INVALID and b"pm_download_map_photons: null context" in err()
    assert fn(None, None, f, 1) == PM_ERR_INVALID and b"pm_download_map_photons: null pointer" in err()
    assert fn(None, f, None, 1) == PM_ERR_INVALID and b"pm_download_map_photons: null pointer" in err()
    assert fn(None, f, f, -1) == PM_ERR_INVALID and b"pm_download_map_photons: negative size" in err()
    fn = lib.pm_map_grid
    assert fn(None, i3, f, u) == PM_ERR_INVALID and b"pm_map_grid: null context" in err()
    for args in ((None, f, u), (i3, None, u), (i3, f, None)):
        assert fn(None, *args) == PM_ERR_INVALID and b"pm_map_grid: null pointer" in err()
    fn = lib.pm_download_tile_list
    assert fn(None, u, 4, ctypes.byref(i64), ctypes.byref(ci)) == PM_ERR_INVALID and b"pm_download_tile_list: null context" in err()
    assert fn(None, u, 4, None, ctypes.byref(ci)) == PM_ERR_INVALID and b"pm_download_tile_list: null pointer" in err()
    assert fn(None, u, 4, ctypes.byref(i64), None) == PM_ERR_INVALID and b"pm_download_tile_list: null pointer" in err()
    assert fn(None, u, -1, ctypes.byref(i64), ctypes.byref(ci)) == PM_ERR_INVALID and b"pm_download_tile_list: negative size" in err()
    fn = lib.pm_record_view_size
    assert fn(None, ctypes.byref(i64)) == PM_ERR_INVALID and b"pm_record_view_size: null context" in err()
    assert fn(None, None) == PM_ERR_INVALID and b"pm_record_view_size: null pointer" in err()
