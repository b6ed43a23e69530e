"""CPU tests of the directed gather cases (gather_ref.py): the brute-force
reference against the oracle's kd-tree gather and against plain float64, the
conditions on the inputs (no record x photon pair whose membership depends on
the rounding; exact flux sums), and per case the tile_profile precondition:
the branch of k_gather_tile the case was built for is the one its inputs
reach. A failing precondition is a failure, never a skip."""
import numpy as np
import pytest

import gather_ref as G
from parity_util import compare_gathered_records, compare_knn_records, knn_term_floor, u32

PPM = sorted(G.CASES)
KNN = sorted(G.KNN_CASES)


def _states(name):
    """the record states a case gathers from: its upload, and for `progressive` the states of its passes"""
    return [st[0] for st in G.states(name)]


def test_fx_shift_of_the_cornell_box():
    """2^40 / (17 * area * 2 pi * (1 / pi) * 4) = 2^40 / (136 * area), area = pi 65^2: S = 19"""
    sc, p, _, _ = G.case("windows")
    assert G.fx_shift(sc, p) == int(np.floor(np.log2(2.0 ** 40 / (136.0 * np.pi * 65.0 ** 2)))) == 19


@pytest.mark.parametrize("name", PPM)
def test_reference_agrees_with_the_oracle(name, oracle_mod):
    """ppm_partial_ref + ppm_update_ref against Oracle.build_kdtree + gather_partial / gather: M, N' and r2
    exact, flux within compare_gathered_records' tolerance"""
    sc, p, _, slots = G.case(name)
    S = G.fx_shift(sc, p)
    orc = sc.load_into(oracle_mod.Oracle())
    nodes = oracle_mod.Oracle.build_kdtree(slots)
    assert len(nodes) == int((slots["bits"] & 1).sum())
    for recs in _states(name):
        M, L = G.ppm_partial_ref(recs, slots, sc.materials, S)
        part = orc.gather_partial(nodes, recs)
        assert np.array_equal(part[:, 0].astype(np.int64), M)
        Lf = L.astype(np.float64) * 2.0 ** -S
        assert (np.abs(part[:, 1:] - Lf) <= 2e-5 * np.maximum(np.abs(Lf), 1e-30)).all()
        ref = recs.copy()
        orc.gather(nodes, ref, p)
        compare_gathered_records(G.apply_update(recs, M, L, S, p.ppm_alpha), ref)
        assert M.max() > 0


@pytest.mark.parametrize("name", PPM)
def test_conditions_on_the_inputs(name):
    """no ambiguous pair (float64 and float32-order membership agree for every pair, none within 8 2^-24 of
    r2 unless exactly decided), the float32-order sums within flux_bound of float64, |sum| < 2^62 and,
    outside beyond_2p53 and signed, every sum below 2^53"""
    sc, p, _, slots = G.case(name)
    S = G.fx_shift(sc, p)
    for recs in _states(name):
        assert len(G.ambiguous_pairs(recs, slots)) == 0
        M, L = G.ppm_partial_ref(recs, slots, sc.materials, S)
        M64, L64, A = G.ppm_partial_f64(recs, slots, sc.materials)
        assert np.array_equal(M, M64)
        assert (np.abs(L.astype(np.float64) * 2.0 ** -S - L64) <= G.flux_bound(A, M, S)).all()
        assert np.abs(L).max() < 2 ** 62
        if name == "beyond_2p53":
            over = (L >= 2 ** 53).all(axis=1)
            assert over.sum() == 1 and over[9] and (L[9] <= 2 ** 61).all()
            assert (L[~over] < 2 ** 53).all() and (M[:64] > 0).all() and (L[:64] > 0).all()
        elif name != "signed":
            assert (L >= 0).all() and L.max() < 2 ** 53
        live = ~G.inactive(recs)
        assert (M[~live] == 0).all() and (L[~live] == 0).all()


def _tiles(name, span=2):
    sc, p, recs, slots = G.case(name)
    prof = G.tile_profile(sc, p, recs, slots, span)
    return prof, prof["tiles"], recs, slots


def _one_group(T, lanes=64):
    return len(T["groups"]) == 1 and T["groups"][0]["lanes"] == lanes and T["pitch_rows"] <= 64


def test_precondition_boundary_exact():
    prof, tiles, recs, slots = _tiles("boundary_exact")
    ph = slots[(slots["bits"] & 1) != 0]
    eq = inside = outside = 0
    for i in range(len(recs)):
        d2 = G.d2_f32(recs["pos"][i], ph["p"])
        eq += int((d2 == recs["radius2"][i]).sum())
        inside += int((np.abs(d2 - 8.0) < 1.0).sum())
        outside += int((np.abs(d2 - 10.0) < 1.0).sum())
    assert eq >= 6 * 4 * 30 and inside > 1000 and outside > 1000
    assert ((slots["bits"] & 1) == 0).sum() > 50
    assert all(_one_group(T) and T["groups"][0]["staged"] for T in tiles)


def test_precondition_cell_edges():
    prof, tiles, recs, slots = _tiles("cell_edges")
    sc, p, _, _ = G.case("cell_edges")
    g = G.Grid(sc, p)
    c = g.cells(slots["p"])
    up = g.cells(np.nextafter(slots["p"], np.float32(np.inf)))
    down = g.cells(np.nextafter(slots["p"], np.float32(-np.inf)))
    assert ((up != c) | (down != c)).any(axis=1).all(), "every photon is the float32 neighbour of a cell plane"
    for a in range(3):
        assert c[:, a].min() == 0 and c[:, a].max() == g.dims[a] - 1, "first and last cell of the axis"
    rq = G.box_reach(recs["radius2"])
    ends = 0
    for a in range(3):
        for e in (recs["pos"][:, a] - rq, recs["pos"][:, a] + rq):
            e = e.astype(np.float32)
            ends += int(((g.cell(np.nextafter(e, np.float32(np.inf)), a) != g.cell(e, a)) |
                         (g.cell(np.nextafter(e, np.float32(-np.inf)), a) != g.cell(e, a))).sum())
    assert ends >= 6 * 24, "records whose box ends within an ulp of a plane"
    assert all(T["groups"] and T["U"] > 0 for T in tiles)


def test_precondition_outside_bbox():
    prof, tiles, recs, slots = _tiles("outside_bbox")
    sc, p, _, _ = G.case("outside_bbox")
    g = G.Grid(sc, p)
    lo, hi = G.pass_plan_ref.scene_bbox(sc)
    for pts in (recs["pos"], slots["p"]):
        for a in range(3):
            below, above = (lo[a] - pts[:, a]) / g.cs, (pts[:, a] - hi[a]) / g.cs
            for d in (below, above):
                assert ((d > 0) & (d < 0.3)).any() and ((d > 2.5) & (d < 3.5)).any() and (d > 49).any()
    c = g.cells(slots["p"])
    assert all((c[:, a] == 0).any() and (c[:, a] == g.dims[a] - 1).any() for a in range(3))
    assert all(len(T["groups"]) in (2, 3) and T["pitch_rows"] > 64 and T["direct"] == 0 for T in tiles), \
        "the lanes of a tile lie far apart: leader groups, all staged"
    assert any(len(T["groups"]) == 3 for T in tiles)


def test_precondition_ragged_13x9():
    prof, tiles, recs, slots = _tiles("ragged_13x9")
    sc = G.case("ragged_13x9")[0]
    assert (sc.width, sc.height) == (13, 9) and len(recs) == 256 == len(tiles) * 64
    from pmrender.abi import record_pixels
    assert (record_pixels(256, 13, 9) < 0).sum() == 256 - 13 * 9
    assert (recs["flags"] == 0).all() and all(_one_group(T) for T in tiles)


def test_precondition_inactive_mix():
    prof, tiles, recs, slots = _tiles("inactive_mix")
    sc = G.case("inactive_mix")[0]
    t = recs[64:128]
    from pmrender.abi import PM_REC_BACKFACE, PM_REC_EXCEPTION, PM_REC_INVALID, PM_REC_MISS
    for f in (PM_REC_MISS, PM_REC_EXCEPTION, PM_REC_INVALID):
        assert (t["flags"] & f).any()
    assert (t["radius2"] == 0).any() and (t["radius2"] < 0).any() and np.isnan(t["radius2"]).any()
    assert (t["material"] == G.mirror_id(sc)).sum() == 2 and (t["flags"] == PM_REC_BACKFACE).sum() == 2
    dead = G.inactive(t)
    assert 10 <= dead.sum() <= 20 and not dead[[0, 3, 6, 9]].any(), "live lanes between the inactive ones"
    assert _one_group(tiles[1], 64 - int(dead.sum())) and tiles[1]["groups"][0]["staged"]
    S, M, L = G.partial_ref("inactive_mix")
    mirror = np.flatnonzero(recs["material"] == G.mirror_id(sc))
    assert (M[mirror] > 0).all() and (L[mirror] == 0).all()


def test_precondition_row_lengths():
    prof, tiles, recs, slots = _tiles("row_lengths")
    assert [tuple(T["row_len"]) for T in tiles] == G.ROW_LENGTHS
    lens, starts = set(), set()
    for T in tiles:
        assert _one_group(T)
        pre = 0
        for n in T["row_len"]:
            lens.add(n)
            if n:
                starts.add(pre & 1)
            pre += n
    assert lens == {0, 1, 2, 3, 4, 5, 7, 8, 9} and starts == {0, 1}
    S, M, L = G.partial_ref("row_lengths")
    assert (M > 0).sum() > 300


def test_precondition_windows():
    prof, tiles, recs, slots = _tiles("windows")
    assert prof["umax"] == G.TILE_UMAX
    assert [T["U"] for T in tiles] == G.WINDOW_U == [127, 128, 129, 257, 512, 513]
    for T in tiles:
        assert _one_group(T) and T["groups"][0]["staged"] == (T["U"] <= G.TILE_UMAX)
        ends = np.cumsum(T["row_len"])
        for b in range(G.TILE_CAP, T["U"], G.TILE_CAP):  # a row straddles every window boundary
            assert b not in ends and (ends > b).any()
    assert tiles[5]["direct"] == 64 and tiles[5]["coop_tot"] > G.COOP_STEPS * 64


def test_precondition_dense_and_sparse():
    prof, tiles, recs, slots = _tiles("dense_and_sparse.dense")
    assert prof["density"] >= 0.4 and prof["umax"] == G.TILE_UMAX_DENSE and prof["group_min"] == G.GROUP_MIN
    assert [T["U"] for T in tiles] == G.DENSE_U
    for T in tiles:
        assert _one_group(T)
        if T["U"] > G.TILE_UMAX_DENSE:
            assert T["U"] <= G.TILE_UMAX and not T["groups"][0]["staged"] and T["direct"] == 64
        else:
            assert T["groups"][0]["staged"] and T["direct"] == 0
    prof, tiles, recs, slots = _tiles("dense_and_sparse.sparse")
    assert prof["density"] < 1.0 / G.SPARSE_CELLS and prof["group_min"] == G.GROUP_MIN_SPARSE
    for T in tiles:
        assert T["pitch_rows"] > 64 and 5 <= T["below"] <= 11 and not T["groups"] and T["direct"] == 64
    tots = [T["coop_tot"] for T in tiles]
    assert min(tots) <= G.COOP_STEPS * 64 < max(tots), "cooperative and per-lane direct scans"


def test_precondition_depth_edge():
    prof, tiles, recs, slots = _tiles("depth_edge")
    assert prof["group_min"] == G.GROUP_MIN and prof["umax"] == G.TILE_UMAX
    T = tiles[0]
    assert T["rows"] > 64 and T["pitch_rows"] > 64
    assert [gr["lanes"] for gr in T["groups"]] == [21, 21, 20] and all(gr["staged"] for gr in T["groups"])
    assert T["below"] == 1 and T["direct"] == 2, "a stray leads a group of one: both strays scan directly"
    T = tiles[1]
    assert T["below"] == 1 and T["direct"] == 64 and not T["groups"]
    S, M, L = G.partial_ref("depth_edge")
    assert M[62] > 0 and M[63] > 0 and M[64] > 0, "the stray lanes find photons"


@pytest.mark.parametrize("span", [2, 4])
def test_precondition_mixed_radii(span):
    prof, tiles, recs, slots = _tiles("mixed_radii", span)
    T = tiles[2]
    r2 = recs["radius2"][128:192]
    assert sorted(set(r2.tolist())) == [4.0, 16.0, 256.0, 6400.0]
    assert T["big"] == int((r2 > 16.0).sum()) == 16
    assert len(T["groups"]) == 1 and T["groups"][0]["lanes"] == 48 and T["groups"][0]["staged"]
    S, M, L = G.partial_ref("mixed_radii")
    assert M[128:192][r2 == 6400.0].min() > M[128:192][r2 == 256.0].max() > M[128:192][r2 == 16.0].max()


def test_precondition_signed():
    prof, tiles, recs, slots = _tiles("signed")
    assert (slots["alpha"] < 0).any(axis=1).sum() > 10 and (slots["alpha"] < 0).sum(axis=1).tolist().count(1) == 1
    S, M, L = G.partial_ref("signed")
    assert (L[:64] > 0).all() and (L[128:192] < 0).all()
    assert (M[64:128] == 4).all() and (L[64:128] == 0).all(), "sums that cancel to exactly 0"
    assert all(_one_group(T) and T["groups"][0]["staged"] for T in tiles[:3])


def test_precondition_beyond_2p53():
    prof, tiles, recs, slots = _tiles("beyond_2p53")
    T = tiles[0]
    assert _one_group(T) and T["groups"][0]["staged"] and T["U"] == 220 <= G.TILE_UMAX_DENSE
    assert (slots["alpha"] == 2.0 ** 30).all(axis=1).sum() == 100


def test_precondition_progressive():
    states = _states("progressive")
    sc, p, recs, slots = G.case("progressive")
    assert len(states) == G.PROGRESSIVE_PASSES + 1
    for a, b in zip(states[:3], states[1:3]):
        assert (b["radius2"] <= a["radius2"]).all() and (b["radius2"] < a["radius2"]).sum() > 300
    assert (recs["radius2"] <= p.initial_radius2).all() and (recs["photon_count"] > 0).any()
    assert all(_one_group(T, 64 - (t in (0, 3))) for t, T in enumerate(_tiles("progressive")[1]))


def test_ppm_update_ref_against_the_oracle(oracle_mod):
    """ppm_update_ref against the oracle's scalar ppm_update, bit for bit, truncation of N + alpha M included"""
    import ctypes
    rng = np.random.RandomState(7)
    lib = oracle_mod.load()
    n = 500
    flux, r2 = rng.uniform(0, 9, (n, 3)).astype(np.float32), rng.uniform(0.1, 30, n).astype(np.float32)
    N, M = rng.randint(0, 50, n).astype(np.float32), rng.randint(0, 40, n)
    L = rng.randint(0, 2 ** 40, (n, 3))
    for alpha in (0.7, 0.5, 1.0):
        f2, r22, N2 = G.ppm_update_ref((flux, r2, N), M, L, 19, alpha)
        for i in range(n):
            rr, nn = ctypes.c_float(r2[i]), ctypes.c_float(N[i])
            ff = (ctypes.c_float * 3)(*flux[i])
            Lf = (ctypes.c_float * 3)(*(L[i].astype(np.float64) * 2.0 ** -19).astype(np.float32))
            lib.orc_ppm_update(ctypes.byref(rr), ctypes.byref(nn), ff, int(M[i]), Lf, alpha)
            got = np.float32([ff[0], ff[1], ff[2], rr.value, nn.value])
            assert np.array_equal(u32(got), u32(np.float32([*f2[i], r22[i], N2[i]]))), i


# ---- kNN ---------------------------------------------------------------------
@pytest.mark.parametrize("name", KNN)
def test_knn_reference_agrees_with_the_oracle(name, oracle_mod):
    sc, p, recs, slots = G.case(name)
    found, r2, Sum, live = G.knn_ref(sc, recs, slots, p.knn_lookup, p.initial_radius2)
    orc = sc.load_into(oracle_mod.Oracle())
    ref = recs.copy()
    ref["flux"] = 0.0
    orc.gather(oracle_mod.Oracle.build_kdtree(slots), ref, p)
    floor = knn_term_floor(sc, found, r2)
    compare_knn_records(ref[live], found[live], r2[live], Sum[live], floor=floor[live])
    assert np.array_equal(u32(ref[~live]["radius2"]), u32(recs[~live]["radius2"]))


def test_precondition_knn_counts():
    for K in (1, 2, 50, 64):
        sc, p, recs, slots = G.case(f"knn_counts[K={K}]")
        found, r2, Sum, live = G.knn_ref(sc, recs, slots, K, p.initial_radius2)
        ph = slots[(slots["bits"] & 1) != 0]
        inside = np.array([(G.d2_f32(recs["pos"][i], ph["p"]) < np.float32(G.KNN_R2)).sum() for i in range(128)])
        assert inside.tolist() == [max(K - 1 + i % 3, 0) for i in range(128)]
        assert (found[:128] == np.minimum(inside, K)).all()
        under = inside < K
        assert (r2[:128][under] == np.float32(G.KNN_R2)).all() and (r2[:128][~under] < np.float32(G.KNN_R2)).all()
        for i in np.flatnonzero(inside == K + 1):  # r_k^2 shrinks to the K-th of the K + 1 distances
            d2 = np.sort(G.d2_f32(recs["pos"][i], ph["p"]))
            assert r2[i] == d2[K - 1] < d2[K]
        assert np.isfinite(Sum).all()  # K = 1: the one photon kept lies at r_k^2, its weight is 0
        assert K == 1 or (Sum[:128][inside >= K] > 0).any()


def test_precondition_knn_ties_and_zero():
    sc, p, recs, slots = G.case("knn_ties")
    found, r2, Sum, live = G.knn_ref(sc, recs, slots, 8, p.initial_radius2)
    ph = slots[(slots["bits"] & 1) != 0]
    for i in range(96):
        d2 = G.d2_f32(recs["pos"][i], ph["p"])
        assert (d2 < 9.0).sum() == 5 and (d2 == 9.0).sum() == 6 and (d2 < np.float32(G.KNN_R2)).sum() == 13
    assert (found[:96] == 8).all() and (r2[:96] == 9.0).all() and (np.abs(Sum[:96]).sum(axis=1) > 0).all()
    sc, p, recs, slots = G.case("knn_zero")
    found, r2, Sum, live = G.knn_ref(sc, recs, slots, 4, p.initial_radius2)
    assert (found[:64] == 4).all()
    assert (r2[0:64:2] == 0).all() and np.isnan(Sum[0:64:2]).all()
    assert (r2[1:64:2] == 5.8125).all() and np.isfinite(Sum[1:64:2]).all() and (Sum[1:64:2] > 0).all()
    sc, p, recs, slots = G.case("knn_ragged")
    found, r2, Sum, live = G.knn_ref(sc, recs, slots, 5, p.initial_radius2)
    assert len(recs) == 256 and (~live).sum() == 5 and (found[live] == 5).sum() > 100 and (found[live] < 5).sum() > 20


def test_precondition_knn_shell():
    sc, p, recs, slots = G.case("knn_shell")
    found, r2, Sum, live = G.knn_ref(sc, recs, slots, 50, p.initial_radius2)
    lo, hi = np.float32(G.SHELL_D2[0]), np.float32(G.SHELL_D2[1])
    assert live.sum() == 64 and (found[live] == 50).all() and (found[~live] == 0).all()
    assert ((r2[live] > lo) & (r2[live] < hi)).all()
    assert (recs["flags"][live] != 0).sum() == 3 and np.isfinite(Sum).all() and (np.abs(Sum[live]).sum(axis=1) > 0).all()
    ph = slots[(slots["bits"] & 1) != 0]
    d2 = G.d2_f32(recs["pos"][0], ph["p"])
    assert len(np.unique(d2)) == len(d2) == 270 and (d2 < 40.0).sum() == 30 and ((d2 >= lo) & (d2 <= hi)).sum() == 240
    # the scalar stream's bins are runs of d2 bit patterns: 2^19 wide at level 0 (maxD^2 = 100 and 64 lie
    # a whole number of them apart), 2^14 after one refinement, 2^9 after two. The shell lies in one
    # level-0 bin, and the bin of the 50th after one refinement holds more than the 12 values a COLLECT keeps
    bits, top, kth = u32(d2).astype(np.int64), int(u32(np.float32([G.KNN_R2]))[0]), int(u32(r2[:1])[0])
    base = int(u32(np.float32([lo]))[0])
    assert (top - base) % (1 << 19) == 0 and (bits[d2 >= lo] - base < (1 << 19)).all()
    assert ((bits - base) >> 14 == (kth - base) >> 14).sum() > 12
    # the tile kernel's first histogram: 32 equal bins of [0, maxD^2), the shell in one of them
    assert len(np.unique((d2[d2 >= lo] * np.float32(32.0 / G.KNN_R2)).astype(np.int64))) == 1
