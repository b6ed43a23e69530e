"""Directed gather cases and their references (numpy only), for
test_gather_directed.py (CPU) and test_gather_directed_gpu.py.

The gathers claim an exact result: M is the number of valid photons with
d^2 < r^2 (d^2 in float32, the kernels' operation order), r^2 follows from M
bit for bit, and the flux is the exact integer sum of rint(c 2^S) over those
photons. ppm_partial_ref states that as a brute force over every record x
photon pair, ppm_update_ref the PPM update (pm_gather_dev.h ppm_apply) on top
of it, ppm_partial_f64 the same query in plain float64 (it certifies the
inputs: no pair whose membership depends on the rounding). tile_profile
restates the prologue of k_gather_tile (pm_gather.hip) so that every case
asserts, on the CPU, that it reaches the branch it was built for.

CASES: name -> builder of (scene, params, recs, slots). Records and photons
are uploaded, so they lie wherever a case needs them: on a dyadic lattice
(multiples of 1/4: every d^2 is exact in float32 and d^2 == r^2 is decided)
unless the case is about float32 neighbours of the grid's cell planes."""
import numpy as np

import pass_plan_ref
from parity_util import knn_reference
from pmrender import scenes
from pmrender.abi import (PHOTON_DTYPE, PM_ESTIMATOR_KNN, PM_GATHER_GRID, PM_MATTE, PM_MIRROR, PM_REC_BACKFACE,
                          PM_REC_EXCEPTION, PM_REC_INACTIVE, PM_REC_INVALID, PM_REC_MISS, RECORD_DTYPE, RenderParams)

f32 = np.float32
INV_PI = f32(0.31830988618379067154)  # pm_math.h INV_PI

# pm_gather.hip, by macro
TILE_CAP = 128          # PM_TILE_CAP: photons per LDS window
TILE_UMAX = 512         # PM_TILE_UMAX: a union above it is scanned per lane
TILE_UMAX_DENSE = 256   # PM_TILE_UMAX_DENSE: the same for a dense map
GROUP_MIN = 4           # PM_GROUP_MIN: lanes a leader group needs
GROUP_MIN_SPARSE = 12   # PM_GROUP_MIN_SPARSE: the same for a sparse map
SPARSE_CELLS = 20       # SPARSE_CELLS: sparse = under one photon per 20 cells
GROUP_R = 3             # PM_GROUP_R: a leader group's reach in cells (span 2)
COOP_STEPS = 8          # GatherParams::coop_steps of a scene traversed from LDS (pm_api_gather.cpp gather_params)

WHITE = 0               # material ids of _scene(): scenes.cornell_box's white matte ...


def _scene(W=24, H=16):
    """The small Cornell box with one extra PM_MIRROR material (the last id)."""
    sc = scenes.cornell_box(W, H)
    sc.material(PM_MIRROR, (1.0, 1.0, 1.0))
    return sc


def mirror_id(scene):
    return len(scene.materials) - 1


def num_records(scene):
    return ((scene.width + 7) // 8) * ((scene.height + 7) // 8) * 64


# ---- the references ----------------------------------------------------------
def inactive(recs):
    """records that gather nothing: a flag of PM_REC_INACTIVE, r2 <= 0 or NaN"""
    return ((recs["flags"] & PM_REC_INACTIVE) != 0) | ~(recs["radius2"] > 0)


def _matte_fv(materials, mat):
    """Kd * float32(1/pi) of a matte material (float32), 0 for any other"""
    mtype, rgb = materials[mat]
    if mtype != PM_MATTE:
        return np.zeros(3, f32)
    return np.asarray(rgb, f32) * INV_PI


def d2_f32(p, q):
    """|p - q|^2 as the kernels form it: diff = p - q, (dx dx + dy dy) + dz dz, all float32"""
    diff = np.asarray(p, f32)[None, :] - np.asarray(q, f32)
    return (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]


def ppm_partial_ref(recs, slots, materials, S):
    """(M [n] int64, L [n, 3] int64): per record the valid photons with d2 < r2 and the exact sum of
    rint(c 2^S), c = |(ns.x wi.x + ns.y wi.y) + ns.z wi.z| (Kd float32(1/pi)) alpha in float32."""
    ph = slots[(slots["bits"] & 1) != 0]
    n = len(recs)
    M, L = np.zeros(n, np.int64), np.zeros((n, 3), np.int64)
    scale = f32(2.0 ** S)
    dead = inactive(recs)
    for i in range(n):
        if dead[i]:
            continue
        hit = d2_f32(recs["pos"][i], ph["p"]) < recs["radius2"][i]
        M[i] = int(hit.sum())
        fv = _matte_fv(materials, int(recs["material"][i]))
        ns, wi, al = recs["ns"][i], ph["wi"][hit], ph["alpha"][hit]
        dot = np.abs((ns[0] * wi[:, 0] + ns[1] * wi[:, 1]) + ns[2] * wi[:, 2])
        c = (dot[:, None] * fv[None, :]) * al
        assert c.dtype == np.float32
        L[i] = np.rint(c * scale).astype(np.int64).sum(axis=0)
    return M, L


def ppm_partial_f64(recs, slots, materials):
    """The same query in float64 throughout: (M, L [n, 3] float64, A [n, 3]: the sum of the terms'
    magnitudes with |ns_i wi_i| summed in place of the signed dot, flux_bound's scale)."""
    ph = slots[(slots["bits"] & 1) != 0]
    n = len(recs)
    M, L, A = np.zeros(n, np.int64), np.zeros((n, 3)), np.zeros((n, 3))
    P, wi64, al64 = ph["p"].astype(np.float64), ph["wi"].astype(np.float64), ph["alpha"].astype(np.float64)
    dead = inactive(recs)
    for i in range(n):
        if dead[i]:
            continue
        d = recs["pos"][i].astype(np.float64)[None, :] - P
        hit = (d * d).sum(axis=1) < np.float64(recs["radius2"][i])
        M[i] = int(hit.sum())
        mtype, rgb = materials[int(recs["material"][i])]
        if mtype != PM_MATTE:
            continue
        fv = np.asarray(rgb, f32).astype(np.float64) / np.pi
        prod = recs["ns"][i].astype(np.float64)[None, :] * wi64[hit]
        L[i] = ((np.abs(prod.sum(axis=1))[:, None] * fv[None, :]) * al64[hit]).sum(axis=0)
        A[i] = ((np.abs(prod).sum(axis=1)[:, None] * fv[None, :]) * np.abs(al64[hit])).sum(axis=0)
    return M, L, A


def ambiguous_pairs(recs, slots):
    """[photon index among the valid ones] of the pairs the no-ambiguity condition forbids: the float64
    membership differs from the float32-order one, or (coordinates off the lattice)
    |d2_64 - r2| <= 8 2^-24 max(d2_64, r2) without d2 being the exactly representable r2."""
    ph = slots[(slots["bits"] & 1) != 0]
    P = ph["p"].astype(np.float64)
    bad = np.zeros(len(ph), bool)
    dead = inactive(recs)
    for i in range(len(recs)):
        if dead[i]:
            continue
        d = recs["pos"][i].astype(np.float64)[None, :] - P
        d64 = (d * d).sum(axis=1)
        d32 = d2_f32(recs["pos"][i], ph["p"])
        r2 = recs["radius2"][i]
        exact = d32.astype(np.float64) == d64
        near = np.abs(d64 - np.float64(r2)) <= 8 * 2.0 ** -24 * np.maximum(d64, np.float64(r2))
        bad |= ((d64 < np.float64(r2)) != (d32 < r2)) | (near & ~exact)
    return np.flatnonzero(bad)


def flux_bound(A, M, S, kd_tree=False):
    """|float32-order reference - float64| per record and channel: per term half a unit of 2^-S (the
    rint) plus 8 2^-24 of its magnitude (three products, two sums, Kd (1/pi), two multiplies, each one
    float32 rounding); A: ppm_partial_f64's magnitudes. kd_tree: the bound of the kd-tree kernel's
    float sum against float64 instead (no per-term rint but M float additions, each 2^-24 of the
    running sum <= A, and one rint of the sum)."""
    M = np.asarray(M, np.float64)[:, None]
    if kd_tree:
        return 0.5 * 2.0 ** -S + (8 + M) * 2.0 ** -24 * A
    return M * 0.5 * 2.0 ** -S + 8 * 2.0 ** -24 * A


def fx_shift(scene, params):
    """S of the gathers' fixed point 2^S (pm_api_gather.cpp gather_params)."""
    em = 0.0
    for L in scene.lights:
        if L[0] == "point":
            em = max(em, float(np.abs(f32(L[2])).max()) * 4.0 * np.pi)
        else:
            assert L[0] == "disk"
            em = max(em, float(np.abs(f32(L[5])).max()) * float(f32(L[6])) * 2.0 * np.pi)
    kd = 1.0
    for mtype, rgb in scene.materials:
        if mtype == PM_MATTE:
            kd = max(kd, float(np.max(np.asarray(rgb, f32))))
    bound = max(em, 1e-30) * kd ** params.max_photon_count  # flux_bound: no physical specular material here
    cmax = bound * (kd / np.pi) * 4.0
    return int(max(-60, min(60, np.floor(np.log2(2.0 ** 40 / max(cmax, 1e-30))))))


def ppm_update_ref(state, M, L_int, S, alpha):
    """ppm_apply (gathering.cu:104-126) of (flux [n, 3], r2 [n], N [n]) float32 with L = float32(L_int 2^-S):
    int total = N + alpha M; ratio = total / (N + M); r2 *= ratio; flux = (flux + L) ratio; N = total."""
    flux, r2, N = (np.array(a, f32) for a in state)
    M = np.asarray(M, np.int64)
    L = (np.asarray(L_int, np.int64).astype(np.float64) * 2.0 ** -S).astype(f32)
    Mf = M.astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        total = (N + f32(alpha) * Mf).astype(np.int32)
        ratio = total.astype(f32) / (N + Mf)
        go = M > 0
        r2n = np.where(go, r2 * ratio, r2)
        fluxn = np.where(go[:, None], (flux + L) * ratio[:, None], flux)
        Nn = np.where(go, total.astype(f32), N)
    return fluxn.astype(f32), r2n.astype(f32), Nn.astype(f32)


def apply_update(recs, M, L_int, S, alpha):
    """recs after one fused gather with those sums"""
    out = recs.copy()
    out["flux"], out["radius2"], out["photon_count"] = ppm_update_ref(
        (recs["flux"], recs["radius2"], recs["photon_count"]), M, L_int, S, alpha)
    return out


def knn_ref(scene, recs, slots, K, maxd2):
    """(found, r_k^2, flux sum) per record of one kNN pass from zero flux: parity_util.knn_reference for
    the live matte records; a live record of another material finds nothing (r2 = maxd2)."""
    ph = slots[(slots["bits"] & 1) != 0]
    found, r2, Sum = knn_reference(recs, ph, K, maxd2)
    for i in range(len(recs)):  # r_k^2 is a d2 of this module's own statement (off the lattice the order shows)
        d2 = np.sort(d2_f32(recs["pos"][i], ph["p"]))
        d2 = d2[d2 < f32(maxd2)]
        assert found[i] == min(len(d2), K)
        r2[i] = d2[K - 1] if len(d2) >= K else f32(maxd2)
    live = (recs["flags"] & PM_REC_INACTIVE) == 0
    matte = np.array([scene.materials[int(m)][0] == PM_MATTE for m in recs["material"]])
    off = ~(live & matte)
    found[off], Sum[off] = 0, 0.0
    r2[off & live] = f32(maxd2)
    return found, r2, Sum, live


# ---- the grid and the tile kernel's prologue ---------------------------------
class Grid:
    """The photon grid of a map built for params.initial_radius2 (pass_plan_ref.make_grid over
    pass_plan_ref.scene_bbox) and cell_axis: floor((v - g0) inv_cs) in float32, clamped to [0, dim - 1]."""

    def __init__(self, scene, params, cell_span=2):
        lo, hi = pass_plan_ref.scene_bbox(scene)
        dx, dy, dz, n, ib = pass_plan_ref.make_grid(lo, hi, params.estimator, cell_span, params.initial_radius2)
        self.lo, self.dims, self.ncells = lo.astype(f32), (dx, dy, dz), n
        self.inv_cs = pass_plan_ref.from_bits(ib)
        self.cs = 1.0 / float(self.inv_cs)

    def cell(self, v, axis):
        c = np.floor((np.asarray(v, f32) - self.lo[axis]) * self.inv_cs)
        assert c.dtype == np.float32
        return np.clip(c, 0, self.dims[axis] - 1).astype(np.int64)

    def cells(self, p):
        p = np.asarray(p, f32).reshape(-1, 3)
        return np.stack([self.cell(p[:, a], a) for a in range(3)], axis=1)

    def first_in_cell(self, k, axis):
        """(v_lo, v_hi): the neighbouring float32 values with cell(v_lo) = k - 1 and cell(v_hi) = k"""
        v = f32(self.lo[axis] + f32(k * self.cs))
        while self.cell(v, axis) >= k:
            v = np.nextafter(v, f32(-np.inf))
        while self.cell(np.nextafter(v, f32(np.inf)), axis) < k:
            v = np.nextafter(v, f32(np.inf))
        return v, np.nextafter(v, f32(np.inf))


def box_reach(r2):
    return np.sqrt(np.asarray(r2, f32)) * f32(1.0001) + f32(1e-4)


def record_boxes(g, recs):
    """(lo [n, 3], hi [n, 3]) cells of [p - r', p + r'] (GatherRec::accept); r2 > 0 only"""
    with np.errstate(invalid="ignore"):
        rq = box_reach(np.where(recs["radius2"] > 0, recs["radius2"], f32(1.0)))
    lo = np.stack([g.cell(recs["pos"][:, a] - rq, a) for a in range(3)], axis=1)
    hi = np.stack([g.cell(recs["pos"][:, a] + rq, a) for a in range(3)], axis=1)
    return lo, hi


def tile_profile(scene, params, recs, slots, cell_span=2):
    """What k_gather_tile's prologue sees: {"density": photons per cell, "umax", "group_min", "tiles":
    per 8x8 tile a dict of
      rows, pitch_rows: (y, z) rows of the union box of the lanes with a box of <= cell_span cells in
                        y and z, and the same with the y count rounded up to a power of two (<= 64: one group)
      U:        the photons in those rows (cells X0..X1)
      row_len:  photons per union row in the concatenation's order
      big:      lanes with a wider box (they scan their own cells)
      groups:   the leader groups as the kernel forms them, [{"lanes", "rows", "U", "staged"}]
      direct:   lanes left to the per-lane / cooperative scans (big, below group_min, union above umax)
      below:    lanes of the leader group that stayed below group_min (0: none did)
      coop_tot: photons in the own cells of the direct lanes with a small box (the kernel's `tot`: at
                most COOP_STEPS * 64 and the wave scans them cooperatively, else each lane its own)}."""
    g = Grid(scene, params, cell_span)
    dx, dy, dz = g.dims
    ph = slots[(slots["bits"] & 1) != 0]
    pc = g.cells(ph["p"])
    lin = np.sort((pc[:, 2] * dy + pc[:, 1]) * dx + pc[:, 0])
    n_map = len(ph)
    group_min = GROUP_MIN_SPARSE if n_map * SPARSE_CELLS < g.ncells else GROUP_MIN
    umax = TILE_UMAX_DENSE if n_map * 5 >= g.ncells * 2 else TILE_UMAX
    GR = GROUP_R if cell_span == 2 else (8 - cell_span) // 2

    def row_count(cy, cz, X0, X1):
        row = (cz * dy + cy) * dx
        return int(np.searchsorted(lin, row + X1, "right") - np.searchsorted(lin, row + X0, "left"))

    def union(lo, hi, sel):
        return lo[sel].min(axis=0), hi[sel].max(axis=0)

    def rows_of(b0, b1, LY):
        lens = []
        for cz in range(b0[2], b1[2] + 1):
            lens += [row_count(cy, cz, b0[0], b1[0]) for cy in range(b0[1], b1[1] + 1)]
            lens += [0] * ((1 << LY) - (b1[1] - b0[1] + 1))  # padding rows of the pitch are empty
        return lens

    lo, hi = record_boxes(g, recs)
    live = ((recs["flags"] & PM_REC_INACTIVE) == 0) & (recs["radius2"] > 0)
    tiles = []
    for t in range(len(recs) // 64):
        s = slice(64 * t, 64 * t + 64)
        tlo, thi, tl = lo[s], hi[s], live[s]
        small = tl & (thi[:, 1] - tlo[:, 1] < cell_span) & (thi[:, 2] - tlo[:, 2] < cell_span)
        big = tl & ~small
        T = dict(rows=0, pitch_rows=0, U=0, row_len=[], big=int(big.sum()), groups=[], direct=int(big.sum()), below=0,
                 coop_tot=0)
        direct_small = np.zeros(64, bool)
        if small.any():
            b0, b1 = union(tlo, thi, small)
            ny = int(b1[1] - b0[1] + 1)
            LY = (ny - 1).bit_length()
            T["rows"], T["pitch_rows"] = ny * int(b1[2] - b0[2] + 1), int(b1[2] - b0[2] + 1) << LY
            if T["pitch_rows"] <= 64:
                T["row_len"] = rows_of(b0, b1, LY)
                T["U"] = sum(T["row_len"])
            else:
                T["U"] = sum(row_count(cy, cz, b0[0], b1[0]) for cz in range(b0[2], b1[2] + 1)
                             for cy in range(b0[1], b1[1] + 1))
        pend = small.copy()
        while pend.any():
            mine = pend.copy()
            b0, b1 = union(tlo, thi, mine)
            LY = int(b1[1] - b0[1]).bit_length()
            if LY > 6 or (int(b1[2] - b0[2] + 1) << LY) > 64:
                lead = tlo[np.flatnonzero(pend)[0]]
                mine = pend & (np.abs(tlo - lead[None, :]) <= GR).all(axis=1)
                if mine.sum() < group_min:
                    T["direct"] += int(pend.sum())
                    T["below"] = int(mine.sum())
                    direct_small |= pend
                    break
                b0, b1 = union(tlo, thi, mine)
                LY = 3
            U = sum(rows_of(b0, b1, LY))
            pend &= ~mine
            staged = 0 < U <= umax
            T["groups"].append(dict(lanes=int(mine.sum()), rows=int((b1[1] - b0[1] + 1) * (b1[2] - b0[2] + 1)),
                                    U=U, staged=staged))
            if U > umax:
                T["direct"] += int(mine.sum())
                direct_small |= mine
        for l in np.flatnonzero(direct_small):  # `tot`: the photons in the small direct lanes' own cells
            T["coop_tot"] += sum(row_count(cy, cz, tlo[l, 0], thi[l, 0]) for cz in range(tlo[l, 2], thi[l, 2] + 1)
                                 for cy in range(tlo[l, 1], thi[l, 1] + 1))
        tiles.append(T)
    return dict(density=n_map / g.ncells, umax=umax, group_min=group_min, tiles=tiles)


# ---- building blocks of the cases --------------------------------------------
def _params(r2, **kw):
    return RenderParams.defaults(initial_radius2=r2, gather_structure=PM_GATHER_GRID, **kw)


def _blank(scene, params):
    """every record a MISS with an uploaded state that must come back bit for bit"""
    recs = np.zeros(num_records(scene), RECORD_DTYPE)
    recs["flags"] = PM_REC_MISS
    recs["radius2"] = params.initial_radius2
    recs["flux"] = (1.0, 2.0, 3.0)
    recs["photon_count"] = 5.0
    recs["ns"] = (0.0, 1.0, 0.0)
    return recs


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(f32)


def _set_live(recs, idx, pos, r2, rng, material=WHITE):
    idx = np.asarray(idx)
    recs["pos"][idx] = np.asarray(pos, f32)
    recs["flags"][idx] = 0
    recs["ns"][idx] = _unit(rng, len(idx))
    recs["material"][idx] = material
    recs["flux"][idx] = 0.0
    recs["radius2"][idx] = r2
    recs["photon_count"][idx] = 0.0


def _slots(p, rng, alpha=None, wi=None):
    p = np.asarray(p, f32).reshape(-1, 3)
    s = np.zeros(len(p), PHOTON_DTYPE)
    s["bits"] = 1
    s["p"] = p
    # thousands, as a traced photon's: the 2^-S rounding of a term stays far below a record's flux
    s["alpha"] = rng.uniform(1024.0, 8192.0, size=(len(p), 3)).astype(f32) if alpha is None else alpha
    s["wi"] = _unit(rng, len(p)) if wi is None else wi
    return s


def _with_invalid(slots, rng, every=7):
    """the same photons with invalid slots (bits 0, a position on top of a record's photons) in between"""
    n = len(slots) + len(slots) // every + 1
    out = np.zeros(n, PHOTON_DTYPE)
    hole = np.zeros(n, bool)
    hole[::every + 1] = True
    hole[np.flatnonzero(~hole)[len(slots):]] = True
    out[~hole] = slots
    src = slots[rng.randint(0, len(slots), size=int(hole.sum()))]
    out["p"][hole], out["alpha"][hole], out["wi"][hole] = src["p"], src["alpha"], src["wi"]
    out["bits"][hole] = 0
    return out


def _lat(rng, n, half):
    """n lattice offsets (multiples of 1/4) in [-half, half]^3"""
    k = int(round(half * 4))
    return rng.randint(-k, k + 1, size=(n, 3)) / 4.0


def _corner(g, k):
    """the lattice point nearest the corner of cell planes k = (kx, ky, kz)"""
    return np.round((g.lo.astype(np.float64) + np.asarray(k) * g.cs) * 4.0) / 4.0


def _corner_tile(recs, tile, g, k, r2, rng, spread=None):
    """64 live records within `spread` (default r / 4) of corner k: every box [p - r', p + r'] covers cells
    {k - 1, k} on each axis, so the tile is one group over 2 x 2 rows of two cells"""
    r = float(np.sqrt(r2))
    c = _corner(g, k)
    _set_live(recs, np.arange(64 * tile, 64 * tile + 64), c[None, :] + _lat(rng, 64, spread or r / 4), r2, rng)
    return c


def _octant_points(g, k, rng, n, ybit, zbit, reach):
    """n lattice points beside corner k in cells (k.x - 1 or k.x, k.y - 1 + ybit, k.z - 1 + zbit), each
    coordinate 1/4 .. reach off the corner"""
    c = _corner(g, k)
    m = int(round(reach * 4))
    off = rng.randint(1, m + 1, size=(n, 3)) / 4.0
    sign = np.stack([rng.choice([-1.0, 1.0], size=n), np.full(n, 2.0 * ybit - 1.0), np.full(n, 2.0 * zbit - 1.0)], 1)
    p = c[None, :] + off * sign
    want = np.asarray(k)[None, 1:] - 1 + np.array([[ybit, zbit]])
    assert (g.cells(p)[:, 1:] == want).all()
    return p


def _row_photons(g, k, rng, counts, reach):
    """photons of one corner tile, counts = (n00, n10, n01, n11): union rows in the order of the
    concatenation, u = (cz - Z0) * 2 + (cy - Y0)"""
    return np.concatenate([_octant_points(g, k, rng, n, u & 1, u >> 1, reach) for u, n in enumerate(counts)])


# six corners far apart (>= 8 cells) in every grid a case uses; x grows with the tile
def _corners(g, n=6):
    dx, dy, dz = g.dims
    return [(3 + (dx - 8) * t // n, 3 + (dy - 8) * ((2 * t + 1) % n) // n, 3 + (dz - 8) * ((3 * t + 2) % n) // n)
            for t in range(n)]


def _filler(g, rng, n, corners):
    """n photons on the lattice, anywhere in the scene box but at least 4 cells from every corner used"""
    out = np.zeros((0, 3))
    ext = np.asarray(g.dims) * g.cs
    while len(out) < n:
        p = np.round(rng.uniform(0.0, 1.0, size=(2 * n, 3)) * (ext - g.cs)[None, :] * 4.0) / 4.0
        c = g.cells(p)
        far = np.ones(len(p), bool)
        for k in corners:
            far &= (np.abs(c - np.asarray(k)[None, :]) > 4).any(axis=1)
        out = np.concatenate([out, p[far]])
    return out[:n]


# ---- the PPM cases -----------------------------------------------------------
def boundary_exact():
    """r2 = 9 = (12/4)^2: the lattice offsets (3, 0, 0), (2, 2, 1) and their images lie at d2 == r2 exactly
    (excluded by the strict <), their neighbours one lattice step inside or outside"""
    rng = np.random.RandomState(101)
    sc, p = _scene(), _params(9.0)
    g = Grid(sc, p)
    recs = _blank(sc, p)
    ties = [(a * s0, b * s1, c * s2) for (a, b, c) in ((3, 0, 0), (0, 3, 0), (0, 0, 3), (2, 2, 1), (2, 1, 2), (1, 2, 2))
            for s0 in (-1, 1) for s1 in (-1, 1) for s2 in (-1, 1)]
    ties = np.unique(np.asarray(ties, np.float64), axis=0)
    pts = []
    for t, k in enumerate(_corners(g)):
        _corner_tile(recs, t, g, k, 9.0, rng)
        for i in rng.choice(64, size=4, replace=False):
            base = recs["pos"][64 * t + i].astype(np.float64)
            for step in (0.0, -0.25, 0.25):  # on the sphere, one step inside, one outside (along the offset)
                pts.append(base[None, :] + ties + step * np.sign(ties))
    return sc, p, recs, _with_invalid(_slots(np.concatenate(pts), rng), rng)


def _redraw(recs, slots, draw, rng):
    """draws again the photons of an ambiguous pair (ambiguous_pairs) until none is left"""
    for _ in range(50):
        bad = ambiguous_pairs(recs, slots)
        if len(bad) == 0:
            return slots
        slots["p"][bad] = draw(bad, rng)
    raise AssertionError("ambiguous pairs remain after 50 redraws")


def cell_edges():
    """photons one float32 ulp to either side of cell planes (one coordinate pinned, the first and the
    last plane of each axis among them) and records whose box [p - r', p + r'] ends within an ulp of one"""
    rng = np.random.RandomState(102)
    sc, p = _scene(), _params(16.0)
    g = Grid(sc, p)
    recs = _blank(sc, p)
    rq = box_reach(f32(16.0))
    dx, dy, dz = g.dims
    corners = [(1, 1, 1), (dx - 1, dy - 1, dz - 1), (1, dy - 1, 20), (dx - 1, 9, 1), (17, 1, dz - 1), (30, 40, 50)]
    planes, pin = [], []
    for t, k in enumerate(corners):
        c = _corner_tile(recs, t, g, k, 16.0, rng)
        edge = [g.first_in_cell(k[a], a) for a in range(3)]
        for i in range(0, 64, 2):  # every other record: one box end within an ulp of a plane
            a, side, hi_end = i // 2 % 3, i // 6 % 2, i // 12 % 2
            target = edge[a][side]
            v = f32(target - rq) if hi_end else f32(target + rq)
            for _ in range(8):  # the float32 p whose p +- r' rounds onto the target
                got = f32(v + rq) if hi_end else f32(v - rq)
                if got == target:
                    break
                v = np.nextafter(v, f32(np.inf) if got < target else f32(-np.inf))
            recs["pos"][64 * t + i, a] = v
        for j in range(120):
            planes.append((t, j % 3, j // 3 % 2))
            pin.append(edge[j % 3][j // 3 % 2])
        corners[t] = (k, c)

    def draw(idx, rng):
        out = np.zeros((len(idx), 3), f32)
        for n, i in enumerate(idx):
            t, a, _ = planes[i]
            out[n] = corners[t][1] + _lat(rng, 1, 3.5)[0]
            out[n, a] = pin[i]
        return out

    slots = _slots(draw(np.arange(len(planes)), rng), rng)
    return sc, p, recs, _redraw(recs, slots, draw, rng)


def outside_bbox():
    """records and photons 0.1, 3 and 50 cell edges outside each face of the scene box (lattice-rounded):
    the clamped edge cells hold them; three groups of a tile's lanes lie far apart"""
    rng = np.random.RandomState(103)
    sc, p = _scene(), _params(16.0)
    g = Grid(sc, p)
    recs = _blank(sc, p)
    lo, hi = pass_plan_ref.scene_bbox(sc)
    mid = (lo.astype(np.float64) + hi) / 2.0
    pts, n = [], 0
    for axis in range(3):
        for side in (0, 1):
            for dist in (0.1, 3.0, 50.0):
                c = np.round(mid * 4.0) / 4.0 + rng.randint(-80, 81, size=3) / 4.0 + 270.0 * (n % 3 - 1)
                off = np.ceil(dist * g.cs * 4.0) / 4.0
                c[axis] = np.floor(lo[axis] * 4) / 4.0 - off if side == 0 else np.ceil(hi[axis] * 4) / 4.0 + off
                tile, part = divmod(n, 3)
                lanes = np.arange(64 * tile + part, 64 * tile + 64, 3)  # interleaved: lane l belongs to group l % 3
                _set_live(recs, lanes, c[None, :] + _lat(rng, len(lanes), 1.0), 16.0, rng)
                pts.append(c[None, :] + _lat(rng, 60, 3.5))
                n += 1
    return sc, p, recs, _slots(np.concatenate(pts), rng)


def ragged_13x9():
    """13 x 9 pixels: four ragged tiles; every record slot, padding lanes too, holds a live record"""
    rng = np.random.RandomState(104)
    sc, p = _scene(13, 9), _params(16.0)
    g = Grid(sc, p)
    recs = _blank(sc, p)
    pts = []
    for t, k in enumerate(_corners(g, 4)):
        _corner_tile(recs, t, g, k, 16.0, rng)
        pts.append(_row_photons(g, k, rng, (40, 33, 29, 51), 3.5))
    assert (recs["flags"] == 0).all() and len(recs) == 256
    return sc, p, recs, _with_invalid(_slots(np.concatenate(pts), rng), rng)


def inactive_mix():
    """one tile of live records interleaved with MISS, EXCEPTION and INVALID ones, r2 = 0, < 0 and NaN,
    a mirror record (M counts, flux 0) and a BACKFACE one; every inactive record carries a state"""
    rng = np.random.RandomState(105)
    sc, p = _scene(), _params(16.0)
    g = Grid(sc, p)
    recs = _blank(sc, p)
    k = _corners(g)[2]
    _corner_tile(recs, 1, g, k, 16.0, rng)
    t = recs[64:128]
    t["flux"], t["photon_count"] = rng.uniform(0, 4, size=(64, 3)).astype(f32), rng.randint(0, 9, size=64).astype(f32)
    for lane, flag in ((1, PM_REC_MISS), (4, PM_REC_EXCEPTION), (7, PM_REC_INVALID), (10, PM_REC_MISS | PM_REC_BACKFACE),
                       (63, PM_REC_INVALID | PM_REC_EXCEPTION), (32, PM_REC_MISS), (33, PM_REC_EXCEPTION)):
        t["flags"][lane] = flag
    t["radius2"][[2, 20]] = 0.0
    t["radius2"][[5, 21]] = -16.0
    t["radius2"][[8, 22]] = np.nan
    t["radius2"][11] = -np.float32(0.0)
    t["material"][[3, 40]] = mirror_id(sc)
    t["flags"][[6, 41]] = PM_REC_BACKFACE
    recs[64:128] = t
    return sc, p, recs, _slots(_row_photons(g, k, rng, (50, 60, 70, 45), 3.5), rng)


ROW_LENGTHS = [(1, 2, 3, 4), (0, 5, 7, 8), (9, 1, 0, 2), (3, 9, 4, 5), (2, 7, 8, 1), (4, 0, 9, 3)]


def row_lengths():
    """union rows of 0, 1, 2, 3, 4, 5, 7, 8 and 9 photons, starting at odd and at even offsets of the
    concatenation: the per-lane kernel's 4-wide loop and its tail, the tile kernel's aligned pairs"""
    rng = np.random.RandomState(106)
    sc, p = _scene(), _params(16.0)
    g = Grid(sc, p)
    recs = _blank(sc, p)
    pts = []
    for t, k in enumerate(_corners(g)):
        _corner_tile(recs, t, g, k, 16.0, rng)
        pts.append(_row_photons(g, k, rng, ROW_LENGTHS[t], 2.0))
    return sc, p, recs, _slots(np.concatenate(pts), rng)


WINDOW_U = [TILE_CAP - 1, TILE_CAP, TILE_CAP + 1, 2 * TILE_CAP + 1, TILE_UMAX, TILE_UMAX + 1]


def _split4(U, first):
    """U photons over the four union rows, the first row `first` long and no row boundary on a multiple of TILE_CAP"""
    rest = U - first
    a = rest // 3 + 1
    b = rest // 3 + 2
    return (first, a, b, rest - a - b)


def windows():
    """one coherent tile per U of WINDOW_U; the rows are cut so that a row straddles every window boundary"""
    rng = np.random.RandomState(107)
    sc, p = _scene(), _params(16.0)
    g = Grid(sc, p)
    recs = _blank(sc, p)
    pts = []
    for t, k in enumerate(_corners(g)):
        _corner_tile(recs, t, g, k, 16.0, rng)
        pts.append(_row_photons(g, k, rng, _split4(WINDOW_U[t], 45), 3.5))
    return sc, p, recs, _slots(np.concatenate(pts), rng)


DENSE_U = [TILE_UMAX_DENSE - 1, TILE_UMAX_DENSE, TILE_UMAX_DENSE + 1, 300, 400, TILE_UMAX]


def dense():
    """dense_and_sparse, the dense map: >= 2 photons per 5 cells, so TILE_UMAX_DENSE applies; the tiles
    of DENSE_U[2:] have 256 < U <= 512 and scan per lane, the first two stage their union"""
    rng = np.random.RandomState(108)
    sc, p = _scene(), _params(100.0)
    g = Grid(sc, p)
    recs = _blank(sc, p)
    ks = _corners(g)
    pts = []
    for t, k in enumerate(ks):
        _corner_tile(recs, t, g, k, 100.0, rng)
        pts.append(_row_photons(g, k, rng, _split4(DENSE_U[t], 45), 9.0))
    pts.append(_filler(g, rng, int(0.45 * g.ncells), ks))
    return sc, p, recs, _slots(np.concatenate(pts), rng)


def sparse():
    """dense_and_sparse, the sparse map: under one photon per 20 cells, so GROUP_MIN_SPARSE applies; each
    tile's lanes lie at far-apart corners in groups of 5 to 11 lanes, all below it"""
    rng = np.random.RandomState(109)
    sc, p = _scene(), _params(16.0)
    g = Grid(sc, p)
    recs = _blank(sc, p)
    ks = _corners(g)
    sizes = [(11, 11, 11, 11, 10, 10), (5, 6, 7, 8, 9, 10, 11, 8), (8,) * 8, (11, 5) * 4, (9, 9, 9, 9, 9, 9, 10), (7,) * 9 + (1,)]
    pts = []
    for t, sz in enumerate(sizes):
        assert sum(sz) == 64
        lane = 0
        for j, n in enumerate(sz):
            k = ks[(t + j) % 6]
            c = _corner(g, k) + np.array([0.0, 0.0, 48.0 * (j // 6)])
            _set_live(recs, np.arange(64 * t + lane, 64 * t + lane + n), c[None, :] + _lat(rng, n, 1.0), 16.0, rng)
            lane += n
    for i, k in enumerate(ks):  # few photons per site (the wave scans them cooperatively) but at one
        for dz in (0.0, 48.0):
            n = 70 if (i, dz) == (0, 48.0) else 5
            pts.append(_corner(g, k)[None, :] + np.array([[0.0, 0.0, dz]]) + _lat(rng, n, 3.5))
    return sc, p, recs, _slots(np.concatenate(pts), rng)


def depth_edge():
    """a tile over three far-apart planes (21, 21 and 20 lanes, interleaved) and two stray lanes far from
    them and from each other: the union has more than 64 rows, three leader groups form, then a stray leads
    a group of one, below GROUP_MIN, and both strays scan directly. Tile 1 has a stray in lane 0: the first
    leader is alone, so every lane scans directly."""
    rng = np.random.RandomState(110)
    sc, p = _scene(), _params(36.0)
    g = Grid(sc, p)
    recs = _blank(sc, p)
    ks = _corners(g)
    pts, stray_cells = [], []
    for t, strays in ((0, (62, 63)), (1, (0,))):
        lanes = np.array([l for l in range(64) if l not in strays])
        for j in range(3):
            k = ks[(3 * t + j) % 6]
            mine = 64 * t + lanes[j::3]
            _set_live(recs, mine, _corner(g, k)[None, :] + _lat(rng, len(mine), 1.5), 36.0, rng)
        for n, l in enumerate(strays):
            c = _corner(g, ks[(3 * t + 1) % 6]) + np.array([0.0, 120.0 if (t + n) % 2 == 0 else -120.0, 144.0 * n])
            _set_live(recs, [64 * t + l], c[None, :], 36.0, rng)
            pts.append(c[None, :] + _lat(rng, 40, 5.0))
            stray_cells.append(tuple(g.cells(c)[0]))
    for k in ks:
        pts.append(_row_photons(g, k, rng, (30, 35, 25, 40), 5.5))
    pts.append(_filler(g, rng, g.ncells // 12, ks + stray_cells))
    return sc, p, recs, _slots(np.concatenate(pts), rng)


def mixed_radii():
    """one tile with r2 of the design radius, a quarter of it, 16 x and 400 x it: the last two are big
    lanes that scan their own cells (the test also runs it with PM_CELL_SPAN 4)"""
    rng = np.random.RandomState(111)
    sc, p = _scene(), _params(16.0)
    g = Grid(sc, p)
    recs = _blank(sc, p)
    ks = _corners(g)
    k = ks[3]
    _corner_tile(recs, 2, g, k, 16.0, rng)
    recs["radius2"][128:192] = np.tile(np.asarray([16.0, 4.0, 256.0, 6400.0, 16.0, 16.0, 4.0, 16.0], f32), 8)
    pts = [_row_photons(g, k, rng, (60, 50, 70, 40), 3.5), _corner(g, k)[None, :] + _lat(rng, 400, 30.0),
           _corner(g, k)[None, :] + _lat(rng, 600, 90.0)]
    return sc, p, recs, _slots(np.concatenate(pts), rng)


def signed():
    """negative alpha components make the launch the signed (int64) instance. Tile 0: a fifth of the
    photons negative at a quarter of the others' size, one with a single negative component; tile 2 the
    mirror image (sums below 0); tile 1 sees only pairs of photons that differ in the sign of alpha: sums
    that cancel to exactly 0"""
    rng = np.random.RandomState(112)
    sc, p = _scene(), _params(16.0)
    g = Grid(sc, p)
    recs = _blank(sc, p)
    ks = _corners(g)
    for t in range(3):
        _corner_tile(recs, t, g, ks[t], 16.0, rng)
    a = _slots(_row_photons(g, ks[0], rng, (40, 30, 50, 35), 3.5), rng)
    a["alpha"][::5] *= f32(-0.25)
    a["alpha"][1, 1] = -a["alpha"][1, 1]  # one component only
    b = _slots(_corner(g, ks[1])[None, :] + np.array([[2.5, 0, 0], [-2.5, 0, 0]]), rng)
    b[1] = b[0]  # one alpha and wi: every term of a record has one magnitude, any float order cancels too
    b["p"][1, 0] -= 5.0
    b = np.concatenate([b, b])
    b["alpha"][2:] *= f32(-1.0)
    c = _slots(_row_photons(g, ks[2], rng, (20, 20, 20, 20), 3.5), rng)
    c["alpha"] *= f32(-1.0)
    c["alpha"][::5] *= f32(-0.25)
    return sc, p, recs, np.concatenate([a, b, c])


def beyond_2p53():
    """lane 9 of tile 0 stands 3 units off its tile's cluster and alone sees 100 photons of alpha 2^30
    (above the scene's bound): its sums reach 2^53, so the tile kernel redoes it in int64; its neighbours
    see ordinary photons of the same staged union (U <= 256) and keep the double path"""
    rng = np.random.RandomState(113)
    sc, p = _scene(), _params(16.0)
    g = Grid(sc, p)
    recs = _blank(sc, p)
    k = _corners(g)[4]
    c = _corner_tile(recs, 0, g, k, 16.0, rng, spread=0.5)
    recs["pos"][9] = c + np.array([3.0, 0.25, -0.25])
    recs["ns"][9] = (0.0, 0.0, 1.0)
    huge = _slots(recs["pos"][9][None, :] + np.array([[3.5, 0.0, 0.0]]) + _lat(rng, 100, 0.25) * [0, 1, 1], rng,
                  alpha=np.full((100, 3), 2.0 ** 30, f32), wi=np.tile(f32([0.0, 0.0, -1.0]), (100, 1)))
    rest = _slots(c[None, :] + _lat(rng, 120, 2.5), rng)
    return sc, p, recs, np.concatenate([rest, huge])


def progressive():
    """records with an uploaded state (N, flux, r2 <= the design radius) for three fused gathers over one
    map, then a reset and a fresh gather; two inactive records keep their state throughout"""
    rng = np.random.RandomState(114)
    sc, p = _scene(), _params(16.0)
    g = Grid(sc, p)
    recs = _blank(sc, p)
    pts = []
    for t, k in enumerate(_corners(g)):
        _corner_tile(recs, t, g, k, 16.0, rng)
        pts.append(_row_photons(g, k, rng, (40, 33, 29, 51), 3.5))
    n = len(recs)
    recs["photon_count"] = rng.randint(0, 40, size=n).astype(f32)
    recs["flux"] = rng.uniform(0, 50, size=(n, 3)).astype(f32)
    recs["radius2"] = rng.choice(f32([16.0, 12.25, 9.0, 6.5]), size=n)
    recs["flags"][[17, 200]] = PM_REC_MISS, PM_REC_INVALID
    return sc, p, recs, _slots(np.concatenate(pts), rng)


CASES = {
    "boundary_exact": boundary_exact, "cell_edges": cell_edges, "outside_bbox": outside_bbox,
    "ragged_13x9": ragged_13x9, "inactive_mix": inactive_mix, "row_lengths": row_lengths, "windows": windows,
    "dense_and_sparse.dense": dense, "dense_and_sparse.sparse": sparse, "depth_edge": depth_edge,
    "mixed_radii": mixed_radii, "signed": signed, "beyond_2p53": beyond_2p53, "progressive": progressive,
}
PROGRESSIVE_PASSES = 3


# ---- the kNN cases -----------------------------------------------------------
KNN_R2 = 100.0  # maxDistSquared of the kNN cases


def _knn_params(K):
    return RenderParams.defaults(initial_radius2=KNN_R2, gather_structure=PM_GATHER_GRID, estimator=PM_ESTIMATOR_KNN,
                                 knn_lookup=K)


def _distinct_offsets(limit2):
    """lattice offsets with pairwise distinct d2 < limit2, nearest first (d2 > 0)"""
    k = int(np.sqrt(limit2) * 4) + 1
    ax = np.arange(0, k + 1) / 4.0
    o = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    d2 = (o * o).sum(axis=1)
    o, d2 = o[(d2 > 0) & (d2 < limit2)], d2[(d2 > 0) & (d2 < limit2)]
    _, first = np.unique(d2, return_index=True)
    return o[first]


def _knn_sites(n, origin=(60.0, 60.0, 60.0), pitch=25.0):
    """n isolated sites: a 4 x 4 x m block, 25 apart (no photon of one site within 10 of another)"""
    i = np.arange(n)
    return np.asarray(origin)[None, :] + pitch * np.stack([i % 4, i // 4 % 4, i // 16], 1)


def _knn_facing(rng, n, ns):
    """wi on the side of ns, except every fifth (Dot(Nf, wi) <= 0: found, but no flux)"""
    wi = _unit(rng, n)
    s = np.sign((wi * ns[None, :]).sum(axis=1))
    s[s == 0] = 1.0
    wi = (wi * s[:, None]).astype(f32)
    wi[::5] = -wi[::5]
    return wi


def knn_counts(K):
    """isolated records with exactly K - 1, K and K + 1 photons inside maxd2, at pairwise distinct d2"""
    def build():
        rng = np.random.RandomState(200 + K)
        sc, p = _scene(), _knn_params(K)
        recs = _blank(sc, p)
        sites = _knn_sites(128)
        offs = _distinct_offsets(90.0)
        assert len(offs) >= K + 1
        slots = []
        for i, c in enumerate(sites):
            n = max(K - 1 + i % 3, 0)
            _set_live(recs, [i], c[None, :], KNN_R2, rng)
            recs["flags"][i] = PM_REC_BACKFACE if i % 4 == 3 else 0
            pick = rng.choice(len(offs), size=n, replace=False)
            sign = rng.choice([-1.0, 1.0], size=(n, 3))
            ns = recs["ns"][i] * (-1.0 if i % 4 == 3 else 1.0)
            if n:
                slots.append(_slots(c[None, :] + offs[pick] * sign, rng, wi=_knn_facing(rng, n, ns.astype(f32))))
        return sc, p, recs, _with_invalid(np.concatenate(slots), rng)
    return build


def knn_ties():
    """K = 8: five photons nearer, then six at the k-th distance exactly ((2, 2, 1)-type offsets): their
    weight (1 - d2 / r_k2)^2 is 0, so found, r_k^2 and the flux do not depend on which three are kept"""
    rng = np.random.RandomState(210)
    sc, p = _scene(), _knn_params(8)
    recs = _blank(sc, p)
    tie = np.asarray([(2, 2, 1), (2, 1, 2), (1, 2, 2), (-2, 2, 1), (2, -1, 2), (-3, 0, 0)], np.float64)
    near = _distinct_offsets(8.0)
    slots = []
    for i, c in enumerate(_knn_sites(96)):
        _set_live(recs, [i], c[None, :], KNN_R2, rng)
        o = np.concatenate([near[rng.choice(len(near), size=5, replace=False)] * rng.choice([-1.0, 1.0], size=(5, 3)),
                            tie[rng.permutation(6)], 2.0 * tie[:2]])
        slots.append(_slots(c[None, :] + o[rng.permutation(len(o))], rng, wi=_knn_facing(rng, len(o), recs["ns"][i])))
    return sc, p, recs, np.concatenate(slots)


def knn_zero():
    """K = 4: records with four photons at distance 0 (r_k^2 = 0: the documented NaN flux) beside records
    with three at distance 0 and one farther (finite)"""
    rng = np.random.RandomState(211)
    sc, p = _scene(), _knn_params(4)
    recs = _blank(sc, p)
    slots = []
    for i, c in enumerate(_knn_sites(64)):
        _set_live(recs, [i], c[None, :], KNN_R2, rng)
        o = np.zeros((5, 3))
        o[3] = (0.0, 0.0, 0.0) if i % 2 == 0 else (1.25, -0.5, 2.0)
        o[4] = (3.0, 3.0, 3.0)
        wi = np.tile(recs["ns"][i], (5, 1)).astype(f32)  # every photon faces the record
        slots.append(_slots(c[None, :] + o, rng, wi=wi))
    return sc, p, recs, np.concatenate(slots)


def knn_ragged():
    """K = 5 on the 13 x 9 image: clustered records in every slot of the ragged tiles, inactive ones and a
    mirror mixed in; positions off the lattice (x 1.1), so r_k^2 carries the roundings of the d2 order"""
    rng = np.random.RandomState(212)
    sc, p = _scene(13, 9), _knn_params(5)
    recs = _blank(sc, p)
    pts = []
    for t in range(4):
        c = np.asarray([80.0 + 110.0 * t, 100.0 + 90.0 * t, 400.0 - 70.0 * t])
        _set_live(recs, np.arange(64 * t, 64 * t + 64), (c[None, :] + _lat(rng, 64, 6.0)) * 1.1, KNN_R2, rng)
        pts.append((c[None, :] + _lat(rng, 300 if t else 7, 9.0)) * 1.1)
    recs["flags"][[3, 70, 71, 130, 255]] = PM_REC_MISS, PM_REC_EXCEPTION, PM_REC_INVALID, PM_REC_MISS, PM_REC_INVALID
    recs["flags"][[5, 90]] = PM_REC_BACKFACE
    recs["material"][[9, 100]] = mirror_id(sc)
    return sc, p, recs, _with_invalid(_slots(np.concatenate(pts), rng), rng)


SHELL_D2 = (64.0, 64.6)  # knn_shell's dense shell: inside one 1/16-octave bin of d2, [64, 68)


def _shell_offsets(lo2, hi2):
    """offsets on the 1/32 lattice (non-negative octant) with pairwise distinct d2 in [lo2, hi2]; every d2
    is a multiple of 2^-10 below 2^7, exact in float32 in any summation order"""
    m = int(np.sqrt(hi2) * 32) + 1
    a, b = np.meshgrid(np.arange(m + 1), np.arange(m + 1), indexing="ij")
    c0 = np.ceil(np.sqrt(np.maximum(lo2 * 1024.0 - a * a - b * b, 0.0))).astype(np.int64)
    o = np.concatenate([np.stack([a, b, c0 + s], -1).reshape(-1, 3) for s in (0, 1, 2)])
    n = (o * o).sum(axis=1)
    o, n = o[(n >= lo2 * 1024) & (n <= hi2 * 1024)], n[(n >= lo2 * 1024) & (n <= hi2 * 1024)]
    _, first = np.unique(n, return_index=True)
    return o[first] / 32.0


def knn_shell():
    """K = 50, one tile of 64 live records at one point: 30 photons at distinct d2 < 40, then 240 at
    distinct d2 inside SHELL_D2, so the 50th nearest is the 20th of a shell that fills one bin of either
    kernel's first histogram and, 32 x finer, still puts more photons into a bin than a COLLECT keeps:
    the scalar stream refines twice, the tile kernel re-bins [min, max] of the shell"""
    rng = np.random.RandomState(213)
    sc, p = _scene(), _knn_params(50)
    recs = _blank(sc, p)
    c = np.asarray([110.0, 110.0, 110.0])
    _set_live(recs, np.arange(64), np.tile(c, (64, 1)), KNN_R2, rng)
    recs["flags"][[3, 17, 40]] = PM_REC_BACKFACE
    near, shell = _distinct_offsets(40.0), _shell_offsets(*SHELL_D2)
    assert len(near) >= 30 and len(shell) >= 240
    o = np.concatenate([near[rng.choice(len(near), size=30, replace=False)],
                        shell[rng.choice(len(shell), size=240, replace=False)]])
    o = (o * rng.choice([-1.0, 1.0], size=o.shape))[rng.permutation(len(o))]
    slots = _slots(c[None, :] + o, rng, wi=_knn_facing(rng, len(o), recs["ns"][0]))
    return sc, p, recs, _with_invalid(slots, rng)


KNN_CASES = {"knn_counts[K=1]": knn_counts(1), "knn_counts[K=2]": knn_counts(2), "knn_counts[K=50]": knn_counts(50),
             "knn_counts[K=64]": knn_counts(64), "knn_ties": knn_ties, "knn_zero": knn_zero, "knn_ragged": knn_ragged,
             "knn_shell": knn_shell}

_built = {}


def case(name):
    """(scene, params, recs, slots) of a case, built once; callers copy what they change"""
    if name not in _built:
        _built[name] = (CASES.get(name) or KNN_CASES[name])()
    return _built[name]


_refs = {}


def states(name):
    """The gathers of a PPM case, computed once: a list of (recs before, M, L, recs after) — one entry,
    or for `progressive` its PROGRESSIVE_PASSES fused gathers from the uploaded state and then the fresh
    gather after a reset (every live record back at flux 0, N 0, r2 = initial_radius2)."""
    if name not in _refs:
        sc, p, recs, slots = case(name)
        S = fx_shift(sc, p)
        out = []

        def step(before):
            M, L = ppm_partial_ref(before, slots, sc.materials, S)
            out.append((before, M, L, apply_update(before, M, L, S, p.ppm_alpha)))

        step(recs)
        if name == "progressive":
            for _ in range(PROGRESSIVE_PASSES - 1):
                step(out[-1][3])
            fresh = out[-1][3].copy()
            live = (recs["flags"] & PM_REC_INACTIVE) == 0
            fresh["flux"][live], fresh["photon_count"][live], fresh["radius2"][live] = 0.0, 0.0, p.initial_radius2
            step(fresh)
        _refs[name] = out
    return _refs[name]


def partial_ref(name):
    """(S, M, L) of a PPM case's uploaded state"""
    sc, p, _, _ = case(name)
    _, M, L, _ = states(name)[0]
    return fx_shift(sc, p), M, L
