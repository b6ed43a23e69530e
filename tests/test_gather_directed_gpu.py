"""Every gather kernel against the brute-force references of gather_ref.py on
its directed cases (test_gather_directed.py certifies the cases and the
references on the CPU).

Grid kernels (per lane, per tile, the tile kernel on finer cells): the partial
gather equals ppm_partial_ref integer for integer, the fused gather equals
ppm_update_ref of those integers bit for bit. The kd-tree kernel sums floats
in tree order: M, N' and r2 exact, flux within gather_ref.flux_bound. kNN
kernels: photons found and r_k^2 exact, the NaN records the same, flux within
parity_util.compare_knn_records' rule."""
import numpy as np
import pytest

import gather_ref as G
from parity_util import assert_bitexact, compare_knn_records, knn_term_floor, u32
from pmrender.abi import PM_GATHER_GRID, PM_GATHER_KDTREE, RenderParams

pytestmark = pytest.mark.gpu

ENV_KEYS = ("PM_GATHER_KERNEL", "PM_CELL_SPAN", "PM_KNN_SS")
PPM_KERNELS = {
    "lane": {"PM_GATHER_KERNEL": "lane"},
    "tile": {"PM_GATHER_KERNEL": "tile"},
    "tile_span3": {"PM_GATHER_KERNEL": "tile", "PM_CELL_SPAN": "3"},
    "tile_span5": {"PM_GATHER_KERNEL": "tile", "PM_CELL_SPAN": "5"},
    "kd": {},
}
KNN_KERNELS = {
    "lane": {"PM_GATHER_KERNEL": "lane"},
    "tile": {"PM_GATHER_KERNEL": "tile", "PM_KNN_SS": "0"},
    "ss": {"PM_GATHER_KERNEL": "tile", "PM_KNN_SS": "1"},
}
PPM_RUNS = [(c, k) for c in sorted(G.CASES) for k in PPM_KERNELS] + [("mixed_radii", "tile_span4")]


def _context(hip_mod, monkeypatch, env, scene):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return scene.load_into(hip_mod.Context(0))


def _partials(ctx, p, n):
    import torch
    part = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.gather_partial(p, part.data_ptr())
    ctx.synchronize()
    return part.cpu().numpy()


def _first_diff(got, M, L):
    bad = np.flatnonzero((got[:, 0] != M) | (got[:, 1:] != L).any(axis=1))
    if bad.size == 0:
        return None
    i = int(bad[0])
    return f"{bad.size} of {len(M)} records differ, first {i} (tile {i // 64} lane {i % 64}): " \
           f"gpu {got[i].tolist()} vs reference {[int(M[i])] + L[i].tolist()}"


@pytest.mark.parametrize("name,kernel", PPM_RUNS)
def test_ppm_case(name, kernel, hip_mod, monkeypatch):
    pytest.importorskip("torch")
    sc, p0, recs, slots = G.case(name)
    S = G.fx_shift(sc, p0)
    steps = G.states(name)
    p = RenderParams.from_buffer_copy(p0)
    env = PPM_KERNELS.get(kernel, {"PM_GATHER_KERNEL": "tile", "PM_CELL_SPAN": kernel[-1]})
    p.gather_structure = PM_GATHER_KDTREE if kernel == "kd" else PM_GATHER_GRID
    ctx = _context(hip_mod, monkeypatch, env, sc)
    try:
        assert ctx.num_records() == len(recs)
        ctx.upload_records(recs)
        ctx.upload_slots(slots)
        ctx.build_photon_map(p, len(slots))
        tol = np.zeros((len(recs), 3))
        for k, (before, M, L, after) in enumerate(steps):
            if name == "progressive" and k == G.PROGRESSIVE_PASSES:
                ctx.reset_records(p)
                tol[:] = 0.0
            else:  # the partial gather leaves the records as they are (a pending reset it would apply first)
                part = _partials(ctx, p, len(recs))
                if kernel != "kd":
                    assert _first_diff(part, M, L) is None, f"{name}/{kernel} pass {k}: {_first_diff(part, M, L)}"
                else:
                    _, _, A = G.ppm_partial_f64(before, slots, sc.materials)
                    dL = G.flux_bound(A, M, S) + G.flux_bound(A, M, S, kd_tree=True)
                    assert np.array_equal(part[:, 0], M), f"{name}/kd pass {k}: M differs"
                    err = np.abs(part[:, 1:] - L).astype(np.float64) * 2.0 ** -S
                    assert (err <= dL).all(), f"{name}/kd pass {k}: flux sum off by {(err - dL).max():.3g} beyond the bound"
            ctx.gather(p)
            got = ctx.download_records()
            if kernel != "kd":
                assert_bitexact(got, after, f"{name}/{kernel} pass {k}: fused gather vs ppm_update_ref")
                continue
            # kd-tree: everything but the flux bit for bit; the flux (flux + L) ratio, ratio <= 1, within the
            # sums' bound plus eight float32 roundings (L, +, * on either side, two to spare) of |flux| + A,
            # on top of what the passes before left
            _, _, A = G.ppm_partial_f64(before, slots, sc.materials)
            dL = G.flux_bound(A, M, S) + G.flux_bound(A, M, S, kd_tree=True)
            tol = tol + dL + 2.0 ** -21 * (np.abs(before["flux"]).astype(np.float64) + A + dL + tol)
            for f in ("pos", "flags", "ns", "material", "radius2", "dl", "photon_count"):
                assert np.array_equal(u32(got[f]), u32(after[f])), f"{name}/kd pass {k}: {f} differs"
            err = np.abs(got["flux"].astype(np.float64) - after["flux"].astype(np.float64))
            assert (err <= tol).all(), f"{name}/kd pass {k}: flux off by {(err - tol).max():.3g} beyond the bound"
            dead = G.inactive(before)
            assert np.array_equal(u32(got["flux"][dead]), u32(before["flux"][dead])), f"{name}/kd pass {k}: inactive records"
    finally:
        ctx.close()


@pytest.mark.parametrize("kernel", list(KNN_KERNELS))
@pytest.mark.parametrize("name", sorted(G.KNN_CASES))
def test_knn_case(name, kernel, hip_mod, monkeypatch):
    sc, p, recs, slots = G.case(name)
    found, r2, Sum, live = G.knn_ref(sc, recs, slots, p.knn_lookup, p.initial_radius2)
    ctx = _context(hip_mod, monkeypatch, KNN_KERNELS[kernel], sc)
    try:
        ctx.upload_records(recs)
        ctx.upload_slots(slots)
        ctx.build_photon_map(p, len(slots))
        ctx.gather(p)
        got = ctx.download_records()
    finally:
        ctx.close()
    assert (recs["flux"][live] == 0).all()
    compare_knn_records(got[live], found[live], r2[live], Sum[live], floor=knn_term_floor(sc, found, r2)[live])
    assert (~live).any()
    assert_bitexact(got[~live], recs[~live], f"{name}/{kernel}: inactive records")
    for f in ("pos", "flags", "ns", "material", "dl"):
        assert np.array_equal(u32(got[f]), u32(recs[f])), f
