"""trace_ref.py's checkers on the CPU: the oracle's slots of every scene that
tests/test_trace_directed_gpu.py traces with an oracle pass them with fewer
than 1 % of the deposits exempt, the bounds are four times the residuals
measured on those slots, and every corruption of a list is rejected by the
checker that owns the rule it breaks (and by assert_same_slots, which names
the slot). No GPU."""
import numpy as np
import pytest

import trace_ref as T
from pmrender import scenes
from pmrender.abi import PHOTON_DTYPE, RenderParams


def params(n, mpc=4, depth=10, **kw):
    return RenderParams.defaults(paths_per_pass=n, max_photon_count=mpc, max_specular_depth=depth, **kw)


@pytest.fixture(scope="module")
def traced(oracle_mod):
    """(scene, params, the oracle's slots, their Residuals) of a case of T.CASES, computed once"""
    orcs, done = {}, {}

    def get(case):
        if case not in done:
            name, n, mpc, pass_, depth = case
            sc = T.scene(name)
            if name not in orcs:
                orcs[name] = sc.load_into(oracle_mod.Oracle())
            p = params(n, mpc, depth)
            slots = orcs[name].trace_photons(p, pass_, 0, n)
            done[case] = (sc, p, slots, T.measure_paths(sc, p, slots))
        return done[case]
    return get


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: "-".join(map(str, c)))
def test_oracle_slots_pass(case, traced):
    sc, p, slots, r = traced(case)
    n = T.assert_layout(slots, p.max_photon_count)
    assert 0 < n.sum() < len(slots) and n.max() == p.max_photon_count, "paths of every length up to mpc"
    got = T.assert_residuals(r, sc, p, what=str(case))
    assert got["exempt"] < 0.01 * got["deposits"], got
    g = T.geometry(sc)
    if g.specular and case[4] > 0:
        assert got["bent"] > 0, "no path of the case meets a mirror or glass"
    else:
        assert got["bent"] == 0


def test_bounds_are_four_times_the_oracle_residuals(traced):
    worst = {k: max(traced(c)[3][k] for c in T.CASES) for k in T.MEASURED}
    for k, v in worst.items():
        assert v == pytest.approx(T.MEASURED[k], rel=1e-6), (k, v, T.MEASURED[k])
    assert (T.UNIT_BOUND, T.POS_BOUND, T.DIR_BOUND, T.DIST_BOUND, T.KD_BOUND) == \
        tuple(4.0 * T.MEASURED[k] for k in ("unit", "pos", "dir", "dist", "kd"))
    # the bounds are fp32 matters: a few ulps of a coordinate of the box (ulp(512) = 6.1e-5), of 1 and of a Kd
    assert T.POS_BOUND < 16 * 6.1e-5 and T.DIR_BOUND < 16 * 6.1e-5 and T.DIST_BOUND < 32 * 6.1e-5
    assert T.UNIT_BOUND < 64 * 2.0 ** -24 and T.KD_BOUND < 256 * 2.0 ** -24


def test_depth_zero_deposits_only_behind_matte_hits(traced):
    """max_specular_depth = 0: no segment bends, and fewer deposits than with the chains allowed"""
    for name in ("spheres_lds", "instanced"):
        d0, d1 = (traced((name, 1000, 4, 0, d))[3] for d in (0, 1))
        assert d0["bent"] == 0 and d0["deposits"] < d1["deposits"]


# ---- corruptions --------------------------------------------------------------------------------
CORNELL = ("cornell", 3000, 4, 0, 10)
KDS = np.float32([scenes.WHITE, scenes.RED, scenes.GREEN]).astype(np.float64)


def _paths_with(slots, mpc, at_least=0, at_most=None):
    n = T.valid(T.by_path(slots, mpc)).sum(axis=1)
    return np.flatnonzero((n >= at_least) & (n <= (mpc if at_most is None else at_most)))


def swap(s, mpc):
    i = _paths_with(s, mpc, 2)[0]
    s[[i * mpc, i * mpc + 1]] = s[[i * mpc + 1, i * mpc]]
    return i * mpc


def shift(s, mpc):
    i = _paths_with(s, mpc, 1, mpc - 1)[0]
    s[i * mpc + 1:(i + 1) * mpc] = s[i * mpc:(i + 1) * mpc - 1].copy()
    s[i * mpc] = np.zeros((), PHOTON_DTYPE)
    return i * mpc


def hole(s, mpc):
    i = _paths_with(s, mpc, 3)[0]
    s[i * mpc + 1] = np.zeros((), PHOTON_DTYPE)
    return i * mpc + 1


def dead_byte(s, mpc):
    i = _paths_with(s, mpc, 0, mpc - 1)[5]
    s.view(np.uint8)[((i + 1) * mpc - 1) * 40 + 39] = 1   # the last byte of the path's last slot
    return (i + 1) * mpc - 1


def other_kd(s, mpc):
    """alpha_1 as if p_0 lay on a wall of another colour"""
    i = _paths_with(s, mpc, 2)[3]
    a0, a1 = s["alpha"][i * mpc].astype(np.float64), s["alpha"][i * mpc + 1].astype(np.float64)
    was = int(np.abs(KDS - a1 / a0).max(axis=1).argmin())
    s["alpha"][i * mpc + 1] = (a0 * KDS[(was + 1) % 3]).astype(np.float32)
    return i * mpc + 1


def negate_wi(s, mpc):
    i = _paths_with(s, mpc, 2)[7]
    s["wi"][i * mpc + 1] *= -1
    return i * mpc + 1


def off_surface(s, mpc):
    j = np.flatnonzero(T.valid(s) & (np.abs(s["p"][:, 1]) < 1e-3))[0]   # on the floor, y = 0
    s["p"][j, 1] += np.float32(10 * T.POS_BOUND)
    return j


def neighbour(s, mpc):
    n = T.valid(T.by_path(s, mpc)).sum(axis=1)
    i = np.flatnonzero((n[:-1] >= 2) & (n[1:] >= 2))[0]
    s[i * mpc + 1] = s[(i + 1) * mpc + 1]
    return i * mpc + 1


PATH_RULES = [swap, other_kd, negate_wi, off_surface, neighbour]
LAYOUT_RULES = [shift, hole, dead_byte]


@pytest.mark.parametrize("corrupt", PATH_RULES + LAYOUT_RULES, ids=lambda f: f.__name__)
def test_corruption_is_rejected(corrupt, traced):
    sc, p, slots, _ = traced(CORNELL)
    bad = slots.copy()
    first = corrupt(bad, 4)
    with pytest.raises(AssertionError, match=f"first slot {first}\n"):
        T.assert_same_slots(bad, slots)
    if corrupt in LAYOUT_RULES:
        with pytest.raises(AssertionError):
            T.assert_layout(bad, 4)
    else:
        T.assert_layout(bad, 4)   # the layout is intact: only the paths' rules see it
    with pytest.raises(AssertionError):
        T.assert_paths(sc, p, bad)
    T.assert_same_slots(slots.copy(), slots)


def test_mark_after_a_diffuse_hit_is_rejected(traced):
    _, _, slots, _ = traced(CORNELL)
    i = _paths_with(slots, 4, 3)[0]
    marked = slots.copy()
    marked["bits"][i * 4:i * 4 + 2] = 3          # 3 3 1: two caustic deposits, then a diffuse hit
    T.assert_layout(marked, 4, marked=True)
    with pytest.raises(AssertionError, match="outside 1"):
        T.assert_layout(marked, 4)               # an unmarked trace writes no 3
    marked["bits"][i * 4] = 1                    # 1 3 1
    with pytest.raises(AssertionError, match=f"first path {i} slot 1"):
        T.assert_layout(marked, 4, marked=True)
    with pytest.raises(AssertionError, match=f"first slot {i * 4 + 1}\n"):
        T.assert_same_slots(marked, slots)
    marked["bits"][i * 4:i * 4 + 2] = (1, 2)     # a caustic bit without the valid bit: a dead slot that is not zero
    with pytest.raises(AssertionError):
        T.assert_layout(marked, 4, marked=True)


def test_geometry_distances():
    """the distance of a point from a triangle, a disk and a sphere, on cases worked by hand"""
    sc = scenes.Scene()
    m = sc.material(scenes.PM_MATTE, (0.5, 0.5, 0.5))
    sc.meshes.append(dict(P=np.float32([[0, 0, 0], [4, 0, 0], [0, 4, 0]]), idx=np.int32([[0, 1, 2]]), N=None, uv=None,
                          material=m, light=-1))
    sc.disks.append((np.float32([10, 0, 0]), np.float32([2, 0, 0]), np.float32([0, 2, 0]), np.float32([0, 0, 1]),
                     np.float32(0.0), np.float32(2 * np.pi), m, -1))
    o2w, w2o = scenes.translate(20.0, 0.0, 0.0)
    sc.spheres.append((np.float32(0.5), o2w, w2o, m, -1))
    g = T.Geometry(sc)
    pts = np.float64([[1, 1, 0.25], [-0.3, -0.4, 0], [5, 0, 0.5], [3, 3, 0],   # above, off the corner, off a vertex, off the hypotenuse
                      [10, 1, 0.125], [10, 2.5, 0], [20, 0, 0.75], [20.25, 0, 0]])
    pi, ki, d = g.near(pts)
    want = {(0, 0): 0.25, (1, 0): 0.5, (2, 0): np.hypot(1, 0.5), (3, 0): np.sqrt(2.0), (4, 1): 0.125, (5, 1): 0.5,
            (6, 2): 0.25, (7, 2): 0.25}
    got = {(int(a), int(b)): float(c) for a, b, c in zip(pi, ki, d)}
    for key, v in want.items():
        assert got[key] == pytest.approx(v, abs=1e-12), key
