"""The photon trace (csrc/pm_trace.hip) over its launch geometries, against two
references: the oracle's slots, bit for bit, and trace_ref.py's float64 rules
for what a slot buffer can hold at all (test_trace_directed.py certifies both
checkers on the CPU). Every kernel family on a tiny scene of its own; path
counts around a wave and a block; the pooled kernel's refill loop under
PM_TRACE_CUS=1, where a few thousand paths make pools of more than 64 paths
per wave; max_photon_count off the held layout's 4, with and without the fused
bucket counts; a slot buffer that is not 16-byte aligned; max_specular_depth 0
and 1; path ids at the top of the 32-bit slot index; shards cut at odd
boundaries; the counting instantiations; and, for what the oracle lacks
(several lights, textures, the physical specular model, caustic marks), every
geometry against the per-lane launch that the feature's own suite holds to its
numpy reference.

Contexts are shared per scene and environment for the whole file (a commit
costs more than a trace here). A buffer of fewer than 1,000 paths is held to
every rule but the exempt share, which is no statistic on a handful of
deposits; the 1,000-path buffers of every scene and setting are held to it.

Not reachable (tests/test_trace_plan.py shows why): a pooled launch with pools
of more than 19 paths whose last block has idle waves. Occupancy comes in whole
blocks, so such a launch fills every wave of its round; the idle waves of a
last block are covered at pools of 4 (70 paths under PM_TRACE_CUS=1)."""
import dataclasses

import numpy as np
import pytest

import trace_ref as T
from pmrender import scenes
from pmrender.abi import PM_ALL_LIGHTS, PM_ERR_INVALID, PM_GATHER_GRID, PM_GATHER_KDTREE, RenderParams
from test_bucket_build_gpu import check_build

pytestmark = pytest.mark.gpu

ENV_KEYS = ("PM_TRACE_HOLD", "PM_TRACE_POOL", "PM_POOL_STACK", "PM_LAZY_ZERO", "PM_BVH8", "PM_TRACE_CUS")
R2 = 64.0   # the fused counts' grid: cells of 16 units in the 556-unit box
SCENE_NAMES = sorted(T.SCENES)
POOLED = ("soup_hbm", "spheres_hbm")


def params(n, mpc=4, depth=10, fused=False, **kw):
    """fused: the call that fills the buffer from its first slot also counts the buckets (PM_GATHER_GRID)"""
    return RenderParams.defaults(paths_per_pass=n, max_photon_count=mpc, max_specular_depth=depth, initial_radius2=R2,
                                 gather_structure=PM_GATHER_GRID if fused else PM_GATHER_KDTREE, **kw)


def soup_around(sc):
    """`sc` with triangle_soup's 2,000 triangles added: traversed from HBM, so the pooled kernel takes it"""
    soup = scenes.triangle_soup(T.HBM_TRIS, 16, 16)
    grey = sc.material(scenes.PM_MATTE, (0.5, 0.5, 0.5))
    sc.meshes.append(dict(soup.meshes[-1], material=grey))
    return sc


FEATURES = {
    "two_lights": lambda: scenes.cornell_two_lights(16, 16),
    "textured": lambda: scenes.cornell_textured(16, 16),
    "fresnel": lambda: scenes.caustic_fresnel(16, 16),
}


class World:
    """contexts per (scene, environment), oracles per scene and the oracle's slots per trace, made once"""

    def __init__(self, hip_mod, oracle_mod):
        self.hip, self.oracle_mod = hip_mod, oracle_mod
        self.scenes, self.ctxs, self.orcs, self.refs, self.checked = {}, {}, {}, {}, {}

    def scene(self, name):
        if name in T.SCENES:
            return T.scene(name)
        if name not in self.scenes:
            base, _, big = name.partition("+")
            self.scenes[name] = soup_around(FEATURES[base]()) if big else FEATURES[base]()
        return self.scenes[name]

    def flat(self, name):
        """the scene with its instances flattened, for check_build's grid (its box takes no instances; the figures
        stand inside the walls, so the box is the same)"""
        sc = self.scene(name)
        if not sc.instances:
            return sc
        if ("flat", name) not in self.scenes:
            self.scenes[("flat", name)] = dataclasses.replace(
                sc, meshes=sc.meshes + [sc.flattened(k) for k in range(len(sc.instances))], instances=[], objects=[])
        return self.scenes[("flat", name)]

    def fresh(self, name, mode=None, **env):
        """a context of its own, made under exactly `env` (the caller closes it)"""
        with pytest.MonkeyPatch.context() as mp:
            for k in ENV_KEYS:
                mp.delenv(k, raising=False)
            for k, v in env.items():
                mp.setenv(k, str(v))
            ctx = self.scene(name).load_into(self.hip.Context(0))
        assert ctx.scene_info()["mode"] == (mode or T.MODE[name]), (name, ctx.scene_info())
        return ctx

    def ctx(self, name, mode=None, **env):
        key = (name, tuple(sorted(env.items())))
        if key not in self.ctxs:
            self.ctxs[key] = self.fresh(name, mode, **env)
        return self.ctxs[key]

    def ref(self, name, p, pass_=0, begin=0, n=None):
        n = p.paths_per_pass if n is None else n
        key = (name, p.max_photon_count, p.max_specular_depth, pass_, begin, n)
        if key not in self.refs:
            if name not in self.orcs:
                self.orcs[name] = self.scene(name).load_into(self.oracle_mod.Oracle())
            self.refs[key] = self.orcs[name].trace_photons(p, pass_, begin, n)
            self.refs[key].setflags(write=False)
        return self.refs[key]

    def rules(self, name, p, slots, what, marked=False):
        """assert_layout and assert_paths; the float64 work once per distinct buffer, and not again for the first
        paths of a buffer that passed (every rule but the exempt share is a rule per path)"""
        mpc = p.max_photon_count
        T.assert_layout(slots, mpc, marked)
        raw = slots.tobytes()
        done = self.checked.setdefault((name, mpc, p.max_specular_depth, marked), {})
        if raw not in done:
            for whole in done:
                if whole.startswith(raw):
                    return done[whole]
            cap = T.EXEMPT_CAP if len(slots) >= 1000 * mpc else None
            done[raw] = T.assert_paths(self.scene(name), p, slots, marked=marked, cap=cap, what=what)
        return done[raw]

    def check(self, name, p, got, want, what):
        T.assert_same_slots(got, want, what)
        return self.rules(name, p, got, what)

    def close(self):
        for c in self.ctxs.values():
            c.close()


@pytest.fixture(scope="module")
def world(hip_mod, oracle_mod):
    w = World(hip_mod, oracle_mod)
    yield w
    w.close()


def trace(ctx, p, n, pass_=0, begin=0, base=None):
    base = begin if base is None else base
    ctx.trace_photons(p, pass_, begin, n, slot_path_base=base)
    return ctx.download_slots((begin + n - base) * p.max_photon_count)


def family_env(name, hold):
    """the environment of a scene's own family; the pooled scenes refill (one compute unit's waves)"""
    return dict(PM_TRACE_HOLD=hold, **({"PM_TRACE_CUS": 1} if name in POOLED else {}))


# ---- path counts ---------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)


@pytest.mark.parametrize("hold", [0, 1])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_path_counts(name, hold, world):
    """around a wave and a block; on the pooled scenes with and without PM_TRACE_CUS=1 (pools of 1 .. 50 paths)"""
    p = params(1000)
    want = world.ref(name, p)
    envs = [family_env(name, hold)] + ([dict(PM_TRACE_HOLD=hold)] if name in POOLED else [])
    for env in envs:
        ctx = world.ctx(name, **env)
        for n in reversed(COUNTS):   # the largest first: the smaller ones are its prefixes
            got = trace(ctx, p, n)
            world.check(name, p, got, want[:4 * n], f"{name} {env} {n} paths")


@pytest.mark.parametrize("name", ["cornell", "soup_hbm"])
def test_no_paths_leaves_the_buffer_alone(name, world):
    ctx = world.ctx(name, **family_env(name, 1))
    fill = np.frombuffer(b"\xa5" * (64 * 40), T.PHOTON_DTYPE)
    ctx.upload_slots(fill)
    ctx.trace_photons(params(1000, fused=True), 0, 0, 0)
    ctx.trace_photons(params(1000), 0, 17, 0, slot_path_base=17)
    T.assert_same_slots(ctx.download_slots(64), fill, "a trace of no paths")


# ---- the pooled kernel's refill loop ----------------------------------------------------------------------
# under PM_TRACE_CUS=1 a round is one CU's 16 or 20 waves: pools of ~150 to ~190 paths, the last one partial (the
# two counts differ by an odd number, so at most one of them divides evenly); 70 paths: pools of 4 or 5 and a last
# block with idle waves
REFILL_COUNTS = (3001, 2934, 70)
REFILL_ENVS = {"hold0": dict(PM_TRACE_HOLD=0), "hold1": dict(PM_TRACE_HOLD=1),
               "stack2": dict(PM_TRACE_HOLD=1, PM_POOL_STACK=2), "stack2-hold0": dict(PM_TRACE_HOLD=0, PM_POOL_STACK=2),
               "stack0": dict(PM_TRACE_HOLD=1, PM_POOL_STACK=0), "bvh8": dict(PM_TRACE_HOLD=1, PM_BVH8=1)}


@pytest.mark.parametrize("setting", sorted(REFILL_ENVS))
@pytest.mark.parametrize("name", POOLED)
def test_pooled_refill(name, setting, world):
    p = params(REFILL_COUNTS[0])
    want = world.ref(name, p)
    lane = world.ctx(name, PM_TRACE_POOL=0, PM_TRACE_HOLD=0)
    ctx = world.ctx(name, PM_TRACE_CUS=1, **REFILL_ENVS[setting])
    for n in REFILL_COUNTS:
        got = trace(ctx, p, n)
        world.check(name, p, got, want[:4 * n], f"{name} {setting} {n} paths")
        if setting != "bvh8":   # the 8-wide tree has no per-lane launch
            T.assert_same_slots(got, trace(lane, p, n), f"{name} {setting} {n} paths against the per-lane kernel")


def test_fewer_paths_than_waves(world):
    """the whole device's round: pools of one path, most waves of the plan's grid never launched"""
    p = params(300)
    for name in POOLED:
        got = trace(world.ctx(name, PM_TRACE_HOLD=1), p, 300)
        world.check(name, p, got, world.ref(name, params(1000))[:1200], f"{name}, 300 paths")


# ---- max_photon_count -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("hold", [0, 1])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_max_photon_count(name, hold, fused, world):
    """off the held layout's 4: per-deposit stores, slot-major (hold 1) or plane-major (hold 0) fused keys"""
    ctx = world.ctx(name, **family_env(name, hold))
    for mpc in (1, 2, 3, 5, 8):
        p = params(1000, mpc, fused=fused)
        got = trace(ctx, p, 1000)
        world.check(name, p, got, world.ref(name, p), f"{name} mpc {mpc} hold {hold} fused {fused}")
        if fused:
            ctx.build_photon_map(p, len(got))
            check_build(ctx, world.flat(name), p, got)


# ---- a slot buffer that is not 16-byte aligned ----------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "soup_hbm"])
def test_misaligned_slot_buffer(name, world):
    """hold wanted, the held launch refused (pm_plan.h's kept oddity): slot-major keys from per-deposit stores"""
    torch = pytest.importorskip("torch")
    n, p = 1000, params(1000, fused=True)
    buf = torch.zeros(4 * n * 40 + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptr = buf.data_ptr() + 8
    assert ptr % 16 == 8
    ctx = world.fresh(name, **family_env(name, 1))
    try:
        ctx.set_slot_buffer(ptr, 4 * n)
        ctx.trace_photons(p, 0, 0, n)
        ctx.build_photon_map(p, 4 * n)
        ctx.synchronize()
        got = np.frombuffer(buf[8:8 + 4 * n * 40].cpu().numpy().tobytes(), T.PHOTON_DTYPE)
        assert not buf[:8].any() and not buf[8 + 4 * n * 40:].any(), "written outside the slots"
        world.check(name, p, got, world.ref(name, p), f"{name}, misaligned buffer")
        check_build(ctx, world.flat(name), p, got)
        ctx.set_slot_buffer(0, 0)
    finally:
        ctx.close()


# ---- max_specular_depth ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,env", [("spheres_lds", {}), ("spheres_hbm", {"PM_TRACE_CUS": 1}),
                                      ("spheres_hbm", {"PM_TRACE_POOL": 0}), ("instanced", {})],
                         ids=["lds", "pooled", "hbm-lane", "instanced"])
def test_specular_depth(name, env, world):
    ctx = world.ctx(name, PM_TRACE_HOLD=1, **env)
    counts = {}
    for depth in (0, 1, 10):
        p = params(1000, depth=depth)
        got = trace(ctx, p, 1000)
        r = world.check(name, p, got, world.ref(name, p), f"{name} {env} depth {depth}")
        counts[depth] = r["deposits"]
        if depth == 0:
            assert r["bent"] == 0   # the first hit and every later one matte: every segment is a straight ray
    assert 0 < counts[0] < counts[1] < counts[10], counts


# ---- the top of the 32-bit slot index ---------------------------------------------------------------------------
@pytest.mark.parametrize("mpc,begin", [(4, 2 ** 30 - 301), (8, 2 ** 29 - 301)])
@pytest.mark.parametrize("name", ["cornell", "soup_hbm", "spheres_lds"])
def test_top_of_the_index_range(name, mpc, begin, world):
    """pid * mpc, the Philox counter pid * mpc + nI and pid - slot_path_base just below 2^32"""
    ctx = world.ctx(name, **family_env(name, 1))
    p = params(300, mpc)
    assert (begin + 300) * mpc == 2 ** 32 - mpc
    got = trace(ctx, p, 300, pass_=1, begin=begin)
    r = world.check(name, p, got, world.ref(name, p, 1, begin, 300), f"{name} mpc {mpc} from path {begin}")
    assert r["deposits"] > 100
    with pytest.raises(world.hip.PMError) as e:
        ctx.trace_photons(p, 1, begin, 301, slot_path_base=begin)
    assert e.value.code == PM_ERR_INVALID
    T.assert_same_slots(ctx.download_slots(300 * mpc), got, "the slots after a refused call")


# ---- shards ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "soup_hbm", "instanced"])
def test_shards_at_odd_boundaries(name, world):
    ctx = world.ctx(name, **family_env(name, 1))
    p = params(1000)
    want = world.ref(name, p)
    for cut in (1, 255, 257):
        ctx.upload_slots(np.zeros(4000, T.PHOTON_DTYPE))
        ctx.trace_photons(p, 0, cut, 1000 - cut, slot_path_base=0)
        ctx.trace_photons(p, 0, 0, cut, slot_path_base=0)
        world.check(name, p, ctx.download_slots(4000), want, f"{name} cut at {cut}")
    p2 = params(2000)
    got = trace(ctx, p2, 1000, begin=1000)
    T.assert_same_slots(got, world.ref(name, p2, 0, 0, 2000)[4000:], f"{name}: a shard at path 1000")
    world.rules(name, p2, got, f"{name}: a shard at path 1000")


# ---- counting launches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", [0, 1])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_counting_launch(name, hold, world):
    """the COUNT = 1 instantiations: the plain launch's slots, and a census that agrees with them"""
    ctx = world.ctx(name, **family_env(name, hold))
    for n, mpc in ((1000, 4), (2934, 4), (1000, 3)) if name in POOLED else ((1000, 4), (1000, 3)):
        p = params(n, mpc)
        plain = trace(ctx, p, n)
        ctx.set_counting(True)
        try:
            counted = trace(ctx, p, n)
            rays, nodes, prims, deposits = ctx.trace_counters()
        finally:
            ctx.set_counting(False)
        T.assert_same_slots(counted, plain, f"{name} hold {hold} {n} paths mpc {mpc}: a counting launch")
        T.assert_same_slots(counted, world.ref(name, params(3001 if n == 2934 else n, mpc))[:n * mpc], "against the oracle")
        assert deposits == int(T.valid(plain).sum()) > 0
        assert n <= rays <= n * (mpc + 1 + p.max_specular_depth), (rays, n)
        assert prims > 0 and (nodes > 0 or name == "cornell")


# ---- what the oracle lacks ---------------------------------------------------------------------------------------------
GEOMETRIES = {"pooled": dict(PM_TRACE_HOLD=0), "refill-hold1": dict(PM_TRACE_HOLD=1, PM_TRACE_CUS=1),
              "refill-stack2": dict(PM_TRACE_HOLD=0, PM_TRACE_CUS=1, PM_POOL_STACK=2),
              "refill-bvh8": dict(PM_TRACE_HOLD=1, PM_TRACE_CUS=1, PM_BVH8=1)}


@pytest.mark.parametrize("feature", sorted(FEATURES))
def test_features_over_every_geometry(feature, world):
    """each feature's trace at 1,000 paths: on its own small scene held and per deposit, and with 2,000 triangles
    around it under four pooled geometries, all bit-equal to the per-lane, hold-0 launch of the same scene"""
    p = params(1000, light_source_index=PM_ALL_LIGHTS if feature == "two_lights" else 0)
    plain = feature == "two_lights"
    small_mode = "brute"
    base = trace(world.ctx(feature, small_mode, PM_TRACE_HOLD=0), p, 1000)
    assert 500 < T.assert_layout(base, 4).sum() < 4000
    T.assert_same_slots(trace(world.ctx(feature, small_mode, PM_TRACE_HOLD=1), p, 1000), base, f"{feature}: held")
    if plain:
        world.rules(feature, p, base, feature)
    big = feature + "+soup"
    base = trace(world.ctx(big, "bvh-hbm", PM_TRACE_POOL=0, PM_TRACE_HOLD=0), p, 1000)
    assert 500 < T.assert_layout(base, 4).sum() < 4000
    if plain:
        world.rules(big, p, base, big)
    for geo, env in GEOMETRIES.items():
        T.assert_same_slots(trace(world.ctx(big, "bvh-hbm", **env), p, 1000), base, f"{big} {geo}")


@pytest.mark.parametrize("name", ["spheres_lds", "spheres_hbm"])
def test_caustic_marks_over_every_geometry(name, world):
    """pm_set_caustic_map on a plain scene: bit 1 aside, the unmarked trace (the oracle's), under every geometry"""
    p = params(1000, fused=True)
    want = world.ref(name, p)
    envs = [dict(PM_TRACE_HOLD=0), dict(PM_TRACE_HOLD=1)]
    if name in POOLED:
        envs = [dict(PM_TRACE_POOL=0, PM_TRACE_HOLD=0)] + list(GEOMETRIES.values())
    marked = []
    for env in envs:
        ctx = world.fresh(name, **env)
        try:
            ctx.set_caustic_map(True)
            got = trace(ctx, p, 1000)
        finally:
            ctx.close()
        marked.append(got)
        T.assert_same_slots(got, marked[0], f"{name} {env}: marked")
    got = marked[0]
    assert ((got["bits"] == 3).sum() > 20) and ((got["bits"] == 1).sum() > 500)
    world.rules(name, p, got, f"{name}: marked", marked=True)
    plain = got.copy()
    plain["bits"] &= np.uint32(1)
    T.assert_same_slots(plain, want, f"{name}: the marks masked off")
