"""The trace launch's plan on the CPU (csrc/pm_plan.cpp plan_trace: kernel
family, LDS stack entries, paths per wave, grid, dynamic LDS bytes, held
deposits, spill area). tests/native/trace_plan_check.cpp runs the commands
this file scripts, with an occupancy table in place of the device; the
expected answers are trace_plan_ref.py's restatement of the contract in
pm_plan.h. Every case also checks what the kernels rely on: the spill
stride is the grid's thread count, the pools cover every path, and the LDS
the launch reserves covers the columns the kernels index. CPU only: compiles
the checker against pm_plan.cpp, once more with the address and
undefined-behaviour sanitizers."""
import itertools
import os
import subprocess

import pytest

import trace_plan_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-raytrace_amd", "csrc")
TB = ref.TRACE_BLOCK


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def run(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("trace_plan")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    exe = str(d / "tcheck")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *flags, "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "trace_plan_check.cpp"), os.path.join(CSRC, "pm_plan.cpp"),
                    "-o", exe], check=True, timeout=300)

    def go(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return go


# The occupancy table: an MI355X CU has 160 KB of LDS; register-bound waves per
# CU as DESIGN.md records them (waves per SIMD x 4): the per-lane kernels 6-7,
# k_trace_pool 5, k_trace_pool8 4. Index 2 * family + hold.
LDS_CU = 160 * 1024
REGS = [24, 24, 24, 24, 28, 28, 24, 24, 20, 20, 16, 16]
ROOMY = 64 << 20  # so much LDS that held deposits never cost a wave

FIELDS = ("family", "pooled", "lstk", "pool_paths", "grid", "lds", "lds_hold", "hold", "hold_launch", "spill_entries",
          "spill_stride")


def case(paths=10000, mpc=4, aligned=1, mode=ref.MODE_GLOBAL, wide=2, depth=24, blob=None, pool_stack=31, trace_pool=1,
         trace_hold=1, cus=8, cap=LDS_CU, regs=REGS):
    if blob is None:  # an LDS-resident scene brings its blob: not a multiple of 16, so the pad shows
        blob = 4100 if mode in (ref.MODE_LDS, ref.MODE_BRUTE) else 0
    return dict(paths=paths, mpc=mpc, aligned=aligned, mode=mode, wide=wide, depth=depth, blob=blob, pool_stack=pool_stack,
                trace_pool=trace_pool, trace_hold=trace_hold, cus=cus, cap=cap, regs=regs)


def command(c):
    return "plan %d %d %d %d %d %d %d %d %d %d %d  %d %s" % (
        c["paths"], c["mpc"], c["aligned"], c["mode"], c["wide"], c["depth"], c["blob"], c["pool_stack"], c["trace_pool"],
        c["trace_hold"], c["cus"], c["cap"], " ".join(map(str, c["regs"])))


def expected(c):
    args = {k: c[k] for k in ("paths", "mpc", "aligned", "mode", "wide", "depth", "blob", "pool_stack", "trace_pool",
                              "trace_hold", "cus")}
    return ref.plan(ask=ref.table(c["cap"], c["regs"]), **args)


def parse(line):
    head, _, tail = line.partition("|")
    words = head.split()
    assert words[0] == "plan" and len(words) == 1 + len(FIELDS), line
    asked = [tuple(int(v) for v in q.split(":")) for q in tail.split()]
    return dict(zip(FIELDS, map(int, words[1:]))), asked


def check(run, cases):
    """-> the parsed plans; every case equals the restatement and keeps the couplings"""
    plans = []
    for c, line in zip(cases, run([command(c) for c in cases])):
        got, asked = parse(line)
        want, want_asked = expected(c)
        assert got == want, (c, got, want)
        assert asked == want_asked, (c, asked, want_asked)
        held = ref.HELD_BYTES
        if got["pooled"]:
            # what the code relies on: the spill area is addressed by blockIdx.x * TRACE_BLOCK + threadIdx.x,
            # and wave w of the grid takes paths [w * pool_paths, (w + 1) * pool_paths)
            assert c["wide"] and c["mode"] == ref.MODE_GLOBAL and got["pool_paths"] > 0, c
            assert got["grid"] * (TB // 64) * got["pool_paths"] >= c["paths"], (c, got)
            assert got["spill_entries"] == c["depth"] - got["lstk"] >= 0, (c, got)
            assert got["spill_stride"] == (got["grid"] * TB if got["spill_entries"] else 0), (c, got)
            # trace_pool_body: stacks of lstk entries, the held columns right after them
            assert got["lds"] == got["lstk"] * TB * 4 and got["lds_hold"] == got["lds"] + held, (c, got)
        else:
            assert got["grid"] * TB >= c["paths"] > (got["grid"] - 1) * TB, (c, got)
            # trace_lane_body: stacks of S.stack_depth entries, the blob (LDS modes), the held columns at
            # word stack_depth * TRACE_BLOCK + ((lds_bytes + 15) / 4 & ~3) (LDS modes; else right after the stacks)
            blob_words = ((c["blob"] + 15) // 4 & ~3) if c["mode"] in (ref.MODE_LDS, ref.MODE_BRUTE) else 0
            assert got["lds"] == c["depth"] * TB * 4 + c["blob"], (c, got)
            assert got["lds_hold"] >= (c["depth"] * TB + blob_words) * 4 + held, (c, got)
            assert got["lds_hold"] - got["lds"] - held in range(16), (c, got)
        assert 0 <= got["lstk"] <= c["depth"] and got["hold_launch"] <= got["hold"] <= c["trace_hold"], (c, got)
        plans.append(got)
    return plans


MODES = (ref.MODE_GLOBAL, ref.MODE_LDS, ref.MODE_BRUTE, ref.MODE_INST)


def test_per_lane_against_pooled_for_every_mode_and_tree(run):
    cases = [case(mode=m, wide=w, trace_pool=tp, trace_hold=h, cap=cap, pool_stack=ps)
             for m, w, tp, h, cap, ps in itertools.product(MODES, (0, 1, 2, 3), (0, 1), (0, 1), (LDS_CU, ROOMY), (31, 16))]
    cases += [case(mode=ref.MODE_INST, wide=w, blob=4100) for w in (0, 2)]  # a small instanced scene: LDS bytes, never used
    for c, p in zip(cases, check(run, cases)):
        # pooled: an HBM scene with a wide tree, unless PM_TRACE_POOL=0 — which the 8-wide tree overrides
        assert p["pooled"] == int(c["mode"] == ref.MODE_GLOBAL and c["wide"] != 0 and (c["trace_pool"] or c["wide"] == 3)), c
        assert p["family"] == ((ref.POOL8 if c["wide"] == 3 else ref.POOL) if p["pooled"] else ref.LANE_OF_MODE[c["mode"]]), c
        if not c["wide"]:
            assert (p["lstk"], p["pool_paths"], p["spill_entries"], p["spill_stride"]) == (0, 0, 0, 0), c


def test_instanced_wide_scene_is_planned_pooled_and_launched_per_lane(run):
    c = case(mode=ref.MODE_INST, wide=2, depth=40, pool_stack=31, paths=5000)
    p, = check(run, [c])
    q, = check(run, [dict(c, mode=ref.MODE_GLOBAL)])
    assert not p["pooled"] and p["family"] == ref.LANE_INST and p["grid"] == 20
    # the kept disagreement: TraceParams still carry the pooled geometry, spill stride included
    assert (p["lstk"], p["pool_paths"], p["hold"], p["spill_entries"], p["spill_stride"]) == \
        (q["lstk"], q["pool_paths"], q["hold"], q["spill_entries"], q["spill_stride"]) == (31, 32, 0, 9, q["grid"] * TB)
    assert p["spill_stride"] != p["grid"] * TB


@pytest.mark.parametrize("wide,depth", [(2, 24), (3, 60)])
def test_pool_stack_against_the_stack_bound(run, wide, depth):
    stacks = (0, 1, depth - 5, depth - 1, depth, depth + 5)
    plans = check(run, [case(wide=wide, depth=depth, pool_stack=ps) for ps in stacks])
    assert [p["lstk"] for p in plans] == [depth, 1, depth - 5, depth - 1, depth, depth]
    assert [p["spill_entries"] for p in plans] == [0, depth - 1, 5, 1, 0, 0]
    for p in plans:
        assert p["pooled"] and (p["spill_stride"] > 0) == (p["spill_entries"] > 0)


def test_hold_kept_and_dropped_by_occupancy(run):
    for mode, wide, fam in ((ref.MODE_BRUTE, 0, ref.LANE_BRUTE), (ref.MODE_LDS, 0, ref.LANE_LDS), (ref.MODE_GLOBAL, 0, ref.LANE_GLOBAL),
                            (ref.MODE_INST, 0, ref.LANE_GLOBAL), (ref.MODE_GLOBAL, 2, ref.POOL), (ref.MODE_GLOBAL, 3, ref.POOL8)):
        kept, dropped, off = check(run, [case(mode=mode, wide=wide, cap=ROOMY), case(mode=mode, wide=wide, cap=LDS_CU),
                                         case(mode=mode, wide=wide, cap=ROOMY, trace_hold=0)])
        assert (kept["hold"], kept["hold_launch"]) == (1, 1), (mode, wide)
        assert (dropped["hold"], dropped["hold_launch"]) == (0, 0), (mode, wide)  # 27 KB more LDS per block: fewer blocks in 160 KB
        assert (off["hold"], off["hold_launch"]) == (0, 0), (mode, wide)
        # both instantiations of one family were asked, the HOLD one with the held columns on top
        asked = expected(case(mode=mode, wide=wide, cap=ROOMY))[1]
        assert sorted((f, h) for f, h, _ in asked) == [(fam, 0), (fam, 1)], (mode, wide)
        by_hold = {h: lds for _, h, lds in asked}
        assert by_hold[1] - by_hold[0] - ref.HELD_BYTES in range(16)
        # PM_TRACE_HOLD=0 asks nothing about held deposits
        assert all(h == 0 for _, h, _ in expected(case(mode=mode, wide=wide, trace_hold=0))[1])
    # equal waves keep the deposits held; the pooled round then counts the HOLD kernel's waves
    tight = list(REGS)
    tight[2 * ref.POOL + 1] = 12
    p, = check(run, [case(cap=ROOMY, regs=tight, paths=100000)])
    assert p["hold"] == 0 and p["pool_paths"] == -(-100000 // (8 * 20))
    tight[2 * ref.POOL] = 12
    p, = check(run, [case(cap=ROOMY, regs=tight, paths=100000)])
    assert p["hold"] == 1 and p["pool_paths"] == -(-100000 // (8 * 12))


def test_the_pooled_occupancy_is_asked_with_the_scene_lds_bytes(run):
    """kept as measured: the query adds S.lds_bytes to the stacks, the pooled launch reserves the stacks alone"""
    c = case(mode=ref.MODE_INST, wide=2, blob=4100, depth=20, pool_stack=0, trace_hold=0)
    check(run, [c])
    assert expected(c)[1] == [(ref.POOL, 0, 20 * TB * 4 + 4100)]
    c = case(mode=ref.MODE_GLOBAL, wide=2, depth=20, pool_stack=0, trace_hold=0)
    p, = check(run, [c])
    assert expected(c)[1] == [(ref.POOL, 0, p["lds"])]


def test_hold_at_another_mpc_or_a_misaligned_slot_buffer(run):
    """TraceParams::hold (the fused keys' layout, the lazy zero fill) stays set; only the launch stores per deposit"""
    for mode, wide in ((ref.MODE_BRUTE, 0), (ref.MODE_GLOBAL, 2), (ref.MODE_INST, 2)):
        base = case(mode=mode, wide=wide, cap=ROOMY)
        plans = check(run, [base, dict(base, mpc=3), dict(base, mpc=5), dict(base, mpc=1), dict(base, aligned=0),
                            dict(base, mpc=8, aligned=0)])
        assert [(p["hold"], p["hold_launch"]) for p in plans] == [(1, 1)] + [(1, 0)] * 5
        for p in plans[1:]:  # nothing else moves
            assert {k: v for k, v in p.items() if k != "hold_launch"} == {k: v for k, v in plans[0].items() if k != "hold_launch"}


def test_occupancy_unknown(run):
    """0 from the occupancy query: 16 waves per CU; an unknown device: 256 CUs"""
    unknown, no_cus, neither = check(run, [case(cap=0, cus=8, paths=1 << 16), case(cus=0, paths=1 << 20, trace_hold=0),
                                           case(cap=0, cus=-1, paths=1 << 20)])
    assert unknown["pool_paths"] == (1 << 16) // (8 * 16) and unknown["hold"] == 1  # 0 waves held, 0 plain: not fewer
    assert no_cus["pool_paths"] == -(-(1 << 20) // (256 * 20))
    assert neither["pool_paths"] == (1 << 20) // (256 * 16) and neither["grid"] == 1024
    lane, = check(run, [case(mode=ref.MODE_BRUTE, wide=0, cap=0)])
    assert lane["hold"] == 1


def test_path_counts_around_a_wave_a_block_and_an_occupancy_round(run):
    cus, per_cu = 8, 20
    round_waves = cus * per_cu  # one occupancy round of the pooled kernel at REGS, no hold
    counts = [0, 1, 63, 64, 65, 255, 256, 257, round_waves - 1, round_waves, round_waves + 1, 64 * round_waves - 1,
              64 * round_waves, 64 * round_waves + 1, 3 * 64 * round_waves + 7]
    pooled = check(run, [case(paths=n, cus=cus, depth=40) for n in counts])
    for n, p in zip(counts, pooled):
        assert p["pool_paths"] == max(1, -(-n // round_waves)), n
        waves = -(-n // p["pool_paths"])
        assert waves <= round_waves and p["grid"] == -(-waves // 4), (n, p)  # never more than one round
        assert p["spill_stride"] == p["grid"] * TB
    assert [p["pool_paths"] for p in pooled[8:14]] == [1, 1, 2, 64, 64, 65]
    lanes = check(run, [case(paths=n, mode=ref.MODE_BRUTE, wide=0) for n in counts])
    assert [p["grid"] for p in lanes[:8]] == [0, 1, 1, 1, 1, 1, 1, 2]


def test_one_compute_unit_gives_small_traces_long_pools(run):
    """PM_TRACE_CUS=1 (the context's planning input, TraceShape::cus): one CU's 20 pooled waves share the trace, so a
    few thousand paths make pools of more than a wave's 64 lanes, whose lanes take second and third paths. Pool,
    grid and spill stride move together. Occupancy comes in whole blocks, so above 19 paths per wave every wave of
    the round has a pool and the last block is full; below, the last block can hold waves without one."""
    round_waves = 20  # REGS and 160 KB of LDS at 31 stack entries: five blocks
    counts = [3001, 2934, 1281, 70, 37, 1]
    for hold, cap in ((0, LDS_CU), (1, ROOMY)):
        cases = [case(paths=n, cus=1, depth=40, trace_hold=hold, cap=cap) for n in counts]
        for n, c, p in zip(counts, cases, check(run, cases)):
            want, _ = expected(c)
            assert (p["grid"], p["spill_stride"], p["lds_hold"], p["pool_paths"]) == \
                (want["grid"], want["spill_stride"], want["lds_hold"], want["pool_paths"])
            assert p["pooled"] and p["hold"] == hold and p["pool_paths"] == -(-n // round_waves)
            assert p["spill_entries"] == 9 and p["spill_stride"] == p["grid"] * TB
            waves, last, idle = ref.pool_layout(p, n)
            assert (waves - 1) * p["pool_paths"] < n <= waves * p["pool_paths"] and 0 <= idle < 4
            if n > 64 * round_waves:
                assert p["pool_paths"] > 64 and (waves, p["grid"], idle) == (round_waves, 5, 0)
        by = {n: (p, ref.pool_layout(p, n)) for n, p in zip(counts, check(run, cases))}
        assert [by[n][0]["pool_paths"] for n in counts] == [151, 147, 65, 4, 2, 1]
        assert by[3001][1] == (20, 132, 0) and by[2934][1] == (20, 141, 0) and by[1281][1] == (20, 46, 0)
        # the last pool partial and the last block not full: 70 paths in pools of 4 are 18 waves, the last of 2
        # paths, in five blocks whose last two waves find their pool empty
        assert by[70][1] == (18, 2, 2) and by[70][0]["grid"] == 5
        assert by[37][1] == (19, 1, 1) and by[1][1] == (1, 1, 3) and by[1][0]["grid"] == 1
    # the same traces on the whole device: pools of one path, no lane takes a second
    assert all(p["pool_paths"] == 1 for p in check(run, [case(paths=n, cus=256, depth=40) for n in counts]))


def test_trace_pool_off_and_the_eight_wide_tree(run):
    off4, off8, on8 = check(run, [case(trace_pool=0, wide=2, depth=40), case(trace_pool=0, wide=3, depth=70),
                                  case(trace_pool=1, wide=3, depth=70)])
    assert (off4["pooled"], off4["pool_paths"], off4["family"]) == (0, 0, ref.LANE_GLOBAL)
    assert off4["lstk"] == 31 and off4["spill_entries"] == 9  # planned all the same; the per-lane kernel reads neither
    assert off8 == on8 and on8["pooled"] and on8["family"] == ref.POOL8 and on8["spill_entries"] == 70 - 31


def test_recorded_points(run):
    """C2 (the Cornell box traced by brute force from LDS, 262,144 paths as one occupancy round of
    4,096 waves; k_trace_lane<0, MODE_BRUTE, 0>: 7 waves per SIMD by registers, so 27 KB of held deposits per block
    would cost blocks and are dropped) and C3 (1M paths over the 4-wide tree: one round of 4,096 pooled waves on
    256 CUs at four blocks per CU, 4 paths per lane)."""
    c2, = check(run, [case(paths=262144, mode=ref.MODE_BRUTE, wide=0, depth=2, blob=4112, cus=256)])
    assert (c2["pooled"], c2["family"], c2["grid"], c2["grid"] * 4, c2["hold"]) == (0, ref.LANE_BRUTE, 1024, 4096, 0)
    four_blocks = list(REGS)
    four_blocks[2 * ref.POOL] = four_blocks[2 * ref.POOL + 1] = 16
    c3, = check(run, [case(paths=1 << 20, wide=2, depth=40, pool_stack=31, cus=256, regs=four_blocks)])
    assert (c3["pooled"], c3["family"], c3["pool_paths"], c3["grid"], c3["grid"] * 4) == (1, ref.POOL, 256, 1024, 4096)
    assert (c3["lstk"], c3["spill_entries"], c3["spill_stride"], c3["lds"]) == (31, 9, 262144, 31744)
