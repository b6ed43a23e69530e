"""Pass planning on the CPU (csrc/pm_plan.cpp: the photon grid of a radius,
the histogram quantile, the adaptive-radius state machine R2Plan and the
device bands of a group render). tests/native/pass_plan_check.cpp runs the
commands this file scripts; the expected answers are pass_plan_ref.py's
restatements, pmrender/dist.py's _bands, and for the state machine the
transcripts below, written from the contract pm_plan.h states. CPU only:
compiles the checker against pm_plan.cpp, once more with the address and
undefined-behaviour sanitizers."""
import json
import os
import subprocess

import numpy as np
import pytest

import pass_plan_ref as ref
from pmrender import dist, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-raytrace_amd", "csrc")


def _compile(exe, *flags):
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *flags, "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "pass_plan_check.cpp"), os.path.join(CSRC, "pm_plan.cpp"),
                    "-o", str(exe)], check=True, timeout=300)
    return str(exe)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def run(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("pass_plan")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    exe = _compile(d / "pcheck", *flags)

    def go(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return go


def hx(x):
    return "%08x" % ref.bits(x)


# ---- the grid ------------------------------------------------------------------
BOXES = {
    "cornell": ref.scene_bbox(scenes.cornell_box(8, 8)),
    "caustic": ref.scene_bbox(scenes.caustic_scene(8, 8)),
    "flat": (np.float32([-3.0, 7.0, 1.5]), np.float32([96.5, 7.0005, 51.25])),  # y extent 5e-4 < 1e-3
}
RADII2 = (1e-4, 1e-2, 0.25, 1.0, 4.0, 25.0, 1e3)


def test_make_grid_matches_float32_restatement(run):
    cases = [(b, est, span, r2) for b in BOXES for est in (ref.PM_ESTIMATOR_PPM, ref.PM_ESTIMATOR_KNN)
             for span in (2, 3, 4, 5) for r2 in RADII2]
    lines = ["grid %s %s %d %d %s" % (" ".join(hx(v) for v in BOXES[b][0]), " ".join(hx(v) for v in BOXES[b][1]), est, span, hx(r2))
             for b, est, span, r2 in cases]
    capped = 0
    for (b, est, span, r2), got in zip(cases, run(lines)):
        dx, dy, dz, ncells, inv_cs = ref.make_grid(*BOXES[b], est, span, r2)
        assert got == "grid %d %d %d %d %08x" % (dx, dy, dz, ncells, inv_cs), (b, est, span, r2)
        # the cap loop ran where the uncapped cell edge (make_grid's first cs) would give more than 2^25 cells
        rq = np.sqrt(np.float32(r2)) * np.float32(1.0001) + np.float32(1e-4)
        cs0 = ((np.float32(0.5) if est else np.float32(2.0) / np.float32(span - 1)) * rq) * np.float32(1.001)
        capped += ref.from_bits(inv_cs) < np.float32(1.0) / cs0
        assert ncells <= 1 << 25
    assert capped >= len(BOXES), "no case entered the 2^25-cell cap loop"


def test_grid_restatement_agrees_with_the_recorded_render():
    """the restated box and grid give the cell count the MI355X recorded for
    the Cornell box at the initial radius (golden/grid_plan_v1.json, pass 0)"""
    with open(os.path.join(ROOT, "tests", "golden", "grid_plan_v1.json")) as f:
        rec = json.load(f)["sequences"]["plain"][0]
    assert ref.make_grid(*BOXES["cornell"], ref.PM_ESTIMATOR_PPM, 2, 25.0)[3] == rec["cells"]


# ---- the quantile ------------------------------------------------------------
def spikes(*pairs):
    h = [0] * ref.R2_BINS
    for b, n in pairs:
        h[b] = n
    return h


HISTS = {
    "bin0": spikes((0, 1000)), "bin63": spikes((63, 1000)), "empty": spikes(),
    "two_spikes": spikes((3, 700), (40, 300)), "uniform": [17] * ref.R2_BINS,
}
SHRUNK = spikes((5, 100), (9, 500), (14, 400))  # a progressive render's radii after a few passes


def test_quantile_pick_matches_float64_restatement(run):
    cases = [(h, q, init) for h in HISTS for q in (0.5, 0.9, 0.99) for init in (25.0, 0.37)]
    lines = ["quant %r %s %s" % (q, hx(init), " ".join(map(str, HISTS[h]))) for h, q, init in cases]
    for (h, q, init), got in zip(cases, run(lines)):
        _, b, r2 = got.split()
        want_b, want_r2 = ref.quantile_radius2(HISTS[h], np.float32(init), q)
        assert int(b) == want_b, (h, q, init)
        assert abs(int(r2, 16) - ref.bits(want_r2)) <= 1, (h, q, init, r2, hx(want_r2))  # libm exp2 vs 2.0 ** x: 1 ulp
        assert ref.from_bits(int(r2, 16)) <= np.float32(init)
        if h == "empty":
            assert int(r2, 16) == 0
    assert ref.quantile_radius2(HISTS["two_spikes"], np.float32(25.0), 0.5)[0] == 3
    assert ref.quantile_radius2(HISTS["two_spikes"], np.float32(25.0), 0.9)[0] == 3
    assert ref.quantile_radius2(HISTS["bin63"], np.float32(25.0), 0.9)[0] == 63


# ---- the bands -----------------------------------------------------------------
def test_device_bands_equal_dist_bands(run):
    cases = [(n, unit, world) for n in (0, 1, 511, 512, 513, 6912, 49152) for unit in (64, 512, 768) for world in range(1, 9)]
    for (n, unit, world), got in zip(cases, run(["bands %d %d %d" % c for c in cases])):
        want = "|".join(",".join("%d:%d" % bc for bc in owned) for owned in dist._bands(n, unit, world))
        assert got == "bands " + want, (n, unit, world)


# ---- the state machine ---------------------------------------------------------
# A step is (command, answer, flags[, field checks]); flags are the plan's
# wanted accum dirty pending valid after the event. The commands of a pass
# come in the order pm_api_photons.cpp's grid_radius2 delivers them: active, landed
# (the pending reduce's event has fired), due, issued (the reduce was
# launched), began, radius; a binning gather (one that finds `wanted`) is
# bin, binned. Streams: 1 = A, 2 = B. INIT: answer `radius` with the initial
# radius; Q(hist): with the restated quantile of hist, within 1 ulp.
I25, I16 = hx(25.0), hx(16.0)
INIT = "init"


class Q:
    def __init__(self, hist, init=25.0, quantile=0.9):
        self.r2 = ref.quantile_radius2(hist, np.float32(init), quantile)[1]


def H(h):
    return " ".join(map(str, h))


def pass_(fresh, radius, flags, init=I25):
    """a pass with nothing landed and no reduce due"""
    return [("active 0", "active 1", None), ("due", "due 0", None), (f"began {fresh}", "began", flags),
            (f"radius {init} {fresh}", radius, flags)]


def gather(stream, clear, flags_after, init=I25, wait=0):
    return [(f"bin {init} {stream}", f"bin wait={wait} clear={clear}", None), (f"binned {init}", "binned", flags_after)]


FRESH_RENDER = [("new 0.9", "new", "00100")] + pass_(1, INIT, "00100")  # 1: wanted stays 0, so the gather bins nothing

PROGRESSIVE = FRESH_RENDER + (
    pass_(0, INIT, "10100") + gather(1, 1, "11000")                                  # pass 1 wants bins; the first bins are cleared
    + [("active 0", "active 1", None), ("due", "due 1", None), ("issued 1", "issued", "10011"),
       ("began 0", "began", "10011"), (f"radius {I25} 0", INIT, "10011")]             # pass 2 issues the reduce, still init
    + gather(1, 0, "11011")
    + [("active 0", "active 1", None), (f"landed {I25} {H(SHRUNK)}", "landed", "11001"),
       ("due", "due 1", None), ("issued 1", "issued", "10011"), ("began 0", "began", "10011"),
       (f"radius {I25} 0", Q(SHRUNK), "10011")]                                       # pass 3: the landed quantile
    + gather(1, 0, "11011"))

SHRUNK2 = spikes((12, 300), (20, 700))
INVALIDATED = PROGRESSIVE + (
    [("invalidate", "invalidate", "10110", {"design_r2": 0})]                          # 3: bins dropped, back to init
    + [("active 0", "active 1", None), (f"landed {I25} {H(SHRUNK)}", "landed", "10100", {"design_r2": 0}),
       ("due", "due 0", None), ("began 0", "began", "10100"), (f"radius {I25} 0", INIT, "10100")]
    + gather(1, 1, "11000")                                                           # told to clear
    + [("due", "due 1", None), ("issued 1", "issued", "10011"), ("began 0", "began", "10011"),
       (f"radius {I25} 0", INIT, "10011")]                                            # reduce in flight: still init
    + gather(1, 0, "11011")
    + [(f"landed {I25} {H(SHRUNK2)}", "landed", "11001"), (f"radius {I25} 0", Q(SHRUNK2), "11001")])

INIT_CHANGES = [("new 0.9", "new", "00100"), ("began 0", "began", "10100")] + (       # 4
    gather(1, 1, "11000") + gather(1, 0, "11000")
    + [(f"bin {I16} 1", "bin wait=0 clear=1", "10000"), (f"binned {I16}", "binned", "11000", {"accum_init": 16.0})])

CROSS_STREAM = [("new 0.9", "new", "00100"), ("began 0", "began", "10100")] + gather(1, 1, "11000") + [  # 5
    ("due", "due 1", None), ("issued 1", "issued", "10011"),
    (f"bin {I25} 2", "bin wait=1 clear=0", "10011"),                                  # reduce on A, gather on B: wait
    (f"bin {I25} 1", "bin wait=0 clear=0", "10011"),                                  # on A the stream orders them
    (f"landed {I25} {H(SHRUNK)}", "landed", "10001"),
    (f"bin {I25} 2", "bin wait=0 clear=0", "10001")]                                  # nothing in flight: no wait

ONE_REDUCE_AT_A_TIME = [("new 0.9", "new", "00100"), ("began 0", "began", "10100")] + gather(1, 1, "11000") + [  # 6
    ("due", "due 1", None), ("issued 1", "issued", "10011")] + gather(1, 0, "11011") + [
    ("due", "due 0", "11011"),                                                        # bins accumulated, first reduce pending
    (f"landed {I25} {H(SHRUNK)}", "landed", "11001"), ("due", "due 1", "11001")]

OTHER_INIT_LANDS = [("new 0.9", "new", "00100"), ("began 0", "began", "10100")] + gather(1, 1, "11000") + [  # 7
    ("due", "due 1", None), ("issued 1", "issued", "10011", {"hist_init": 25.0}),
    (f"landed {I16} {H(SHRUNK)}", "landed", "10001", {"design_r2": 0}),               # the pass's init is 16: ignored
    (f"radius {I16} 0", INIT, "10001"), (f"radius {I25} 0", INIT, "10001")]

INACTIVE = PROGRESSIVE + [("active 1", "active 0", "11011")] + [                      # 8: kNN; then quantile 0 and below
    ("new 0", "new", "00100"), ("active 0", "active 0", "00100"), ("active 1", "active 0", "00100"),
    ("new -1", "new", "00100"), ("active 0", "active 0", "00100")]

FAILED_ISSUE = [("new 0.9", "new", "00100"), ("began 0", "began", "10100")] + gather(1, 1, "11000") + [  # 9
    ("due", "due 1", "11000"),                                                        # the launch failed: no `issued`
    ("began 0", "began", "11000"), (f"radius {I25} 0", INIT, "11000"),
    ("due", "due 1", "11000")]                                                        # still due at the next pass

SCENARIOS = {"fresh_render": FRESH_RENDER, "progressive": PROGRESSIVE, "invalidated": INVALIDATED,
             "init_changes": INIT_CHANGES, "cross_stream": CROSS_STREAM, "one_reduce_at_a_time": ONE_REDUCE_AT_A_TIME,
             "other_init_lands": OTHER_INIT_LANDS, "inactive": INACTIVE, "failed_issue": FAILED_ISSUE}


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_adaptive_radius_state_machine(run, name):
    steps = SCENARIOS[name]
    out = run([s[0] for s in steps])
    prev_state = None
    for k, (step, got) in enumerate(zip(steps, out)):
        cmd, answer, flags = step[:3]
        got_answer, state = got.split(" | ")
        st = state.split()
        where = f"{name} step {k}: {cmd[:40]} -> {got}"
        if answer is INIT or isinstance(answer, Q):
            word, r2 = got_answer.split()
            init = ref.from_bits(int(cmd.split()[1], 16))
            assert word == "radius", where
            if answer is INIT:
                assert int(r2, 16) == ref.bits(init), where
            else:
                assert abs(int(r2, 16) - ref.bits(answer.r2)) <= 1, where
                assert ref.from_bits(int(r2, 16)) < init, where  # SHRUNK radii: below init (never above it)
        else:
            assert got_answer == answer, where
        if flags is None:  # a query: no state changes
            flags = prev_state[:5] if not cmd.startswith("bin ") else None
        if flags is not None:
            assert "".join(st[:5]) == "".join(flags), where
        if cmd.split()[0] in ("active", "due", "radius"):
            assert prev_state is None or st == prev_state, where + " (a query changed the state)"
        for field, want in (step[3] if len(step) > 3 else {}).items():
            assert st[5 + ("accum_init", "hist_init", "design_r2").index(field)] == hx(want), where
        prev_state = st
