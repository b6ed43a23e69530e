"""The caustic map of final gathering (pm_set_caustic_map, pm_build_caustic_map,
pm_caustic_gather and their test hooks), the parts that need no device: the
argument checks the C-ABI makes on a null context, the .pbrt key and the
command-line flag, and the trace plan's choice under marking (deposits stored
one by one: HOLD = 0), driven through tests/native/caustic_plan_check.cpp.
"""
import ctypes
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import trace_plan_ref as ref
from pmrender import hip
from pmrender.abi import PM_ERR_INVALID, RenderParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-raytrace_amd", "csrc")
CLI = os.path.join(ROOT, "cuda-raytrace_amd", "lib", "pm_render_cli")
SCENES = os.path.join(ROOT, "cuda-raytrace_amd", "scenes")


def test_argument_checks_on_a_null_context():
    lib = hip.load_library()
    p = RenderParams.defaults()
    ref_p = ctypes.byref(p)
    err = lambda: lib.pm_last_error(None)
    u32 = (ctypes.c_uint32 * 4)()
    rgb = np.zeros(3, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.pm_set_caustic_map(None, 1) == PM_ERR_INVALID and b"null context" in err()
    assert lib.pm_build_caustic_map(None, None) == PM_ERR_INVALID and b"null context" in err()
    # what needs no context is checked before the context is
    assert lib.pm_caustic_gather(None, None, 0, None) == PM_ERR_INVALID and b"null params" in err()
    assert lib.pm_caustic_gather(None, ref_p, -1, None) == PM_ERR_INVALID and b"negative" in err()
    assert lib.pm_caustic_gather(None, ref_p, 0, None) == PM_ERR_INVALID and b"null context" in err()
    assert lib.pm_caustic_map_count(None) == -1
    assert lib.pm_download_caustic_slots(None, u32, 1) == PM_ERR_INVALID and b"null context" in err()
    assert lib.pm_download_caustic_cell_start(None, u32, 1) == PM_ERR_INVALID and b"null context" in err()
    assert lib.pm_download_caustic_radiance(None, rgb, 1) == PM_ERR_INVALID and b"null context" in err()


# ------------------------------------------------------------------ parser
SCENE = """
LookAt 278 273 -800  278 273 0  0 1 0
Camera "perspective" "float fov" [39.3]
Film "image" "integer xresolution" [16] "integer yresolution" [16] "string filename" "cm.pfm"
Renderer "cuda" "string rendername" "photonmapping" "integer paths" [4096] %s
WorldBegin
LightSource "point" "point from" [278 500 279.5] "rgb I" [150000 150000 150000]
Material "matte" "rgb Kd" [0.5 0.5 0.5]
Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0  556 0 0  556 0 559]
WorldEnd
"""


def dump(path, *flags):
    r = subprocess.run([CLI, "--pbrt", str(path), "--dump", *flags], capture_output=True, text=True, timeout=60)
    return r, (json.loads(r.stdout) if r.returncode == 0 else None)


def test_causticmap_key_and_flag(tmp_path):
    f = tmp_path / "cm.pbrt"
    f.write_text(SCENE % '"integer finalgathersamples" [8] "bool causticmap" ["true"]')
    r, d = dump(f)
    assert r.returncode == 0, r.stderr
    assert d["caustic_map"] == 1 and d["final_gather"] == 8 and d["warnings"] == 0
    f.write_text(SCENE % '"integer finalgathersamples" [8] "bool causticmap" ["false"]')
    r, d = dump(f)
    assert d["caustic_map"] == 0 and d["warnings"] == 0
    r, d = dump(f, "--caustic-map")                      # the flag switches it on
    assert d["caustic_map"] == 1 and d["final_gather"] == 8 and d["warnings"] == 0
    # honoured only together with final gathering: without it a warning, and the switch stays off
    f.write_text(SCENE % '"bool causticmap" ["true"]')
    r, d = dump(f)
    assert r.returncode == 0 and d["caustic_map"] == 0 and d["final_gather"] == 0 and d["warnings"] == 1
    assert "causticmap" in r.stderr and "final gathering" in r.stderr
    r, d = dump(f, "--final-gather", "4")                # ... which the command line can supply
    assert d["caustic_map"] == 1 and d["final_gather"] == 4 and d["warnings"] == 0
    f.write_text(SCENE % '"integer finalgathersamples" [8] "bool causticmap" ["true"]')
    r, d = dump(f, "--final-gather", "0")                # ... or take away
    assert d["caustic_map"] == 0 and d["warnings"] == 1 and "--caustic-map" in r.stderr
    f.write_text(SCENE % "")
    r, d = dump(f, "--caustic-map")
    assert d["caustic_map"] == 0 and d["warnings"] == 1
    for name in ("cornell-box.pbrt", "caustic-glass.pbrt"):  # every key is off by default: nothing parsed today changes
        r, d = dump(os.path.join(SCENES, name))
        assert d["caustic_map"] == 0 and d["final_gather"] == 0 and d["warnings"] == 0
    r = subprocess.run([CLI, "--caustic-map"], capture_output=True, text=True, timeout=60)  # the flag needs a scene file
    assert r.returncode == 2 and "--caustic-map" in r.stderr


# ------------------------------------------------------------------ the trace plan under marking
LDS_CU = 160 * 1024
REGS = [24, 24, 24, 24, 28, 28, 24, 24, 20, 20, 16, 16]
ROOMY = 64 << 20  # so much LDS that held deposits never cost a wave: the unmarked plan holds them
FIELDS = ("family", "pooled", "lstk", "pool_paths", "grid", "lds", "lds_hold", "hold", "hold_launch", "spill_entries",
          "spill_stride")
ARGS = ("paths", "mpc", "aligned", "mode", "wide", "depth", "blob", "pool_stack", "trace_pool", "trace_hold", "cus")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("caustic_plan")
    exe = str(d / "ccheck")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "caustic_plan_check.cpp"), os.path.join(CSRC, "pm_plan.cpp"),
                    "-o", exe], check=True, timeout=300)

    def go(cases):
        lines = ["plan %d %s  %d %s" % (c["mark"], " ".join(str(c[k]) for k in ARGS), c["cap"], " ".join(map(str, REGS)))
                 for c in cases]
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out = []
        for line in r.stdout.splitlines():
            head, _, tail = line.partition("|")
            words = head.split()
            assert words[0] == "plan" and len(words) == 1 + len(FIELDS), line
            out.append((dict(zip(FIELDS, map(int, words[1:]))), [tuple(int(v) for v in q.split(":")) for q in tail.split()]))
        assert len(out) == len(cases)
        return out
    return go


def case(mark, mode, wide, cap, trace_hold=1, mpc=4, aligned=1, trace_pool=1):
    blob = 4100 if mode in (ref.MODE_LDS, ref.MODE_BRUTE) else 0
    return dict(mark=mark, paths=10000, mpc=mpc, aligned=aligned, mode=mode, wide=wide, depth=24, blob=blob, pool_stack=31,
                trace_pool=trace_pool, trace_hold=trace_hold, cus=8, cap=cap)


def test_marking_plans_per_deposit_stores(run):
    """Under TraceShape::mark the plan is the plan of PM_TRACE_HOLD=0 — hold and hold_launch 0, no HOLD kernel's
    occupancy asked, the same family, grid, LDS bytes, pool and spill — in every traversal mode, with either wide
    tree, pooled or per lane; and without the mark nothing moves (the unmarked plan of the same shape still holds
    its deposits where the LDS is roomy)."""
    modes = (ref.MODE_GLOBAL, ref.MODE_LDS, ref.MODE_BRUTE, ref.MODE_INST)
    shapes = list(itertools.product(modes, (0, 2, 3), (LDS_CU, ROOMY), (0, 1), (0, 1)))
    marked = run([case(1, m, w, cap, th, trace_pool=tp) for m, w, cap, th, tp in shapes])
    plain = run([case(0, m, w, cap, th, trace_pool=tp) for m, w, cap, th, tp in shapes])
    held_somewhere = False
    for (m, w, cap, th, tp), (got, asked), (unmarked, asked_u) in zip(shapes, marked, plain):
        c = case(1, m, w, cap, th, trace_pool=tp)
        want, want_asked = ref.plan(ask=ref.table(cap, REGS), **{**{k: c[k] for k in ARGS}, "trace_hold": 0})
        assert got == want and asked == want_asked, (c, got, want)
        assert got["hold"] == 0 and got["hold_launch"] == 0 and all(h == 0 for _, h, _ in asked), (c, got, asked)
        want_u, asked_want_u = ref.plan(ask=ref.table(cap, REGS), **{k: c[k] for k in ARGS})
        assert unmarked == want_u and asked_u == asked_want_u, c
        held_somewhere |= bool(unmarked["hold_launch"])
        # the launch itself is the unmarked one's but for the held columns
        for k in ("family", "pooled", "lstk", "grid", "lds", "spill_entries"):
            if not (k in ("grid",) and unmarked["pooled"] and unmarked["hold"]):  # a held pooled round may count other waves
                assert got[k] == unmarked[k], (c, k, got, unmarked)
    assert held_somewhere, "no unmarked case holds its deposits: the comparison shows nothing"
