"""The committed scene blob, byte for byte (pm_commit: csrc/pm_scene.cpp's
host assembly and pm_api_scene.cpp's device-build path): scene_info and a sha256 of
every section the binding exposes equal tests/golden/scene_sections.json,
recorded before scene assembly moved out of pm_api.cpp. The scenes are the
smallest that reach each assembly path (id order + triangle pairs, mesh
light, selection table, disks and spheres, LDS binary tree in leaf order,
HBM quantized 4-wide / breadth-first / 8-wide / device-built, two-level
instancing). Sections the binding does not expose are covered by the
bit-exact trace, eye-pass and render tests on the same scenes."""
import hashlib
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_sections.json")
# every build knob pm_commit reads: a case sets the ones it names, the rest are unset
KNOBS = ("PM_BVH_BUILD", "PM_BVH_GPU_MIN", "PM_PLOC_RADIUS", "PM_BVH4_BFS", "PM_BVH8", "PM_COMMIT_TIMES")

with open(GOLDEN) as f:
    CASES = json.load(f)["cases"]


def snapshot(hip_mod, case):
    """scene_info and (sha256, bytes) per section of `case`'s scene, committed in a fresh context."""
    from pmrender import scenes
    ctx = getattr(scenes, case["scene"])(*case["args"]).load_into(hip_mod.Context(0))
    try:
        sections = {}
        for name in sorted(hip_mod.Context.SCENE_SECTIONS):
            raw = ctx.scene_section(name).tobytes()
            sections[name] = {"sha256": hashlib.sha256(raw).hexdigest(), "bytes": len(raw)}
        return {"info": ctx.scene_info(), "sections": sections}
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_committed_scene_equals_recorded_bytes(hip_mod, monkeypatch, case):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    got = snapshot(hip_mod, case)
    assert got["info"] == case["info"]
    assert sorted(got["sections"]) == sorted(case["sections"])
    for name, want in case["sections"].items():
        assert got["sections"][name] == want, name
