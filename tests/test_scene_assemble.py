"""Scene assembly on the CPU (csrc/pm_scene.cpp: the bytes pm_commit uploads
for the kernels): tests/native/scene_assemble_check.cpp assembles four scenes
and checks the layout, the refs, the storage order and triangle records, the
relocated object trees and the layout planner against the device-build
path's sizes; the blob is the same for 1 and 4 build threads. CPU only:
compiles the checker against pm_scene.cpp and pm_build.cpp. (The bytes
themselves are pinned on the GPU: test_scene_commit_gpu.py.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-raytrace_amd", "csrc")


def test_assembled_scenes_are_consistent_and_thread_independent(tmp_path):
    exe = tmp_path / "scheck"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "scene_assemble_check.cpp"), os.path.join(CSRC, "pm_scene.cpp"),
                    os.path.join(CSRC, "pm_build.cpp"), "-o", str(exe)], check=True, timeout=300)
    outs = []
    for t in ("1", "4"):
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={**os.environ, "PM_BUILD_THREADS": t})
        assert r.returncode == 0, r.stdout + r.stderr
        assert "bad 0" in r.stdout
        outs.append(r.stdout.strip())
    assert outs[0] == outs[1] and outs[0].count("hash") == 4
