"""bench.py's N > 1 entry: `python bench.py --gpus N` started as a plain
process launches torch.distributed.run itself (child process, before torch
is imported) and relays rank 0's JSON line; with --full the N > 1 line carries
roofline, cpu_baseline and both exchanges (VERDICT r05 "next" item 1)."""
import io
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    sys.path.insert(0, ROOT)
    import importlib
    import bench
    return importlib.reload(bench)


def test_self_launch_command_and_relay(monkeypatch, capsys):
    bench = _bench_module()
    seen = {}

    class FakeProc:
        def __init__(self, cmd, stdout=None, text=None, env=None):
            seen["cmd"], seen["env"] = cmd, env
            self.stdout = io.StringIO("[Gloo] Rank 0 is connected to 1 peer ranks.\n"
                                      '{"metric": "m", "value": 1.0, "n_gpus": 2}\n'
                                      "{not json\n")

        def wait(self):
            return 0

    monkeypatch.setattr(bench.subprocess, "Popen", FakeProc)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "3"])
    assert bench.self_launch(2) == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=2" in cmd and "127.0.0.1" in cmd
    assert cmd[-4:] == ["--gpus", "2", "--steps", "3"]
    assert seen["env"]["PM_BENCH_LAUNCHED"] == "1"
    out, err = capsys.readouterr()
    assert out.strip().splitlines() == ['{"metric": "m", "value": 1.0, "n_gpus": 2}']   # only the JSON line
    assert "Gloo" in err and "{not json" in err


def test_self_launched_rank_without_world_fails(monkeypatch):
    bench = _bench_module()
    monkeypatch.setenv("PM_BENCH_LAUNCHED", "1")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "WORLD_SIZE" in str(e.value.code)


@pytest.mark.gpu
def test_bench_gpus2_self_launch_one_device():
    """Two ranks on the test box's one GPU over gloo (PM_BENCH_ONE_DEVICE /
    PM_BENCH_BACKEND: rehearsal knobs — the times are not measurements)."""
    env = dict(os.environ, PM_BENCH_ONE_DEVICE="1", PM_BENCH_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "c1",
                        "--steps", "3", "--warmup", "1", "--cpu-threads", "4", "--full"],
                       capture_output=True, text=True, timeout=400, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["value"] > 0
    assert d["roofline"] is not None and d["roofline"]["frac"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["cores"] == 4
    assert d["config"]["exchange"] == "reduce"
    assert d["alt_exchange"]["exchange"] == "allgather" and d["alt_exchange"]["value"] > 0
    assert d["exchange"]["bytes_per_pass"] > 0


def test_dump_outputs_full_and_sampled(tmp_path, monkeypatch):
    """dump_outputs writes float32 arrays whole below the byte budget and, above
    it, one seeded sample of rows shared by every array (record_index.npy)."""
    import numpy as np
    bench = _bench_module()
    n = 1000
    arrays = {"radiance": np.arange(3 * n, dtype=np.float64).reshape(n, 3), "radius2": np.arange(n, dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / "whole"), arrays)
    assert sorted(os.listdir(tmp_path / "whole")) == ["radiance.npy", "radius2.npy"]
    got = np.load(tmp_path / "whole" / "radiance.npy")
    assert got.dtype == np.float32 and np.array_equal(got, arrays["radiance"])
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4800)        # 16 B of arrays + 8 B of index per kept row
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    idx = np.load(tmp_path / "a" / "record_index.npy")
    assert idx.dtype == np.float64 and len(idx) == 200 and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(idx, np.load(tmp_path / "b" / "record_index.npy"))      # the same sample every run
    keep = idx.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "radiance.npy"), arrays["radiance"][keep])
    assert np.array_equal(np.load(tmp_path / "a" / "radius2.npy"), arrays["radius2"][keep])
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 4800 + 3 * 128                                                # payload + three .npy headers


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run prints the headline fields only (nothing that needs runs of
    its own) and --dump-outputs writes the last timed step's arrays."""
    import numpy as np
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c1",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["unit"] == "Mphotons/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - 25_000 / d["ms_per_step"] / 1e3) <= 1e-3 * d["value"]     # paths per step / step time
    assert d["roofline"] is None and d["trace_roofline"] is None and d["stages_ms"] == {}
    assert "cpu_baseline" not in d and "alt_exchange" not in d
    out = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert sorted(out) == ["flux", "photon_count", "radiance", "radius2"]
    n = 256 * 256
    assert all(a.dtype == np.float32 and len(a) >= n for a in out.values())
    assert out["radiance"].shape == out["flux"].shape == (len(out["radius2"]), 3)
    assert np.isfinite(out["radiance"]).all() and out["radiance"].max() > 0
    lit = out["photon_count"] > 0
    assert lit.any() and np.all(out["radius2"][lit] < 4.0) and np.all(out["radius2"] <= 4.0)
