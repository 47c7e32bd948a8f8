"""bench.py --gpus N started without a launcher re-runs itself under torch.distributed.run (CPU check of the command;
the GPU suite runs it for real: tests/test_gpu_bench_launch.py)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_spawn_command_is_the_drivers_launch_line(monkeypatch):
    import bench
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 0

    monkeypatch.setattr(subprocess, "call", fake_call)
    assert bench.spawn_ranks(4, ["--gpus", "4", "--steps", "7", "--warmup", "3"]) == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and 1024 <= int(cmd[cmd.index("--master-port") + 1]) < 65536
    k = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[k + 1:] == ["--gpus", "4", "--steps", "7", "--warmup", "3"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_gpus_above_one_without_world_size_takes_the_spawn_path(monkeypatch):
    import bench
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "5"])
    monkeypatch.setattr(bench, "spawn_ranks", lambda n, argv=None: 17 + n)
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 19
    else:
        raise AssertionError("main() should have exited with the launcher's code")


def test_dump_outputs_writes_finite_float64_arrays_and_samples_large_batches_the_same_way(tmp_path, monkeypatch):
    import numpy as np
    import bench
    x = np.linspace(-5.0, 5.0, 1000)
    x[::7] = np.nan
    x[3::11] = -np.inf
    x[5::13] = np.inf
    bench.dump_outputs(str(tmp_path / "a"), x)
    got, kind = (np.load(tmp_path / "a" / f) for f in ("lnpost.npy", "lnpost_nonfinite.npy"))
    assert got.dtype == kind.dtype == np.float64 and np.isfinite(got).all() and np.isfinite(kind).all()
    assert kind.shape == x.shape and np.array_equal(got, x[np.isfinite(x)])
    assert np.array_equal(kind == -1, np.isneginf(x)) and np.array_equal(kind == 1, np.isposinf(x))
    assert np.array_equal(kind == 2, np.isnan(x)) and np.array_equal(kind == 0, np.isfinite(x))
    # above the size cap: a fixed seeded subset of the rows, in row order, within the cap
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8192 + 16 * 100)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), x)
    for f in ("lnpost.npy", "lnpost_nonfinite.npy"):
        assert np.array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "c" / f))
    b, kb = (np.load(tmp_path / "b" / f) for f in ("lnpost.npy", "lnpost_nonfinite.npy"))
    assert kb.size == 100 and b.size == int((kb == 0).sum())
    assert np.all(np.diff(b) > 0) and np.isin(b, x).all()
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in ("lnpost.npy", "lnpost_nonfinite.npy")) <= bench.DUMP_MAX_BYTES


def test_steps_below_one_is_an_error(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 2
    else:
        raise AssertionError("--steps 0 should be refused")
