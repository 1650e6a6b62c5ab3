"""bench.py host logic that needs no GPU: the launch contract of `--gpus N` and the host description."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_gpus_flag_must_match_world_size():
    """Under a torchrun environment WORLD_SIZE must equal --gpus: a mismatch exits non-zero BEFORE anything touches the GPU."""
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout)
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--gpus 4" in (r.stderr + r.stdout)


def test_gpus_flag_self_launches_ranks(monkeypatch):
    """`python bench.py --gpus 4` outside torchrun spawns `torch.distributed.run --nproc-per-node 4 ... bench.py --gpus 4` as a CHILD
    process (never an exec) and exits with its return code."""
    b = _load_bench()
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7
    monkeypatch.setattr(b.subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        b.main()
    assert e.value.code == 7
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_host_cpu_reports_physical_cores_and_model():
    b = _load_bench()
    cores, model = b.host_cpu()
    assert 1 <= cores <= (os.cpu_count() or 1) and isinstance(model, str) and model


def test_full_is_off_by_default_and_implied_by_full_only_options(monkeypatch):
    """A plain run measures only its headline figure; the options whose output lives in the --full part switch it on."""
    b = _load_bench()
    for argv, full in ((["--gpus", "1", "--steps", "3", "--warmup", "1"], False), (["--full"], True),
                       (["--workload", "sam2l", "--full-cpu-baseline"], True), (["--workload", "pipeline", "--scaling-proxy", "8"], True)):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        assert b.parse().full is full, argv


def test_dump_outputs_fits_the_budget_and_repeats(tmp_path, monkeypatch):
    """--dump-outputs: float32 .npy per stage output, small arrays whole, large ones a seeded sample; the total stays within the budget
    and two dumps of the same outputs are identical."""
    import numpy as np
    import torch
    b = _load_bench()
    monkeypatch.setattr(b, "DUMP_BUDGET_BYTES", 1 << 20)

    class Stage:
        def __init__(self, seed):
            g = torch.Generator().manual_seed(seed)
            self.outs = {"det": torch.randn(4, 300, 6, generator=g), "det_count": torch.arange(4),
                         "high_res": torch.randn(2, 1, 1024, 1024, generator=g)}

        def outputs(self):
            return self.outs

    stages = [("yolo11n", Stage(0)), ("sam2l[0]", Stage(1)), ("sam2l[1]", Stage(2))]
    b.dump_outputs(stages, str(tmp_path / "a"))
    b.dump_outputs(stages, str(tmp_path / "b"))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(f"{s}_{k}.npy" for s in ("yolo11n", "sam2l_0", "sam2l_1") for k in ("det", "det_count", "high_res"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 1 << 20
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float32 and np.array_equal(x, y)
    det = np.load(tmp_path / "a" / "sam2l_0_det.npy")
    assert det.shape == (4, 300, 6) and np.array_equal(det, stages[1][1].outs["det"].numpy())
    hi = np.load(tmp_path / "a" / "sam2l_1_high_res.npy")
    assert hi.ndim == 1 and 0 < hi.size < 2 * 1024 * 1024 and np.isin(hi, stages[2][1].outs["high_res"].numpy()).all()
