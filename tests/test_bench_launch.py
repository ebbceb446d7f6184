"""bench.py's N-GPU launch (host only): `python bench.py --gpus N` without a
torch.distributed environment starts N ranks under torch.distributed.run as a
child process (127.0.0.1 rendezvous), before anything touches the GPU. Also
the host side of the plain / --full split and of --dump-outputs."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_n_launches_torchrun_child(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 0

    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    try:
        bench.main()
        code = None
    except SystemExit as e:
        code = e.code
    assert code == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "127.0.0.1" in cmd
    assert cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (3, 1)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_writes_bounded_float_arrays_with_a_fixed_sample(tmp_path):
    """--dump-outputs: float32 / float64 .npy files within the 64 MB budget; a
    large array keeps the same ascending sample of its rows on every call."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    big = torch.arange(40_000, dtype=torch.float32).reshape(-1, 1).expand(-1, 1536).contiguous()  # 245 MB
    arrays = {"big": big, "half": torch.ones(5, 8, dtype=torch.float16), "idx": np.arange(7, dtype=np.int32),
              "wide": torch.full((3,), 0.1, dtype=torch.float64), "scalar": np.float32(2.5)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {f[:-4]: np.load(str(tmp_path / "a" / f)) for f in sorted(os.listdir(str(tmp_path / "a")))}
    assert sorted(got) == sorted(arrays)
    assert sum(v.nbytes for v in got.values()) <= 64 * 1000 * 1000
    assert {k: str(v.dtype) for k, v in got.items()} == {
        "big": "float32", "half": "float32", "idx": "float64", "wide": "float64", "scalar": "float32"}
    rows = got["big"][:, 0]
    assert got["big"].shape[1:] == (1536,) and 1000 < len(rows) < 40_000
    assert (np.diff(rows) > 0).all() and (got["big"] == rows[:, None]).all()  # whole rows of the source, in order
    np.testing.assert_array_equal(got["big"], np.load(str(tmp_path / "b" / "big.npy")))
    np.testing.assert_array_equal(got["idx"], np.arange(7))
    assert got["wide"][0] == 0.1 and got["scalar"].tolist() == [2.5]
