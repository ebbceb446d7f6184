"""bench.py's headline (config 5) end to end on the device at a small size
(10,240 clips per step: 80 augmentation batches, 102 train steps = two 50-step
graphs + a 2-step tail; no evaluation passes): what a plain run does and leaves
out, what --full adds, and what --dump-outputs writes (the embedding pool and
the 8-step train probe), twice, so that the dump's repeatability is checked.

The sequential stage-timing steps are seen through the profiling markers that
bracket them (tags 3 -> 4; the timed region is 1 -> 2)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIPS = 10_240
TRAIN_STEPS = CLIPS // 2 // 50
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--clips", str(CLIPS), "--validation-steps", "0",
         "--other-configs", "1"]


def _bench(monkeypatch, capsys, extra):
    """bench.main() with SMALL + extra: its JSON line and the marker tags it launched."""
    sys.path.insert(0, ROOT)
    import bench
    tags = []
    real = bench.prof_mark

    def spy(tag, dev):
        tags.append(tag)
        real(tag, dev)

    monkeypatch.setattr(bench, "prof_mark", spy)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", *SMALL, *extra])
    capsys.readouterr()
    bench.main()
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1  # ONE JSON line
    return json.loads(lines[0]), tags


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_one(monkeypatch, capsys, tmp_path):
    dumps = []
    for d in ("a", "b"):
        line, tags = _bench(monkeypatch, capsys, ["--dump-outputs", str(tmp_path / d)])
        # only the timed region: no stage steps, rooflines, CPU baseline or other configs
        assert tags == [1, 2]
        assert line["full"] is False and line["roofline"] is None and line["roofline_other"] == []
        assert line["cpu_baseline"] is None and "configs_other" not in line and "cli_path" not in line
        assert (line["steps"], line["warmup"], line["n_gpus"]) == (2, 1, 1)
        assert line["unit"] == "clips/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["config"]["clips_per_rank"] == CLIPS and line["config"]["train_steps_per_rank"] == TRAIN_STEPS
        # value = clips per step / the time of one step (both rounded in the line)
        assert line["ms_per_step"] > 0
        assert abs(line["value"] * line["ms_per_step"] * 1e-3 - CLIPS) <= 2e-3 * CLIPS
        dumps.append({f[:-4]: np.load(str(tmp_path / d / f)) for f in sorted(os.listdir(str(tmp_path / d)))})
    a, b = dumps
    assert sorted(a) == ["embeddings", "train_probe_history", "train_probe_parameters"]
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    rows = 60 * 2 ** 20 // 3 // (16 * 96 * 4)  # the embeddings' share of the budget, in rows
    assert a["embeddings"].shape == (min(CLIPS, rows), 16, 96) and np.abs(a["embeddings"]).max() > 0
    # seeded: the same arguments give the same inputs, and the featurization is the same bits
    np.testing.assert_array_equal(a["embeddings"], b["embeddings"])
    # the train probe: 8 steps of B = 1,100 (50 positives) from fixed weights; every step fires an update
    h, hb = a["train_probe_history"], b["train_probe_history"]
    assert h.shape == (8, 8) and a["train_probe_parameters"].shape == (256417,)
    assert (h[:, 0] >= 1).all() and (h[:, 0] <= 1100).all() and (h[:, 6] <= 50).all() and (h[:, 3] > 0).all()
    assert h[-1, 3] < h[0, 3]  # the loss falls: the updates are applied
    # Run to run the probe differs only by the order of its float-atomic sums: per step a relative
    # 2^-24 sqrt(1,100) = 2e-6 of the loss, and Adam can move a parameter whose gradient is below its
    # eps = 1e-8 by at most 8 lr = 8e-3, i.e. the loss by 256,417 x 1e-8 x 8e-3 = 2e-5: 1e-4 in all.
    # A count changes only if a sample's loss is within that of the filter's threshold: at most a few rows.
    print("probe run to run: loss max|d| %.3e, counts max|d| %g, parameters max|d| %.3e" % (
        np.abs(h[:, 3] - hb[:, 3]).max(), np.abs(np.delete(h - hb, 3, 1)).max(),
        np.abs(a["train_probe_parameters"] - b["train_probe_parameters"]).max()))
    np.testing.assert_allclose(h[:, 3], hb[:, 3], rtol=0, atol=1e-4)
    assert np.abs(np.delete(h - hb, 3, 1)).max() <= 3


@pytest.mark.gpu
def test_full_run_adds_stage_steps_rooflines_and_other_configs(monkeypatch, capsys):
    line, tags = _bench(monkeypatch, capsys, ["--full", "--no-cpu", "--stage-steps", "1"])
    assert tags == [3, 4, 1, 2]  # the sequential stage steps, then the timed region
    assert line["full"] is True and line["cpu_baseline"] is None  # --no-cpu
    roofs = [line["roofline"]] + line["roofline_other"]
    assert line["roofline"]["ms_per_step"] > 0 and all(0 <= r["frac"] < 1 for r in roofs)
    kernels = " | ".join(r["kernel"] for r in roofs)
    for part in ("augment stage", "mel_frames_v2_kernel", "hbk_embed_clips", "fused train step",
                 "conv_chain_x3_kernel only", "mel_frames_mfma_kernel"):  # the stages and the untimed variants
        assert part in kernels, part
    assert "per-stage ms from 1 sequential steps" in line["config"]["schedule"]
    other = line["configs_other"]  # --other-configs 1: the host mel-only config
    assert len(other) == 1 and other[0]["n_gpus"] == 0 and other[0]["value"] > 0
