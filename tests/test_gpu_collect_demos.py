"""GPU: tools/collect_demos.py run as a caller runs it -- `main()` on a small rig (2 scenes, 40 ticks of 0.1 s, stride 2, 64 x 96
frames) -- writes a dataset `TrajDataset` reads back, and what it reads back is what the tool's own drive recorded: the same rig
driven again with the same seed gives the frames byte for byte and `waypoints` and `target` bit for bit."""
import os
import sys

import pytest
import torch

from autonomous_driving_with_diffusion_model_amd.dataset.carla_dataset import TrajDataset

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import collect_demos  # noqa: E402

pytestmark = pytest.mark.gpu
S, TICKS, STRIDE, H, HW = 2, 40, 2, 16, (64, 96)


def test_the_tool_runs_and_trajdataset_reads_back_what_it_wrote(tmp_path, capsys):
    out = str(tmp_path / "demos")
    assert collect_demos.main(["--out", out, "--scenes", str(S), "--ticks", str(TICKS), "--stride", str(STRIDE), "--width", str(HW[1]),
                               "--height", str(HW[0]), "--seed", "3"]) == 0
    n = (TICKS - H * STRIDE) * S                                              # t + 32 <= 39: t in 0..7, nothing ends within 4 s
    assert f"{n} samples of {TICKS} ticks x {S} scenes" in capsys.readouterr().out
    ds = TrajDataset(out, horizon=H)
    assert len(ds) == n and sorted(os.listdir(os.path.join(out, "waypoints"))) == [f"{i:06d}.txt" for i in range(n)]
    demo, report, expert = collect_demos.collect(S, TICKS, STRIDE, HW[1], HW[0], seed=3)      # the same drive again
    assert report["ticks"].tolist() == [TICKS] * S and report["events"].tolist() == [0] * S and report["signals"]["red_runs"].tolist() == [0] * S
    index, wps, target = demo.labels()
    assert index.tolist() == [[t, s] for t in range(TICKS - H * STRIDE) for s in range(S)]
    frames = demo.frames_log[index[:, 0], index[:, 1]].cpu()
    moved = False
    for i in range(n):
        img, w, t = ds[i]
        assert img.dtype == torch.uint8 and tuple(img.shape) == (*HW, 3) and torch.equal(img, frames[i]), i
        assert tuple(w.shape) == (H, 7) and torch.equal(w.view(torch.int32), wps[i].cpu().view(torch.int32)), i
        assert torch.equal(t.view(torch.int32), target[i].cpu().view(torch.int32)), i
        moved |= bool((w[:, 1] > 0).any())
    assert moved                                                              # the expert drove: later rows lie ahead of the first
