"""Wall time of the B = 64 training step (H = 32, 3x256x900, bench.py's sizes) under three fine-tuning settings of the camera
encoder, each in a process of its own:
  default  -- model.train(): every BatchNorm on batch statistics, every parameter trained;
  eval     -- model.train(); model.perception.eval(): every BatchNorm on its running statistics;
  recipe   -- as eval, and the stem + layer1 with requires_grad=False (the backward stops at layer2).
usage: python tools/finetune_time.py [default|eval|recipe ...]   (no argument: all three)"""
import contextlib
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(mode, steps=8, warm=3):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    from autonomous_driving_with_diffusion_model_amd.modeling import build_model
    from autonomous_driving_with_diffusion_model_amd.optim import FusedAdamWEMA
    from autonomous_driving_with_diffusion_model_amd.utils import procedural as P
    dev = torch.device("cuda:0")
    cfg = create_cfg()
    cfg.MODEL.HORIZON = bench.H
    with contextlib.redirect_stdout(sys.stderr):
        model = build_model(cfg)
    P.load_procedural(model, 0)
    model = model.to(dev).train()
    if mode in ("eval", "recipe"):
        model.perception.eval()
    if mode == "recipe":
        for k, p in model.perception.named_parameters():
            p.requires_grad_(not k.startswith(("conv1.", "bn1.", "layer1.")))
    opt = FusedAdamWEMA(model.parameters(), lr=1e-4, warmup_steps=1000)
    sch = S.DDPMScheduler(**bench.SCHED_KW)
    d = {k: v.to(dev) for k, v in P.synthetic_batch(bench.B, bench.H, image_hw=bench.IMG, seed=7).items()}

    def step():
        noisy = sch.add_noise(d["trajs"], d["noise"], d["t"], zero_first=True)
        loss = torch.nn.functional.mse_loss(model(noisy, d["imgs"], d["t"]), d["trajs"])
        loss.backward()
        opt.step()
        opt.zero_grad()
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    print(f"{mode}: {1e3 * (time.perf_counter() - t0) / steps:.2f} ms per step ({steps} steps, B = {bench.B})", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1].startswith("--one="):
        run(sys.argv[1][6:])
        sys.exit(0)
    for mode in sys.argv[1:] or ["default", "eval", "recipe"]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), f"--one={mode}"], capture_output=True, text=True)
        print(r.stdout.strip() if r.returncode == 0 else f"{mode}: failed ({r.returncode}) {r.stderr[-500:]}", flush=True)
        if r.returncode != 0:
            sys.exit(r.returncode)
