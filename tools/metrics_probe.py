#!/usr/bin/env python
"""Time of the two open-loop metrics launches (adx_traj_metrics + adx_metrics_accumulate) beside the sampling tick they follow.

    python tools/metrics_probe.py [--json out.json]

At (S, K) = (1, 8) and (64, 32): one OpenLoopMetrics.update on the tick's K * S candidates against S logged rows, and the tick
itself (a GraphedSampler replay: 10-step DDIM, classifier-free guidance, 256x900 frames, H = 16), both between HIP events on the
stream after a warm-up of every shape.  A recorded measurement (profiles/README.md, "Open-loop metrics"), not a threshold: the
launches are outside the driving tick.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCHED_KW = dict(num_train_timesteps=100, prediction_type="sample", beta_schedule="squaredcos_cap_v2", beta_start=1e-4, beta_end=0.02)


def timed(fn, warmup: int, iters: int) -> float:
    """Mean milliseconds of `fn` over `iters` calls between two events, after `warmup` calls."""
    import torch
    for _ in range(warmup):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args(argv)
    import torch
    from autonomous_driving_with_diffusion_model_amd import DeviceNoise, OpenLoopMetrics, TrajectorySelector
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    from autonomous_driving_with_diffusion_model_amd.modeling import build_model
    from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler
    from autonomous_driving_with_diffusion_model_amd.utils import procedural as P
    dev = "cuda:0"
    cfg = create_cfg()
    cfg.MODEL.HORIZON = 16
    cfg.TRAIN.USE_COND = cfg.GUIDANCE.USE_COND = "FREE_GUIDANCE"
    cfg.GUIDANCE.FREE_SCALE, cfg.EVAL.SAMPLE_STEPS = 7.5, args.steps
    model = build_model(cfg)
    P.load_procedural(model, 0)
    model = model.to(dev).eval()
    rows = []
    for scenes, K in ((1, 8), (64, 32)):
        sch = S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
        d = {k: v.to(dev) for k, v in P.synthetic_batch(scenes, 16, image_hw=(256, 900), seed=1).items()}
        sampler = GraphedSampler(model, sch, cfg, scale_xy=False, noise=DeviceNoise(3, dev), candidates=K,
                                 selector=TrajectorySelector(1.0, 0.5, 0.25))
        tick = lambda: sampler(d["imgs"], d["target"])      # noqa: E731
        tick_ms = timed(tick, 2, 5 if scenes > 1 else 50)
        cands, sel = sampler.last_candidates, sampler.last_selection
        gt = d["init_trajs"][:scenes, :, :2].clamp(-1, 1).contiguous()
        metrics = OpenLoopMetrics(xy_scale=float(model.magic_num))
        update = lambda: metrics.update(cands, gt, index=sel.index)      # noqa: E731
        both_ms = timed(update, 20, 500)
        rows.append({"scenes": scenes, "candidates": K, "horizon": 16, "ddim_steps": args.steps, "tick_ms": round(tick_ms, 3),
                     "metrics_two_launches_us": round(both_ms * 1e3, 2), "share_of_tick": round(both_ms / tick_ms, 5)})
        print(json.dumps(rows[-1]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
