#!/usr/bin/env python
"""Open-loop evaluation of sampling variants over a dataset in the reference's format (front/*.png + waypoints/*.txt).

    python tools/open_loop_eval.py DATA_ROOT [--checkpoint CKPT] --variants ddim:50:1:0,dpm:10:8:0,ddim:50:1:10 [--batch 16]
                                   [--modes 6[:2.0]]

A variant is `scheduler:steps:candidates:warm_steps` (scheduler: ddim, ddpm or dpm).  Every variant walks the same frames under
the same DeviceNoise seed and prints one JSON line: ADE / FDE of the chosen plan, minADE_K / minFDE_K, the miss rates, the
selector's regret, the displacement per waypoint (evaluation.py: `evaluate_open_loop`; the numbers are formed on the device by
csrc/metrics.hip and read once per variant).  Without --checkpoint the weights are the procedural ones of the tests: the numbers
then say nothing about driving, only that the path runs.  `--modes M[:radius_m]` adds the multi-modal row to every variant with
more than one candidate: the candidates of a scene are clustered into at most M modes under a radius in metres (default: the miss
radius; control/modes.py) and the line gains `"modes"`: minADE / minFDE over the M modes, the majority-vote plan's ADE / FDE beside
the selector's, modes per scene, the top mode's share, the outlier rate.  The measurement DESIGN.md's "not measured here" sentences point to.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCHED_KW = dict(num_train_timesteps=100, prediction_type="sample", beta_schedule="squaredcos_cap_v2", beta_start=1e-4, beta_end=0.02)


def parse_variant(text: str):
    parts = text.split(":")
    if len(parts) != 4 or parts[0] not in ("ddim", "ddpm", "dpm"):
        raise SystemExit(f"variant {text!r}: expected scheduler:steps:candidates:warm_steps with scheduler ddim, ddpm or dpm")
    return parts[0], int(parts[1]), int(parts[2]), int(parts[3])


def parse_modes(text, miss_radius: float):
    """`M[:radius_m]` -> (M, radius in metres); None stays None."""
    if text is None:
        return None
    parts = text.split(":")
    try:
        if len(parts) not in (1, 2):
            raise ValueError(text)
        return int(parts[0]), float(parts[1]) if len(parts) == 2 else float(miss_radius)
    except ValueError:
        raise SystemExit(f"--modes {text!r}: expected M[:radius_m], e.g. 6 or 6:2.0") from None


def _strict(v):
    """An average over nothing is NaN (waypoint 0 is never scored at h0 = 1): null in the JSON line."""
    if isinstance(v, dict):
        return {k: _strict(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_strict(x) for x in v]
    return None if isinstance(v, float) and v != v else v


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("root", help="dataset root (front/*.png, waypoints/%%06d.txt)")
    ap.add_argument("--checkpoint", default=None, help="a checkpoint in the reference's format (default: procedural weights)")
    ap.add_argument("--variants", default="ddim:50:1:0", help="comma-separated scheduler:steps:candidates:warm_steps")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--max-batches", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0, help="the DeviceNoise seed every variant starts from")
    ap.add_argument("--cond", default="FREE_GUIDANCE", choices=("NO_GUIDANCE", "FREE_GUIDANCE", "CLASSIFIER_GUIDANCE"))
    ap.add_argument("--select", default="1,0,0", help="w_goal,w_smooth,w_consensus of the selector at candidates > 1")
    ap.add_argument("--horizon", type=int, default=None, help="MODEL.HORIZON = waypoint rows per sample (default: the config's)")
    ap.add_argument("--miss-radius", type=float, default=2.0, help="metres")
    ap.add_argument("--modes", default=None, metavar="M[:radius_m]",
                    help="cluster the candidates of every variant with candidates > 1 into at most M modes (radius in metres; "
                         "default: the miss radius)")
    ap.add_argument("--graphed", action="store_true", help="run every tick as a GraphedSampler replay")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    variants = [parse_variant(v) for v in args.variants.split(",") if v]
    mode_args = parse_modes(args.modes, args.miss_radius)

    import torch
    from autonomous_driving_with_diffusion_model_amd import DeviceNoise, OpenLoopMetrics, TrajectoryModes, TrajectorySelector, WarmStart
    from autonomous_driving_with_diffusion_model_amd import evaluate_open_loop
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    from autonomous_driving_with_diffusion_model_amd.checkpoint import load_checkpoint
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    from autonomous_driving_with_diffusion_model_amd.dataset import get_loader
    from autonomous_driving_with_diffusion_model_amd.modeling import build_model
    from autonomous_driving_with_diffusion_model_amd.utils import procedural as P

    cfg = create_cfg()
    cfg.TRAIN.USE_COND = cfg.GUIDANCE.USE_COND = args.cond
    if args.horizon is not None:
        cfg.MODEL.HORIZON = args.horizon
    cfg.TRAIN.ROOT, cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.NUM_WORKERS = args.root, args.batch, 0
    if args.cond == "CLASSIFIER_GUIDANCE":
        cfg.GUIDANCE.LOSS_LIST = [["TargetGuidance", []]]
    model = build_model(cfg)
    if args.checkpoint:
        load_checkpoint(args.checkpoint, model)
    else:
        P.load_procedural(model, 0)
    model = model.to(args.device).eval()
    selector = TrajectorySelector(*(float(v) for v in args.select.split(",")))
    for name, steps, K, warm_steps in variants:
        cfg.EVAL.SAMPLE_STEPS = steps
        sch = {"ddim": lambda: S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW),
               "ddpm": lambda: S.GuidanceDDPMScheduler(cfg=cfg, **SCHED_KW),
               "dpm": lambda: S.GuidanceDPMSolverMultistepScheduler(cfg=cfg, thresholding=True, lambda_min_clipped=-5.1, **SCHED_KW)}[name]()
        metrics = OpenLoopMetrics(miss_radius=args.miss_radius, xy_scale=float(model.magic_num))
        # the radius in model units; a variant with one candidate per scene has nothing to cluster
        modes = TrajectoryModes(mode_args[0], mode_args[1] / float(model.magic_num), metrics.h0) if mode_args and K > 1 else None
        t0 = time.perf_counter()
        out = evaluate_open_loop(model, sch, cfg, get_loader(cfg, train=False), candidates=K, selector=selector if K > 1 else None,
                                 noise=DeviceNoise(args.seed, args.device), warm=WarmStart(steps=warm_steps) if warm_steps > 0 else None,
                                 graphed=args.graphed, max_batches=args.max_batches, metrics=metrics, modes=modes)
        torch.cuda.synchronize()
        out.update(variant={"scheduler": name, "steps": steps, "candidates": K, "warm_steps": warm_steps, "graphed": args.graphed},
                   weights=args.checkpoint or "procedural", seconds=round(time.perf_counter() - t0, 3))
        print(json.dumps(_strict(out)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
