#!/usr/bin/env python
"""Time of the manoeuvre-commitment launch (adx_traj_commit) and of the sampling tick with and without it as a graph node.

    python tools/commit_probe.py [--json out.json]

At (S, K) = (1, 8) and (64, 32): the tick (a GraphedSampler replay: 10-step DDIM, classifier-free guidance, 256x900 frames,
H = 16) without and with `commit=ManoeuvreCommit(...)`, interleaved in rounds so that both see the same clocks, and one launch of
`ManoeuvreCommit` alone on the tick's K * S candidates and the selector's outputs (its state valid: the second and later
launches) -- all between HIP events on the stream after a warm-up of every shape.  A recorded measurement (profiles/README.md,
"Manoeuvre commitment"), not a threshold: no test asserts a time.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from metrics_probe import SCHED_KW, timed      # noqa: E402  (tools/ is the script's directory)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds of (tick without, tick with); the median is kept")
    args = ap.parse_args(argv)
    import torch
    from autonomous_driving_with_diffusion_model_amd import DeviceNoise, ManoeuvreCommit, Selection, TrajectorySelector
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
        d = {k: v.to(dev) for k, v in P.synthetic_batch(scenes, 16, image_hw=(256, 900), seed=1).items()}
        motion = torch.zeros(scenes, 3, device=dev)
        samplers = {}
        for name, commit in (("without", None), ("with", ManoeuvreCommit(scenes, 16, dev))):
            sch = S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
            samplers[name] = GraphedSampler(model, sch, cfg, scale_xy=False, noise=DeviceNoise(3, dev), candidates=K,
                                            selector=TrajectorySelector(1.0, 0.5, 0.25), commit=commit)
        calls = {"without": lambda: samplers["without"](d["imgs"], d["target"]),
                 "with": lambda: samplers["with"](d["imgs"], d["target"], motion=motion)}
        iters = 5 if scenes > 1 else 50
        ms = {"without": [], "with": []}
        for r in range(args.rounds):
            for name in ("without", "with") if r % 2 == 0 else ("with", "without"):
                ms[name].append(timed(calls[name], 2, iters))
        sampler = samplers["with"]
        cands, sel = sampler.last_candidates, sampler.last_selection
        alone = ManoeuvreCommit(scenes, 16, dev)
        selection = Selection(None, sampler.commit.selected.clone(), sel.cost)
        node_ms = timed(lambda: alone(cands, scenes, selection, motion), 20, 500)
        status = sampler.last_commit.status
        base, withn = statistics.median(ms["without"]), statistics.median(ms["with"])
        rows.append({"scenes": scenes, "candidates": K, "horizon": 16, "ddim_steps": args.steps,
                     "tick_ms": round(base, 3), "tick_with_commit_ms": round(withn, 3),
                     "tick_ms_rounds": [round(v, 3) for v in ms["without"]], "tick_with_commit_ms_rounds": [round(v, 3) for v in ms["with"]],
                     "commit_launch_us": round(node_ms * 1e3, 2), "share_of_tick": round(node_ms / base, 5),
                     "held_share_last_tick": round((status == 3).float().mean().item(), 3)})
        print(json.dumps(rows[-1]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
