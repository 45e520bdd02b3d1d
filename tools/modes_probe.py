#!/usr/bin/env python
"""Time of the trajectory-modes launch (adx_traj_modes) and of the sampling tick with and without it as a graph node.

    python tools/modes_probe.py [--json out.json]

At (S, K) = (1, 8) and (64, 32): the tick (a GraphedSampler replay: 10-step DDIM, classifier-free guidance, 256x900 frames,
H = 16) without and with `modes=TrajectoryModes(6)`, interleaved in rounds so that both see the same clocks, and one launch of
`TrajectoryModes` alone on the tick's K * S candidates -- all between HIP events on the stream after a warm-up of every shape.  A
recorded measurement (profiles/README.md, "Trajectory modes"), not a threshold: no test asserts a time.
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
    ap.add_argument("--max-modes", type=int, default=6)
    args = ap.parse_args(argv)
    import torch
    from autonomous_driving_with_diffusion_model_amd import DeviceNoise, TrajectoryModes, TrajectorySelector
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
        samplers = {}
        for name, modes in (("without", None), ("with", TrajectoryModes(args.max_modes))):
            sch = S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
            samplers[name] = GraphedSampler(model, sch, cfg, scale_xy=False, noise=DeviceNoise(3, dev), candidates=K,
                                            selector=TrajectorySelector(1.0, 0.5, 0.25), modes=modes)
        iters = 5 if scenes > 1 else 50
        ms = {"without": [], "with": []}
        for r in range(args.rounds):
            for name in ("without", "with") if r % 2 == 0 else ("with", "without"):
                sampler = samplers[name]
                ms[name].append(timed(lambda: sampler(d["imgs"], d["target"]), 2, iters))
        cands = samplers["with"].last_candidates
        alone = TrajectoryModes(args.max_modes)
        node_ms = timed(lambda: alone(cands, scenes), 20, 500)
        count = samplers["with"].last_modes.count.float().mean().item()
        base, withn = statistics.median(ms["without"]), statistics.median(ms["with"])
        rows.append({"scenes": scenes, "candidates": K, "horizon": 16, "ddim_steps": args.steps, "max_modes": args.max_modes,
                     "tick_ms": round(base, 3), "tick_with_modes_ms": round(withn, 3),
                     "tick_ms_rounds": [round(v, 3) for v in ms["without"]], "tick_with_modes_ms_rounds": [round(v, 3) for v in ms["with"]],
                     "modes_launch_us": round(node_ms * 1e3, 2), "share_of_tick": round(node_ms / base, 5),
                     "mean_count": round(count, 3)})
        print(json.dumps(rows[-1]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
