"""What does a driving tick cost with the DPM-Solver++ (2M) sampler at 10, 15 and 20 steps, next to DDIM at the same step counts
and at the 50 steps of the deployed configuration?  One scene, H = 16, FREE guidance (scale 7.5), full-size camera frame,
perception pass inside the tick, every arm a GraphedSampler (one HIP graph launch per tick).

    dpm{10,15,20}    GuidanceDPMSolverMultistepScheduler, solver_order = 2, lambda_min_clipped = -5.1
    ddim{10,15,20,50} GuidanceDDIMScheduler (eta = 0)

The arms alternate in one process, `--rounds` times, each window timed with device events around >= `--ticks` ticks (at least
`--seconds` of them).  The comparison that matters is 2M against DDIM AT THE SAME STEP COUNT: the 2M step reads one more
[B, H, D] tensor than the DDIM step and nothing else, so the two ticks should agree within the spread of the arms' own windows.
Prints a table and one JSON line; `--json PATH` also writes the record.  This measures time only: whether a trained model keeps
its driving quality at 10-20 steps is not something the repository can measure (it has no trained weights).

    python tools/dpm_tick_probe.py --json profiles/dpm_tick_probe.json
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autonomous_driving_with_diffusion_model_amd import scheduler as S  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.config import create_cfg  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.modeling import build_model  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.utils import procedural as P  # noqa: E402

SCHED_KW = dict(num_train_timesteps=100, prediction_type="sample", beta_schedule="squaredcos_cap_v2", beta_start=1e-4, beta_end=0.02)
IMG = (256, 900)
ARMS = (("dpm", 10), ("ddim", 10), ("dpm", 15), ("ddim", 15), ("dpm", 20), ("ddim", 20), ("ddim", 50))


def make_cfg(steps):
    cfg = create_cfg()
    cfg.MODEL.HORIZON = 16
    cfg.TRAIN.USE_COND = cfg.GUIDANCE.USE_COND = "FREE_GUIDANCE"
    cfg.GUIDANCE.FREE_SCALE, cfg.EVAL.SAMPLE_STEPS = 7.5, steps
    return cfg


def arms(dev):
    with contextlib.redirect_stdout(sys.stderr):
        model = build_model(make_cfg(10))
    P.load_procedural(model, 0)
    model = model.to(dev).eval()
    d = {k: v.to(dev) for k, v in P.synthetic_batch(1, 16, image_hw=IMG, seed=3).items()}
    img, tgt, init = d["imgs"], d["target"], d["init_trajs"]
    fns = {}
    for kind, steps in ARMS:
        cfg = make_cfg(steps)
        if kind == "dpm":
            sch = S.GuidanceDPMSolverMultistepScheduler(cfg=cfg, thresholding=True, lambda_min_clipped=-5.1, **SCHED_KW)
        else:
            sch = S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
        gs = GraphedSampler(model, sch, cfg)
        fns[f"{kind}{steps}"] = (lambda gs=gs: gs(img, tgt, init))
    return fns


def timed(fn, ticks):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ticks):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / ticks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=100, help="least number of ticks per window (x rounds = ticks per arm)")
    ap.add_argument("--seconds", type=float, default=0.5, help="least length of a window")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    with torch.no_grad():
        fns = arms(dev)
        ticks = {}
        for fn in fns.values():                 # warm every arm (captures included) ...
            for _ in range(3):
                fn()
        for k, fn in fns.items():               # ... then size the windows, once no arm's capture can move the model's buffers
            fn()                                # (a sampler re-captures by itself when a later arm's warm-up grew a workspace)
            torch.cuda.synchronize()
            ticks[k] = max(a.ticks, int(a.seconds * 1e3 / timed(fn, 5)) + 1)
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ms[k].append(timed(fn, ticks[k]))
    record = {"device": torch.cuda.get_device_name(0), "image": list(IMG), "horizon": 16, "scenes": 1, "guidance": "FREE_GUIDANCE",
              "rounds": a.rounds, "arms": {}, "dpm_over_ddim_same_steps": {}, "dpm_over_ddim50": {}}
    for (kind, steps), k in zip(ARMS, fns):
        med = statistics.median(ms[k])
        record["arms"][k] = {"sampler": kind, "steps": steps, "ticks_per_window": ticks[k], "ticks": ticks[k] * a.rounds,
                             "ms_per_tick": [round(v, 4) for v in ms[k]], "median_ms": round(med, 4),
                             "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4),
                             "spread_pct": round(100 * (max(ms[k]) - min(ms[k])) / med, 2),
                             "median_us_per_step": round(med * 1e3 / steps, 2)}
    for n in (10, 15, 20):
        record["dpm_over_ddim_same_steps"][str(n)] = round(record["arms"][f"dpm{n}"]["median_ms"] / record["arms"][f"ddim{n}"]["median_ms"], 4)
        record["dpm_over_ddim50"][str(n)] = round(record["arms"][f"dpm{n}"]["median_ms"] / record["arms"]["ddim50"]["median_ms"], 4)
    print(f"one scene, H = 16, FREE guidance, {IMG[0]}x{IMG[1]} frame, graph ticks ({a.rounds} alternating rounds)", file=sys.stderr)
    print(f"{'arm':<10}{'median ms':>10}{'min':>9}{'max':>9}{'spread %':>10}{'us/step':>9}{'ticks':>8}", file=sys.stderr)
    for k, v in record["arms"].items():
        print(f"{k:<10}{v['median_ms']:>10.3f}{v['min_ms']:>9.3f}{v['max_ms']:>9.3f}{v['spread_pct']:>10.2f}{v['median_us_per_step']:>9.1f}"
              f"{v['ticks']:>8}", file=sys.stderr)
    print("2M / DDIM at the same step count: " + ", ".join(f"{n}: {r:.4f}" for n, r in record["dpm_over_ddim_same_steps"].items()),
          file=sys.stderr)
    print(json.dumps(record))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
