"""What does a warm-started driving tick cost?  One scene, H = 16, FREE guidance (scale 7.5), full-size camera frame, perception
pass inside the tick, n = `--steps` (20) sampling steps; every arm a GraphedSampler with a DeviceNoise (one HIP graph launch per
tick), for DDIM and for the DPM-Solver++ (2M) sampler:

    cold         the tick as it was: the initial draw and all n steps
    warm m       GraphedSampler(warm=WarmStart(m)) once its state is valid, m in {n, n/2, n/5}: adx_warm_init, the last m steps,
                 the copy into the static state

The arms alternate in one process, `--rounds` times, each window timed with device events around >= `--ticks` ticks (at least
`--seconds` of them).  A tick is a chain of dependent launches behind one perception pass, so the expectation is
tick(m) ~ perception + m * step; `warm n` against `cold` is what the warm-start node and the state copy cost by themselves.
Prints a table and one JSON line; `--json PATH` also writes the record.  This measures time only: what m steps do to a trained
model's driving quality is not something the repository can measure (it has no trained weights).

    python tools/warm_tick_probe.py --json profiles/warm_tick_probe.json
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autonomous_driving_with_diffusion_model_amd import DeviceNoise, WarmStart  # noqa: E402
from autonomous_driving_with_diffusion_model_amd import scheduler as S  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.config import create_cfg  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.modeling import build_model  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.utils import procedural as P  # noqa: E402

SCHED_KW = dict(num_train_timesteps=100, prediction_type="sample", beta_schedule="squaredcos_cap_v2", beta_start=1e-4, beta_end=0.02)
IMG = (256, 900)


def make_cfg(steps):
    cfg = create_cfg()
    cfg.MODEL.HORIZON = 16
    cfg.TRAIN.USE_COND = cfg.GUIDANCE.USE_COND = "FREE_GUIDANCE"
    cfg.GUIDANCE.FREE_SCALE, cfg.EVAL.SAMPLE_STEPS = 7.5, steps
    return cfg


def arms(dev, n):
    cfg = make_cfg(n)
    with contextlib.redirect_stdout(sys.stderr):
        model = build_model(cfg)
    P.load_procedural(model, 0)
    model = model.to(dev).eval()
    d = {k: v.to(dev) for k, v in P.synthetic_batch(1, 16, image_hw=IMG, seed=3).items()}
    img, tgt = d["imgs"], d["target"]
    motion = torch.tensor([[0.02, 0.0, 0.01]], device=dev)
    fns, meta = {}, {}
    for kind in ("ddim", "dpm"):
        for m in (0, n, n // 2, n // 5):
            if kind == "dpm":
                sch = S.GuidanceDPMSolverMultistepScheduler(cfg=cfg, thresholding=True, lambda_min_clipped=-5.1, **SCHED_KW)
            else:
                sch = S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
            warm = WarmStart(m) if m else None
            gs = GraphedSampler(model, sch, cfg, noise=DeviceNoise(7, dev), warm=warm)
            name = f"{kind}.cold" if m == 0 else f"{kind}.warm{m}"
            fns[name] = (lambda gs=gs, mo=(motion if m else None): gs(img, tgt, motion=mo))
            meta[name] = (kind, m if m else n, bool(m))
    return fns, meta


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
    ap.add_argument("--steps", type=int, default=20, help="n = EVAL.SAMPLE_STEPS (a multiple of 10)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=100, help="least number of ticks per window (x rounds = ticks per arm)")
    ap.add_argument("--seconds", type=float, default=0.5, help="least length of a window")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.steps
    with torch.no_grad():
        fns, meta = arms(dev, n)
        ticks = {}
        for fn in fns.values():                 # warm every arm: the cold capture, then the warm one, then replays ...
            for _ in range(4):
                fn()
        for k, fn in fns.items():               # ... then size the windows, once no arm's capture can move the model's buffers
            fn()                                # (a sampler re-captures by itself when a later arm's warm-up grew a workspace)
            fn()
            torch.cuda.synchronize()
            ticks[k] = max(a.ticks, int(a.seconds * 1e3 / timed(fn, 5)) + 1)
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ms[k].append(timed(fn, ticks[k]))
    record = {"device": torch.cuda.get_device_name(0), "image": list(IMG), "horizon": 16, "scenes": 1, "guidance": "FREE_GUIDANCE",
              "sample_steps": n, "rounds": a.rounds, "arms": {}, "warm_over_cold": {}}
    for k in fns:
        kind, steps, is_warm = meta[k]
        med = statistics.median(ms[k])
        record["arms"][k] = {"sampler": kind, "warm": is_warm, "steps_run": steps, "ticks_per_window": ticks[k],
                             "ticks": ticks[k] * a.rounds, "ms_per_tick": [round(v, 4) for v in ms[k]], "median_ms": round(med, 4),
                             "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4),
                             "spread_pct": round(100 * (max(ms[k]) - min(ms[k])) / med, 2)}
    for k, v in record["arms"].items():
        if v["warm"]:
            record["warm_over_cold"][k] = round(v["median_ms"] / record["arms"][v["sampler"] + ".cold"]["median_ms"], 4)
    print(f"one scene, H = 16, FREE guidance, {IMG[0]}x{IMG[1]} frame, n = {n}, graph ticks ({a.rounds} alternating rounds)", file=sys.stderr)
    print(f"{'arm':<14}{'steps':>6}{'median ms':>11}{'min':>9}{'max':>9}{'spread %':>10}{'/ cold':>9}{'ticks':>8}", file=sys.stderr)
    for k, v in record["arms"].items():
        r = record["warm_over_cold"].get(k)
        print(f"{k:<14}{v['steps_run']:>6}{v['median_ms']:>11.3f}{v['min_ms']:>9.3f}{v['max_ms']:>9.3f}{v['spread_pct']:>10.2f}"
              f"{('' if r is None else format(r, '.4f')):>9}{v['ticks']:>8}", file=sys.stderr)
    print(json.dumps(record))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
