"""What does pinning waypoints cost a driving tick?  FREE guidance (scale 7.5), full-size camera frame, perception pass inside the
tick, n = `--steps` (20) DDIM sampling steps; every arm a GraphedSampler with a DeviceNoise (one HIP graph launch per tick), at
one scene (H = 16) and at 64 scenes (H = 32):

    none         the tick as it was: no pin
    clean        pin=Pin(known, mask, "clean"): one extra launch at loop entry (adx_pin_apply), the PIN variant of every step
    repaint      pin=Pin(known, mask, "repaint"): the PIN variant of every step, which then also draws from the noise stream

The pin holds (x, y) of waypoints 1..4 (a commit horizon) and changes nothing else; its values travel through the sampler's static
buffers on every tick.  The arms alternate in one process, `--rounds` times, each window timed with device events around
>= `--ticks` ticks (at least `--seconds` of them).  The pinned step reads two more 4-byte values per element of a kernel of a few
hundred to a few tens of thousands of elements, so the expectation is a difference inside the arms' own spread.  Prints a table
and one JSON line; `--json PATH` also writes the record.  This measures time only: what a pin does to a trained model's driving
quality is not something the repository can measure (it has no trained weights).

    python tools/pin_tick_probe.py --json profiles/pin_tick_probe.json
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autonomous_driving_with_diffusion_model_amd import DeviceNoise, Pin  # noqa: E402
from autonomous_driving_with_diffusion_model_amd import scheduler as S  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.config import create_cfg  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.modeling import build_model  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.utils import procedural as P  # noqa: E402

SCHED_KW = dict(num_train_timesteps=100, prediction_type="sample", beta_schedule="squaredcos_cap_v2", beta_start=1e-4, beta_end=0.02)
IMG = (256, 900)
SIZES = ((1, 16), (64, 32))            # (scenes, horizon)
MODES = (None, "clean", "repaint")


def make_cfg(steps, horizon):
    cfg = create_cfg()
    cfg.MODEL.HORIZON = horizon
    cfg.TRAIN.USE_COND = cfg.GUIDANCE.USE_COND = "FREE_GUIDANCE"
    cfg.GUIDANCE.FREE_SCALE, cfg.EVAL.SAMPLE_STEPS = 7.5, steps
    return cfg


def arms(dev, n):
    fns, meta = {}, {}
    for scenes, horizon in SIZES:
        cfg = make_cfg(n, horizon)
        with contextlib.redirect_stdout(sys.stderr):
            model = build_model(cfg)
        P.load_procedural(model, 0)
        model = model.to(dev).eval()
        d = {k: v.to(dev) for k, v in P.synthetic_batch(scenes, horizon, image_hw=IMG, seed=3).items()}
        img, tgt = d["imgs"], d["target"]
        xy = d["trajs"][:, 1:5, :2].contiguous()
        for mode in MODES:
            sch = S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
            gs = GraphedSampler(model, sch, cfg, noise=DeviceNoise(7, dev))
            pin = None if mode is None else Pin.points(horizon, cfg.MODEL.TRANSITION_DIM, [1, 2, 3, 4], xy, mode)
            name = f"s{scenes}.{mode or 'none'}"
            fns[name] = (lambda gs=gs, img=img, tgt=tgt, pin=pin: gs(img, tgt, pin=pin))
            meta[name] = (scenes, horizon, mode or "none")
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
    ap.add_argument("--steps", type=int, default=20, help="n = EVAL.SAMPLE_STEPS")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=50, help="least number of ticks per window (x rounds = ticks per arm)")
    ap.add_argument("--seconds", type=float, default=0.5, help="least length of a window")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.steps
    with torch.no_grad():
        fns, meta = arms(dev, n)
        ticks = {}
        for fn in fns.values():                 # warm every arm: the capture, then replays ...
            for _ in range(3):
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
    record = {"device": torch.cuda.get_device_name(0), "image": list(IMG), "guidance": "FREE_GUIDANCE", "sampler": "ddim",
              "sample_steps": n, "rounds": a.rounds, "pinned": "xy of waypoints 1..4", "arms": {}, "pinned_over_none": {}}
    for k in fns:
        scenes, horizon, mode = meta[k]
        med = statistics.median(ms[k])
        record["arms"][k] = {"scenes": scenes, "horizon": horizon, "pin": mode, "ticks_per_window": ticks[k], "ticks": ticks[k] * a.rounds,
                             "ms_per_tick": [round(v, 4) for v in ms[k]], "median_ms": round(med, 4), "min_ms": round(min(ms[k]), 4),
                             "max_ms": round(max(ms[k]), 4), "spread_pct": round(100 * (max(ms[k]) - min(ms[k])) / med, 2)}
    for k, v in record["arms"].items():
        if v["pin"] != "none":
            record["pinned_over_none"][k] = round(v["median_ms"] / record["arms"][f"s{v['scenes']}.none"]["median_ms"], 4)
    print(f"FREE guidance, DDIM, {IMG[0]}x{IMG[1]} frame, n = {n}, graph ticks ({a.rounds} alternating rounds)", file=sys.stderr)
    print(f"{'arm':<14}{'scenes':>7}{'H':>4}{'median ms':>11}{'min':>9}{'max':>9}{'spread %':>10}{'/ none':>9}{'ticks':>8}", file=sys.stderr)
    for k, v in record["arms"].items():
        r = record["pinned_over_none"].get(k)
        print(f"{k:<14}{v['scenes']:>7}{v['horizon']:>4}{v['median_ms']:>11.3f}{v['min_ms']:>9.3f}{v['max_ms']:>9.3f}"
              f"{v['spread_pct']:>10.2f}{('' if r is None else format(r, '.4f')):>9}{v['ticks']:>8}", file=sys.stderr)
    print(json.dumps(record))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
