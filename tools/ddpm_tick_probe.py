"""What does a stochastic (DDPM) driving tick cost, with the noise drawn by torch.randn, drawn inside the step kernel, and as one
HIP graph?  One scene, H = 16, full-size camera frame, perception pass inside the tick:

    NO_GUIDANCE at EVAL.SAMPLE_STEPS = 100 (the config default) and FREE_GUIDANCE at the 10 steps of free_guidance.yaml
    (a) eager DDPM loop, torch.randn per step and for the initial trajectory (the only DDPM path before DeviceNoise)
    (b) eager DDPM loop with DeviceNoise (no noise tensor: the step kernel draws)
    (c) GraphedSampler on the DDPM scheduler with DeviceNoise (begin_tick + initial draw + steps in the graph)
    (d) GraphedSampler on the DDIM scheduler at the same step count (the deterministic product path)

The four alternate on one box in one process, `--rounds` times, each timed with device events around >= `--seconds` of ticks.
Prints a table and one JSON line; `--json PATH` also writes the record.  `--only c --ticks N` runs N ticks of one variant and
nothing else (for a kernel trace in a run of its own).

    python tools/ddpm_tick_probe.py --json profiles/ddpm_tick_probe.json
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autonomous_driving_with_diffusion_model_amd import DeviceNoise  # noqa: E402
from autonomous_driving_with_diffusion_model_amd import scheduler as S  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.config import create_cfg  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.modeling import build_model  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler, generate_traj  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.utils import procedural as P  # noqa: E402

SCHED_KW = dict(num_train_timesteps=100, prediction_type="sample", beta_schedule="squaredcos_cap_v2", beta_start=1e-4, beta_end=0.02)
IMG = (256, 900)
LEGS = (("NO_GUIDANCE", 100), ("FREE_GUIDANCE", 10))
NAMES = {"a": "eager DDPM, torch.randn", "b": "eager DDPM, DeviceNoise", "c": "graphed DDPM, DeviceNoise", "d": "graphed DDIM"}


def variants(use_cond, steps, dev):
    cfg = create_cfg()
    cfg.MODEL.HORIZON = 16
    cfg.TRAIN.USE_COND = cfg.GUIDANCE.USE_COND = use_cond
    cfg.GUIDANCE.FREE_SCALE, cfg.EVAL.SAMPLE_STEPS = 7.5, steps
    with contextlib.redirect_stdout(sys.stderr):
        model = build_model(cfg)
    P.load_procedural(model, 0)
    model = model.to(dev).eval()
    d = {k: v.to(dev) for k, v in P.synthetic_batch(1, 16, image_hw=IMG, seed=3).items()}
    img, tgt = d["imgs"], (None if use_cond == "NO_GUIDANCE" else d["target"])
    ddpm = S.GuidanceDDPMScheduler(cfg=cfg, **SCHED_KW)
    ddim = S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
    zb, zc = DeviceNoise(1, dev), DeviceNoise(1, dev)
    gc, gd = GraphedSampler(model, ddpm, cfg, noise=zc), GraphedSampler(model, ddim, cfg)
    # the eager loops get a fresh frame tensor per tick, as a camera delivers one (the perception pass runs every tick, as it
    # does inside the graphs)
    return {"a": lambda: generate_traj(model, ddpm, cfg, img.clone(), tgt),
            "b": lambda: generate_traj(model, ddpm, cfg, img.clone(), tgt, noise=zb),
            "c": lambda: gc(img, tgt),
            "d": lambda: gd(img, tgt)}


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
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default=None, choices=sorted(NAMES))
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--leg", type=int, default=None, help="index into LEGS (default: all)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    legs = LEGS if a.leg is None else (LEGS[a.leg],)
    record = {"device": torch.cuda.get_device_name(0), "image": list(IMG), "horizon": 16, "scenes": 1, "rounds": a.rounds,
              "seconds_per_window": a.seconds, "legs": []}
    with torch.no_grad():
        for use_cond, steps in legs:
            fns = variants(use_cond, steps, dev)
            if a.only:
                for _ in range(3):
                    fns[a.only]()
                torch.cuda.synchronize()
                print(f"{use_cond} {steps} steps, ({a.only}) {NAMES[a.only]}: {timed(fns[a.only], a.ticks):.3f} ms/tick over {a.ticks} ticks")
                continue
            ticks = {}
            for k, fn in fns.items():               # warm every variant (captures included), then size the windows
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                ticks[k] = max(3, int(a.seconds * 1e3 / timed(fn, 5)) + 1)
            ms = {k: [] for k in fns}
            for _ in range(a.rounds):
                for k, fn in fns.items():
                    ms[k].append(timed(fn, ticks[k]))
            leg = {"use_cond": use_cond, "steps": steps, "variants": {}}
            for k in fns:
                med = statistics.median(ms[k])
                leg["variants"][k] = {"what": NAMES[k], "ticks_per_window": ticks[k], "ms_per_tick": [round(v, 4) for v in ms[k]],
                                      "median_ms": round(med, 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4),
                                      "median_us_per_step": round(med * 1e3 / steps, 2)}
            va, vc, vd = (leg["variants"][k] for k in "acd")
            leg["a_spread_ms"] = round(va["max_ms"] - va["min_ms"], 4)
            leg["c_not_slower_than_a_beyond_a_spread"] = vc["median_ms"] <= va["median_ms"] + leg["a_spread_ms"]
            leg["c_over_d_per_step"] = round(vc["median_ms"] / vd["median_ms"], 4)
            record["legs"].append(leg)
            print(f"\n{use_cond}, {steps} steps, one scene, H = 16, {IMG[0]}x{IMG[1]} frame ({a.rounds} alternating rounds)")
            print(f"{'variant':<32}{'median ms':>10}{'min':>9}{'max':>9}{'us/step':>9}")
            for k in fns:
                v = leg["variants"][k]
                print(f"({k}) {v['what']:<28}{v['median_ms']:>10.3f}{v['min_ms']:>9.3f}{v['max_ms']:>9.3f}{v['median_us_per_step']:>9.1f}")
            print(f"(c) <= (a) + spread of (a) [{leg['a_spread_ms']:.3f} ms]: {leg['c_not_slower_than_a_beyond_a_spread']};  "
                  f"(c) / (d) = {leg['c_over_d_per_step']:.4f}")
    if not a.only:
        print(json.dumps(record))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(record, f, indent=1)
                f.write("\n")
        if not all(leg["c_not_slower_than_a_beyond_a_spread"] for leg in record["legs"]):
            sys.exit("the graphed DDPM tick is slower than the eager torch.randn tick beyond the latter's own spread")


if __name__ == "__main__":
    main()
