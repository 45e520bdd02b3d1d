"""What does cost guidance cost a driving tick?  FREE guidance (scale 7.5), full-size camera frame, perception pass inside the
tick, n = `--steps` (20) DDIM sampling steps; every arm a GraphedSampler with a DeviceNoise (one HIP graph launch per tick), at
one scene (H = 16) and at 64 scenes (H = 32):

    none         the tick as it was: no guide
    m4p2i1       guide=Guide(discs [S, 4, 5], planes [S, 2, 3], iters=1): the GUIDE variant of every step, a light scene
    m32p8i8      guide=Guide(discs [S, 32, 5], planes [S, 8, 3], iters=8): the contract's largest scene, 320 constraint
                 evaluations per xy element and step
    f64i1        guide=Guide(field=CostField([S, 64, 64]), iters=1): "cost guidance v2", a cost raster alone -- four cells read per
                 xy element, iteration and step
    m4p2i1.f256  the m4p2i1 guide with a [S, 256, 256] field beside it (64 scenes: 16 MiB of cells, read where the waypoints are)
    m4p2i8.f256  the same at iters=8
    m4p2i1.occ   m4p2i1.f256 with `CostField.from_occupancy` (256 x 256, window radius 16: "cost field from occupancy v1") run on
                 every tick before the replay, into the buffer the tick's field then reads: one more launch per tick

The obstacles lie where a clamped trajectory meets them (centres in [-0.5, 0.5]^2, radii 0.2 .. 0.5, no empty slot), and their
values travel through the sampler's static buffers on every tick.  The arms alternate in one process, `--rounds` times, each
window timed with device events around >= `--ticks` ticks (at least `--seconds` of them).  Nobody has measured the guided step
before, so there is no expectation to hold it against (the field arms have none either: their ratios over `none` and over
`m4p2i1` are recorded); the step stays one launch of a few hundred to a few tens of thousands of
threads, two in seven of which loop over the constraints.  Prints a table and one JSON line; `--json PATH` also writes the
record.  This measures time only: what a guide does to a trained model's driving quality is not something the repository can
measure (it has no trained weights).

`--motion` runs another leg instead ("cost guidance v3", motion limits): the graph tick with the largest guide with and without
limits (`m32p8i8` and `m32p8i8.lim`, beside `none`) at 1 and 64 scenes, and the three step launches alone -- DDIM, DDPM and
DPM-Solver++ `scheduler.step` with that guide, 20 calls captured in one graph and replayed, with limits (the row-wise kernel: a
wave per row) and without (the element-wise kernel), per launch.  The limits (0.05, 0.03) are ones a fresh draw exceeds.

`--route` runs a third leg instead ("cost guidance v4", a route corridor): the graph tick at 1 and 64 scenes with no guide, with
the largest guide (`m32p8i8`) and with the same plus a route of 32 points (`m32p8i8.r32`, iters=8 like the rest: 31 segments with
one division each per iteration, twice per waypoint in the element-wise kernel), and the last two again with limits beside them
(`m32p8i8.lim`, `m32p8i8.lim.r32`: the row-wise kernel, once per waypoint).  The route winds through [-0.8, 0.8]^2 at half-width
0.1, which a fresh draw mostly lies outside of.

`--capsule` runs a fourth leg instead ("cost guidance v5", moving capsules): the graph tick at 1 and 64 scenes with no guide, with
32 discs alone (`m32i8`), with 32 capsules alone (`c32i8`: the discs' potential around a segment -- one division, a clamp and a
residual more per slot), with the largest v1 guide (`m32p8i8`), with the route beside it (`m32p8i8.r32`) and with 32 capsules
beside it (`m32p8i8.c32`), all at iters=8 in one run.  The capsules lie where the discs do, about 0.25 long.

    python tools/guide_tick_probe.py --json profiles/guide_tick_probe.json
    python tools/guide_tick_probe.py --motion --json profiles/motion_tick_probe.json
    python tools/guide_tick_probe.py --route --json profiles/route_tick_probe.json
    python tools/guide_tick_probe.py --capsule --json profiles/capsule_tick_probe.json
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autonomous_driving_with_diffusion_model_amd import Capsules, CostField, DeviceNoise, Guide, MotionLimits, Route  # noqa: E402
from autonomous_driving_with_diffusion_model_amd import scheduler as S  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.config import create_cfg  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.modeling import build_model  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.utils import procedural as P  # noqa: E402

SCHED_KW = dict(num_train_timesteps=100, prediction_type="sample", beta_schedule="squaredcos_cap_v2", beta_start=1e-4, beta_end=0.02)
IMG = (256, 900)
SIZES = ((1, 16), (64, 32))            # (scenes, horizon)
# (name, (M, P, iters) or None, G of a [S, G, G] field or None, from_occupancy on every tick)
ARMS = (("none", None, None, False), ("m4p2i1", (4, 2, 1), None, False), ("m32p8i8", (32, 8, 8), None, False),
        ("f64i1", (0, 0, 1), 64, False), ("m4p2i1.f256", (4, 2, 1), 256, False), ("m4p2i8.f256", (4, 2, 8), 256, False),
        ("m4p2i1.occ", (4, 2, 1), 256, True))
MARGIN = 0.125                         # of the occupancy arm: 16 cells of 2 / 256
# the --motion leg: (name, (M, P, iters) or None, motion limits or not, points of a route or 0)
MOTION_ARMS = (("none", None, False, 0), ("m32p8i8", (32, 8, 8), False, 0), ("m32p8i8.lim", (32, 8, 8), True, 0))
# the --route leg
ROUTE_ARMS = (("none", None, False, 0), ("m32p8i8", (32, 8, 8), False, 0), ("m32p8i8.r32", (32, 8, 8), False, 32),
              ("m32p8i8.lim", (32, 8, 8), True, 0), ("m32p8i8.lim.r32", (32, 8, 8), True, 32))
# the --capsule leg: one more entry, the number of capsule slots
CAPSULE_ARMS = (("none", None, False, 0, 0), ("m32i8", (32, 0, 8), False, 0, 0), ("c32i8", (0, 0, 8), False, 0, 32),
                ("m32p8i8", (32, 8, 8), False, 0, 0), ("m32p8i8.r32", (32, 8, 8), False, 32, 0), ("m32p8i8.c32", (32, 8, 8), False, 0, 32))
HALF_WIDTH = 0.1                       # of every scene's route
LIMITS = (0.05, 0.03)                  # (s_max, a_max) of every scene
STEP_CALLS = 20                        # step launches per captured graph


def make_cfg(steps, horizon):
    cfg = create_cfg()
    cfg.MODEL.HORIZON = horizon
    cfg.TRAIN.USE_COND = cfg.GUIDANCE.USE_COND = "FREE_GUIDANCE"
    cfg.GUIDANCE.FREE_SCALE, cfg.EVAL.SAMPLE_STEPS = 7.5, steps
    return cfg


def occupancy(scenes, G, dev):
    """About one node in 200 occupied, over [-1, 1]^2."""
    g = torch.Generator().manual_seed(13)
    return (torch.rand(scenes, G, G, generator=g) < 0.005).float().to(dev)


def field(scenes, G, dev):
    """A [scenes, G, G] field over [-1, 1]^2 (where a clamped trajectory lives), made from `occupancy` with margin 16 cells."""
    cell = 2.0 / (G - 1)
    return CostField.from_occupancy(occupancy(scenes, G, dev), (-1.0, -1.0), (cell, cell), 16 * cell)


def route(scenes, R, dev):
    """A [scenes, R, 2] polyline: x walks from -0.8 to 0.8, y = 0.5 sin(3 x + the scene's phase)."""
    x = torch.linspace(-0.8, 0.8, R).repeat(scenes, 1)
    y = 0.5 * torch.sin(3.0 * x + torch.arange(scenes, dtype=torch.float32)[:, None])
    return Route(torch.stack([x, y], dim=2).to(dev), HALF_WIDTH)


def capsules(scenes, C, dev):
    """[scenes, C, 7] slots where `obstacles` puts its discs: middles in [-0.5, 0.5]^2, a quarter long in a random direction, the
    discs' velocities and radii, no empty slot."""
    g = torch.Generator().manual_seed(17)
    mid = torch.rand(scenes, C, 2, generator=g) - 0.5
    yaw = torch.rand(scenes, C, generator=g) * 6.2831853
    half = 0.125 * torch.stack([torch.cos(yaw), torch.sin(yaw)], dim=2)
    s = torch.zeros(scenes, C, 7)
    s[..., 0:2], s[..., 2:4] = mid - half, mid + half
    s[..., 4:6] = (torch.rand(scenes, C, 2, generator=g) - 0.5) * 0.02
    s[..., 6] = 0.2 + 0.3 * torch.rand(scenes, C, generator=g)
    return Capsules(s.to(dev))


def obstacles(scenes, M, P, iters, dev, field=None, motion=False, points=0, slots=0):
    g = torch.Generator().manual_seed(11)
    discs = torch.zeros(scenes, M, 5)
    discs[..., :2] = torch.rand(scenes, M, 2, generator=g) - 0.5
    discs[..., 2:4] = (torch.rand(scenes, M, 2, generator=g) - 0.5) * 0.02
    discs[..., 4] = 0.2 + 0.3 * torch.rand(scenes, M, generator=g)
    planes = torch.zeros(scenes, P, 3)
    planes[..., :2] = torch.rand(scenes, P, 2, generator=g) * 2 - 1
    planes[..., 2] = torch.rand(scenes, P, generator=g) * 0.5
    return Guide(discs.to(dev) if M else None, planes.to(dev) if P else None, scale=0.2, schedule="variance", cap=0.1, iters=iters,
                 field=field, motion=MotionLimits(torch.tensor([LIMITS] * scenes, device=dev)) if motion else None,
                 route=route(scenes, points, dev) if points else None, capsules=capsules(scenes, slots, dev) if slots else None)


def motion_arms(dev, n, which=MOTION_ARMS):
    """The graph ticks of the --motion, --route and --capsule legs: `arms` with MOTION_ARMS, ROUTE_ARMS or CAPSULE_ARMS."""
    fns, meta = {}, {}
    for scenes, horizon in SIZES:
        cfg = make_cfg(n, horizon)
        with contextlib.redirect_stdout(sys.stderr):
            model = build_model(cfg)
        P.load_procedural(model, 0)
        model = model.to(dev).eval()
        d = {k: v.to(dev) for k, v in P.synthetic_batch(scenes, horizon, image_hw=IMG, seed=3).items()}
        for arm, mpi, lim, points, *rest in which:
            sch = S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
            gs = GraphedSampler(model, sch, cfg, noise=DeviceNoise(7, dev))
            guide = None if mpi is None else obstacles(scenes, *mpi, dev, motion=lim, points=points, slots=rest[0] if rest else 0)
            fns[f"s{scenes}.{arm}"] = (lambda gs=gs, img=d["imgs"], tgt=d["target"], guide=guide: gs(img, tgt, guide=guide))
            meta[f"s{scenes}.{arm}"] = (scenes, horizon, arm)
    return fns, meta


def step_launches(dev, rounds):
    """us per `scheduler.step` launch with the largest guide, with and without limits: STEP_CALLS calls in one captured graph."""
    out = {}
    for scenes, horizon in SIZES:
        cfg = make_cfg(20, horizon)
        g = torch.Generator().manual_seed(5)
        x = torch.randn(scenes, horizon, 7, generator=g).to(dev)
        mo = (torch.randn(scenes, horizon, 7, generator=g) * 0.7).to(dev)
        for sampler in ("ddim", "ddpm", "dpm"):
            for lim in (False, True):
                q = {"ddim": lambda: S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW),
                     "ddpm": lambda: S.GuidanceDDPMScheduler(cfg=cfg, **SCHED_KW),
                     "dpm": lambda: S.GuidanceDPMSolverMultistepScheduler(cfg=cfg, thresholding=True, lambda_min_clipped=-5.1, **SCHED_KW)}[sampler]()
                q.set_timesteps(20, device=dev)
                guide, noise, t = obstacles(scenes, 32, 8, 8, dev, motion=lim), DeviceNoise(3, dev), q.timesteps[0]
                noise.begin_tick()

                def run():
                    for _ in range(STEP_CALLS):
                        q.step(mo, t, x, generator=noise, guide=guide)
                run()
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    run()
                for _ in range(5):
                    graph.replay()
                us = [1e3 * timed(graph.replay, 200) / STEP_CALLS for _ in range(rounds)]
                out[f"s{scenes}.{sampler}.{'rows' if lim else 'element'}"] = {
                    "scenes": scenes, "horizon": horizon, "us_per_launch": [round(v, 3) for v in us], "median_us": round(statistics.median(us), 3)}
    return out


def arms(dev, n, only=None):
    fns, meta = {}, {}
    for scenes, horizon in SIZES:
        cfg = make_cfg(n, horizon)
        with contextlib.redirect_stdout(sys.stderr):
            model = build_model(cfg)
        P.load_procedural(model, 0)
        model = model.to(dev).eval()
        d = {k: v.to(dev) for k, v in P.synthetic_batch(scenes, horizon, image_hw=IMG, seed=3).items()}
        img, tgt = d["imgs"], d["target"]
        for arm, mpi, G, per_tick in ARMS:
            if only is not None and arm not in only:
                continue
            sch = S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
            gs = GraphedSampler(model, sch, cfg, noise=DeviceNoise(7, dev))
            guide = None if mpi is None else obstacles(scenes, *mpi, dev, None if G is None else field(scenes, G, dev))
            name = f"s{scenes}.{arm}"
            if per_tick:
                occ, f = occupancy(scenes, G, dev), guide.field

                def tick(gs=gs, img=img, tgt=tgt, guide=guide, occ=occ, f=f):
                    CostField.from_occupancy(occ, (f.x_min, f.y_min), (f.dx, f.dy), 16 * f.dx, out=f.cells)
                    return gs(img, tgt, guide=guide)
                fns[name] = tick
            else:
                fns[name] = (lambda gs=gs, img=img, tgt=tgt, guide=guide: gs(img, tgt, guide=guide))
            meta[name] = (scenes, horizon, arm)
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
    ap.add_argument("--arms", default=None, help="comma-separated arm names (default: all); the ratios need `none` and `m4p2i1` among them")
    ap.add_argument("--motion", action="store_true", help="the motion-limits leg instead: see the module docstring")
    ap.add_argument("--route", action="store_true", help="the route-corridor leg instead: see the module docstring")
    ap.add_argument("--capsule", action="store_true", help="the moving-capsules leg instead: see the module docstring")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.steps
    with torch.no_grad():
        if a.capsule:
            fns, meta = motion_arms(dev, n, CAPSULE_ARMS)
        elif a.route:
            fns, meta = motion_arms(dev, n, ROUTE_ARMS)
        elif a.motion:
            fns, meta = motion_arms(dev, n)
        else:
            fns, meta = arms(dev, n, None if a.arms is None else a.arms.split(","))
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
              "sample_steps": n, "rounds": a.rounds, "guide": "scale 0.2, variance schedule, cap 0.1", "arms": {}, "guided_over_none": {},
              "guided_over_m4p2i1": {}}
    if a.motion:
        with torch.no_grad():
            record["limits"], record["step_launches"] = list(LIMITS), step_launches(dev, a.rounds)
        record["limits_over_m32p8i8"] = {}
    if a.route and not a.capsule:
        record["route"] = {"points": 32, "half_width": HALF_WIDTH, "weight": 1.0}
        record["added_ms"] = {}
    if a.capsule:
        record["capsules"] = {"slots": 32, "length": 0.25, "weight": 1.0}
        record["added_ms"] = {}
    for k in fns:
        scenes, horizon, mode = meta[k]
        med = statistics.median(ms[k])
        record["arms"][k] = {"scenes": scenes, "horizon": horizon, "guide": mode, "ticks_per_window": ticks[k], "ticks": ticks[k] * a.rounds,
                             "ms_per_tick": [round(v, 4) for v in ms[k]], "median_ms": round(med, 4), "min_ms": round(min(ms[k]), 4),
                             "max_ms": round(max(ms[k]), 4), "spread_pct": round(100 * (max(ms[k]) - min(ms[k])) / med, 2)}
    for k, v in record["arms"].items():
        for over, base in (("guided_over_none", "none"), ("guided_over_m4p2i1", "m4p2i1")):
            ref = record["arms"].get(f"s{v['scenes']}.{base}")
            if v["guide"] != "none" and ref is not None:
                record[over][k] = round(v["median_ms"] / ref["median_ms"], 4)
    if a.capsule:                   # what 32 capsules add to the tick next to what 32 discs and the 32-point route add, in one run
        for scenes, _ in SIZES:
            med = {arm[0]: record["arms"][f"s{scenes}.{arm[0]}"]["median_ms"] for arm in CAPSULE_ARMS}
            record["added_ms"][f"s{scenes}"] = {"m32i8 over none": round(med["m32i8"] - med["none"], 4),
                                                "c32i8 over none": round(med["c32i8"] - med["none"], 4),
                                                "m32p8i8 over none": round(med["m32p8i8"] - med["none"], 4),
                                                "r32 over m32p8i8": round(med["m32p8i8.r32"] - med["m32p8i8"], 4),
                                                "c32 over m32p8i8": round(med["m32p8i8.c32"] - med["m32p8i8"], 4)}
        print(json.dumps(record["added_ms"]), file=sys.stderr)
    if a.route and not a.capsule:   # what each layer adds to the tick: the 32 discs and 8 planes over none, the route over those
        for scenes, _ in SIZES:
            med = {arm: record["arms"][f"s{scenes}.{arm}"]["median_ms"] for arm, _, _, _ in ROUTE_ARMS}
            record["added_ms"][f"s{scenes}"] = {"m32p8i8 over none": round(med["m32p8i8"] - med["none"], 4),
                                                "r32 over m32p8i8": round(med["m32p8i8.r32"] - med["m32p8i8"], 4),
                                                "r32 over m32p8i8.lim": round(med["m32p8i8.lim.r32"] - med["m32p8i8.lim"], 4)}
        print(json.dumps(record["added_ms"]), file=sys.stderr)
    if a.motion:
        for scenes, _ in SIZES:
            record["limits_over_m32p8i8"][f"s{scenes}"] = round(record["arms"][f"s{scenes}.m32p8i8.lim"]["median_ms"] /
                                                                record["arms"][f"s{scenes}.m32p8i8"]["median_ms"], 4)
        for k, v in record["step_launches"].items():
            print(f"{k:<24}{v['median_us']:>9.3f} us per launch", file=sys.stderr)
    print(f"FREE guidance, DDIM, {IMG[0]}x{IMG[1]} frame, n = {n}, graph ticks ({a.rounds} alternating rounds)", file=sys.stderr)
    print(f"{'arm':<14}{'scenes':>7}{'H':>4}{'median ms':>11}{'min':>9}{'max':>9}{'spread %':>10}{'/ none':>9}{'/ m4p2i1':>10}{'ticks':>8}", file=sys.stderr)
    for k, v in record["arms"].items():
        r, r1 = record["guided_over_none"].get(k), record["guided_over_m4p2i1"].get(k)
        print(f"{k:<14}{v['scenes']:>7}{v['horizon']:>4}{v['median_ms']:>11.3f}{v['min_ms']:>9.3f}{v['max_ms']:>9.3f}"
              f"{v['spread_pct']:>10.2f}{('' if r is None else format(r, '.4f')):>9}{('' if r1 is None else format(r1, '.4f')):>10}"
              f"{v['ticks']:>8}", file=sys.stderr)
    print(json.dumps(record))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
