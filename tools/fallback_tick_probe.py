"""What does the stop-short fallback cost a driving tick?  FREE guidance (scale 7.5), full-size camera frames, perception pass inside
the tick, DDIM (eta = 0), a guide of one disc per scene and a PID controller, at S = 1 and S = 64 scenes and H = 16 and 32:

    graph           GraphedSampler(controller=...) called with the guide -- the tick without the node
    graph_fb_free   the same with fallback=StopShort(...): every row free (the disc slot is empty), the node's copy path
    graph_fb_stop   the same, every row blocked at its last waypoint: a disc of radius 10 that reaches the origin at time H - 1 and is
                    20 away one waypoint earlier, so `first` = H - 1 whatever the plan is -- both sequential passes and the longest
                    lookup

The guide's scale is 0, so the steps read the disc and move nothing: all three arms of a shape sample the same plan.  The arms
alternate in one process, `--rounds` times; a window is >= `--ticks` ticks (at least `--seconds`) between two `perf_counter` reads
with a device synchronisation before each.  Reported: the median over the rounds, the spread, and every arm minus `graph` of the same
shape.

A node is tens of microseconds in a tick of tens of milliseconds, less than the spread of a window, so the nodes are also timed on
their own: `--chain` launches of one node captured as one graph and replayed, time per launch, for the stop-short node on free and
on blocked rows, the control node and the select node (K = 4, guided, hard) on the same [S, H, D] rows.  Time only: nothing here is
asserted anywhere.

    python tools/fallback_tick_probe.py --json profiles/fallback_tick_probe.json
"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

SCENES = (1, 64)
HORIZONS = (16, 32)
SCHED_KW = dict(num_train_timesteps=100, prediction_type="sample", beta_schedule="squaredcos_cap_v2", beta_start=1e-4, beta_end=0.02)
IMG = (256, 900)
ARMS = ("graph", "graph_fb_free", "graph_fb_stop")
NODES = ("stop_short_free", "stop_short_stop", "control", "select_k4")
PARAMS = (0.02, 0.004)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_cfg(steps, horizon):
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    cfg = create_cfg()
    cfg.MODEL.HORIZON = horizon
    cfg.TRAIN.USE_COND = cfg.GUIDANCE.USE_COND = "FREE_GUIDANCE"
    cfg.GUIDANCE.FREE_SCALE, cfg.EVAL.SAMPLE_STEPS = 7.5, steps
    return cfg


def guides(scenes, horizon, dev):
    """(free, stop): one disc slot per scene, empty, or the disc of the docstring."""
    import torch
    from autonomous_driving_with_diffusion_model_amd import Guide
    free = torch.zeros(scenes, 1, 5, device=dev)
    stop = free.clone()
    stop[:, 0] = torch.tensor([-20.0 * (horizon - 1), 0.0, 20.0, 0.0, 10.0], device=dev)
    return Guide(free, scale=0.0, schedule="constant"), Guide(stop, scale=0.0, schedule="constant")


def arms(dev, steps, chain):
    import torch
    from autonomous_driving_with_diffusion_model_amd import DeviceController, StopShort, TrajectorySelector
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    from autonomous_driving_with_diffusion_model_amd.modeling import build_model
    from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler
    from autonomous_driving_with_diffusion_model_amd.utils import procedural as P
    ticks, nodes, keep = {}, {}, []
    for horizon in HORIZONS:
        cfg = make_cfg(steps, horizon)
        with contextlib.redirect_stdout(sys.stderr):
            model = build_model(cfg)
        P.load_procedural(model, 0)
        model = model.to(dev).eval()
        for scenes in reversed(SCENES):        # the larger batch first: its warm-up sizes the model's workspace once
            d = {k: v.to(dev) for k, v in P.synthetic_batch(scenes, horizon, image_hw=IMG, seed=3).items()}
            img, tgt, init = d["imgs"], d["target"], d["init_trajs"]
            vel = torch.full((scenes,), 1.5, device=dev)
            free, stop = guides(scenes, horizon, dev)
            sch = lambda: S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)      # noqa: E731
            ctl = lambda: DeviceController(cfg, scenes, dev, source="pid")                      # noqa: E731
            fb = lambda: StopShort(torch.tensor([PARAMS] * scenes, device=dev))                 # noqa: E731
            plain = GraphedSampler(model, sch(), cfg, controller=ctl())
            with_fb = GraphedSampler(model, sch(), cfg, controller=ctl(), fallback=fb())
            tag = f"s{scenes}_h{horizon}"
            ticks[f"graph_{tag}"] = (lambda gs=plain, img=img, tgt=tgt, init=init, vel=vel, g=free: gs(img, tgt, init, velocity=vel, guide=g))
            ticks[f"graph_fb_free_{tag}"] = (lambda gs=with_fb, img=img, tgt=tgt, init=init, vel=vel, g=free:
                                             gs(img, tgt, init, velocity=vel, guide=g))
            ticks[f"graph_fb_stop_{tag}"] = (lambda gs=with_fb, img=img, tgt=tgt, init=init, vel=vel, g=stop:
                                             gs(img, tgt, init, velocity=vel, guide=g))
            # the nodes on their own, on a plan that walks 0.02 per waypoint along x: `chain` launches as one graph
            rows = torch.zeros(scenes, horizon, init.shape[2], device=dev)
            rows[:, :, 0] = 0.02 * torch.arange(horizon, device=dev)
            cands = rows.repeat(4, 1, 1).contiguous()
            one_fb, one_ctl, sel = fb(), ctl(), TrajectorySelector(1.0, 0.5, 0.25, w_guide=1.0, hard=True)
            launches = {"stop_short_free": lambda rows=rows, f=one_fb, g=free: f(rows, g),
                        "stop_short_stop": lambda rows=rows, f=one_fb, g=stop: f(rows, g),
                        "control": lambda rows=rows, c=one_ctl, vel=vel, tgt=tgt, mn=model.magic_num: c.step(rows, vel, tgt, xy_scale=mn),
                        "select_k4": lambda cands=cands, sel=sel, tgt=tgt, g=stop, n=scenes: sel(cands, n, tgt, g)}
            for name, launch in launches.items():
                launch()
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    for _ in range(chain):
                        launch()
                keep.append(graph)
                nodes[f"{name}_{tag}"] = graph.replay
    return ticks, nodes


def timed(fn, ticks):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ticks):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / ticks


def stats(samples, scale=1.0):
    med = statistics.median(samples)
    return {"per_round": [round(v * scale, 4) for v in samples], "median": round(med * scale, 4), "min": round(min(samples) * scale, 4),
            "max": round(max(samples) * scale, 4), "spread_pct": round(100 * (max(samples) - min(samples)) / med, 2)}


def measure(a):
    import torch
    dev = torch.device("cuda:0")
    with torch.no_grad():
        ticks, nodes = arms(dev, a.steps, a.chain)
        fns = dict(ticks, **nodes)
        count = {}
        for fn in fns.values():                 # warm every arm (captures included) ...
            for _ in range(2):
                fn()
        for k, fn in fns.items():               # ... then size the windows, once no arm's capture can move the model's buffers
            count[k] = max(a.ticks, int(a.seconds * 1e3 / timed(fn, 2)) + 1)
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ms[k].append(timed(fn, count[k]))
    record = {"device": torch.cuda.get_device_name(0), "image": list(IMG), "guidance": "FREE_GUIDANCE", "sampler": "ddim", "steps": a.steps,
              "rounds": a.rounds, "chain": a.chain, "params": list(PARAMS),
              "clock": "perf_counter around a window, device synchronised at both ends", "ticks_ms": {}, "added_ms_over_graph": {},
              "nodes_us_per_launch": {}}
    print(f"FREE guidance, {IMG[0]}x{IMG[1]} frames, DDIM {a.steps} steps ({a.rounds} alternating rounds)", file=sys.stderr)
    print(f"{'tick':<26}{'median ms':>10}{'min':>9}{'max':>9}{'spread %':>10}{'- graph':>10}{'ticks':>7}", file=sys.stderr)
    for horizon in HORIZONS:
        for scenes in SCENES:
            tag = f"s{scenes}_h{horizon}"
            base = statistics.median(ms[f"graph_{tag}"])
            for arm in ARMS:
                k = f"{arm}_{tag}"
                v = record["ticks_ms"][k] = dict(stats(ms[k]), ticks_per_window=count[k])
                record["added_ms_over_graph"][k] = round(statistics.median(ms[k]) - base, 4)
                print(f"{k:<26}{v['median']:>10.3f}{v['min']:>9.3f}{v['max']:>9.3f}{v['spread_pct']:>10.2f}"
                      f"{record['added_ms_over_graph'][k]:>10.3f}{count[k]:>7}", file=sys.stderr)
    print(f"{'node (us per launch)':<26}{'median':>10}{'min':>9}{'max':>9}{'spread %':>10}", file=sys.stderr)
    for horizon in HORIZONS:
        for scenes in SCENES:
            for node in NODES:
                k = f"{node}_s{scenes}_h{horizon}"
                v = record["nodes_us_per_launch"][k] = stats(ms[k], 1e3 / a.chain)
                print(f"{k:<26}{v['median']:>10.2f}{v['min']:>9.2f}{v['max']:>9.2f}{v['spread_pct']:>10.2f}", file=sys.stderr)
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=10, help="least number of ticks (or chain replays) per window")
    ap.add_argument("--seconds", type=float, default=0.5, help="least length of a window")
    ap.add_argument("--steps", type=int, default=50, help="EVAL.SAMPLE_STEPS")
    ap.add_argument("--chain", type=int, default=200, help="launches of one node per captured chain")
    ap.add_argument("--json", default=None, help="write the record here")
    a = ap.parse_args()
    record = measure(a)
    print(json.dumps(record))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
