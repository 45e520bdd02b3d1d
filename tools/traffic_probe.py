#!/usr/bin/env python
"""Time of the traffic launch: alone, beside the vehicle, the signals and the drive-metrics launches, and in the closed loop with
and without traffic.

    python tools/traffic_probe.py [--json out.json]

The launch alone at (S, N) = (1, 8) and (64, 64): agents 9 m apart on 8 paths of 64 points 5 m apart with 16 stops per scene, an
ego that stands on path 0 ahead of its agents; `traffic_us`, `signals_us`, `vehicle_us` and `metrics_us` are the four launches
alone, eager calls back to back between HIP events (which measures the rate at which the host issues them: no kernel trace is
taken), the metrics with the traffic's boxes.

The loop at S = 1 and S = 64 scenes, as tools/signals_probe.py sets it up: the tick is a GraphedSampler replay (10-step DDIM,
classifier-free guidance, 256x900 frames, H = 16) with `navigator=` (a plan of 200 points 2 m apart) and `controller=`.
`loop_boxes` is the body of `simulation.drive` with `World(boxes=, signals=)`: tick with the default world guide (the signals'
planes and the boxes as capsules), vehicle, signals, `World.advance`, metrics; `loop_traffic` is the same with
`World(traffic=, signals=)`: the same guide, vehicle, signals, traffic, metrics.  Both arms carry the same number of boxes (at
most 32 in the loop: what `Capsules.from_boxes` takes), so the difference is the traffic launch against the torch op of
`World.advance`.  The arms alternate in rounds so that both see the same clocks; the median is the figure.  The launch time has no
target: it is a recorded measurement against its sibling launches (profiles/README.md, "Traffic"), not a threshold, and no test
asserts a time.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from metrics_probe import SCHED_KW, timed      # noqa: E402  (tools/ is the script's directory)

G, K, DT, N_LINES, PLANES = 200, 23.315, 0.05, 16, 4
PATHS, POINTS, SPACING = 8, 64, 5.0


def world_parts(np, scenes, agents, origin, heading, n_lines):
    """Paths, agents and stops of `scenes` scenes: path q runs parallel to the route, 3.5 q metres to its left, and begins 100 m
    behind `origin` (so the ego starts ahead of every agent of path 0); agents 9 m apart from the start of their path on, spread
    over the paths; a stop every 6 m from 110 m on, on path t % 8."""
    unit = np.stack([np.cos(heading), np.sin(heading)], axis=-1)                                     # [S, 2]
    left = np.stack([-unit[:, 1], unit[:, 0]], axis=-1)
    along = SPACING * np.arange(POINTS) - 100.0
    paths = origin[:, None, None] + unit[:, None, None] * along[None, None, :, None] + left[:, None, None] * (3.5 * np.arange(PATHS))[None, :, None, None]
    rows = np.zeros((scenes, agents, 9))
    k = np.arange(agents)
    rows[..., 0] = k % PATHS
    rows[..., 1] = 9.0 * (k // PATHS)
    rows[..., 2:] = (5.0, 8.0, 4.5, 2.0, 1.5, 1.5, 2.0)
    t = np.arange(16)
    stops = np.zeros((scenes, 16, 3))
    stops[..., 0], stops[..., 1], stops[..., 2] = t % PATHS, 110.0 + 6.0 * t, t % n_lines
    return paths, np.full((scenes, PATHS), POINTS, dtype=np.int32), rows, stops


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds of the loop arms; the median is kept")
    ap.add_argument("--iters", type=int, default=5000, help="eager calls per timed window of the launches alone")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from autonomous_driving_with_diffusion_model_amd import (DeviceController, DeviceNoise, DriveMetrics, EgoFrame, KinematicVehicle, Navigator,
                                                             Signals, Traffic)
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    from autonomous_driving_with_diffusion_model_amd.modeling import build_model
    from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler
    from autonomous_driving_with_diffusion_model_amd.simulation import World, _world_guide
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
    for scenes, agents in ((1, 8), (64, 64)):
        rng = np.random.default_rng(scenes)
        heading = rng.uniform(-3, 3, scenes)
        unit = np.stack([np.cos(heading), np.sin(heading)], axis=-1)
        route = unit[:, None] * (2.0 * np.arange(G))[None, :, None]                                      # [S, G, 2]
        pose0 = np.concatenate([route[:, 0], np.arctan2(np.cos(heading), -np.sin(heading))[:, None]], axis=1)
        img = P.synthetic_batch(scenes, 16, image_hw=(256, 900), seed=1)["imgs"].to(dev)
        j = np.arange(N_LINES)
        timing = np.stack([0.5 * j, np.full(N_LINES, 2.0), np.full(N_LINES, 1.0), np.full(N_LINES, 5.0)], axis=-1)
        rec = Signals.from_lines(route[:, 10 + 10 * j], heading[:, None], 8.0, np.ones(N_LINES)[None], 15.0, timing[None])
        paths, plen, agent_rows, stops = world_parts(np, scenes, agents, route[:, 0], heading, N_LINES)
        loop_rows = agent_rows[:, :32]                                                                   # the default world guide's limit

        def stack(with_traffic, alone=False):
            nav = Navigator(torch.from_numpy(route), torch.zeros(scenes, G, dtype=torch.int32), torch.full((scenes,), G, dtype=torch.int32),
                            xy_scale=K, device=dev)
            sch = S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
            sampler = GraphedSampler(model, sch, cfg, noise=DeviceNoise(3, dev), controller=DeviceController(cfg, scenes, dev), navigator=nav)
            veh = KinematicVehicle(scenes, dev, dt=DT)
            veh.reset(pose0)
            met = DriveMetrics(nav, dt=DT, max_ticks=0, max_time=1e9, offroad_min=1e9, offroad_max=1e9, completion_tol=0.0)
            sig = Signals(rec, device=dev, dt=DT, xy_scale=K, planes=PLANES)
            tr = Traffic(paths, plen, agent_rows if alone else loop_rows, stops=stops, signals=sig, dt=DT, device=dev)
            world = World(signals=sig, traffic=tr) if with_traffic else World(signals=sig, boxes=tr.boxes.clone())
            sig.step(veh.pose, veh.velocity, hold=met.done)
            return sampler, veh, met, sig, tr, world, EgoFrame(veh.pose, K, DT)

        (s0, v0, m0, g0, _, w0, f0), (s1, v1, m1, g1, t1, w1, f1) = stack(False), stack(True)

        def loop_boxes():
            s0(img, pose=v0.pose, velocity=v0.velocity, guide=_world_guide(f0, w0))
            v0.step(s0.last_control, hold=m0.done)
            g0.step(v0.pose, v0.velocity, hold=m0.done)
            w0.advance(DT)
            m0.step(v0.pose, v0.velocity, v0.yaw_rate, None, w0.boxes)

        def loop_traffic():
            s1(img, pose=v1.pose, velocity=v1.velocity, guide=_world_guide(f1, w1))
            v1.step(s1.last_control, hold=m1.done)
            g1.step(v1.pose, v1.velocity, hold=m1.done)
            t1.step(v1.pose, v1.velocity, hold=m1.done)
            m1.step(v1.pose, v1.velocity, v1.yaw_rate, None, w1.boxes)

        arms = (("loop_boxes", loop_boxes), ("loop_traffic", loop_traffic))
        iters = 5 if scenes > 1 else 50
        ms = {name: [] for name, _ in arms}
        for r in range(args.rounds):
            for name, fn in arms if r % 2 == 0 else arms[::-1]:
                ms[name].append(timed(fn, 2, iters))
        control = s1.last_control
        _, veh, met, sig, tr, _, _ = stack(True, alone=True)
        veh.reset(pose0, np.full(scenes, 5.0))
        # on the start pose first (no scene ends, nothing is held); the vehicle last, which drives off
        traffic_us = [round(timed(lambda: tr.step(veh.pose, veh.velocity, hold=met.done), 20, args.iters) * 1e3, 2) for _ in range(3)]
        signals_us = [round(timed(lambda: sig.step(veh.pose, veh.velocity, hold=met.done), 20, args.iters) * 1e3, 2) for _ in range(3)]
        metrics_us = [round(timed(lambda: met.step(veh.pose, veh.velocity, veh.yaw_rate, None, tr.boxes), 20, args.iters) * 1e3, 2) for _ in range(3)]
        assert not met.done.any().item()
        vehicle_us = [round(timed(lambda: veh.step(control), 20, args.iters) * 1e3, 2) for _ in range(3)]
        med = {name: statistics.median(v) for name, v in ms.items()}
        rows.append({"scenes": scenes, "agents": agents, "loop_agents": int(loop_rows.shape[1]), "paths": PATHS, "path_points": POINTS, "stops": 16, "route_points": G, "signals": N_LINES,
                     "planes": PLANES, "ddim_steps": args.steps, "horizon": 16,
                     **{f"{name}_ms": round(v, 3) for name, v in med.items()},
                     **{f"{name}_ms_rounds": [round(x, 3) for x in v] for name, v in ms.items()},
                     "traffic_minus_boxes_us": round((med["loop_traffic"] - med["loop_boxes"]) * 1e3, 1),
                     "traffic_us": statistics.median(traffic_us), "traffic_us_rounds": traffic_us,
                     "signals_us": statistics.median(signals_us), "signals_us_rounds": signals_us,
                     "vehicle_us": statistics.median(vehicle_us), "vehicle_us_rounds": vehicle_us,
                     "metrics_us": statistics.median(metrics_us), "metrics_us_rounds": metrics_us, "calls_per_round": args.iters,
                     "traffic_report": {k: np.asarray(v).tolist() for k, v in t1.compute().items() if k in ("ego_yields", "overlaps", "arrived", "alive")},
                     "alone_report": {k: int(np.asarray(v).sum()) for k, v in tr.compute().items() if k in ("ticks", "arrived", "alive", "overlaps")}})
        print(json.dumps(rows[-1]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
