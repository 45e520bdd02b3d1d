#!/usr/bin/env python
"""Time of the expert's launch: alone, as a captured replay, and the whole `Expert.__call__` (navigator step, ego frame, launch,
controller), beside the vehicle launch it feeds.

    python tools/expert_probe.py [--json out.json]

At (S, N, M, K) = (1, 8, 0, 4) and (64, 64, 64, 8): a route of 200 points 2 m apart and a window of 32, boxes and discs scattered
along the first 60 m of the route, the planes of a `Signals` of 16 lights, H = 16 rows of 7.  `plan_us` is `Expert.plan` alone and
`call_us` the whole call, eager calls back to back between HIP events as tools/traffic_probe.py takes them (which measures the rate
at which the host issues them: no kernel trace is taken); `replay_us` is a captured graph of 20 `plan` launches replayed, divided
by 20 -- the launch without the host in front of it.  `vehicle_us` is the vehicle launch for scale.  The time has no target: it
is a recorded measurement beside its sibling launches (profiles/README.md, "Expert"), not a threshold, and no test asserts a time.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from metrics_probe import timed      # noqa: E402  (tools/ is the script's directory)

G, K, DT, N_LINES = 200, 23.315, 0.05, 16
CHAIN = 20


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--iters", type=int, default=5000, help="eager calls per timed window")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from autonomous_driving_with_diffusion_model_amd import DeviceController, Expert, KinematicVehicle, Navigator, Signals
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    from autonomous_driving_with_diffusion_model_amd.simulation import World
    dev = "cuda:0"
    cfg = create_cfg()
    rows = []
    for scenes, n_boxes, n_discs, n_planes in ((1, 8, 0, 4), (64, 64, 64, 8)):
        rng = np.random.default_rng(scenes)
        heading = rng.uniform(-3, 3, scenes)
        unit = np.stack([np.cos(heading), np.sin(heading)], axis=-1)
        route = unit[:, None] * (2.0 * np.arange(G))[None, :, None]                                      # [S, G, 2]
        pose0 = np.concatenate([route[:, 0], np.arctan2(np.cos(heading), -np.sin(heading))[:, None]], axis=1)
        j = np.arange(N_LINES)
        timing = np.stack([0.5 * j, np.full(N_LINES, 2.0), np.full(N_LINES, 1.0), np.full(N_LINES, 5.0)], axis=-1)
        rec = Signals.from_lines(route[:, 10 + 10 * j], heading[:, None], 8.0, np.ones(N_LINES)[None], 15.0, timing[None])

        def scatter(n, width):
            at = route[:, 0][:, None] + unit[:, None] * rng.uniform(5.0, 60.0, (scenes, n, 1)) + rng.normal(0.0, 3.0, (scenes, n, 2))
            vel = unit[:, None] * rng.uniform(0.0, 6.0, (scenes, n, 1))
            rest = np.broadcast_to(heading[:, None, None], (scenes, n, 1)) if width == 7 else None
            cols = [at, vel] + ([rest, np.full((scenes, n, 1), 4.5), np.full((scenes, n, 1), 2.0)] if width == 7 else [np.full((scenes, n, 1), 0.8)])
            return torch.from_numpy(np.ascontiguousarray(np.concatenate(cols, axis=-1))).to(dev)

        sig = Signals(rec, device=dev, dt=DT, xy_scale=K, planes=n_planes)
        world = World(boxes=scatter(n_boxes, 7), discs=scatter(n_discs, 5) if n_discs else None, signals=sig)
        nav = Navigator(torch.from_numpy(route), torch.zeros(scenes, G, dtype=torch.int32), torch.full((scenes,), G, dtype=torch.int32),
                        xy_scale=K, points=32, first=0, device=dev)
        expert = Expert(nav, DeviceController(cfg, scenes, dev), horizon=16, dim=7, waypoint_dt=0.5, world=world)
        veh = KinematicVehicle(scenes, dev, dt=DT)
        veh.reset(pose0, np.full(scenes, 5.0))
        sig.step(veh.pose, veh.velocity)
        expert(None, pose=veh.pose, velocity=veh.velocity)                                               # the window and the ego-frame world
        control = expert.last_control.clone()
        plan_us = [round(timed(lambda: expert.plan(veh.velocity), 20, args.iters) * 1e3, 2) for _ in range(3)]
        call_us = [round(timed(lambda: expert(None, pose=veh.pose, velocity=veh.velocity), 20, args.iters) * 1e3, 2) for _ in range(3)]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(CHAIN):
                expert.plan(veh.velocity)
        replay_us = [round(timed(graph.replay, 5, max(args.iters // CHAIN, 10)) * 1e3 / CHAIN, 2) for _ in range(3)]
        leaders = expert.compute()["leader"]
        vehicle_us = [round(timed(lambda: veh.step(control), 20, args.iters) * 1e3, 2) for _ in range(3)]
        rows.append({"scenes": scenes, "boxes": n_boxes, "discs": n_discs, "planes": n_planes, "window": 32, "horizon": 16, "dim": 7,
                     "plan_us": statistics.median(plan_us), "plan_us_rounds": plan_us, "call_us": statistics.median(call_us),
                     "call_us_rounds": call_us, "replay_us": statistics.median(replay_us), "replay_us_rounds": replay_us,
                     "vehicle_us": statistics.median(vehicle_us), "vehicle_us_rounds": vehicle_us, "calls_per_round": args.iters,
                     "leaders": {"none": int((leaders < 0).sum()), "box": int(((leaders >= 0) & (leaders < 64)).sum()),
                                 "disc": int(((leaders >= 64) & (leaders < 128)).sum()), "plane": int(((leaders >= 128) & (leaders < 136)).sum()),
                                 "end": int((leaders == 136).sum())}})
        print(json.dumps(rows[-1]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
