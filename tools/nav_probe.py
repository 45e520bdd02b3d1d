#!/usr/bin/env python
"""Time of the navigator's step (adx_nav_step) and of every EgoFrame launch, beside the host work they replace.

    python tools/nav_probe.py [--json out.json]

At S = 1 and S = 64 scenes, each with a plan of 200 points 3 m apart and a window of 16: `Navigator.step` on a device pose, the
four `EgoFrame` kinds (16 points, 8 discs, 4 planes and 8 boxes per scene) and `to_world` of a [S, 16, 7] plan -- `--iters` eager
calls back to back between HIP events on the stream after a warm-up, `--rounds` times over (the median is the figure, the rounds
are in the JSON) --, and the host's version of the same tick input, written the way the reference's agent
does it: per scene the RoutePlanner walk over a deque with `np.linalg.norm`, the rotation of the next waypoint and of the
16-point route ahead by the compass, and one host-to-device copy of the target, the window and the motion, timed with the wall
clock up to the copies' completion.  A recorded measurement (profiles/README.md, "Route planner"), not a threshold: no test
asserts a time.
"""
import argparse
import json
import math
import os
import sys
import time
from collections import deque

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from metrics_probe import timed      # noqa: E402  (tools/ is the script's directory)

G, R, K = 200, 16, 23.315


def host_walk(route: deque, pos, min_distance=7.0, max_distance=50.0):
    """RoutePlanner.run_step (e2e_driving/planner.py:55-92) without its plotter."""
    import numpy as np
    if len(route) == 1:
        return route[0]
    to_pop, far, cum = 0, -np.inf, 0.0
    for i in range(1, len(route)):
        if cum > max_distance:
            break
        cum += np.linalg.norm(route[i] - route[i - 1])
        d = np.linalg.norm(route[i] - pos)
        if d <= min_distance and d > far:
            far, to_pop = d, i
    for _ in range(to_pop):
        if len(route) > 2:
            route.popleft()
    return route[1]


def host_to_ego(points, pos, compass):
    """process_next_waypoint (interact.py:185-202)."""
    import numpy as np
    yaw = (0.0 if math.isnan(compass) else compass) + math.pi / 2.0
    rot = np.array([[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]])
    local = rot.T.dot((points - pos).T).T
    return np.stack([local[:, 1] / K, -local[:, 0] / K], axis=-1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--iters", type=int, default=20000, help="calls per timed window (about 0.15 s of 8 us calls)")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args(argv)
    import statistics
    import numpy as np
    import torch
    from autonomous_driving_with_diffusion_model_amd import EgoFrame, Navigator
    dev = "cuda:0"
    rows = []

    def us(fn):
        rounds = [round(timed(fn, 20, args.iters) * 1e3, 2) for _ in range(args.rounds)]
        return statistics.median(rounds), rounds

    for S in (1, 64):
        rng = np.random.default_rng(S)
        heading = rng.uniform(-3, 3, S)
        route = np.stack([np.stack([np.cos(h), np.sin(h)]) * (3.0 * np.arange(G))[:, None] for h in heading])        # [S, G, 2]
        pose_h = np.concatenate([route[:, 40] + rng.uniform(-1, 1, (S, 2)), heading[:, None]], axis=1)
        nav = Navigator(torch.from_numpy(route), torch.zeros(S, G, dtype=torch.int32), torch.full((S,), G, dtype=torch.int32),
                        xy_scale=K, points=R, device=dev)
        pose = torch.from_numpy(pose_h).to(dev)
        step_us, step_rounds = us(lambda: nav.step(pose))
        ef = EgoFrame(pose, K, dt=0.5)
        ins = {"points": torch.randn(S, R, 2, dtype=torch.float64, device=dev), "discs": torch.randn(S, 8, 5, dtype=torch.float64, device=dev),
               "planes": torch.randn(S, 4, 3, dtype=torch.float64, device=dev), "boxes": torch.randn(S, 8, 7, dtype=torch.float64, device=dev)}
        row = {"scenes": S, "route_points": G, "window": R, "calls_per_round": args.iters, "nav_step_us": step_us,
               "nav_step_us_rounds": step_rounds}
        for name, t in ins.items():
            out = getattr(ef, name)(t)
            row[f"ego_{name}_us"], row[f"ego_{name}_us_rounds"] = us(lambda: getattr(ef, name)(t, out=out))
        plan = torch.randn(S, 16, 7, device=dev)
        world = ef.to_world(plan)
        row["to_world_us"], row["to_world_us_rounds"] = us(lambda: ef.to_world(plan, out=world))

        # the host's version: a fresh deque per scene at the same cursor every time, so that every repetition does the same work
        plans = [[route[s, i] for i in range(38, G)] for s in range(S)]
        prev = pose_h - 0.5

        def host_tick():
            tgt, win, mo = np.empty((S, 2)), np.empty((S, R, 2)), np.empty((S, 3))
            for s in range(S):
                dq = deque(plans[s])
                nxt = host_walk(dq, pose_h[s, :2])
                ahead = np.array([dq[min(k, len(dq) - 1)] for k in range(R)])
                tgt[s] = host_to_ego(nxt[None], pose_h[s, :2], pose_h[s, 2])[0]
                win[s] = host_to_ego(ahead, pose_h[s, :2], pose_h[s, 2])
                mo[s, :2] = host_to_ego(pose_h[s:s + 1, :2], prev[s, :2], prev[s, 2])[0]
                mo[s, 2] = pose_h[s, 2] - prev[s, 2]
            out = [torch.from_numpy(a).to(torch.float32).to(dev, non_blocking=True) for a in (tgt, win, mo)]
            torch.cuda.synchronize()
            return out

        for _ in range(3):
            host_tick()
        n = 50 if S > 1 else 2000                      # about 0.2 s per round
        host = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            for _ in range(n):
                host_tick()
            host.append(round((time.perf_counter() - t0) / n * 1e6, 1))
        row["host_loops_us"], row["host_loops_us_rounds"] = statistics.median(host), host
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
