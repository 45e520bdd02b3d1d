#!/usr/bin/env python
"""Time of a closed-loop tick: the graph tick alone, the tick followed by the vehicle and the drive-metrics launches, the two
launches alone, and a host loop doing the two launches' arithmetic in NumPy.

    python tools/closed_loop_probe.py [--json out.json]

At S = 1 and S = 64 scenes: the tick is a GraphedSampler replay (10-step DDIM, classifier-free guidance, 256x900 frames, H = 16)
with `navigator=` (a plan of 200 points 2 m apart) and `controller=`; `loop` is that call followed by
`KinematicVehicle.step(last_control, hold=metrics.done)` and `DriveMetrics.step(...)` with 8 world discs and 8 boxes per scene,
the body of `simulation.drive`.  The two arms alternate in rounds so that both see the same clocks; the median is the figure.
`vehicle_us` and `metrics_us` are the two launches alone, eager calls back to back between HIP events (which measures the rate
at which the host issues them: no kernel trace is taken).  `host_us` is what a host loop would do in their place at every tick:
one device-to-host copy of the controls, the restatements of the two contracts (tests/vehicle_ref.py, vectorised NumPy;
tests/drive_ref.py, a Python loop over scenes and segments as the reference's criteria are Python loops over actors), and one
host-to-device copy of pose and speed, by the wall clock up to the copies' completion.  The vehicle stands at rest under the timed
loop's controls or moves, as the procedural weights have it: the launches do the same work either way.  A recorded measurement
(profiles/README.md, "Closed loop"), not a threshold: no test asserts a time.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from metrics_probe import SCHED_KW, timed      # noqa: E402  (tools/ is the script's directory)

G, K, DT = 200, 23.315, 0.05      # 398 m of route: at most 20 m/s * 0.05 s * 260 timed ticks = 260 m are driven


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds of (tick, loop); the median is kept")
    ap.add_argument("--iters", type=int, default=5000, help="eager calls per timed window of the two launches alone")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    import drive_ref
    import vehicle_ref
    from autonomous_driving_with_diffusion_model_amd import DeviceController, DeviceNoise, DriveMetrics, KinematicVehicle, Navigator
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
    for scenes in (1, 64):
        rng = np.random.default_rng(scenes)
        heading = rng.uniform(-3, 3, scenes)
        route = np.stack([np.stack([np.cos(h), np.sin(h)]) * (2.0 * np.arange(G))[:, None] for h in heading])        # [S, G, 2]
        pose0 = np.concatenate([route[:, 0], np.arctan2(np.cos(heading), -np.sin(heading))[:, None]], axis=1)
        img = P.synthetic_batch(scenes, 16, image_hw=(256, 900), seed=1)["imgs"].to(dev)
        discs = torch.from_numpy(np.concatenate([route[:, 20:28] + 4.0, np.zeros((scenes, 8, 2)), np.full((scenes, 8, 1), 1.0)], axis=-1)).to(dev)
        boxes = torch.from_numpy(np.concatenate([route[:, 40:48] - 5.0, np.zeros((scenes, 8, 3)), np.full((scenes, 8, 1), 4.0),
                                                 np.full((scenes, 8, 1), 2.0)], axis=-1)).to(dev)

        def stack():
            nav = Navigator(torch.from_numpy(route), torch.zeros(scenes, G, dtype=torch.int32), torch.full((scenes,), G, dtype=torch.int32),
                            xy_scale=K, device=dev)
            sch = S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
            sampler = GraphedSampler(model, sch, cfg, noise=DeviceNoise(3, dev), controller=DeviceController(cfg, scenes, dev), navigator=nav)
            veh = KinematicVehicle(scenes, dev, dt=DT)
            veh.reset(pose0)
            return sampler, veh, DriveMetrics(nav, dt=DT, max_ticks=0, max_time=1e9, offroad_min=1e9, offroad_max=1e9, completion_tol=0.0)

        (s_tick, v_tick, _), (s_loop, v_loop, m_loop) = stack(), stack()

        def tick():
            s_tick(img, pose=v_tick.pose, velocity=v_tick.velocity)

        def loop():
            s_loop(img, pose=v_loop.pose, velocity=v_loop.velocity)
            v_loop.step(s_loop.last_control, hold=m_loop.done)
            m_loop.step(v_loop.pose, v_loop.velocity, v_loop.yaw_rate, discs, boxes)

        iters = 5 if scenes > 1 else 50
        ms = {"tick": [], "loop": []}
        for r in range(args.rounds):
            for name, fn in (("tick", tick), ("loop", loop)) if r % 2 == 0 else (("loop", loop), ("tick", tick)):
                ms[name].append(timed(fn, 2, iters))
        control = s_loop.last_control
        _, veh, met = stack()
        veh.reset(pose0, np.full(scenes, 5.0))
        # the metrics first, on the start pose (no scene ends, so no launch takes the frozen exit); then the vehicle, which drives off
        metrics_us = [round(timed(lambda: met.step(veh.pose, veh.velocity, veh.yaw_rate, discs, boxes), 20, args.iters) * 1e3, 2) for _ in range(3)]
        assert not met.done.any().item()
        vehicle_us = [round(timed(lambda: veh.step(control), 20, args.iters) * 1e3, 2) for _ in range(3)]

        # the host's version of the two launches
        cfg_h = dict(drive_ref.CFG, dt=DT, max_time=1e9, offroad_min=1e9, offroad_max=1e9, completion_tol=0.0)
        cums = [drive_ref.cumulative(route[s]) for s in range(scenes)]
        discs_h, boxes_h = discs.cpu().numpy(), boxes.cpu().numpy()
        state = vehicle_ref.reset(vehicle_ref.fresh_state(scenes), pose0, np.full(scenes, 5.0))
        recs = [drive_ref.step(drive_ref.fresh(), cfg_h, pose0[s], 5.0, 0.0, route[s], G, cums[s]) for s in range(scenes)]

        def host_tick():      # from the same state and the same records every time, so that every repetition does the same work
            c = control.cpu().numpy()
            out = vehicle_ref.step(state, c, dt=DT)
            done = [drive_ref.step(recs[s], cfg_h, out["pose"][s], out["velocity"][s], out["yaw_rate"][s], route[s], G, cums[s], discs_h[s],
                                   boxes_h[s]) for s in range(scenes)]
            assert len(done) == scenes
            back = [torch.from_numpy(out["pose"]).to(dev, non_blocking=True), torch.from_numpy(out["velocity"]).to(dev, non_blocking=True)]
            torch.cuda.synchronize()
            return back

        for _ in range(3):
            host_tick()
        n = 20 if scenes > 1 else 500
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(n):
                host_tick()
            host.append(round((time.perf_counter() - t0) / n * 1e6, 1))
        tick_ms, loop_ms = statistics.median(ms["tick"]), statistics.median(ms["loop"])
        rows.append({"scenes": scenes, "route_points": G, "world_discs": 8, "boxes": 8, "ddim_steps": args.steps, "horizon": 16,
                     "tick_ms": round(tick_ms, 3), "loop_ms": round(loop_ms, 3), "tick_ms_rounds": [round(v, 3) for v in ms["tick"]],
                     "loop_ms_rounds": [round(v, 3) for v in ms["loop"]], "loop_minus_tick_us": round((loop_ms - tick_ms) * 1e3, 1),
                     "vehicle_us": statistics.median(vehicle_us), "vehicle_us_rounds": vehicle_us, "metrics_us": statistics.median(metrics_us),
                     "metrics_us_rounds": metrics_us, "calls_per_round": args.iters, "host_us": statistics.median(host), "host_us_rounds": host,
                     "host_repetitions": n})
        print(json.dumps(rows[-1]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
