"""The device rig of the expert's closed-loop GPU tests: expert_loop_ref.RIG on the device -- the small rig of the closed-loop camera
and traffic tests (S = 2 straight roads of traffic_ref.follow_scenario, 64 x 96 frames, a light 12 m down each road, the queue of
three agents) with a light that is red on arrival and green after 10 s, driven by an `Expert`."""
import torch

import expert_loop_ref as LR
import traffic_ref as TR
from autonomous_driving_with_diffusion_model_amd import (Camera, DeviceController, DriveMetrics, Expert, KinematicVehicle, Navigator, Signals,
                                                         Traffic)
from autonomous_driving_with_diffusion_model_amd.config import create_cfg
from autonomous_driving_with_diffusion_model_amd.simulation import World

DEV = "cuda:0"
S, K, DT = 2, LR.K, LR.DT
SC = TR.follow_scenario()
RED_TICKS = int(round(LR.RIG["red"] / DT))
HW = (64, 96)


class Rig:
    def __init__(self, max_ticks=0, camera=True):
        r = LR.RIG
        rec = Signals.from_lines(SC["line_centre"], SC["heading"], 6.0, 1.0, 20.0, LR.light_timing(r["red"]))[:, None]
        self.signals = Signals(rec, device=DEV, dt=DT, xy_scale=K, planes=r["planes"])
        self.traffic = Traffic(SC["paths"], SC["plen"], LR.queue(), stops=SC["stops"], signals=self.signals, dt=DT, device=DEV)
        self.world = World(signals=self.signals, traffic=self.traffic)
        self.navigator = Navigator(torch.from_numpy(SC["route"]), torch.zeros(S, 60, dtype=torch.int32), torch.full((S,), 60, dtype=torch.int32),
                                   xy_scale=K, points=r["window"], first=0, device=DEV)
        self.controller = DeviceController(create_cfg(), S, DEV)
        e = {k: v for k, v in r["expert"].items() if k not in ("xy_scale", "waypoint_dt", "desired_v")}
        self.expert = Expert(self.navigator, self.controller, horizon=r["horizon"], dim=r["dim"], waypoint_dt=r["waypoint_dt"], world=self.world,
                             desired_speed=r["expert"]["desired_v"], **e)
        self.vehicle = KinematicVehicle(S, DEV, dt=DT)
        self.vehicle.reset(SC["pose"])
        self.metrics = DriveMetrics(self.navigator, dt=DT, max_ticks=max_ticks)
        self.camera = None
        if camera:
            roads, lengths = Camera.roads_from(traffic=self.traffic, navigator=self.navigator)
            self.camera = Camera(S, DEV, width=HW[1], height=HW[0], world=self.world, roads=roads, road_lengths=lengths, lamp_radius=1.5)

    def same(self, other, where):
        def bits(t):
            return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)
        for name, a, b in (("vehicle", self.vehicle.state, other.vehicle.state), ("metrics", self.metrics.words(), other.metrics.words()),
                           ("done", self.metrics.done, other.metrics.done), ("navigator", self.navigator.state, other.navigator.state),
                           ("controller", self.controller.state, other.controller.state), ("signals", self.signals.state, other.signals.state),
                           ("planes", bits(self.signals.planes), bits(other.signals.planes)), ("traffic", self.traffic.state, other.traffic.state),
                           ("boxes", bits(self.traffic.boxes), bits(other.traffic.boxes)), ("plan", bits(self.expert.traj), bits(other.expert.traj)),
                           ("leader", self.expert.leader, other.expert.leader), ("info", bits(self.expert.info), bits(other.expert.info)),
                           ("control", bits(self.expert.last_control), bits(other.expert.last_control))):
            assert torch.equal(a, b), (where, name)
        if self.camera is not None:
            assert torch.equal(self.camera.frames, other.camera.frames), (where, "frames")
