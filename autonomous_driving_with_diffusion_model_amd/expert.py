"""A privileged driver for the closed loop, on the device: it sees the world and not the pixels.

The reference collects its demonstrations with CARLA's autopilot and a Roach expert (misc/data_collect.py); this package rules
the simulator out, so the expert is ours.  `Expert.plan(velocity)` is one launch of `adx_expert_plan`
(csrc/expert.hip, "expert v1" of include/adx.h): for every scene it follows the navigator's window, queues behind whatever is
nearest ahead of it inside its corridor -- a box, a disc, a stop plane of the world's `Signals`, the end of the route -- by the
Intelligent Driver Model of `Traffic`, slows for bends, and rolls the law out into the plan `DeviceController` takes as it is.
The contract has no library call on the way to any word, so the device equals the restatement (tests/expert_ref.py) bit for bit.

`Expert(...)` is a sampler for `drive`: `drive(Expert(navigator, controller, ...), vehicle, metrics, image=camera, world=world)`
drives the loop with it, and `Demonstrations` (demos.py) records such a drive as training samples.  How it differs from a driver
that reads a map is in the contract ("differs"): crossing traffic is not predicted, there are no lane changes and no overtaking,
and the curve limit is evaluated once per launch.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Optional

import torch

from . import _lib as L
from .navigation import EgoFrame, Navigator, _describe, _positive
from .simulation import MAX_SLOTS, World, _nonneg, _no_cpu, _static

MIN_HORIZON, MAX_HORIZON, MIN_DIM, MAX_DIM, MAX_PLANES, INFO_WIDTH = 2, 64, 2, 16, 8, 8
LEADER_NONE, LEADER_DISC, LEADER_PLANE, LEADER_END = -1, 64, 128, 136      # 0..63 a box, 64 + i a disc, 128 + k a plane
INFO = ("s_e", "d_e", "desired", "r", "u", "acc_0", "v_H", "a_H")


class Expert:
    """The privileged drivers of S scenes ("expert v1" of include/adx.h) and the static outputs of `plan`.

    `navigator`: the `Navigator` whose `window` is the path (best built with `first=0`, so that the window covers the segment
    the ego is on) and whose `xy_scale` is the expert's; `controller`: a `DeviceController` (None: `plan` only, no control).
    `horizon` = H (2..64) rows of `dim` = D (2..16) columns, `waypoint_dt` seconds apart -- `DeviceController` reads a plan's
    spacing as metres per 0.5 s.  `world`: a `World` whose `boxes`, `discs` and `signals.planes` are read IN PLACE at every call
    (None: an empty road).  The law's parameters, all metres and seconds: `desired_speed`, `accel`, `brake` (comfortable),
    `brake_max` (the hard cap), `headway` s, `jam` (the standstill gap), `gap_min` (the floor under a gap before it is divided
    by), `corridor_half` (an obstacle counts while its near side is within it of the path), `lat_accel` (the curve limit is
    sqrt(lat_accel / curvature)), `look_min` + speed * `look_time` (how far ahead bends count), `ego_front` (the front bumper
    ahead of the pose), `end_margin` (stop this far short of the route's end).
    All static, the same storage at every call, so a captured graph can hold them:
      `traj`   float32 `[S, H, D]`  the plan in model units: `DeviceController.step`'s `traj`; columns 2.. are 0
      `leader` int32 `[S]`          -1 none, 0..63 box i, 64 + i disc i, 128 + k plane k, 136 the route's end
      `info`   float32 `[S, 8]`     (s_e, d_e, desired, r, u, acc_0, v_H, a_H): why it did what it did
      `boxes_ego` float32 `[S, N, 8]`, `discs_ego` float32 `[S, M, 5]`: the world in this tick's ego frame (None without)
    An object on a CPU device can be built and inspected; its launches refuse (there is no CPU path)."""

    def __init__(self, navigator: Navigator, controller=None, *, horizon: int, dim: int, waypoint_dt: float,
                 world: Optional[World] = None, desired_speed: float = 8.0, accel: float = 1.5, brake: float = 2.0,
                 brake_max: float = 8.0, headway: float = 1.5, jam: float = 2.0, gap_min: float = 0.25, corridor_half: float = 1.75,
                 lat_accel: float = 2.0, look_time: float = 2.0, look_min: float = 10.0, ego_front: float = 2.25,
                 end_margin: float = 1.0):
        if not isinstance(navigator, Navigator):
            raise TypeError(f"Expert: navigator must be a Navigator, got {type(navigator).__name__}")
        if world is not None and not isinstance(world, World):
            raise TypeError(f"Expert: world must be a World, got {type(world).__name__}")
        H, D = int(horizon), int(dim)
        if not MIN_HORIZON <= H <= MAX_HORIZON:
            raise ValueError(f"Expert: horizon must be {MIN_HORIZON}..{MAX_HORIZON}, got {H}")
        if not MIN_DIM <= D <= MAX_DIM:
            raise ValueError(f"Expert: dim must be {MIN_DIM}..{MAX_DIM}, got {D}")
        S, dev = navigator.scenes, navigator.device
        self.navigator, self.controller, self.world = navigator, controller, world
        self.scenes, self.device, self.horizon, self.dim, self.points = S, dev, H, D, navigator.points
        self.xy_scale = navigator.xy_scale
        self.waypoint_dt = _positive(waypoint_dt, "Expert: waypoint_dt")
        for name, v in (("desired_speed", desired_speed), ("accel", accel), ("brake", brake), ("brake_max", brake_max),
                        ("headway", headway), ("jam", jam), ("gap_min", gap_min), ("corridor_half", corridor_half),
                        ("lat_accel", lat_accel), ("look_time", look_time)):
            setattr(self, name, _positive(v, f"Expert: {name}"))
        for name, v in (("look_min", look_min), ("ego_front", ego_front), ("end_margin", end_margin)):
            setattr(self, name, _nonneg(v, f"Expert: {name}"))
        if controller is not None:
            if not hasattr(controller, "step") or getattr(controller, "scenes", S) != S:
                raise ValueError(f"Expert: controller must be a DeviceController of {S} scenes, got {controller!r}")
            if hasattr(controller, "check"):
                controller.check(H, D, True)
        self.n_boxes = self.n_discs = self.n_planes = 0
        if world is not None:
            for name, t in (("boxes", world.boxes), ("discs", world.discs)):
                if t is not None and (t.shape[0] != S or t.device != dev or not 1 <= t.shape[1] <= MAX_SLOTS):
                    raise ValueError(f"Expert: the world's {name} are {_describe(t)}, the navigator holds {S} scenes on {dev}")
            sig = world.signals
            if sig is not None:
                if sig.scenes != S or sig.device != dev:
                    raise ValueError(f"Expert: the world's signals hold {sig.scenes} scenes on {sig.device}, the navigator {S} on {dev}")
                if sig.xy_scale != self.xy_scale:
                    raise ValueError(f"Expert: the signals were built with xy_scale {sig.xy_scale}, the navigator's is {self.xy_scale}")
                self.n_planes = int(sig.planes.shape[1])
                if not 1 <= self.n_planes <= MAX_PLANES:
                    raise ValueError(f"Expert: the signals emit {self.n_planes} planes, supported 1..{MAX_PLANES}")
            self.n_boxes = 0 if world.boxes is None else int(world.boxes.shape[1])
            self.n_discs = 0 if world.discs is None else int(world.discs.shape[1])
        # `drive` asks its sampler for the model's xy scale when it is given a world
        self.model = SimpleNamespace(magic_num=self.xy_scale)
        self.traj = torch.zeros((S, H, D), dtype=torch.float32, device=dev)
        self.leader = torch.full((S,), LEADER_NONE, dtype=torch.int32, device=dev)
        self.info = torch.zeros((S, INFO_WIDTH), dtype=torch.float32, device=dev)
        self.boxes_ego = torch.zeros((S, self.n_boxes, 8), dtype=torch.float32, device=dev) if self.n_boxes else None
        self.discs_ego = torch.zeros((S, self.n_discs, 5), dtype=torch.float32, device=dev) if self.n_discs else None
        self.last_control = None
        self._cfg = L.ExpertCfg(S, self.points, self.n_boxes, self.n_discs, self.n_planes, H, D, 0, self.xy_scale, self.waypoint_dt,
                                self.desired_speed, self.accel, self.brake, self.brake_max, self.headway, self.jam, self.gap_min,
                                self.corridor_half, self.lat_accel, self.look_time, self.ego_front, self.end_margin, self.look_min)

    @property
    def planes(self) -> Optional[torch.Tensor]:
        """The world's stop planes, float32 `[S, K, 3]`, read in place (None without signals)."""
        return None if self.world is None or self.world.signals is None else self.world.signals.planes

    def key(self) -> tuple:
        """What a captured launch bakes in."""
        return (self.scenes, self.points, self.n_boxes, self.n_discs, self.n_planes, self.horizon, self.dim, self.xy_scale,
                self.waypoint_dt, self.desired_speed, self.accel, self.brake, self.brake_max, self.headway, self.jam, self.gap_min,
                self.corridor_half, self.lat_accel, self.look_time, self.look_min, self.ego_front, self.end_margin,
                self.navigator.window.data_ptr(), L.ptr(self.boxes_ego), L.ptr(self.discs_ego), L.ptr(self.planes),
                L.ptr(None if self.world is None else self.world.boxes), L.ptr(None if self.world is None else self.world.discs),
                self.traj.data_ptr(), self.leader.data_ptr(), self.info.data_ptr(),
                None if self.controller is None or not hasattr(self.controller, "key") else self.controller.key())

    def plan(self, velocity: torch.Tensor) -> torch.Tensor:
        """ONE launch on the current stream, no allocation, no synchronisation: `velocity` float32 `[S]` m/s (a
        `KinematicVehicle`'s static output).  It reads the navigator's `window`, `boxes_ego`, `discs_ego` and the signals'
        planes as they stand and writes `traj`, `leader` and `info`.  Returns `traj`."""
        S, dev = self.scenes, self.device
        _static(velocity, (S,), torch.float32, dev, "Expert: velocity")
        _no_cpu(dev, "the expert")
        planes = self.planes
        if (0 if planes is None else int(planes.shape[1])) != self.n_planes:
            raise ValueError("Expert: the world's signals changed shape since the expert was built")
        L.check(L.lazy("adx_expert_plan")(C.byref(self._cfg), self.navigator.window.data_ptr(), velocity.data_ptr(), L.ptr(self.boxes_ego),
                                          L.ptr(self.discs_ego), L.ptr(planes), self.traj.data_ptr(), self.leader.data_ptr(),
                                          self.info.data_ptr(), L.stream_ptr(dev)), "adx_expert_plan")
        return self.traj

    def __call__(self, image=None, *, pose: torch.Tensor, velocity: torch.Tensor, guide=None, pin=None) -> torch.Tensor:
        """What `drive` calls, once per tick: step the navigator on `pose`, put the world's boxes and discs into this tick's ego
        frame (`EgoFrame(pose, xy_scale, waypoint_dt)`, into the static `boxes_ego` and `discs_ego`), read the signals' planes in
        place, launch, and run `controller.step(traj, velocity, navigator.target)`.  Sets `last_control` and returns `traj`.
        `image`, `guide` and `pin` are IGNORED: the expert is privileged -- it reads the world itself, not the pixels, and
        nothing steers or pins its plan.  No allocation beyond the controller's `[S, 3]` result and no synchronisation, so the
        whole call is capturable."""
        S, dev, w = self.scenes, self.device, self.world
        _static(pose, (S, 3), torch.float64, dev, "Expert: pose")
        _static(velocity, (S,), torch.float32, dev, "Expert: velocity")
        _no_cpu(dev, "the expert")
        self.navigator.step(pose)
        if self.n_boxes or self.n_discs:
            if (0 if w.boxes is None else int(w.boxes.shape[1])) != self.n_boxes or \
                    (0 if w.discs is None else int(w.discs.shape[1])) != self.n_discs:
                raise ValueError("Expert: the world's boxes or discs changed shape since the expert was built")
            frame = EgoFrame(pose, self.xy_scale, self.waypoint_dt)
            if self.n_boxes:
                frame.boxes(w.boxes, out=self.boxes_ego)
            if self.n_discs:
                frame.discs(w.discs, out=self.discs_ego)
        self.plan(velocity)
        if self.controller is not None:
            self.last_control = self.controller.step(self.traj, velocity, self.navigator.target, xy_scale=self.xy_scale)
        return self.traj

    def compute(self) -> dict:
        """ONE device read: `leader` int32 `[S]` and the columns of `info` by name, NumPy arrays."""
        packed = torch.cat([self.info, self.leader.view(torch.float32)[:, None]], dim=1).cpu().numpy()
        out = {n: packed[:, i].copy() for i, n in enumerate(INFO)}
        out["leader"] = packed[:, INFO_WIDTH].copy().view("int32")
        return out

    def __repr__(self):
        return (f"Expert(scenes={self.scenes}, window={self.points}, boxes={self.n_boxes}, discs={self.n_discs}, planes={self.n_planes}, "
                f"horizon={self.horizon}, dim={self.dim}, waypoint_dt={self.waypoint_dt}, desired_speed={self.desired_speed}, "
                f"device={self.device})")
