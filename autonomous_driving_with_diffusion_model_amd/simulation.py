"""The smallest honest closed loop, on the device: a kinematic vehicle that takes a tick's controls to the next pose, the
closed-loop criteria of a drive, and the runner that strings navigator, tick, vehicle and metrics together.

The reference closes its loop through CARLA and scores a drive with CARLA's criteria (carla_gym/core/task_actor/common/criteria);
this package rules the simulator out.  What is here instead:

`KinematicVehicle.step(control)` is one launch of `adx_vehicle_step` (csrc/vehicle.hip, "vehicle v1" of include/adx.h): a
kinematic bicycle in fp64 for S scenes, whose static `pose` is the float64 `[S, 3]` buffer `Navigator.step` and `EgoFrame` read and
whose static `velocity` is the float32 `[S]` buffer `DeviceController.step` and `GraphedSampler(velocity=)` read.

`DriveMetrics.step(pose, velocity, yaw_rate, discs, boxes)` is one launch of `adx_drive_step` (csrc/drive.hip, "drive metrics
v1"): progress along the route and cross-track error, collisions of the ego's discs with world discs and boxes, the reference's
RouteDeviation and Blocked, comfort, the odometer and `done` per scene, all in one device record per scene; `compute()` is the one
device read.

`World(discs, boxes, signals, traffic)` holds what else is on the road; its `signals` (signals.py: traffic lights and stop signs,
"signals v1") are stepped by `drive` once per tick, bind the plans through the default guide's planes and score the reference's
RunRedLight and RunStopSign; its `traffic` (traffic.py: car-following agents, "traffic v1") is stepped after them, and its boxes
are the world's boxes.

`drive(sampler, vehicle, metrics, ticks=, image=)` runs the loop without a host synchronisation.  THE LOOP IS BLIND UNLESS `image=`
IS A `Camera` (camera.py): otherwise the images are whatever the caller supplies (one tensor for every tick, or a callable of the
tick and the pose) and do not show what the vehicle would see.  What the loop does exercise is everything behind the camera:
target conditioning, the
guide, pins, selection, commit, fallback, control and the navigator, tick after tick on the poses their own output produced.
Whether a number it reports says anything about driving in a town is a property of weights -- a `Camera`'s frames are
flat-shaded geometry, not a town -- and is not measurable in this repository.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Optional, Union

import numpy as np
import torch

from . import _lib as L
from .guide import MAX_CAPSULES, Capsules, Guide
from .navigation import MAX_POINTS, MAX_SCENES, EgoFrame, Navigator, _describe, _device, _positive

STEER_SIGN = 1              # tests/test_sim_cpu.py decides it: the host Controller with sign_x = -1 converges onto an offset route
MAX_SUBSTEPS = 16
MAX_SLOTS = 64              # world discs and boxes per scene
MAX_EGO_DISCS = 4
VEHICLE_WORDS, DRIVE_WORDS = 10, 48
DONE = ("running", "completed", "collision", "off_route", "blocked", "timeout")
_DRIVE_INTS = ("cursor", "ticks", "done", "flags", "contact", "events", "contact_ticks", "first_tick", "first_slot", "have")
_DRIVE_F64 = ("px", "py", "v_prev", "a_prev", "progress", "progress_max", "xtrack", "xtrack_max", "xtrack_sum", "xtrack_sq", "distance",
              "offroad", "stall", "acc_max", "acc_sq", "jerk_max", "jerk_sq", "lat_max", "lat_sq")


def _nonneg(v, what: str) -> float:
    v = float(v)
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"{what} must be finite and >= 0, got {v}")
    return v


def _no_cpu(device, who: str) -> None:
    if device.type != "cuda":
        raise L.AdxError(f"{who} lives on {device}; the adx kernels only run on an MI355X (there is no CPU path)")


def _mask(mask, scenes: int, device) -> Optional[torch.Tensor]:
    if mask is None:
        return None
    if not torch.is_tensor(mask) or tuple(mask.shape) != (scenes,) or mask.device != device or mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"mask must be [{scenes}] bool or uint8 on {device}, got {_describe(mask)}")
    return mask.contiguous().view(torch.uint8)


def _static(t, shape, dtype, device, what: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != device or not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous {dtype} {list(shape)} on {device}, got {_describe(t)}")
    return t


class KinematicVehicle:
    """S kinematic bicycles on `device` ("vehicle v1" of include/adx.h) and the static outputs of `step`.

    `dt`: the seconds of one step (one tick); `substeps` (1..16) semi-implicit Euler sub-steps of dt / substeps; `wheelbase` m,
    `accel_max` and `brake_max` m/s^2 at full pedal, `drag` 1/s, `roll` m/s^2 (while moving), `v_max` m/s, `steer_max` rad at steer
    = +-1 (below 1.5), `steer_sign` +1 or -1: +1 is the sign under which control v1 with the callers' `sign_x = -1` steers onto
    its route.  All static, the same storage at every step, so a captured graph, a navigator and a controller can hold them:
      `pose` float64 `[S, 3]`   (x, y, compass): `Navigator.step`'s and `EgoFrame`'s pose
      `velocity` float32 `[S]`  `DeviceController.step`'s and `GraphedSampler(velocity=)`'s speed
      `yaw_rate` float32 `[S]`  rad/s over the step
      `state` int32 `[S, 10]`   the contract's record: fp64 x, y, compass, speed, then `valid` and a zero
    An object on a CPU device can be built and inspected; its launches refuse (there is no CPU path)."""

    def __init__(self, scenes: int, device, *, dt: float, substeps: int = 4, wheelbase: float = 2.9, accel_max: float = 3.0,
                 brake_max: float = 8.0, drag: float = 0.05, roll: float = 0.1, v_max: float = 20.0, steer_max: float = 0.6,
                 steer_sign: int = STEER_SIGN):
        scenes, substeps = int(scenes), int(substeps)
        if not 1 <= scenes <= MAX_SCENES:
            raise ValueError(f"KinematicVehicle: scenes must be 1..{MAX_SCENES}, got {scenes}")
        if not 1 <= substeps <= MAX_SUBSTEPS:
            raise ValueError(f"KinematicVehicle: substeps must be 1..{MAX_SUBSTEPS}, got {substeps}")
        if steer_sign not in (1, -1):
            raise ValueError(f"KinematicVehicle: steer_sign must be +1 or -1, got {steer_sign!r}")
        self.dt = _positive(dt, "KinematicVehicle: dt")
        self.wheelbase = _positive(wheelbase, "KinematicVehicle: wheelbase")
        self.accel_max = _positive(accel_max, "KinematicVehicle: accel_max")
        self.brake_max = _positive(brake_max, "KinematicVehicle: brake_max")
        self.v_max = _positive(v_max, "KinematicVehicle: v_max")
        self.drag = _nonneg(drag, "KinematicVehicle: drag")
        self.roll = _nonneg(roll, "KinematicVehicle: roll")
        self.steer_max = float(steer_max)
        if not 0.0 < self.steer_max < 1.5:
            raise ValueError(f"KinematicVehicle: steer_max must lie in (0, 1.5) radians, got {self.steer_max}")
        self.scenes, self.substeps, self.steer_sign, self.device = scenes, substeps, int(steer_sign), _device(device)
        nbytes = int(L.lazy("adx_vehicle_state_bytes")(scenes))
        if nbytes != scenes * 4 * VEHICLE_WORDS:
            raise L.AdxError(f"adx_vehicle_state_bytes({scenes}) = {nbytes}: not the state of vehicle v1")
        dev = self.device
        self.state = torch.zeros((scenes, VEHICLE_WORDS), dtype=torch.int32, device=dev)
        self.pose = torch.zeros((scenes, 3), dtype=torch.float64, device=dev)
        self.velocity = torch.zeros((scenes,), dtype=torch.float32, device=dev)
        self.yaw_rate = torch.zeros((scenes,), dtype=torch.float32, device=dev)
        self._cfg = L.VehicleCfg(scenes, substeps, self.steer_sign, 0, self.dt, self.wheelbase, self.accel_max, self.brake_max,
                                 self.drag, self.roll, self.v_max, self.steer_max)

    def key(self) -> tuple:
        """What a captured launch bakes in."""
        return (self.scenes, self.substeps, self.steer_sign, self.dt, self.wheelbase, self.accel_max, self.brake_max, self.drag,
                self.roll, self.v_max, self.steer_max, self.state.data_ptr())

    # ---- views of the state ---------------------------------------------------------------------------------------------------
    @property
    def valid(self) -> torch.Tensor:
        """[S] int32, a view: not 0 once a scene's vehicle has been placed or stepped."""
        return self.state[:, 8]

    @property
    def speed(self) -> torch.Tensor:
        """[S] float64, a view: the speed the next step starts from."""
        return self.state.view(torch.float64)[:, 3]

    def step(self, control: torch.Tensor, hold: Optional[torch.Tensor] = None) -> "KinematicVehicle":
        """One launch on the current stream, no allocation, no synchronisation: `control` float32 `[S, 3]` = (throttle, steer,
        brake) on the device (`DeviceController.step`'s result, `GraphedSampler.last_control`); `hold` int32 `[S]` or None: where it
        is not 0 the scene stands still (`DriveMetrics.done`).  `pose`, `velocity`, `yaw_rate` and the state hold the new values."""
        S, dev = self.scenes, self.device
        if not torch.is_tensor(control):
            raise TypeError(f"KinematicVehicle: control must be a tensor, got {type(control).__name__}")
        if control.dtype != torch.float32:
            raise TypeError(f"KinematicVehicle: control must be float32, got {control.dtype}")
        if tuple(control.shape) != (S, 3):
            raise ValueError(f"KinematicVehicle: control must be [{S}, 3] = (throttle, steer, brake), got {tuple(control.shape)}")
        if hold is not None:
            if not torch.is_tensor(hold) or hold.dtype != torch.int32 or tuple(hold.shape) != (S,):
                raise ValueError(f"KinematicVehicle: hold must be int32 [{S}], got {_describe(hold)}")
        _no_cpu(dev, "the vehicle")
        for name, t in (("control", control), ("hold", hold)):
            if t is not None and t.device != dev:
                raise ValueError(f"KinematicVehicle: {name} lives on {t.device}, the vehicle on {dev}")
        control = control.contiguous()
        hold = None if hold is None else hold.contiguous()
        L.check(L.lazy("adx_vehicle_step")(C.byref(self._cfg), control.data_ptr(), L.ptr(hold), self.state.data_ptr(), self.pose.data_ptr(),
                                           self.velocity.data_ptr(), self.yaw_rate.data_ptr(), L.stream_ptr(dev)), "adx_vehicle_step")
        return self

    def reset(self, pose=None, speed=None, mask: Optional[torch.Tensor] = None) -> None:
        """Place every vehicle, or those where `mask` [S] (bool or uint8, on the device) is set, at `pose` `[S, 3]` = (x, y,
        compass) with `speed` `[S]` m/s (None: at rest); float64 device tensors are read in place, host values (CPU tensors or
        nested sequences) are copied first.  `pose=None`: back to the all-zero state.  The static `pose`, `velocity` and `yaw_rate`
        of those scenes show the new values at once, so a navigator can take the start pose.  One launch, capturable with device
        arguments."""
        S, dev = self.scenes, self.device
        if pose is None and speed is not None:
            raise ValueError("KinematicVehicle.reset: a speed needs a pose")
        args = []
        for name, v, shape in (("pose", pose, (S, 3)), ("speed", speed, (S,))):
            if v is None:
                args.append(None)
                continue
            if torch.is_tensor(v) and v.is_cuda:
                args.append(_static(v, shape, torch.float64, dev, f"KinematicVehicle.reset: {name}"))
            else:
                host = torch.as_tensor(v, dtype=torch.float64)
                if tuple(host.shape) != shape:
                    raise ValueError(f"KinematicVehicle.reset: {name} must be {list(shape)}, got {tuple(host.shape)}")
                args.append(host)
        mask = _mask(mask, S, dev)
        _no_cpu(dev, "the vehicle")
        pose_d, speed_d = (None if v is None else v.to(dev) for v in args)
        L.check(L.lazy("adx_vehicle_reset")(self.state.data_ptr(), S, L.ptr(pose_d), L.ptr(speed_d), L.ptr(mask), self.pose.data_ptr(),
                                            self.velocity.data_ptr(), self.yaw_rate.data_ptr(), L.stream_ptr(dev)), "adx_vehicle_reset")

    def state_snapshot(self) -> torch.Tensor:
        return self.state.clone()

    def state_restore(self, snapshot: torch.Tensor) -> None:
        if not torch.is_tensor(snapshot) or snapshot.shape != self.state.shape or snapshot.dtype != self.state.dtype:
            raise ValueError("state_restore: not a snapshot of this KinematicVehicle")
        self.state.copy_(snapshot)

    def __repr__(self):
        return (f"KinematicVehicle(scenes={self.scenes}, dt={self.dt}, substeps={self.substeps}, wheelbase={self.wheelbase}, "
                f"v_max={self.v_max}, steer_max={self.steer_max}, steer_sign={self.steer_sign:+d}, device={self.device})")


class World:
    """The other road users of a closed loop, in `EgoFrame`'s world formats on the device: `discs` float64 `[S, M, 5]` = (cx, cy,
    vx, vy, r) and / or `boxes` float64 `[S, N, 7]` = (cx, cy, vx, vy, yaw, length, width), M, N in 1..64 (None: none); a radius
    or size <= 0 or NaN marks an empty slot.  `advance(dt)` moves every centre by its velocity, in place, with plain torch ops.
    `signals`: the scenes' traffic lights and stop signs (a `Signals`, signals.py; None: none), which `drive` steps once per tick:
    their stop lines join the default guide as planes, and their record scores red lights and stop signs run.
    `traffic`: the scenes' reactive road users (a `Traffic`, traffic.py; None: none), which `drive` steps once per tick after the
    signals: `boxes` must then be None, `world.boxes` is `traffic.boxes` and `advance` leaves them alone (discs still advance)."""

    def __init__(self, discs: Optional[torch.Tensor] = None, boxes: Optional[torch.Tensor] = None, signals=None, traffic=None):
        for name, t, w in (("discs", discs, 5), ("boxes", boxes, 7)):
            if t is None:
                continue
            if not torch.is_tensor(t) or t.dtype != torch.float64 or t.dim() != 3 or t.shape[2] != w or not 1 <= t.shape[1] <= MAX_SLOTS \
                    or not t.is_contiguous():
                raise ValueError(f"World: {name} must be contiguous float64 [S, 1..{MAX_SLOTS}, {w}], got {_describe(t)}")
        if discs is not None and boxes is not None and (discs.shape[0] != boxes.shape[0] or discs.device != boxes.device):
            raise ValueError(f"World: discs are {_describe(discs)}, boxes {_describe(boxes)}: one scene count, one device")
        if signals is not None:
            from .signals import Signals
            if not isinstance(signals, Signals):
                raise TypeError(f"World: signals must be a Signals, got {type(signals).__name__}")
            for name, t in (("discs", discs), ("boxes", boxes)):
                if t is not None and (t.shape[0] != signals.scenes or t.device != signals.device):
                    raise ValueError(f"World: {name} are {_describe(t)}, the signals hold {signals.scenes} scenes on {signals.device}: "
                                     f"one scene count, one device")
        if traffic is not None:
            from .traffic import Traffic
            if not isinstance(traffic, Traffic):
                raise TypeError(f"World: traffic must be a Traffic, got {type(traffic).__name__}")
            if boxes is not None:
                raise ValueError("World: with traffic= the boxes are the traffic's; boxes must be None")
            if discs is not None and (discs.shape[0] != traffic.scenes or discs.device != traffic.device):
                raise ValueError(f"World: discs are {_describe(discs)}, the traffic holds {traffic.scenes} scenes on {traffic.device}: "
                                 f"one scene count, one device")
            if signals is not None and (signals.scenes != traffic.scenes or signals.device != traffic.device):
                raise ValueError(f"World: the signals hold {signals.scenes} scenes on {signals.device}, the traffic {traffic.scenes} on "
                                 f"{traffic.device}: one scene count, one device")
            if traffic.signals is not None and traffic.signals is not signals:
                raise ValueError("World: the traffic reads the phases of another Signals than the world's signals=")
            boxes = traffic.boxes
        self.discs, self.boxes, self.signals, self.traffic = discs, boxes, signals, traffic

    def advance(self, dt: float) -> None:
        for t in (self.discs, None if self.traffic is not None else self.boxes):
            if t is not None:
                t[..., 0:2].add_(t[..., 2:4], alpha=float(dt))


class DriveMetrics:
    """The closed-loop criteria of S drives on the device ("drive metrics v1" of include/adx.h).

    `navigator_or_route`: a `Navigator` (its `route_m` and `lengths` buffers are shared, not copied) or a float64 `[S, G, 2]` route
    in world metres with `lengths=` int32 `[S]` and `device=`.  The cumulative arclength `[S, G]` is summed sequentially on the
    host once, here (`refresh_route()` again after a `Navigator.set_route`).  `dt`: the seconds of a tick.  `window`: how many
    segments from the cursor on the nearest point is looked for in (it keeps the cursor from jumping to a far leg of a route that
    doubles back).  The ego is `len(offsets)` (1..4) discs of radius `r_ego` m at `offsets` m along its heading.  `offroad_min`,
    `offroad_max`, `max_route_percentage`: the reference's RouteDeviation; `speed_threshold`, `max_time`: its Blocked;
    `completion_tol` m; `stop_on_collision`; `max_ticks` (0: no timeout); `collision_penalty`: `compute()`'s score factor per event.

    `done` int32 `[S]` is static (0 running, 1 completed, 2 collision, 3 off route, 4 blocked, 5 timeout): a vehicle's `hold`;
    a scene whose `done` is set is frozen.  `state` is the int32 `[S, 48]` record."""

    def __init__(self, navigator_or_route: Union[Navigator, torch.Tensor], *, dt: float, lengths: Optional[torch.Tensor] = None,
                 device=None, window: int = 32, r_ego: float = 1.0, offsets=(0.0,), offroad_min: float = 15.0, offroad_max: float = 30.0,
                 max_route_percentage: float = 0.3, speed_threshold: float = 0.1, max_time: float = 90.0, completion_tol: float = 1.0,
                 stop_on_collision: bool = False, max_ticks: int = 0, collision_penalty: float = 0.6):
        if isinstance(navigator_or_route, Navigator):
            if lengths is not None or device is not None:
                raise ValueError("DriveMetrics: a Navigator brings its own lengths and device")
            nav = navigator_or_route
            self.route_m, self.lengths, self.device = nav.route_m, nav.lengths, nav.device
        else:
            route = navigator_or_route
            if not torch.is_tensor(route) or not torch.is_tensor(lengths):
                raise TypeError(f"DriveMetrics: a Navigator, or a route tensor with lengths=, got {type(route).__name__} and "
                                f"{type(lengths).__name__}")
            if route.dtype != torch.float64 or lengths.dtype != torch.int32:
                raise TypeError(f"DriveMetrics: the route must be float64 and lengths int32, got {route.dtype} and {lengths.dtype}")
            if route.dim() != 3 or route.shape[2] != 2 or not 1 <= route.shape[0] <= MAX_SCENES or not 1 <= route.shape[1] <= MAX_POINTS:
                raise ValueError(f"DriveMetrics: the route must be [S, G, 2] world metres with S <= {MAX_SCENES} and G <= {MAX_POINTS}, "
                                 f"got {tuple(route.shape)}")
            if tuple(lengths.shape) != (route.shape[0],):
                raise ValueError(f"DriveMetrics: lengths must be [{route.shape[0]}], got {tuple(lengths.shape)}")
            lens = lengths.detach().cpu()
            if int(lens.min()) < 1 or int(lens.max()) > route.shape[1]:
                raise ValueError(f"DriveMetrics: lengths must lie in 1..{route.shape[1]} (G), got {lens.tolist()}")
            if device is None:
                raise ValueError("DriveMetrics: a route tensor needs device=")
            self.device = _device(device)
            self.route_m = route.detach().to(self.device).contiguous().clone()
            self.lengths = lengths.detach().to(self.device).contiguous().clone()
        S, G = int(self.route_m.shape[0]), int(self.route_m.shape[1])
        self.scenes, self.max_points = S, G
        self.dt = _positive(dt, "DriveMetrics: dt")
        self.window = int(window)
        if not 1 <= self.window <= MAX_POINTS:
            raise ValueError(f"DriveMetrics: window must be 1..{MAX_POINTS}, got {self.window}")
        self.offsets = tuple(float(o) for o in offsets)
        if not 1 <= len(self.offsets) <= MAX_EGO_DISCS or not all(math.isfinite(o) for o in self.offsets):
            raise ValueError(f"DriveMetrics: offsets must be 1..{MAX_EGO_DISCS} finite values, got {offsets!r}")
        self.r_ego = _nonneg(r_ego, "DriveMetrics: r_ego")
        self.offroad_min = _nonneg(offroad_min, "DriveMetrics: offroad_min")
        self.offroad_max = _nonneg(offroad_max, "DriveMetrics: offroad_max")
        self.max_route_percentage = _nonneg(max_route_percentage, "DriveMetrics: max_route_percentage")
        self.speed_threshold = _nonneg(speed_threshold, "DriveMetrics: speed_threshold")
        self.max_time = _nonneg(max_time, "DriveMetrics: max_time")
        self.completion_tol = _nonneg(completion_tol, "DriveMetrics: completion_tol")
        self.stop_on_collision, self.max_ticks = bool(stop_on_collision), int(max_ticks)
        if self.max_ticks < 0:
            raise ValueError(f"DriveMetrics: max_ticks must be >= 0 (0: no timeout), got {self.max_ticks}")
        self.collision_penalty = float(collision_penalty)
        if not 0.0 <= self.collision_penalty <= 1.0:
            raise ValueError(f"DriveMetrics: collision_penalty must lie in 0..1, got {self.collision_penalty}")
        nbytes = int(L.lazy("adx_drive_state_bytes")(S))
        if nbytes != S * 4 * DRIVE_WORDS:
            raise L.AdxError(f"adx_drive_state_bytes({S}) = {nbytes}: not the state of drive metrics v1")
        dev = self.device
        self.state = torch.zeros((S, DRIVE_WORDS), dtype=torch.int32, device=dev)
        self.done = torch.zeros((S,), dtype=torch.int32, device=dev)
        self.cum = torch.zeros((S, G), dtype=torch.float64, device=dev)
        self.refresh_route()

    def refresh_route(self) -> None:
        """The cumulative arclength of the route buffers as they are now: cum[0] = 0, cum[i] = cum[i-1] + |p[i] - p[i-1]|, the
        sequential sum in index order (one device read, one copy)."""
        r = self.route_m.detach().cpu().numpy()
        d = r[:, 1:] - r[:, :-1]
        xx, yy = d[..., 0] * d[..., 0], d[..., 1] * d[..., 1]
        cum = np.zeros(r.shape[:2], dtype=np.float64)
        cum[:, 1:] = np.cumsum(np.sqrt(xx + yy), axis=1)      # cumsum adds in index order
        self.cum.copy_(torch.from_numpy(cum))

    def _cfg(self, M: int, N: int) -> L.DriveCfg:
        off = (C.c_double * 4)(*(self.offsets + (0.0,) * (4 - len(self.offsets))))
        return L.DriveCfg(self.scenes, self.max_points, self.window, M, N, len(self.offsets), int(self.stop_on_collision), self.max_ticks,
                          self.dt, self.r_ego, off, self.offroad_min, self.offroad_max, self.max_route_percentage,
                          self.speed_threshold, self.max_time, self.completion_tol)

    def step(self, pose: torch.Tensor, velocity: torch.Tensor, yaw_rate: torch.Tensor, discs: Optional[torch.Tensor] = None,
             boxes: Optional[torch.Tensor] = None) -> "DriveMetrics":
        """One launch on the current stream, no allocation, no synchronisation: `pose` float64 `[S, 3]`, `velocity` and `yaw_rate`
        float32 `[S]` (a `KinematicVehicle`'s static outputs, or a simulator's or a log's), `discs` float64 `[S, M, 5]` and `boxes`
        float64 `[S, N, 7]` in world metres as of this tick (M, N in 1..64; None: none).  Every running scene's record moves on by
        one tick and `done` holds the verdicts."""
        S, dev = self.scenes, self.device
        _static(pose, (S, 3), torch.float64, dev, "DriveMetrics: pose")
        _static(velocity, (S,), torch.float32, dev, "DriveMetrics: velocity")
        _static(yaw_rate, (S,), torch.float32, dev, "DriveMetrics: yaw_rate")
        counts = []
        for name, t, w in (("discs", discs, 5), ("boxes", boxes, 7)):
            if t is None:
                counts.append(0)
                continue
            if not torch.is_tensor(t) or t.dtype != torch.float64 or t.dim() != 3 or t.shape[0] != S or t.shape[2] != w or \
                    not 1 <= t.shape[1] <= MAX_SLOTS or t.device != dev or not t.is_contiguous():
                raise ValueError(f"DriveMetrics: {name} must be contiguous float64 [{S}, 1..{MAX_SLOTS}, {w}] on {dev}, got {_describe(t)}")
            counts.append(int(t.shape[1]))
        _no_cpu(dev, "the drive record")
        cfg = self._cfg(*counts)
        L.check(L.lazy("adx_drive_step")(C.byref(cfg), pose.data_ptr(), velocity.data_ptr(), yaw_rate.data_ptr(), self.route_m.data_ptr(),
                                         self.lengths.data_ptr(), self.cum.data_ptr(), L.ptr(discs), L.ptr(boxes), self.state.data_ptr(),
                                         self.done.data_ptr(), L.stream_ptr(dev)), "adx_drive_step")
        return self

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """A drive not yet begun for every scene, or for the scenes where `mask` [S] (bool or uint8, on the device) is set; their
        `done` becomes 0.  One launch on the current stream, capturable."""
        mask = _mask(mask, self.scenes, self.device)
        _no_cpu(self.device, "the drive record")
        L.check(L.lazy("adx_drive_reset")(self.state.data_ptr(), self.scenes, L.ptr(mask), self.done.data_ptr(), L.stream_ptr(self.device)),
                "adx_drive_reset")

    def words(self) -> torch.Tensor:
        """A clone of the int32 `[S, 48]` record (on the device, no synchronisation)."""
        return self.state.clone()

    @staticmethod
    def fields(words) -> dict:
        """The contract's named fields of a host copy of `words()`: int32 `[S]` and float64 `[S]` NumPy arrays."""
        w = np.ascontiguousarray(words.detach().cpu().numpy() if torch.is_tensor(words) else words, dtype=np.int32)
        f = w.view(np.float64)
        out = {n: w[:, i].copy() for i, n in enumerate(_DRIVE_INTS)}
        out.update({n: f[:, len(_DRIVE_INTS) // 2 + i].copy() for i, n in enumerate(_DRIVE_F64)})
        return out

    def compute(self) -> dict:
        """ONE device read (the records, the route lengths and the cumulative arclength's last column), then host arithmetic.
        Per scene NumPy arrays `[S]`: `done`, `ticks`, `time` s, `distance` m, `route_length` m, `completion` in 0..1, `events`,
        `collisions_per_km`, `contact_ticks`, `first_tick`, `first_slot`, `xtrack_mean`, `xtrack_rms`, `xtrack_max`, `off_route`,
        `blocked`, `timeout`, `completed` (bool: that condition held when the scene ended), `acc_max`, `acc_rms`, `jerk_max`,
        `jerk_rms`, `lat_max`, `lat_rms`, `score` = completion * collision_penalty ** events; and floats `mean_completion`,
        `mean_score`, `mean_collisions_per_km`."""
        S = self.scenes
        length = self.cum.gather(1, (self.lengths.clamp(1, self.max_points) - 1).to(torch.int64)[:, None])[:, 0]
        packed = torch.cat([self.state.view(torch.float64).reshape(-1), length]).cpu().numpy()      # the one read
        f = self.fields(packed[:S * DRIVE_WORDS // 2].view(np.int32).reshape(S, DRIVE_WORDS))
        length = packed[S * DRIVE_WORDS // 2:]
        ticks = f["ticks"].astype(np.float64)
        n = np.maximum(ticks, 1.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            completion = np.where(length > 0.0, np.clip(f["progress_max"] / length, 0.0, 1.0), (ticks > 0).astype(np.float64))
            per_km = np.where(f["distance"] > 0.0, f["events"] / (f["distance"] / 1000.0), 0.0)
        out = dict(done=f["done"], ticks=f["ticks"], time=ticks * self.dt, distance=f["distance"], route_length=length,
                   completion=completion, events=f["events"], collisions_per_km=per_km, contact_ticks=f["contact_ticks"],
                   first_tick=f["first_tick"], first_slot=f["first_slot"], xtrack_mean=f["xtrack_sum"] / n,
                   xtrack_rms=np.sqrt(f["xtrack_sq"] / n), xtrack_max=f["xtrack_max"],
                   completed=(f["flags"] & 1) != 0, off_route=(f["flags"] & 4) != 0, blocked=(f["flags"] & 8) != 0,
                   timeout=(f["flags"] & 16) != 0,
                   acc_max=f["acc_max"], acc_rms=np.sqrt(f["acc_sq"] / np.maximum(ticks - 1.0, 1.0)),
                   jerk_max=f["jerk_max"], jerk_rms=np.sqrt(f["jerk_sq"] / np.maximum(ticks - 2.0, 1.0)),
                   lat_max=f["lat_max"], lat_rms=np.sqrt(f["lat_sq"] / n))
        out["score"] = completion * self.collision_penalty ** f["events"].astype(np.float64)
        out["mean_completion"] = float(completion.mean())
        out["mean_score"] = float(out["score"].mean())
        out["mean_collisions_per_km"] = float(per_km.mean())
        return out

    def __repr__(self):
        return (f"DriveMetrics(scenes={self.scenes}, max_points={self.max_points}, dt={self.dt}, window={self.window}, "
                f"ego={len(self.offsets)} x r {self.r_ego}, device={self.device})")


class EagerTick:
    """`generate_traj(model, scheduler, cfg, image, navigator=, controller=, ...)` as a sampler `drive` can call: the call takes
    what `GraphedSampler.__call__` takes (`pose`, `velocity`, `guide`, `pin`) and `last_control` is the tick's control."""

    def __init__(self, model, scheduler, cfg, *, navigator: Navigator, controller, **tick_kwargs):
        self.model, self.scheduler, self.cfg, self.navigator, self.controller = model, scheduler, cfg, navigator, controller
        self.tick_kwargs = tick_kwargs
        self.last_control = None

    def __call__(self, image, *, pose, velocity, guide=None, pin=None):
        from .sampling import generate_traj
        out = generate_traj(self.model, self.scheduler, self.cfg, image, navigator=self.navigator, pose=pose,
                            controller=self.controller, velocity=velocity, guide=guide, pin=pin, **self.tick_kwargs)
        self.last_control = out[-1]
        return out[0]


def _world_guide(frame: EgoFrame, world: World) -> Optional[Guide]:
    discs = None if world.discs is None else frame.discs(world.discs)
    capsules = None if world.boxes is None else Capsules.from_boxes(frame.boxes(world.boxes))
    if world.signals is not None:
        return Guide(discs=discs, planes=world.signals.planes, capsules=capsules)
    return None if discs is None and capsules is None else Guide(discs=discs, capsules=capsules)


@torch.no_grad()
def drive(sampler, vehicle: KinematicVehicle, metrics: DriveMetrics, *, ticks: int, image, world: Optional[World] = None,
          guide_fn: Optional[Callable] = None, pin_fn: Optional[Callable] = None, waypoint_dt: Optional[float] = None,
          check_every: int = 0) -> int:
    """The closed loop: `ticks` times
        guide  = guide_fn(tick, EgoFrame(vehicle.pose, ...), world)     (default with a `world`: its discs, its boxes as capsules,
                                                                         the planes of its signals)
        sampler(image_t, pose=vehicle.pose, velocity=vehicle.velocity, guide=guide, pin=pin_fn(tick, vehicle.pose))
        vehicle.step(sampler.last_control, hold=metrics.done)
        world.signals.step(vehicle.pose, vehicle.velocity, hold=metrics.done)      (with signals; the hold the vehicle saw, so a
                                                                                    scene that ends this tick has its last
                                                                                    movement scored)
        world.traffic.step(vehicle.pose, vehicle.velocity, hold=metrics.done)      (with traffic: after the signals, whose new
                                                                                    phases it reads, and before the metrics, which
                                                                                    see its new boxes)
        world.advance(vehicle.dt)
        metrics.step(vehicle.pose, vehicle.velocity, vehicle.yaw_rate, world.discs, world.boxes)
    on the current stream and without a host synchronisation, except `bool(metrics.done.all())` every `check_every` ticks (0:
    never), which ends the loop early once every scene is done.  Returns the ticks run.

    `sampler`: a `GraphedSampler` built with `navigator=` and `controller=`, or an `EagerTick`; anything callable like them with a
    `last_control`.  `image`: a tensor used at every tick, or a callable `(tick, pose) -> image`.  THE LOOP IS BLIND unless that
    callable is a `Camera` (camera.py), which renders what the vehicle would see from `world`.  `waypoint_dt`: the seconds
    between two waypoints of a plan, which scales obstacle
    velocities in the guide (default: the vehicle's dt).  Place the vehicle (`vehicle.reset(pose)`) before the first tick.

    With `world.signals` the planes a tick's guide reads are those of the signals' last step -- the one after the previous tick's
    vehicle step, which saw this tick's pose.  Signals that have not stepped since their last reset (`not signals.primed`) are
    stepped once on the start pose before the first guide is built: time 0 of their clock.  So repeated calls with `ticks=1`
    equal one call with `ticks=T`.  With `world.traffic` the boxes a tick's guide reads are those of the traffic's last step or
    reset, which are valid from its construction on: it needs no priming."""
    ticks, check_every = int(ticks), int(check_every)
    if ticks < 1 or check_every < 0:
        raise ValueError(f"drive: ticks must be >= 1 and check_every >= 0, got {ticks} and {check_every}")
    if vehicle.scenes != metrics.scenes or vehicle.device != metrics.device:
        raise ValueError(f"drive: the vehicle holds {vehicle.scenes} scenes on {vehicle.device}, the metrics {metrics.scenes} on "
                         f"{metrics.device}")
    if not callable(image) and not torch.is_tensor(image):
        raise TypeError(f"drive: image must be a tensor or a callable (tick, pose) -> image, got {type(image).__name__}")
    if world is not None and not isinstance(world, World):
        raise TypeError(f"drive: world must be a World, got {type(world).__name__}")
    if guide_fn is not None and not callable(guide_fn) or pin_fn is not None and not callable(pin_fn):
        raise TypeError("drive: guide_fn and pin_fn must be callables")
    if world is not None and world.traffic is not None and guide_fn is None and world.traffic.n_agents > MAX_CAPSULES:
        raise ValueError(f"drive: the traffic holds {world.traffic.n_agents} agents per scene and the default world guide shows the "
                         f"planner at most {MAX_CAPSULES} boxes as capsules; pass guide_fn=, which picks the boxes the planner sees")
    _no_cpu(vehicle.device, "the closed loop")
    signals = None if world is None else world.signals
    if signals is not None and (signals.scenes != vehicle.scenes or signals.device != vehicle.device):
        raise ValueError(f"drive: the signals hold {signals.scenes} scenes on {signals.device}, the vehicle {vehicle.scenes} on "
                         f"{vehicle.device}")
    traffic = None if world is None else world.traffic
    if traffic is not None and (traffic.scenes != vehicle.scenes or traffic.device != vehicle.device or traffic.dt != vehicle.dt):
        raise ValueError(f"drive: the traffic holds {traffic.scenes} scenes on {traffic.device} with dt {traffic.dt}, the vehicle "
                         f"{vehicle.scenes} on {vehicle.device} with dt {vehicle.dt}")
    frame = None
    if world is not None or guide_fn is not None:
        xy_scale = getattr(getattr(sampler, "model", None), "magic_num", None)
        if xy_scale is None:
            raise ValueError("drive: a guide needs the model's xy scale; the sampler has no `model.magic_num`")
        frame = EgoFrame(vehicle.pose, float(xy_scale), vehicle.dt if waypoint_dt is None else waypoint_dt)
        if signals is not None and (signals.xy_scale != float(xy_scale) or signals.dt != vehicle.dt):
            raise ValueError(f"drive: the signals were built with xy_scale {signals.xy_scale} and dt {signals.dt}, the model's scale is "
                             f"{float(xy_scale)} and the vehicle's dt {vehicle.dt}")
    done_ticks = 0
    for t in range(ticks):
        if signals is not None and not signals.primed:
            signals.step(vehicle.pose, vehicle.velocity, hold=metrics.done)
        guide = None
        if guide_fn is not None:
            guide = guide_fn(t, frame, world)
        elif world is not None:
            guide = _world_guide(frame, world)
        kw = {}
        if guide is not None:
            kw["guide"] = guide
        if pin_fn is not None:
            kw["pin"] = pin_fn(t, vehicle.pose)
        sampler(image(t, vehicle.pose) if callable(image) else image, pose=vehicle.pose, velocity=vehicle.velocity, **kw)
        control = sampler.last_control
        if control is None:
            raise ValueError("drive: the sampler produced no control; build it with controller=DeviceController(...)")
        vehicle.step(control, hold=metrics.done)
        if signals is not None:
            signals.step(vehicle.pose, vehicle.velocity, hold=metrics.done)
        if traffic is not None:
            traffic.step(vehicle.pose, vehicle.velocity, hold=metrics.done)
        if world is not None:
            world.advance(vehicle.dt)
        metrics.step(vehicle.pose, vehicle.velocity, vehicle.yaw_rate, None if world is None else world.discs,
                     None if world is None else world.boxes)
        done_ticks = t + 1
        if check_every and done_ticks % check_every == 0 and bool((metrics.done != 0).all()):
            break
    return done_ticks


def evaluate_closed_loop(sampler, vehicle: KinematicVehicle, metrics: DriveMetrics, *, ticks: int, image, start_pose=None,
                         start_speed=None, **kw) -> dict:
    """`drive(...)` from a fresh record and `metrics.compute()`: with `start_pose` `[S, 3]` the vehicles are placed there first
    (`start_speed` `[S]` or at rest); the navigator's walk is the caller's to reset.  With `world=World(signals=...)` the signals
    are reset as well and the report gains `"signals"`: their `compute()`; with `world=World(traffic=...)` the traffic is reset
    and the report gains `"traffic"` likewise."""
    if start_pose is not None:
        vehicle.reset(start_pose, start_speed)
    metrics.reset()
    signals = getattr(kw.get("world"), "signals", None)
    if signals is not None:
        signals.reset()
    traffic = getattr(kw.get("world"), "traffic", None)
    if traffic is not None:
        traffic.reset()
    drive(sampler, vehicle, metrics, ticks=ticks, image=image, **kw)
    report = metrics.compute()
    if signals is not None:
        report["signals"] = signals.compute()
    if traffic is not None:
        report["traffic"] = traffic.compute()
    return report
