"""What feeds a tick, on the device: the walk along the global plan, the target point and the route ahead in this tick's ego frame,
the odometry between two ticks, and the transform between world metres and the ego frame for everything else a guide takes.

The reference's agent does this on the host at every tick: `RoutePlanner.run_step(cur_pos)` (e2e_driving/planner.py) pops the
waypoints the vehicle has passed and returns the next one with its command, `process_next_waypoint` (interact.py:185-202) rotates
it by the compass into the ego frame, `get_future_waypoints` (interact.py:174) is the route ahead and `agent_to_world`
(interact.py:249-260) takes a plan back.  With S scenes per launch that is S host loops, S small copies and S sets of
trigonometry in front of a tick that otherwise needs no host work.

`Navigator.step(pose)` is one launch of `adx_nav_step` (csrc/nav.hip, "route planner v1" of include/adx.h) for all scenes: the
reference's walk in fp64, decision for decision; `target`, `command` and the `points`-long window of the route in the ego frame
in model units; and `motion = (tx, ty, phi)` as `WarmStart` and `ManoeuvreCommit` take it.  The walk's cursor and the previous
pose live in one device buffer the launch reads and advances through its address, so the step is capturable and the first tick is
the same launch as every later one.  `EgoFrame` is the same transform ("ego frame v1") for points, discs, planes and boxes, and
`EgoFrame.to_world` its inverse for plans.  Whether the planner's distances suit a given town is the caller's to say; nothing here
measures driving.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib as L
from .guide import Route

MAX_POINTS = 65536          # G: the points of a scene's plan
MIN_WINDOW, MAX_WINDOW = 2, 32
MAX_SCENES = 65535
POINTS, DISCS, PLANES, BOXES = 0, 1, 2, 3      # `kind` of adx_world_to_ego
_WIDTH_IN, _WIDTH_OUT = (2, 5, 3, 7), (2, 5, 3, 8)
_KIND_NAMES = ("points", "discs", "planes", "boxes")


def _positive(v, what: str) -> float:
    v = float(v)
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"{what} must be finite and > 0, got {v}")
    return v


def _device(device) -> torch.device:
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:      # "cuda" names the current device; tensors say "cuda:0"
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _describe(t) -> str:
    return f"{tuple(t.shape)} {t.dtype} on {t.device}" if torch.is_tensor(t) else type(t).__name__


class Navigator:
    """The global plans of S scenes on `device`, the walk along them, and the static outputs of `step`.

    `route_m` float64 `[S, G, 2]` world metres, `commands` int32 `[S, G]`, `lengths` int32 `[S]` with 1 <= length <= G <= 65536
    (tensors on any device; they are copied): scene s's plan is its first `lengths[s]` points, the rest is padding and never read.
    `xy_scale`: the metres of one model unit (`model.magic_num`); `min_distance`, `max_distance`: the reference RoutePlanner's, in
    metres; `points` = R (2..32): the length of the window; `first`: 0 keeps the point just passed at the head of the window, so
    that a corridor covers the segment the ego is on, 1 is the reference's `get_future_waypoints`.

    After `step(pose)`, all static (the same storage at every tick, so a captured graph and a `Guide` can hold them):
      `target` float32 `[S, 2]`   the next waypoint in this tick's ego frame, model units: a tick's `target`
      `command` int32 `[S]`       that waypoint's command, as stored
      `window` float32 `[S, R, 2]`  the route ahead; `route(half_width, weight)` is a `Route` on this very buffer
      `motion` float32 `[S, 3]`   (tx, ty, phi) since the last step: a tick's `motion`; zeros on a scene's first step
      `fresh` int32 `[S]`         1 on a scene's first step (no odometry yet)
      `head` int32 `[S]`          the walk's cursor: the points before it are popped
    `state` is the int32 `[S, 8]` buffer of the contract (head, valid, then the previous pose as three doubles).  An object on a
    CPU device can be built and inspected; its launches refuse (there is no CPU path)."""

    def __init__(self, route_m: torch.Tensor, commands: torch.Tensor, lengths: torch.Tensor, *, xy_scale: float,
                 min_distance: float = 7.0, max_distance: float = 50.0, points: int = 16, first: int = 0, device):
        for name, t, dtype in (("route_m", route_m, torch.float64), ("commands", commands, torch.int32), ("lengths", lengths, torch.int32)):
            if not torch.is_tensor(t):
                raise TypeError(f"Navigator: {name} must be a tensor, got {type(t).__name__} (from_physical takes sequences)")
            if t.dtype != dtype:
                raise TypeError(f"Navigator: {name} must be {dtype}, got {t.dtype}")
        if route_m.dim() != 3 or route_m.shape[2] != 2 or route_m.shape[0] < 1 or route_m.shape[1] < 1:
            raise ValueError(f"Navigator: route_m must be [S, G, 2] world metres, got {tuple(route_m.shape)}")
        S, G = int(route_m.shape[0]), int(route_m.shape[1])
        if S > MAX_SCENES:
            raise ValueError(f"Navigator: {S} scenes, supported 1..{MAX_SCENES}")
        if G > MAX_POINTS:
            raise ValueError(f"Navigator: {G} route points per scene, supported 1..{MAX_POINTS}")
        if tuple(commands.shape) != (S, G):
            raise ValueError(f"Navigator: commands must be [{S}, {G}], got {tuple(commands.shape)}")
        if tuple(lengths.shape) != (S,):
            raise ValueError(f"Navigator: lengths must be [{S}], got {tuple(lengths.shape)}")
        lens = lengths.detach().cpu()
        if int(lens.min()) < 1 or int(lens.max()) > G:
            raise ValueError(f"Navigator: lengths must lie in 1..{G} (G), got {lens.tolist()}")
        points, first = int(points), int(first)
        if not MIN_WINDOW <= points <= MAX_WINDOW:
            raise ValueError(f"Navigator: points must be {MIN_WINDOW}..{MAX_WINDOW}, got {points}")
        if first not in (0, 1):
            raise ValueError(f"Navigator: first must be 0 or 1, got {first}")
        self.xy_scale = _positive(xy_scale, "Navigator: xy_scale")
        self.min_distance = _positive(min_distance, "Navigator: min_distance")
        self.max_distance = _positive(max_distance, "Navigator: max_distance")
        self.scenes, self.max_points, self.points, self.first, self.device = S, G, points, first, _device(device)
        dev = self.device
        self.route_m = route_m.detach().to(dev).contiguous().clone()
        self.commands = commands.detach().to(dev).contiguous().clone()
        self.lengths = lengths.detach().to(dev).contiguous().clone()
        nbytes = int(L.lazy("adx_nav_state_bytes")(S))
        if nbytes != S * 32:
            raise L.AdxError(f"adx_nav_state_bytes({S}) = {nbytes}: not the state of route planner v1")
        self.state = torch.zeros((S, 8), dtype=torch.int32, device=dev)
        self.pose = torch.zeros((S, 3), dtype=torch.float64, device=dev)      # where host poses land
        self.target = torch.zeros((S, 2), dtype=torch.float32, device=dev)
        self.command = torch.zeros((S,), dtype=torch.int32, device=dev)
        self.window = torch.zeros((S, points, 2), dtype=torch.float32, device=dev)
        self.motion = torch.zeros((S, 3), dtype=torch.float32, device=dev)
        self.fresh = torch.zeros((S,), dtype=torch.int32, device=dev)
        self.head = torch.zeros((S,), dtype=torch.int32, device=dev)
        self._cfg = L.NavCfg(S, G, points, first, self.min_distance, self.max_distance, self.xy_scale)

    @staticmethod
    def from_physical(routes_m, commands=None, *, xy_scale: float, device, **kw) -> "Navigator":
        """From nested sequences: `routes_m` holds per scene a sequence of (x, y) world metres, of any length >= 1 each (shorter
        plans are padded with their last point); `commands` per scene as many integers (None: zeros).  Python floats are doubles
        and are read as such."""
        if len(routes_m) < 1 or any(len(r) < 1 for r in routes_m):
            raise ValueError("Navigator.from_physical: every scene needs a route of at least one point")
        S, G = len(routes_m), max(len(r) for r in routes_m)
        route = torch.zeros((S, G, 2), dtype=torch.float64)
        cmd = torch.zeros((S, G), dtype=torch.int32)
        for s, r in enumerate(routes_m):
            pts = torch.as_tensor(r, dtype=torch.float64)
            if pts.dim() != 2 or pts.shape[1] != 2:
                raise ValueError(f"Navigator.from_physical: scene {s}'s route must be [n, 2], got {tuple(pts.shape)}")
            route[s, :len(r)], route[s, len(r):] = pts, pts[-1]
            if commands is not None:
                if len(commands[s]) != len(r):
                    raise ValueError(f"Navigator.from_physical: scene {s} has {len(r)} points and {len(commands[s])} commands")
                cmd[s, :len(r)] = torch.as_tensor(commands[s], dtype=torch.int32)
                cmd[s, len(r):] = cmd[s, len(r) - 1]
        lengths = torch.tensor([len(r) for r in routes_m], dtype=torch.int32)
        return Navigator(route, cmd, lengths, xy_scale=xy_scale, device=device, **kw)

    # ---- views of the state ---------------------------------------------------------------------------------------------------
    @property
    def valid(self) -> torch.Tensor:
        """[S] int32, a view: not 0 where the state holds a previous pose."""
        return self.state[:, 1]

    @property
    def previous_pose(self) -> torch.Tensor:
        """[S, 3] float64, a view: (px, py, compass) of the last step."""
        return self.state.view(torch.float64)[:, 1:]

    def route(self, half_width, weight: float = 1.0) -> Route:
        """A `Route` whose `points` IS the window buffer: a guide built on it sees every step's window (in a GraphedSampler
        through the usual `Guide.copy_`)."""
        return Route(self.window, half_width, weight)

    def _pose(self, pose) -> torch.Tensor:
        S = self.scenes
        if torch.is_tensor(pose) and pose.is_cuda:
            if pose.dtype != torch.float64 or tuple(pose.shape) != (S, 3) or pose.device != self.device or not pose.is_contiguous():
                raise ValueError(f"Navigator: pose must be contiguous float64 [{S}, 3] = (x, y, compass) on {self.device}, got "
                                 f"{_describe(pose)}")
            return pose
        host = torch.as_tensor(pose, dtype=torch.float64)      # host values: one copy into the static buffer
        if tuple(host.shape) != (S, 3):
            raise ValueError(f"Navigator: pose must be [{S}, 3] = (x, y, compass) per scene, got {tuple(host.shape)}")
        L.require_gpu_f32(self.pose, "the navigator", torch.float64)      # there is no CPU path
        self.pose.copy_(host)
        return self.pose

    def step(self, pose) -> "Navigator":
        """One launch on the current stream, no allocation, no synchronisation: `pose` is a device float64 `[S, 3]` tensor (read
        in place), or host values (a CPU tensor or nested sequences), which are copied into the static `self.pose` first.  The
        walk moves on and every output buffer holds this tick's values."""
        pose = self._pose(pose)
        L.require_gpu_f32(self.state, "the navigator", torch.int32)
        L.check(L.lazy("adx_nav_step")(C.byref(self._cfg), self.route_m.data_ptr(), self.commands.data_ptr(), self.lengths.data_ptr(),
                                       pose.data_ptr(), self.state.data_ptr(), self.target.data_ptr(), self.command.data_ptr(),
                                       self.window.data_ptr(), self.motion.data_ptr(), self.fresh.data_ptr(), self.head.data_ptr(),
                                       L.stream_ptr(self.device)), "adx_nav_step")
        return self

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """A fresh walk from point 0 for every scene, or for the scenes where `mask` [S] (bool or uint8, on the device) is set; their
        next step reports `fresh`.  A launch on the current stream, capturable."""
        if mask is not None:
            if not torch.is_tensor(mask) or tuple(mask.shape) != (self.scenes,) or mask.device != self.device or \
                    mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError(f"mask must be [{self.scenes}] bool or uint8 on {self.device}, got {_describe(mask)}")
            mask = mask.contiguous().view(torch.uint8)
        L.require_gpu_f32(self.state, "the navigator", torch.int32)
        L.check(L.lazy("adx_nav_reset")(self.state.data_ptr(), self.scenes, L.ptr(mask), L.stream_ptr(self.device)), "adx_nav_reset")

    def set_route(self, scene: int, route_m, commands=None) -> None:
        """A new plan for one scene: `route_m` [n, 2] world metres with 1 <= n <= G (a tensor or nested sequences), `commands` [n]
        (None: zeros).  Copied into the static buffers (padded with the last point), then that scene's walk is reset."""
        scene = int(scene)
        if not 0 <= scene < self.scenes:
            raise ValueError(f"Navigator.set_route: scene must be 0..{self.scenes - 1}, got {scene}")
        pts = torch.as_tensor(route_m, dtype=torch.float64)
        if pts.dim() != 2 or pts.shape[1] != 2 or not 1 <= pts.shape[0] <= self.max_points:
            raise ValueError(f"Navigator.set_route: route_m must be [n, 2] with 1 <= n <= {self.max_points}, got {tuple(pts.shape)}")
        n = int(pts.shape[0])
        cmd = torch.zeros((n,), dtype=torch.int32) if commands is None else torch.as_tensor(commands, dtype=torch.int32)
        if tuple(cmd.shape) != (n,):
            raise ValueError(f"Navigator.set_route: commands must be [{n}], got {tuple(cmd.shape)}")
        L.require_gpu_f32(self.state, "the navigator", torch.int32)
        self.route_m[scene, :n] = pts.to(self.device)
        self.route_m[scene, n:] = pts[-1].to(self.device)
        self.commands[scene, :n] = cmd.to(self.device)
        self.commands[scene, n:] = cmd[-1].to(self.device)
        self.lengths[scene] = n
        mask = torch.zeros((self.scenes,), dtype=torch.uint8)
        mask[scene] = 1
        self.reset(mask.to(self.device))

    def state_snapshot(self) -> torch.Tensor:
        return self.state.clone()

    def state_restore(self, snapshot: torch.Tensor) -> None:
        if snapshot.shape != self.state.shape or snapshot.dtype != self.state.dtype:
            raise ValueError("state_restore: not a snapshot of this Navigator")
        self.state.copy_(snapshot)

    def __repr__(self):
        return (f"Navigator(scenes={self.scenes}, max_points={self.max_points}, points={self.points}, first={self.first}, "
                f"min_distance={self.min_distance}, max_distance={self.max_distance}, xy_scale={self.xy_scale}, device={self.device})")


class EgoFrame:
    """World metres to this tick's ego frame in model units and back ("ego frame v1" of include/adx.h), one launch per call.

    `pose` float64 `[S, 3]` = (x, y, compass) on the device, read at every call (new values need no new object); `xy_scale`: the
    metres of one model unit; `dt`: the seconds between two waypoints, which `discs` and `boxes` need for velocities.  Inputs are
    float64 device tensors `[S, N, w]` in world metres, m/s and radians; outputs float32 in the formats the guide takes, written to
    `out=` when given (a static buffer of a captured graph):
      `points`  [S, N, 2] (X, Y)                               -> [S, N, 2]: `Route.points`, a `target`
      `discs`   [S, M, 5] (cx, cy, vx, vy, r)                  -> [S, M, 5]: `Guide` discs
      `planes`  [S, P, 3] (nx, ny, b), n . p <= b in the world -> [S, P, 3]: `Guide` planes
      `boxes`   [S, N, 7] (cx, cy, vx, vy, yaw, length, width) -> [S, N, 8]: the input of `Capsules.from_boxes`
    A radius or size <= 0 (or NaN) stays one: an empty slot stays empty.  `to_world(traj)`: float32 plans `[rows, H, D >= 2]` in
    model units, rows a multiple of S (candidate-major: row r is scene r % S), to float64 `[rows, H, 2]` world metres -- the
    reference's `agent_to_world` on `traj / magic_num`."""

    def __init__(self, pose: torch.Tensor, xy_scale: float, dt: Optional[float] = None):
        if not torch.is_tensor(pose):
            raise TypeError(f"EgoFrame: pose must be a tensor, got {type(pose).__name__}")
        if pose.dtype != torch.float64:
            raise TypeError(f"EgoFrame: pose must be float64, got {pose.dtype}")
        if pose.dim() != 2 or pose.shape[1] != 3 or not 1 <= pose.shape[0] <= MAX_SCENES or not pose.is_contiguous():
            raise ValueError(f"EgoFrame: pose must be contiguous [S, 3] = (x, y, compass), got {tuple(pose.shape)}")
        self.pose, self.xy_scale = pose, _positive(xy_scale, "EgoFrame: xy_scale")
        self.dt = None if dt is None else float(dt)
        if self.dt is not None and not math.isfinite(self.dt):
            raise ValueError(f"EgoFrame: dt must be finite, got {self.dt}")

    @property
    def scenes(self) -> int:
        return int(self.pose.shape[0])

    def _to_ego(self, kind: int, rec: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
        name, w_in, w_out, S = _KIND_NAMES[kind], _WIDTH_IN[kind], _WIDTH_OUT[kind], self.scenes
        if not torch.is_tensor(rec):
            raise TypeError(f"EgoFrame.{name}: the input must be a tensor, got {type(rec).__name__}")
        if rec.dtype != torch.float64:
            raise TypeError(f"EgoFrame.{name}: the input must be float64, got {rec.dtype}")
        if rec.dim() != 3 or rec.shape[0] != S or rec.shape[2] != w_in or not 1 <= rec.shape[1] <= MAX_POINTS:
            raise ValueError(f"EgoFrame.{name}: the input must be [{S}, N, {w_in}] with 1 <= N <= {MAX_POINTS}, got {tuple(rec.shape)}")
        if rec.device != self.pose.device:
            raise ValueError(f"EgoFrame.{name}: the pose lives on {self.pose.device}, the input on {rec.device}")
        moving = kind in (DISCS, BOXES)
        if moving and self.dt is None:
            raise ValueError(f"EgoFrame.{name}: velocities need dt, the seconds between two waypoints (EgoFrame(pose, xy_scale, dt))")
        N = int(rec.shape[1])
        if out is not None:
            if not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (S, N, w_out) or out.device != rec.device \
                    or not out.is_contiguous():
                raise ValueError(f"EgoFrame.{name}: out must be contiguous float32 {(S, N, w_out)} on {rec.device}, got {_describe(out)}")
        rec = L.require_gpu_f32(rec, f"EgoFrame.{name}: the input", torch.float64)
        if out is None:
            out = torch.empty((S, N, w_out), dtype=torch.float32, device=rec.device)
        L.check(L.lazy("adx_world_to_ego")(kind, rec.data_ptr(), self.pose.data_ptr(), out.data_ptr(), S, N, self.xy_scale,
                                           self.dt / self.xy_scale if moving else 0.0, L.stream_ptr(rec.device)), "adx_world_to_ego")
        return out

    def points(self, points_m: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._to_ego(POINTS, points_m, out)

    def discs(self, discs_m: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._to_ego(DISCS, discs_m, out)

    def planes(self, planes_m: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._to_ego(PLANES, planes_m, out)

    def boxes(self, boxes_m: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._to_ego(BOXES, boxes_m, out)

    def to_world(self, traj: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        S = self.scenes
        if not torch.is_tensor(traj):
            raise TypeError(f"EgoFrame.to_world: traj must be a tensor, got {type(traj).__name__}")
        if traj.dtype != torch.float32:
            raise TypeError(f"EgoFrame.to_world: traj must be float32, got {traj.dtype}")
        if traj.dim() != 3 or traj.shape[0] < 1 or traj.shape[0] % S != 0 or traj.shape[1] < 1 or not 2 <= traj.shape[2] <= 16:
            raise ValueError(f"EgoFrame.to_world: traj must be [K * {S}, H, D] with 2 <= D <= 16, got {tuple(traj.shape)}")
        if traj.device != self.pose.device:
            raise ValueError(f"EgoFrame.to_world: the pose lives on {self.pose.device}, traj on {traj.device}")
        rows, H, D = (int(v) for v in traj.shape)
        if out is not None:
            if not torch.is_tensor(out) or out.dtype != torch.float64 or tuple(out.shape) != (rows, H, 2) or out.device != traj.device \
                    or not out.is_contiguous():
                raise ValueError(f"EgoFrame.to_world: out must be contiguous float64 {(rows, H, 2)} on {traj.device}, got {_describe(out)}")
        traj = L.require_gpu_f32(traj, "EgoFrame.to_world: traj")
        if out is None:
            out = torch.empty((rows, H, 2), dtype=torch.float64, device=traj.device)
        L.check(L.lazy("adx_ego_to_world")(traj.data_ptr(), self.pose.data_ptr(), out.data_ptr(), rows, S, H, D, self.xy_scale,
                                           L.stream_ptr(traj.device)), "adx_ego_to_world")
        return out

    def __repr__(self):
        return f"EgoFrame(scenes={self.scenes}, xy_scale={self.xy_scale}, dt={self.dt}, device={self.pose.device})"
