"""Reactive traffic of a closed loop, on the device: car-following agents on caller-laid paths that queue behind each other, stop
at the red and yellow lights of a `Signals`, and yield to the ego.

The reference gets its traffic from CARLA: zombie vehicles on autopilot and scenario actors that run BasicAgent (carla_gym/core/
task_actor/scenario_actor/agents/basic_agent.py: follow a route plan, full brake on a vehicle hazard ahead, a red light or the
destination).  This package rules the simulator out, so the traffic is ours and the paths are the caller's: a
polyline per lane, agents that start at an arc length along one, and the Intelligent Driver Model between an agent and whatever is
nearest ahead of it on its path -- another agent, the ego where it is within `lane_half_width` of the path, or a stop line whose
light shows red (or yellow, while the agent can still stop comfortably).

`Traffic.step(pose, velocity, hold=None)` is one launch of `adx_traffic_step` (csrc/traffic.hip, "traffic v1" of include/adx.h);
its static `boxes` float64 `[S, N, 7]` are what `World`, `EgoFrame.boxes` and `DriveMetrics` take, so `World(traffic=...)` puts
the agents in front of the planner and of the collision criterion.  `compute()` is the one device read.  The contract has no
library call on the way to any word, so the device equals the restatement (tests/traffic_ref.py) bit for bit.  How the rules
deviate from BasicAgent, and why, is in the contract ("differs"): no walkers, no lane changes, no junction priority -- paths that
cross do not see each other -- and stop signs are not obeyed.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .navigation import MAX_SCENES, _describe, _device, _positive
from .simulation import _mask, _no_cpu, _static

MAX_AGENTS, MAX_PATHS, MAX_PATH_POINTS, MAX_STOPS = 64, 8, 64, 16
AGENT_WIDTH, STOP_WIDTH, BOX_WIDTH, HEAD_WORDS = 9, 3, 7, 32
LEADER_NONE, LEADER_EGO = -1, 64                             # 0..63 an agent, 65 + t stop t
_TRAFFIC_INTS = ("ticks", "have", "arrived", "ego_yields", "ego_hard", "overlaps")


def _host(v, what: str, dtype=np.float64) -> np.ndarray:
    try:
        a = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        return np.ascontiguousarray(a, dtype=dtype)
    except (TypeError, ValueError) as e:
        raise TypeError(f"Traffic: {what} must be {np.dtype(dtype).name} values, got {type(v).__name__}") from e


def state_words(n_agents: int) -> int:
    """The 32-bit words of one scene's state ("traffic v1")."""
    return HEAD_WORDS + 5 * n_agents + (n_agents & 1)


class Traffic:
    """The car-following agents of S scenes ("traffic v1" of include/adx.h) and the static outputs of `step`.

    `paths`: float64 `[S, Q, G, 2]` world metres, Q in 1..8 polylines of G in 2..64 points; `lengths` int `[S, Q]`: the points of
    each that count (0..G; below 2 the path is empty).  `agents`: float64 `[S, N, 9]`, N in 1..64, slot = (path, start_s, start_v,
    desired_v, length, width, headway, accel, brake); a slot the contract calls EMPTY (a path that is no index of a path with
    points, a size, speed or rate that is not > 0, a start beyond the path) is no agent.  `stops`: float64 `[S, T, 3]`, T in
    1..16, = (path, s_stop, slot of `signals`), None: none; they need `signals`, a `Signals` of the same scenes, device and `dt`,
    whose `phase` is read in place at every step.  Host values all (arrays, CPU tensors, nested sequences; a device tensor is
    copied): validated here, uploaded once.  `dt`: the seconds of a tick; `lane_half_width` m: the ego is on a path within it;
    `ego_length` m; `jam` m: the standstill gap; `gap_min` m: the floor under a gap before it is divided by; `brake_max` m/s^2: the
    hard cap on deceleration.  All static, the same storage at every step, so a captured launch and a `World` can hold them:
      `boxes`  float64 `[S, N, 7]`  (cx, cy, vx, vy, yaw, length, width): `World`'s, `EgoFrame.boxes`' and `DriveMetrics`' format
      `leader` int32 `[S, N]`       -1 none, 0..63 an agent, 64 the ego, 65 + t stop t
      `state`  int32 `[S, W]`       the contract's record, W = 32 + 5 N (+ 1 when N is odd)
    On a GPU the constructor ends with `reset()`, so the boxes are valid before the first step.  `drive`'s default world guide
    turns the boxes into capsules, of which a guide takes 32 per scene: with more agents than that `drive` asks for a `guide_fn`.
    An object on a CPU device can be built and inspected; its launches refuse (there is no CPU path)."""

    def __init__(self, paths, lengths, agents, *, dt: float, stops=None, signals=None, lane_half_width: float = 1.75,
                 ego_length: float = 4.5, jam: float = 2.0, gap_min: float = 0.25, brake_max: float = 8.0, device=None):
        p, n, a = _host(paths, "paths"), _host(lengths, "lengths", np.int32), _host(agents, "agents")
        if p.ndim != 4 or p.shape[3] != 2:
            raise ValueError(f"Traffic: paths must be [S, Q, G, 2] world metres, got {p.shape}")
        S, Q, G = (int(v) for v in p.shape[:3])
        if not 1 <= S <= MAX_SCENES:
            raise ValueError(f"Traffic: scenes must be 1..{MAX_SCENES}, got {S}")
        if not 1 <= Q <= MAX_PATHS:
            raise ValueError(f"Traffic: paths per scene must be 1..{MAX_PATHS}, got {Q}")
        if not 2 <= G <= MAX_PATH_POINTS:
            raise ValueError(f"Traffic: points per path must be 2..{MAX_PATH_POINTS}, got {G}")
        if n.shape != (S, Q) or n.min() < 0 or n.max() > G:
            raise ValueError(f"Traffic: lengths must be [{S}, {Q}] values in 0..{G}, got {n.shape} in {int(n.min()) if n.size else 0}.."
                             f"{int(n.max()) if n.size else 0}")
        if a.ndim != 3 or a.shape[0] != S or a.shape[2] != AGENT_WIDTH or not 1 <= a.shape[1] <= MAX_AGENTS:
            raise ValueError(f"Traffic: agents must be [{S}, 1..{MAX_AGENTS}, {AGENT_WIDTH}] = (path, start_s, start_v, desired_v, length, "
                             f"width, headway, accel, brake), got {a.shape}")
        N = int(a.shape[1])
        used = np.arange(G)[None, None, :] < n[:, :, None]                                 # [S, Q, G]
        if not np.isfinite(p[used]).all():
            raise ValueError("Traffic: a path point that counts is not finite")
        cum, heading = self.path_tables(p)
        seg = used[:, :, 1:] & (cum[:, :, 1:] - cum[:, :, :-1] <= 0.0)
        if seg.any():
            s, q, g = (int(v[0]) for v in np.nonzero(seg))
            raise ValueError(f"Traffic: path {q} of scene {s} has a zero-length segment at point {g + 1}")
        if signals is not None:
            from .signals import Signals
            if not isinstance(signals, Signals):
                raise TypeError(f"Traffic: signals must be a Signals, got {type(signals).__name__}")
        dev = _device(device) if device is not None else (signals.device if signals is not None else torch.device("cpu"))
        self.dt = _positive(dt, "Traffic: dt")
        T, st = 0, None
        if stops is not None:
            st = _host(stops, "stops")
            if st.ndim != 3 or st.shape[0] != S or st.shape[2] != STOP_WIDTH or not 1 <= st.shape[1] <= MAX_STOPS:
                raise ValueError(f"Traffic: stops must be [{S}, 1..{MAX_STOPS}, {STOP_WIDTH}] = (path, s_stop, signal slot), got {st.shape}")
            if signals is None:
                raise ValueError("Traffic: stops need signals=, the Signals whose phases they read")
            if not (st[..., 2] < signals.n_signals).all():
                raise ValueError(f"Traffic: a stop names signal slot {float(np.nanmax(st[..., 2]))}, the signals hold {signals.n_signals}")
            T = int(st.shape[1])
        if signals is not None:
            if signals.scenes != S or signals.device != dev:
                raise ValueError(f"Traffic: the signals hold {signals.scenes} scenes on {signals.device}, the traffic {S} on {dev}: one "
                                 f"scene count, one device")
            if signals.dt != self.dt:
                raise ValueError(f"Traffic: dt is {self.dt}, the signals were built with dt {signals.dt}")
        self.lane_half_width = _positive(lane_half_width, "Traffic: lane_half_width")
        self.ego_length = _positive(ego_length, "Traffic: ego_length")
        self.jam = _positive(jam, "Traffic: jam")
        self.gap_min = _positive(gap_min, "Traffic: gap_min")
        self.brake_max = _positive(brake_max, "Traffic: brake_max")
        self.scenes, self.n_agents, self.n_paths, self.n_points, self.n_stops, self.device = S, N, Q, G, T, dev
        self.signals = signals
        nbytes = int(L.lazy("adx_traffic_state_bytes")(S, N))
        if nbytes != S * 4 * state_words(N):
            raise L.AdxError(f"adx_traffic_state_bytes({S}, {N}) = {nbytes}: not the state of traffic v1")

        def up(x):
            return torch.from_numpy(x).to(dev, copy=True).contiguous()
        self.paths, self.lengths, self.cum, self.heading, self.agents = up(p), up(n), up(cum), up(heading), up(a)
        self.stops = None if st is None else up(st)
        self.state = torch.zeros((S, state_words(N)), dtype=torch.int32, device=dev)
        self.boxes = torch.zeros((S, N, BOX_WIDTH), dtype=torch.float64, device=dev)
        self.leader = torch.full((S, N), LEADER_NONE, dtype=torch.int32, device=dev)
        self._cfg = L.TrafficCfg(S, N, Q, G, T, signals.n_signals if T else 0, self.dt, self.lane_half_width, self.ego_length, self.jam,
                                 self.gap_min, self.brake_max)
        if dev.type == "cuda":
            self.reset()

    @staticmethod
    def path_tables(paths):
        """(`cum`, `heading`), float64 `[..., G]` NumPy arrays, of `paths` `[..., G, 2]`: cum[0] = 0, cum[g] = cum[g-1] + |p[g] -
        p[g-1]|, the sequential sum in index order of drive metrics v1; heading[g] = atan2 of segment g -> g+1, the last point
        repeating the last segment's.  Every point is taken, whatever a path's length: the kernel never reads a table beyond it."""
        p = np.asarray(paths, dtype=np.float64)
        if p.ndim < 2 or p.shape[-1] != 2 or p.shape[-2] < 2:
            raise ValueError(f"Traffic.path_tables: paths must be [..., G >= 2, 2], got {p.shape}")
        d = p[..., 1:, :] - p[..., :-1, :]
        xx, yy = d[..., 0] * d[..., 0], d[..., 1] * d[..., 1]
        cum = np.zeros(p.shape[:-1], dtype=np.float64)
        cum[..., 1:] = np.cumsum(np.sqrt(xx + yy), axis=-1)      # cumsum adds in index order
        heading = np.zeros(p.shape[:-1], dtype=np.float64)
        heading[..., :-1] = np.arctan2(d[..., 1], d[..., 0])
        heading[..., -1] = heading[..., -2]
        return cum, heading

    @staticmethod
    def from_lanes(path, count: int, spacing: float, *, first: float = 0.0, speed: float = 0.0, desired_v: float = 8.0,
                   length: float = 4.5, width: float = 2.0, headway: float = 1.5, accel: float = 1.5, brake: float = 2.0) -> torch.Tensor:
        """float64 host rows `[len(path) * count, 9]`: on every path index of `path` (an int or a sequence of them) `count`
        agents, the rearmost at arc length `first` and the others `spacing` m apart ahead of it, all at `speed` m/s with the same
        law parameters.  Concatenate and pad with zero rows (empty slots) to build `agents`."""
        idx = np.atleast_1d(np.asarray(path, dtype=np.float64))
        count, spacing = int(count), float(spacing)
        if idx.ndim != 1 or count < 1 or not spacing > 0.0:
            raise ValueError(f"Traffic.from_lanes: path indices, count >= 1 and spacing > 0, got {path!r}, {count} and {spacing}")
        rows = np.zeros((len(idx), count, AGENT_WIDTH), dtype=np.float64)
        rows[..., 0] = idx[:, None]
        rows[..., 1] = float(first) + spacing * np.arange(count)[None, :]
        rows[..., 2:] = (speed, desired_v, length, width, headway, accel, brake)
        return torch.from_numpy(rows.reshape(-1, AGENT_WIDTH))

    def key(self) -> tuple:
        """What a captured launch bakes in."""
        return (self.scenes, self.n_agents, self.n_paths, self.n_points, self.n_stops, self.dt, self.lane_half_width, self.ego_length,
                self.jam, self.gap_min, self.brake_max, self.paths.data_ptr(), self.lengths.data_ptr(), self.cum.data_ptr(),
                self.heading.data_ptr(), self.agents.data_ptr(),
                0 if self.stops is None else self.stops.data_ptr(), 0 if self.signals is None else self.signals.phase.data_ptr(),
                self.state.data_ptr(), self.boxes.data_ptr(), self.leader.data_ptr())

    def step(self, pose: torch.Tensor, velocity: torch.Tensor, hold: Optional[torch.Tensor] = None) -> "Traffic":
        """One launch on the current stream, no allocation, no synchronisation: `pose` float64 `[S, 3]` and `velocity` float32
        `[S]` (a `KinematicVehicle`'s static outputs, or a simulator's or a log's); `hold` int32 `[S]` or None: where it is not 0
        the scene is frozen and its boxes are written again unchanged (`DriveMetrics.done`).  The phases of `signals` are read as
        they stand.  `boxes`, `leader` and the state hold the new values."""
        S, dev = self.scenes, self.device
        _static(pose, (S, 3), torch.float64, dev, "Traffic: pose")
        _static(velocity, (S,), torch.float32, dev, "Traffic: velocity")
        if hold is not None:
            _static(hold, (S,), torch.int32, dev, "Traffic: hold")
        _no_cpu(dev, "the traffic")
        phase = self.signals.phase if self.n_stops else None
        L.check(L.lazy("adx_traffic_step")(C.byref(self._cfg), self.paths.data_ptr(), self.lengths.data_ptr(), self.cum.data_ptr(),
                                           self.heading.data_ptr(), self.agents.data_ptr(), L.ptr(self.stops), L.ptr(phase), pose.data_ptr(),
                                           velocity.data_ptr(), L.ptr(hold), self.state.data_ptr(), self.boxes.data_ptr(),
                                           self.leader.data_ptr(), L.stream_ptr(dev)), "adx_traffic_step")
        return self

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """Every scene's agents, or those of the scenes where `mask` [S] (bool or uint8, on the device) is set, back at their
        starts with a fresh record; their boxes are written and their leaders cleared.  One launch on the current stream,
        capturable."""
        mask = _mask(mask, self.scenes, self.device)
        _no_cpu(self.device, "the traffic")
        L.check(L.lazy("adx_traffic_reset")(C.byref(self._cfg), self.paths.data_ptr(), self.lengths.data_ptr(), self.cum.data_ptr(),
                                            self.heading.data_ptr(), self.agents.data_ptr(), L.ptr(mask), self.state.data_ptr(),
                                            self.boxes.data_ptr(), self.leader.data_ptr(), L.stream_ptr(self.device)), "adx_traffic_reset")

    def state_snapshot(self) -> torch.Tensor:
        """A clone of the int32 `[S, W]` record (on the device, no synchronisation): what `state_restore` and `fields` take."""
        return self.state.clone()

    def state_restore(self, snapshot: torch.Tensor) -> None:
        if not torch.is_tensor(snapshot) or snapshot.shape != self.state.shape or snapshot.dtype != self.state.dtype:
            raise ValueError("state_restore: not a snapshot of this Traffic")
        self.state.copy_(snapshot)

    @staticmethod
    def fields(words) -> dict:
        """The contract's named fields of a host copy of the record (`state_snapshot()`): int32 `[S]` counters, float64 `[S]` `min_ego_gap`, `se_prev`
        float64 and `on_prev` int32 `[S, 8]`, `s`, `v` float64 and `alive` int32 `[S, N]`."""
        w = np.ascontiguousarray(words.detach().cpu().numpy() if torch.is_tensor(words) else words, dtype=np.int32)
        N = (w.shape[1] - HEAD_WORDS) // 5
        f = w.view(np.float64)
        out = {n: w[:, i].copy() for i, n in enumerate(_TRAFFIC_INTS)}
        out["min_ego_gap"] = f[:, 3].copy()
        out["se_prev"], out["on_prev"] = f[:, 4:12].copy(), w[:, 24:32].copy()
        out["s"], out["v"] = f[:, HEAD_WORDS // 2:HEAD_WORDS // 2 + N].copy(), f[:, HEAD_WORDS // 2 + N:HEAD_WORDS // 2 + 2 * N].copy()
        out["alive"] = w[:, HEAD_WORDS + 4 * N:HEAD_WORDS + 5 * N].copy()
        return out

    def compute(self) -> dict:
        """ONE device read (the records).  Per scene NumPy arrays `[S]`: `ticks`, `arrived`, `alive` (agents on the road now),
        `ego_yields` (agent-ticks whose leader was the ego), `ego_hard` (those that hit the `brake_max` clamp: the ego cut
        someone off), `overlaps` (agent-ticks with a negative gap to an agent leader; 0 in every sane run), `min_ego_gap` m (+inf
        until the ego leads someone; of a scene that never stepped or reset: +inf as well); and the int `total_overlaps`."""
        f = self.fields(self.state.cpu())
        gap = np.where(f["have"] != 0, f["min_ego_gap"], np.inf)
        return dict(ticks=f["ticks"], arrived=f["arrived"], alive=(f["alive"] != 0).sum(axis=1).astype(np.int32), ego_yields=f["ego_yields"],
                    ego_hard=f["ego_hard"], overlaps=f["overlaps"], min_ego_gap=gap, total_overlaps=int(f["overlaps"].sum()))

    def __repr__(self):
        return (f"Traffic(scenes={self.scenes}, agents={self.n_agents}, paths={self.n_paths} x {self.n_points}, stops={self.n_stops}, "
                f"dt={self.dt}, lane_half_width={self.lane_half_width}, device={self.device})")
