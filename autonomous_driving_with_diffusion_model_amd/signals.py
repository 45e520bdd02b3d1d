"""Traffic lights and stop signs of a closed loop, on the device: which stop lines bind the ego at this tick, as the half-planes a
`Guide` takes, and the two criteria the reference applies to every drive besides collisions, route deviation and blocked.

The reference asks CARLA: its RunRedLight and RunStopSign (carla_gym/core/task_actor/common/criteria) read the map's stop
waypoints and the signs' trigger volumes, and the leaderboard multiplies a drive's score by 0.7 per red light run and 0.8 per stop
sign run.  This package rules the simulator out, so the lines are the caller's: a segment A B per light or sign,
ordered so that its normal points the way the governed traffic drives (`Signals.from_lines` builds them from a centre, a heading
and a width).

`Signals.step(pose, velocity, hold=None)` is one launch of `adx_signals_step` (csrc/signals.hip, "signals v1" of include/adx.h):
the phase of every light from a per-scene tick clock, the gate that says a line binds the ego, the red-light run as the crossing of
a tail point swept over the tick, the stop sign machine, and the static `planes` float32 `[S, P, 3]` a `Guide(planes=)` reads: the
emitting lines first, `margin` metres short of them, inert planes (0, 0, 1) behind.  `compute()` is the one device read.  How the
rules deviate from the reference's two criteria, and why, is in the contract ("differs").
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .navigation import MAX_SCENES, _describe, _device, _positive
from .simulation import _mask, _no_cpu, _nonneg, _static

MAX_SIGNALS, MAX_PLANES = 64, 8
SIGNAL_WORDS, SIGNAL_WIDTH = 16, 10
LIGHT, STOP = 1.0, 2.0
PHASES = ("empty", "green", "yellow", "red", "stop")
RED_LIGHT_PENALTY, STOP_SIGN_PENALTY = 0.7, 0.8      # leaderboard/utils/statistics_manager.py
_SIGNAL_INTS = ("ticks", "have", "target", "stop_done", "red_runs", "stop_runs", "stops_met", "first_tick", "first_slot", "emitted",
                "flags", "pad")
_SIGNAL_F64 = ("qx", "qy")


class Signals:
    """The lights and stop signs of S scenes ("signals v1" of include/adx.h) and the static outputs of `step`.

    `records`: float64 `[S, N, 10]`, N in 1..64, slot = (ax, ay, bx, by, kind, reach, offset, green, yellow, red) in world metres
    and seconds; kind 1.0 a light, 2.0 a stop sign, anything else an empty slot.  A device tensor is read in place at every step
    (so a caller may move or re-time lines between steps); host values (a CPU tensor with `device=`, an array, nested sequences)
    are copied to `device`.  `dt`: the seconds of a tick; `xy_scale`: the metres of one model unit (`model.magic_num`); `planes`
    = P (1..8): the plane slots of the guide; `margin` m: how far short of a line its plane lies; `probe` m along the heading:
    the point whose crossing is a run (the reference's tail point is behind the centre: negative); `min_cos` in [-1, 1): a line
    binds an ego whose heading has a larger cosine with the line's; `stop_on_yellow`; `speed_threshold` m/s: below it a stop counts.
    All static, the same storage at every step, so a captured launch and a `Guide` can hold them:
      `planes` float32 `[S, P, 3]`  (nx, ny, b) in the ego frame and model units: `Guide(planes=)`
      `phase`  int32 `[S, N]`       0 empty, 1 green, 2 yellow, 3 red, 4 a stop sign
      `state`  int32 `[S, 16]`      the contract's record
    An object on a CPU device can be built and inspected; its launches refuse (there is no CPU path)."""

    def __init__(self, records, *, dt: float, xy_scale: float, planes: int = 4, margin: float = 3.0, probe: float = -2.0,
                 min_cos: float = 0.0, stop_on_yellow: bool = False, speed_threshold: float = 0.1, device=None):
        if torch.is_tensor(records) and records.is_cuda:
            if records.dtype != torch.float64:
                raise TypeError(f"Signals: records must be float64, got {records.dtype}")
            if device is not None and _device(device) != records.device:
                raise ValueError(f"Signals: records live on {records.device}, device= says {_device(device)}")
            if not records.is_contiguous():
                raise ValueError(f"Signals: records on the device are read in place and must be contiguous, got {_describe(records)}")
            rec, dev = records, records.device
        else:
            if torch.is_tensor(records) and records.dtype != torch.float64:
                raise TypeError(f"Signals: records must be float64, got {records.dtype}")
            try:
                rec = torch.as_tensor(records, dtype=torch.float64)
            except (TypeError, ValueError) as e:
                raise TypeError(f"Signals: records must be float64 [S, N, {SIGNAL_WIDTH}] values, got {type(records).__name__}") from e
            dev = rec.device if device is None else _device(device)
        if rec.dim() != 3 or rec.shape[2] != SIGNAL_WIDTH:
            raise ValueError(f"Signals: records must be [S, N, {SIGNAL_WIDTH}] = (ax, ay, bx, by, kind, reach, offset, green, yellow, "
                             f"red), got {tuple(rec.shape)}")
        S, N, P = int(rec.shape[0]), int(rec.shape[1]), int(planes)
        if not 1 <= S <= MAX_SCENES:
            raise ValueError(f"Signals: scenes must be 1..{MAX_SCENES}, got {S}")
        if not 1 <= N <= MAX_SIGNALS:
            raise ValueError(f"Signals: signals per scene must be 1..{MAX_SIGNALS}, got {N}")
        if not 1 <= P <= MAX_PLANES:
            raise ValueError(f"Signals: planes must be 1..{MAX_PLANES}, got {P}")
        self.dt = _positive(dt, "Signals: dt")
        self.xy_scale = _positive(xy_scale, "Signals: xy_scale")
        self.margin = _nonneg(margin, "Signals: margin")
        self.speed_threshold = _nonneg(speed_threshold, "Signals: speed_threshold")
        self.probe, self.min_cos = float(probe), float(min_cos)
        if not math.isfinite(self.probe):
            raise ValueError(f"Signals: probe must be finite, got {self.probe}")
        if not -1.0 <= self.min_cos < 1.0:
            raise ValueError(f"Signals: min_cos must lie in [-1, 1), got {self.min_cos}")
        self.scenes, self.n_signals, self.n_planes, self.stop_on_yellow, self.device = S, N, P, bool(stop_on_yellow), dev
        self.records = rec if rec.is_cuda else rec.detach().to(dev, copy=True).contiguous()
        nbytes = int(L.lazy("adx_signals_state_bytes")(S))
        if nbytes != S * 4 * SIGNAL_WORDS:
            raise L.AdxError(f"adx_signals_state_bytes({S}) = {nbytes}: not the state of signals v1")
        self.state = torch.zeros((S, SIGNAL_WORDS), dtype=torch.int32, device=dev)
        self.phase = torch.zeros((S, N), dtype=torch.int32, device=dev)
        self.planes = torch.zeros((S, P, 3), dtype=torch.float32, device=dev)
        self.planes[..., 2] = 1.0                                  # inert: 0 <= 1 everywhere
        self.primed = False
        self._cfg = L.SignalsCfg(S, N, P, int(self.stop_on_yellow), self.dt, self.xy_scale, self.margin, self.probe, self.min_cos,
                                 self.speed_threshold)

    @staticmethod
    def from_lines(centre, yaw, width, kind, reach, timing=(0.0, 0.0, 0.0, 0.0)) -> torch.Tensor:
        """float64 host records `[..., 10]` from `centre` `[..., 2]` of a stop line, `yaw` the world angle of the governed
        traffic's heading, the line's `width`, `kind` (1.0 a light, 2.0 a stop sign), `reach` m behind the line in which it binds,
        and `timing` `[..., 4]` = (offset, green, yellow, red) seconds (read for lights only); everything broadcasts.  A = c - w/2
        (sin yaw, -cos yaw), B = c + w/2 (sin yaw, -cos yaw): the line's normal is the heading."""
        centre, timing = np.asarray(centre, dtype=np.float64), np.asarray(timing, dtype=np.float64)
        if centre.shape[-1:] != (2,) or timing.shape[-1:] != (4,):
            raise ValueError(f"Signals.from_lines: centre must be [..., 2] and timing [..., 4], got {centre.shape} and {timing.shape}")
        yaw, width = np.asarray(yaw, dtype=np.float64), np.asarray(width, dtype=np.float64)
        kind, reach = np.asarray(kind, dtype=np.float64), np.asarray(reach, dtype=np.float64)
        hx, hy = width / 2.0 * np.sin(yaw), width / 2.0 * -np.cos(yaw)
        shape = np.broadcast(centre[..., 0], hx, kind, reach, timing[..., 0]).shape
        rec = np.zeros(shape + (SIGNAL_WIDTH,), dtype=np.float64)
        rec[..., 0], rec[..., 1] = centre[..., 0] - hx, centre[..., 1] - hy
        rec[..., 2], rec[..., 3] = centre[..., 0] + hx, centre[..., 1] + hy
        rec[..., 4], rec[..., 5] = kind, reach
        rec[..., 6:10] = timing
        return torch.from_numpy(rec)

    def key(self) -> tuple:
        """What a captured launch bakes in."""
        return (self.scenes, self.n_signals, self.n_planes, self.stop_on_yellow, self.dt, self.xy_scale, self.margin, self.probe,
                self.min_cos, self.speed_threshold, self.records.data_ptr(), self.state.data_ptr(), self.planes.data_ptr(),
                self.phase.data_ptr())

    def step(self, pose: torch.Tensor, velocity: torch.Tensor, hold: Optional[torch.Tensor] = None) -> "Signals":
        """One launch on the current stream, no allocation, no synchronisation: `pose` float64 `[S, 3]` and `velocity` float32
        `[S]` (a `KinematicVehicle`'s static outputs, or a simulator's or a log's); `hold` int32 `[S]` or None: where it is not 0
        the scene's record is frozen and its planes are inert (`DriveMetrics.done`).  `planes`, `phase` and the state hold the
        new values."""
        S, dev = self.scenes, self.device
        _static(pose, (S, 3), torch.float64, dev, "Signals: pose")
        _static(velocity, (S,), torch.float32, dev, "Signals: velocity")
        if hold is not None:
            _static(hold, (S,), torch.int32, dev, "Signals: hold")
        _no_cpu(dev, "the signals")
        L.check(L.lazy("adx_signals_step")(C.byref(self._cfg), self.records.data_ptr(), pose.data_ptr(), velocity.data_ptr(), L.ptr(hold),
                                           self.state.data_ptr(), self.planes.data_ptr(), self.phase.data_ptr(), L.stream_ptr(dev)),
                "adx_signals_step")
        self.primed = True
        return self

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """A fresh record and inert planes for every scene, or for the scenes where `mask` [S] (bool or uint8, on the device) is
        set.  One launch on the current stream, capturable.  Without a mask `primed` is cleared."""
        mask = _mask(mask, self.scenes, self.device)
        _no_cpu(self.device, "the signals")
        L.check(L.lazy("adx_signals_reset")(self.state.data_ptr(), self.scenes, L.ptr(mask), self.planes.data_ptr(), self.n_planes,
                                            L.stream_ptr(self.device)), "adx_signals_reset")
        if mask is None:
            self.primed = False

    def state_snapshot(self) -> torch.Tensor:
        return self.state.clone()

    def state_restore(self, snapshot: torch.Tensor) -> None:
        if not torch.is_tensor(snapshot) or snapshot.shape != self.state.shape or snapshot.dtype != self.state.dtype:
            raise ValueError("state_restore: not a snapshot of this Signals")
        self.state.copy_(snapshot)

    def words(self) -> torch.Tensor:
        """A clone of the int32 `[S, 16]` record (on the device, no synchronisation)."""
        return self.state.clone()

    @staticmethod
    def fields(words) -> dict:
        """The contract's named fields of a host copy of `words()`: int32 `[S]` and float64 `[S]` NumPy arrays."""
        w = np.ascontiguousarray(words.detach().cpu().numpy() if torch.is_tensor(words) else words, dtype=np.int32)
        f = w.view(np.float64)
        out = {n: w[:, i].copy() for i, n in enumerate(_SIGNAL_INTS)}
        out.update({n: f[:, len(_SIGNAL_INTS) // 2 + i].copy() for i, n in enumerate(_SIGNAL_F64)})
        return out

    def compute(self) -> dict:
        """ONE device read (the records), then host arithmetic.  Per scene NumPy arrays `[S]`: `ticks`, `red_runs`, `stop_runs`,
        `stops_met`, `first_tick` (0: no infraction), `first_slot`, `overflow` (bool: more lines bound the ego at some step than
        there are planes), `penalty` = 0.7 ** red_runs * 0.8 ** stop_runs, the leaderboard's factors; and the float
        `mean_penalty`."""
        f = self.fields(self.state.cpu())
        penalty = RED_LIGHT_PENALTY ** f["red_runs"].astype(np.float64) * STOP_SIGN_PENALTY ** f["stop_runs"].astype(np.float64)
        return dict(ticks=f["ticks"], red_runs=f["red_runs"], stop_runs=f["stop_runs"], stops_met=f["stops_met"],
                    first_tick=f["first_tick"], first_slot=f["first_slot"], overflow=(f["flags"] & 1) != 0, penalty=penalty,
                    mean_penalty=float(penalty.mean()))

    def __repr__(self):
        return (f"Signals(scenes={self.scenes}, signals={self.n_signals}, planes={self.n_planes}, dt={self.dt}, margin={self.margin}, "
                f"probe={self.probe}, min_cos={self.min_cos}, stop_on_yellow={self.stop_on_yellow}, device={self.device})")
