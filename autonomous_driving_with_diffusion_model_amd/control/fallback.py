"""The stop-short fallback: re-time a blocked plan so that it brakes to a halt before its first conflict.

`StopShort.__call__` is one launch of `adx_stop_short` (csrc/fallback.hip, "stop-short fallback v1" of include/adx.h).  Cost
guidance pushes samples away from obstacles and a hard selection prefers a free candidate, but neither promises that the plan a
tick ends with is free; every sampling planner keeps a deterministic last resort for that case: keep the path, change the speed
profile, stop short of the first conflict.  The launch keeps the plan's geometry, finds its first waypoint that conflicts with the
guide's point-wise terms (discs, planes and the records guide.py declares POINTWISE -- motion limits are not places) and moves
the waypoints along the plan's own polyline so that the spacing shrinks by at most `decel` per waypoint and the last one rests `gap` before the
conflict.  `DeviceController` takes its desired speed from that spacing, so the re-timed plan brakes through the controller as it
is.  No host decision and no synchronisation, so the call can be a node of a captured graph
(`GraphedSampler(..., fallback=...)`).  No reference counterpart.

Whether stopping short makes a trained model drive better is a property of weights and a simulator and is not measured in this
repository.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import torch

from .. import _lib as L
from ..guide import Guide

MAX_HORIZON = 64
NO_POINTWISE_TERM = "stop short: the guide holds no point-wise term (discs, planes, a field, a route or capsules)"


def _numbers(v, name: str) -> list:
    """A number (a Python or NumPy scalar, a 0-dim or one-element tensor) as a list of one float, a sequence of numbers as a list
    of floats."""
    try:
        return [float(v)]
    except (TypeError, ValueError, RuntimeError):      # not one number: a sequence, or nothing this takes
        pass
    try:
        return [float(t) for t in v]
    except (TypeError, ValueError, RuntimeError):
        raise TypeError(f"StopShort.from_physical: {name} must be a number or a sequence of numbers, got {type(v).__name__}") from None


class StopResult(NamedTuple):
    traj: Optional[torch.Tensor]       # [rows, H, D]: the re-timed plan; a free row is its input bit for bit
    first: torch.Tensor                # [rows] int32: the first conflicting waypoint, H where there is none
    status: torch.Tensor               # [rows] int32: 0 free, 1 re-timed, 2 re-timed and the first step sheds more than decel
    stop_at: torch.Tensor              # [rows] float32: the arc length at which the plan halts (+inf on a free row)
    active_after: torch.Tensor         # [rows] int32: what the re-timed plan still violates; NOT promised to be 0


class StopShort:
    """`params` float32 `[S, 2]` = per scene `(gap, decel)` in the model's own units (the clamped result before xy scaling).
    `gap`: the arc length to keep between the halt and the last free waypoint before the conflict (negative or NaN: 0).  `decel`:
    the most the length of a step may shrink from one waypoint to the next -- for this model speed IS the spacing of the
    waypoints, so this is a deceleration; `inf`, a NaN or a negative value switch the limit off (the plan keeps its own speed and
    lands on the stop point in one step), `0` means "do not move".  The params are read at every launch: new values need no new
    object (and, in a GraphedSampler, no new capture).  `last`: the report of the last tick this object ran in
    (`generate_traj(..., fallback=...)`), a StopResult without `traj`.

    `status` 2 says the plan cannot stop in time under `decel` (its first step already has to shed more): a consumer may want full
    brake.  `active_after` is what the re-timed plan still violates: the launch looks at waypoints only, as the guide does, and a
    moving obstacle can reach a stopped ego -- the caller gets the number instead of a promise."""

    def __init__(self, params: torch.Tensor):
        if not torch.is_tensor(params):
            raise TypeError(f"StopShort: params must be a tensor, got {type(params).__name__}")
        if params.dim() != 2 or params.shape[1] != 2 or params.shape[0] < 1:
            raise ValueError(f"StopShort: params must be [S, 2] = (gap, decel) per scene, got {tuple(params.shape)}")
        if params.dtype != torch.float32:
            raise TypeError(f"StopShort: params must be float32, got {params.dtype}")
        self.params = params.contiguous()
        self.last: Optional[StopResult] = None

    @property
    def scenes(self) -> int:
        return int(self.params.shape[0])

    @property
    def device(self) -> torch.device:
        return self.params.device

    def key(self) -> tuple:
        """What a captured graph bakes: everything but the values of the params -- which is their presence alone."""
        return ("stop_short_v1",)

    def like(self, params: torch.Tensor) -> "StopShort":
        """The same fallback over other params."""
        return StopShort(params)

    @staticmethod
    def from_physical(gap_m, decel_mps2, dt: float, xy_scale: float, device=None) -> "StopShort":
        """Params from physical ones, on the host: `gap_m` (m) and `decel_mps2` (m/s^2) are numbers or sequences of S numbers
        (one per scene; a number stands for all), `dt` the seconds between two waypoints, `xy_scale` the metres of one model unit
        (`model.magic_num`).  gap = gap_m / xy_scale and decel = decel_mps2 * dt * dt / xy_scale, formed in double and rounded to
        fp32 once.  `inf` stays `inf`."""
        dt, xy_scale = float(dt), float(xy_scale)
        if not (math.isfinite(dt) and dt > 0.0 and math.isfinite(xy_scale) and xy_scale > 0.0):
            raise ValueError(f"StopShort.from_physical: dt and xy_scale must be finite and > 0, got {dt} and {xy_scale}")
        g, a = _numbers(gap_m, "gap_m"), _numbers(decel_mps2, "decel_mps2")
        S = max(len(g), len(a))
        if len(g) not in (1, S) or len(a) not in (1, S) or S < 1:
            raise ValueError(f"StopShort.from_physical: gap_m holds {len(g)} scenes, decel_mps2 {len(a)}")
        g, a = g * (S // len(g)), a * (S // len(a))
        for name, t in (("gap_m", g), ("decel_mps2", a)):
            if not all(q >= 0.0 for q in t):
                raise ValueError(f"StopShort.from_physical: {name} must be >= 0 (decel inf: no limit), got {t}")
        rows = [[g[i] / xy_scale, a[i] * dt * dt / xy_scale] for i in range(S)]
        return StopShort(torch.tensor(rows, dtype=torch.float64).to(torch.float32).to(device or "cpu"))

    def __call__(self, traj: torch.Tensor, guide: Guide, out: Optional[torch.Tensor] = None) -> StopResult:
        """traj [rows, H, D] in the MODEL's units (a result before xy scaling), row r against scene r % S of the guide and of the
        params; `out`: where to write -- None allocates, `traj` itself re-times in place.  One launch."""
        if not isinstance(guide, Guide):
            raise TypeError(f"StopShort: `guide` must be a Guide, got {type(guide).__name__}")
        traj = L.require_gpu_f32(traj, "traj")
        params = L.require_gpu_f32(self.params, "fallback.params")
        if params.device != traj.device:
            raise ValueError(f"fallback.params lives on {params.device}, the plan on {traj.device}")
        g = guide.desc(traj)
        rows, H, D = traj.shape
        if out is None:
            out = torch.empty_like(traj)
        elif not (torch.is_tensor(out) and out.shape == traj.shape and out.dtype == torch.float32 and out.device == traj.device and
                  out.is_contiguous()):
            raise ValueError(f"StopShort: out must be a contiguous float32 tensor {tuple(traj.shape)} on {traj.device}")
        first = torch.empty(rows, dtype=torch.int32, device=traj.device)
        status = torch.empty(rows, dtype=torch.int32, device=traj.device)
        stop_at = torch.empty(rows, dtype=torch.float32, device=traj.device)
        after = torch.empty(rows, dtype=torch.int32, device=traj.device)
        records = [None if r is None else r.desc(traj) for r in guide.pointwise()]      # kept alive until the launch is enqueued
        L.check(L.lazy("adx_stop_short")(traj.data_ptr(), C.byref(g), *(None if d is None else C.byref(d) for d in records),
                                         params.data_ptr(), self.scenes, out.data_ptr(),
                                         first.data_ptr(), status.data_ptr(), stop_at.data_ptr(), after.data_ptr(), rows, H, D,
                                         L.stream_ptr(traj.device)), "adx_stop_short")
        return StopResult(out, first, status, stop_at, after)

    def __repr__(self):
        return f"StopShort(params={tuple(self.params.shape)})"


def pointwise(guide: Guide) -> bool:
    """Whether the guide holds a term that names places: discs, planes, a field, a route or capsules (motion limits do not)."""
    return guide.M > 0 or guide.P > 0 or any(r is not None for r in guide.pointwise())
