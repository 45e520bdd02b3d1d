"""Guide: where a sampling tick must NOT go ("cost guidance v1", include/adx.h).

A guide is what the caller knows of the scene's obstacles -- moving discs (a parked car, a crossing pedestrian) and half-planes (a
stop line, a lane edge) -- per scene, in the model's own units (the units of `target` and of the clamped result before xy
scaling) and in THIS tick's ego frame.  Every sampler step moves the xy of its predicted clean trajectory down the gradient of
the cost of those constraints, inside the step kernel, and derives the rest of the step from the moved x0: analytic cost guidance
as Diffuser-style planners use it, and how the reference's classifier guidance acts for its own PRED_TYPE = "sample".

    discs    [S, M, 5] = (cx, cy, vx, vy, r), M <= 32: at waypoint h the centre is (cx + h * vx, cy + h * vy); a slot with
             r <= 0 (or NaN) is empty, so scenes with fewer obstacles pad with zeros.
    planes   [S, P, 3] = (nx, ny, b), P <= 8: the half-plane nx * x + ny * y <= b is allowed.
    scale    the step size; `schedule` "variance" multiplies it by the step's noise variance (guidance fades as the sample gets
             clean, Diffuser's Sigma-scaling), "constant" uses it as it is.
    cap      the largest move of one coordinate in one iteration (inf: none); `iters`: gradient iterations per step, 1..8.

No reference counterpart as a caller-facing object: the reference names the idea (GUIDANCE.LOSS_LIST) and has one entry, under
CLASSIFIER_GUIDANCE only.  Whether guided plans drive better is a property of trained weights and is not measured in this
repository.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import _lib as L

SCHEDULES = ("variance", "constant")
MAX_DISCS, MAX_PLANES, MAX_ITERS = 32, 8, 8


class Guide:
    """`discs` float32 `[S, M, 5]` and / or `planes` float32 `[S, P, 3]` on one device (None: no such constraint); `scale`,
    `schedule`, `cap`, `iters` as the module docstring says.  The tensors are read at every step: new values need no new object
    (and, in a GraphedSampler, no new capture)."""

    def __init__(self, discs: Optional[torch.Tensor] = None, planes: Optional[torch.Tensor] = None, scale: float = 1.0,
                 schedule: str = "variance", cap: float = float("inf"), iters: int = 1):
        for name, t, last, most in (("discs", discs, 5, MAX_DISCS), ("planes", planes, 3, MAX_PLANES)):
            if t is None:
                continue
            if not torch.is_tensor(t):
                raise TypeError(f"Guide: {name} must be a tensor or None, got {type(t).__name__}")
            if t.dim() != 3 or t.shape[2] != last or t.shape[0] < 1:
                raise ValueError(f"Guide: {name} must be [S, {'M' if last == 5 else 'P'}, {last}], got {tuple(t.shape)}")
            if t.shape[1] > most:
                raise ValueError(f"Guide: at most {most} {name} per scene, got {t.shape[1]}")
            if t.dtype != torch.float32:
                raise TypeError(f"Guide: {name} must be float32, got {t.dtype}")
        if discs is not None and planes is not None:
            if discs.device != planes.device:
                raise ValueError(f"Guide: discs live on {discs.device}, planes on {planes.device}")
            if discs.shape[0] != planes.shape[0]:
                raise ValueError(f"Guide: discs hold {discs.shape[0]} scenes, planes {planes.shape[0]}")
        if schedule not in SCHEDULES:
            raise ValueError(f"Guide: schedule must be one of {SCHEDULES}, got {schedule!r}")
        scale, cap = float(scale), float(cap)
        if math.isnan(scale):
            raise ValueError("Guide: scale is NaN")
        if not cap >= 0.0:
            raise ValueError(f"Guide: cap must be >= 0 (inf: no cap), got {cap}")
        if int(iters) != iters or not 1 <= int(iters) <= MAX_ITERS:
            raise ValueError(f"Guide: iters must be an integer in 1..{MAX_ITERS}, got {iters!r}")
        self.discs = None if discs is None else discs.contiguous()
        self.planes = None if planes is None else planes.contiguous()
        self.scale, self.schedule, self.cap, self.iters = scale, schedule, cap, int(iters)

    # ---- shape ----
    @property
    def M(self) -> int:
        return 0 if self.discs is None else int(self.discs.shape[1])

    @property
    def P(self) -> int:
        return 0 if self.planes is None else int(self.planes.shape[1])

    @property
    def scenes(self) -> Optional[int]:
        """S of the tensors; None for a guide without any (which fits every batch)."""
        t = self.discs if self.discs is not None else self.planes
        return None if t is None else int(t.shape[0])

    @property
    def device(self) -> Optional[torch.device]:
        t = self.discs if self.discs is not None else self.planes
        return None if t is None else t.device

    def key(self) -> tuple:
        """What a captured graph bakes: everything but the values of discs and planes."""
        return (self.M, self.P, self.scale, self.schedule, self.cap, self.iters)

    def like(self, discs: Optional[torch.Tensor], planes: Optional[torch.Tensor]) -> "Guide":
        """The same settings over other tensors."""
        return Guide(discs, planes, self.scale, self.schedule, self.cap, self.iters)

    # ---- launches ----
    def desc(self, x: torch.Tensor, lam: float = 0.0) -> L.GuideDesc:
        """The `adx_guide` of a launch on `x` [B, H, D] with lambda = `lam` (a scheduler's `guide_level`).  The struct holds
        addresses: keep this object alive until the launch is enqueued."""
        S = self.scenes
        for name, t in (("guide.discs", self.discs), ("guide.planes", self.planes)):
            if t is not None and (L.require_gpu_f32(t, name).device != x.device):
                raise ValueError(f"{name} lives on {t.device}, the sample on {x.device}")
        if x.dim() != 3 or x.shape[2] < 2 or (S is not None and x.shape[0] % S != 0):
            raise ValueError(f"the guide holds {S} scenes; the sample is {tuple(x.shape)}: [B, H, D] with D >= 2 and rows a multiple "
                             "of the guide's scenes")
        g = L.GuideDesc()
        g.discs, g.planes = L.ptr(self.discs), L.ptr(self.planes)
        g.scene_rows, g.n_discs, g.n_planes = 1 if S is None else S, self.M, self.P
        g.iters, g.lambda_, g.cap = self.iters, float(lam), self.cap
        return g

    def cost(self, traj: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """What a plan still violates, one launch of `adx_guide_cost`: `(cost [rows] float32, active [rows] int32)` of `traj`
        [rows, H, D] -- the contract's cost summed over a row's waypoints and the number of active (waypoint, constraint) pairs.
        `traj` is in the MODEL's units: a result before xy scaling (`scale_xy=False`, `warm.prev`), row r against scene r % S."""
        traj = L.require_gpu_f32(traj, "traj")
        g = self.desc(traj)
        rows, H, D = traj.shape
        cost = torch.empty(rows, dtype=torch.float32, device=traj.device)
        active = torch.empty(rows, dtype=torch.int32, device=traj.device)
        L.check(L.lazy("adx_guide_cost")(traj.data_ptr(), C.byref(g), cost.data_ptr(), active.data_ptr(), rows, H, D,
                                         L.stream_ptr(traj.device)), "adx_guide_cost")
        return cost, active

    def __repr__(self):
        return (f"Guide(discs={None if self.discs is None else tuple(self.discs.shape)}, "
                f"planes={None if self.planes is None else tuple(self.planes.shape)}, scale={self.scale}, schedule={self.schedule!r}, "
                f"cap={self.cap}, iters={self.iters})")
