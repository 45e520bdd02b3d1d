"""Manoeuvre commitment: hold the manoeuvre the previous tick chose unless the selector's new choice is clearly better.

A selector that takes the arg-min of a cost over fresh samples can change its mind on sampling noise alone wherever two
manoeuvres cost nearly the same (pass left / pass right, go / yield), and the controller then steers after another plan every
tick.  `ManoeuvreCommit.__call__` is one launch of `adx_traj_commit` (csrc/commit.hip, "manoeuvre commitment v1" of
include/adx.h) directly after selection: the plan chosen on the last tick, moved on by `shift` waypoints and the odometry exactly
as a warm start moves it, is the prior; the candidates within `radius` of it (mean squared xy distance over the waypoints from
`h0` on) are the same manoeuvre; and the cheapest of those is kept while its cost is at most
`(cost[sel] + margin) + ratio * |cost[sel]|` -- at most `max_hold` ticks in a row when `max_hold` > 0.  A follower that violates
the guide never replaces a winner that does not.  The previous plan, a validity flag and the hold counter live in one device
buffer the launch reads and advances through its address, so the call can be a node of a captured graph
(`GraphedSampler(..., commit=...)`) and the first tick is the same node as every later one.  Whether commitment makes a trained
model drive better is a property of the weights and of the closed loop and is not measured in this repository.  No reference
counterpart: the reference samples one trajectory per tick (interact.py:110-140).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import torch

from .. import _lib as L
from .select import Selection

MAX_CANDIDATES = 64
MAX_HORIZON = 64
NO_PRIOR, SAME, LOST, HELD, SWITCHED = 0, 1, 2, 3, 4      # `status`: the rule of the contract's table that decided the scene


class CommitResult(NamedTuple):
    best: Optional[torch.Tensor]       # [S, H, D]: the committed plan of every scene, a candidate's row bit for bit (None in a
                                       # tick's `last`: the tick returned it)
    index: torch.Tensor                # [S] int32: which candidate that is (the selector's own: `ManoeuvreCommit.selected`)
    status: torch.Tensor               # [S] int32: NO_PRIOR, SAME, LOST, HELD or SWITCHED
    follower: torch.Tensor             # [S] int32: the cheapest eligible candidate near the prior, -1 where none was formed
    dist2: torch.Tensor                # [S, K]: every candidate's distance to the prior (unspecified without a prior)
    blocked: Optional[torch.Tensor] = None      # [S] int32: 1 where the committed plan is not free (a guided selection only)


class ManoeuvreCommit:
    """The commitment state of `scenes` agents over a horizon of `horizon` waypoints on `device`, and the rule's settings.

    `radius` is in the units of the trajectories: the default is the open-loop metrics' 2 m miss radius in model units
    (2 / `model.magic_num`).  `margin` and `ratio`: how much cheaper than the follower, absolutely and relative to its own cost,
    the selector's choice must be to take over.  `max_hold`: 0 = no limit.  `h0` = 1: waypoint 0 is the ego pose the sampling
    loops zero.  `shift`: the waypoints the vehicle passed between two ticks; None reads EVAL.WARM_SHIFT (default 1) when a tick
    is planned, and 1 in a direct call.  `state` is the int32 buffer [S, 2 + 2H] of the contract; `valid`, `held` and `prior` are
    views of it.  An object on a CPU device can be built and planned with; its launches refuse (there is no CPU path).  `last`:
    the CommitResult of the last tick this object ran in (`generate_traj(..., commit=...)`) without `best`, which the tick
    returned; `selected`: the selector's own index [S] of that tick (it differs from `last.index` exactly where the status is
    HELD)."""

    def __init__(self, scenes: int, horizon: int, device, *, radius: float = 2.0 / 23.315, margin: float = 0.0, ratio: float = 0.1,
                 max_hold: int = 0, h0: int = 1, shift: Optional[int] = None):
        scenes, horizon, max_hold, h0 = int(scenes), int(horizon), int(max_hold), int(h0)
        radius, margin, ratio = float(radius), float(margin), float(ratio)
        if not 1 <= scenes <= 65535:
            raise ValueError(f"ManoeuvreCommit: scenes must be 1..65535, got {scenes}")
        if not 2 <= horizon <= MAX_HORIZON:
            raise ValueError(f"ManoeuvreCommit: horizon must be 2..{MAX_HORIZON}, got {horizon}")
        for name, v in (("radius", radius), ("margin", margin), ("ratio", ratio)):
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"ManoeuvreCommit: {name} must be finite and >= 0, got {v}")
        if max_hold < 0:
            raise ValueError(f"ManoeuvreCommit: max_hold must be >= 0, got {max_hold}")
        if not 0 <= h0 <= horizon - 1:
            raise ValueError(f"ManoeuvreCommit: h0 must be 0..{horizon - 1} (horizon - 1), got {h0}")
        if shift is not None:
            shift = int(shift)
            if not 0 <= shift <= horizon - 1:
                raise ValueError(f"ManoeuvreCommit: shift must be 0..{horizon - 1} (horizon - 1), got {shift}")
        self.scenes, self.horizon, self.device = scenes, horizon, torch.device(device)
        self.radius, self.margin, self.ratio, self.max_hold, self.h0, self.shift = radius, margin, ratio, max_hold, h0, shift
        if self.device.type == "cuda" and self.device.index is None:      # "cuda" names the current device; tensors say "cuda:0"
            self.device = torch.device("cuda", torch.cuda.current_device())
        nbytes = int(L.lazy("adx_commit_state_bytes")(scenes, horizon))
        if nbytes != scenes * (2 + 2 * horizon) * 4:
            raise L.AdxError(f"adx_commit_state_bytes({scenes}, {horizon}) = {nbytes}: not the state of manoeuvre commitment v1")
        self.state = torch.zeros((scenes, 2 + 2 * horizon), dtype=torch.int32, device=self.device)
        self.last: Optional[CommitResult] = None
        self.selected: Optional[torch.Tensor] = None

    # ---- views of the state -------------------------------------------------------------------------------------------------
    @property
    def valid(self) -> torch.Tensor:
        """[S] int32, a view: not 0 where the state holds a plan."""
        return self.state[:, 0]

    @property
    def held(self) -> torch.Tensor:
        """[S] int32, a view: the consecutive ticks the node has overridden the selector."""
        return self.state[:, 1]

    @property
    def prior(self) -> torch.Tensor:
        """[S, H, 2] float32, a view: x and y of the plan chosen on the last tick, in that tick's frame."""
        return self.state[:, 2:].view(torch.float32).view(self.scenes, self.horizon, 2)

    # ---- what a captured graph bakes in ------------------------------------------------------------------------------------
    def key(self) -> tuple:
        """Every by-value setting of the node, and the address of the state it reads and advances."""
        return ("commit_v1", self.scenes, self.horizon, self.radius, self.margin, self.ratio, self.max_hold, self.h0, self.shift,
                self.state.data_ptr())

    def resolve_shift(self, cfg=None) -> int:
        if self.shift is not None:
            return self.shift
        return 1 if cfg is None else int(getattr(cfg.EVAL, "WARM_SHIFT", 1))

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """A fresh state for every scene, or for the scenes where `mask` [S] (bool or uint8, on the device) is set: their next
        tick is NO_PRIOR.  A launch on the current stream, capturable.  Call it after a scene cut or a teleport."""
        if mask is not None:
            if not torch.is_tensor(mask) or tuple(mask.shape) != (self.scenes,) or mask.device != self.device or \
                    mask.dtype not in (torch.bool, torch.uint8):
                what = (tuple(mask.shape), mask.dtype, mask.device) if torch.is_tensor(mask) else type(mask).__name__
                raise ValueError(f"mask must be [{self.scenes}] bool or uint8 on {self.device}, got {what}")
            mask = mask.contiguous().view(torch.uint8)
        L.require_gpu_f32(self.state, "the commit state", torch.int32)      # there is no CPU path
        L.check(L.lazy("adx_commit_reset")(self.state.data_ptr(), self.scenes, self.horizon, L.ptr(mask), L.stream_ptr(self.device)),
                "adx_commit_reset")

    def state_snapshot(self) -> torch.Tensor:
        return self.state.clone()

    def state_restore(self, snapshot: torch.Tensor) -> None:
        if snapshot.shape != self.state.shape or snapshot.dtype != self.state.dtype:
            raise ValueError("state_restore: not a snapshot of this ManoeuvreCommit")
        self.state.copy_(snapshot)

    def __call__(self, trajs: torch.Tensor, scenes: int, selection: Selection, motion: Optional[torch.Tensor] = None,
                 shift: Optional[int] = None) -> CommitResult:
        """trajs [K * scenes, H, D] in candidate-major order (candidate k of scene s is row k * scenes + s), or
        [K, scenes, H, D]: the clamped, unscaled candidates the selector scored; `selection`: what it returned (`cost`, `index` and,
        from a guided call, `active` are read); `motion` [scenes, 3] = (tx, ty, phi) as a warm start takes it, or None; `shift`
        overrides the object's for this call.  One launch on the current stream; the state moves on one tick."""
        if not torch.is_tensor(trajs):
            raise TypeError(f"ManoeuvreCommit: trajs must be a tensor, got {type(trajs).__name__}")
        if not isinstance(selection, Selection):
            raise TypeError(f"ManoeuvreCommit: selection must be a Selection, got {type(selection).__name__}")
        scenes = int(scenes)
        if trajs.dim() == 4:
            if trajs.shape[1] != scenes:
                raise ValueError(f"trajs {tuple(trajs.shape)} is not [K, {scenes}, H, D]")
            trajs = trajs.reshape(-1, trajs.shape[2], trajs.shape[3])
        if trajs.dim() != 3 or scenes < 1 or trajs.shape[0] == 0 or trajs.shape[0] % scenes != 0:
            raise ValueError(f"trajs must be [K * {scenes}, H, D], got {tuple(trajs.shape)}")
        rows, H, D = (int(v) for v in trajs.shape)
        K = rows // scenes
        if scenes != self.scenes or H != self.horizon:
            raise ValueError(f"ManoeuvreCommit: the state holds {self.scenes} scenes over a horizon of {self.horizon}, the call has "
                             f"{scenes} over {H}")
        if K > MAX_CANDIDATES:
            raise ValueError(f"ManoeuvreCommit: {K} candidates per scene, supported 1..{MAX_CANDIDATES}")
        shift = self.resolve_shift() if shift is None else int(shift)
        if not 0 <= shift <= H - 1:
            raise ValueError(f"ManoeuvreCommit: shift must be 0..{H - 1} (horizon - 1), got {shift}")
        trajs = L.require_gpu_f32(trajs, "trajs")
        dev = trajs.device
        if dev != self.device:
            raise ValueError(f"ManoeuvreCommit: the state lives on {self.device}, trajs on {dev}")
        cost = L.require_gpu_f32(selection.cost, "selection.cost")
        sel = L.require_gpu_f32(selection.index, "selection.index", torch.int32)
        if tuple(cost.shape) != (scenes, K) or tuple(sel.shape) != (scenes,):
            raise ValueError(f"selection must hold cost [{scenes}, {K}] and index [{scenes}], got {tuple(cost.shape)} and "
                             f"{tuple(sel.shape)}")
        active = selection.active
        if active is not None:
            active = L.require_gpu_f32(active, "selection.active", torch.int32)
            if tuple(active.shape) != (scenes, K):
                raise ValueError(f"selection.active must be [{scenes}, {K}], got {tuple(active.shape)}")
        if motion is not None:
            motion = L.require_gpu_f32(motion, "motion")
            if tuple(motion.shape) != (scenes, 3):
                raise ValueError(f"motion must be [{scenes}, 3] = (tx, ty, phi) per scene, got {tuple(motion.shape)}")
        best = torch.empty((scenes, H, D), dtype=torch.float32, device=dev)
        index = torch.empty((scenes,), dtype=torch.int32, device=dev)
        status = torch.empty((scenes,), dtype=torch.int32, device=dev)
        follower = torch.empty((scenes,), dtype=torch.int32, device=dev)
        blocked = None if active is None else torch.empty((scenes,), dtype=torch.int32, device=dev)
        dist2 = torch.empty((scenes, K), dtype=torch.float32, device=dev)
        cfg = L.CommitCfg(scenes, K, H, D, self.h0, shift, self.max_hold, self.radius, self.margin, self.ratio)
        L.check(L.lazy("adx_traj_commit")(C.byref(cfg), trajs.data_ptr(), cost.data_ptr(), sel.data_ptr(), L.ptr(active), L.ptr(motion),
                                          self.state.data_ptr(), best.data_ptr(), index.data_ptr(), status.data_ptr(),
                                          follower.data_ptr(), L.ptr(blocked), dist2.data_ptr(), L.stream_ptr(dev)), "adx_traj_commit")
        return CommitResult(best, index, status, follower, dist2, blocked)

    def __repr__(self):
        return (f"ManoeuvreCommit(scenes={self.scenes}, horizon={self.horizon}, radius={self.radius}, margin={self.margin}, "
                f"ratio={self.ratio}, max_hold={self.max_hold}, h0={self.h0}, shift={self.shift}, device={self.device})")
