"""Trajectory modes: which different manoeuvres a scene's K candidates contain, and how much of the sample mass backs each one.

`TrajectoryModes.__call__` is one launch of `adx_traj_modes` (csrc/modes.hip, "trajectory modes v1" of include/adx.h): the
pairwise distances of a scene's candidates, a greedy cover under a radius -- the candidate with the most neighbours becomes a
mode, takes its neighbours with it, and the same runs on what is left -- and the copy of the representatives' rows all run on the
GPU with no host decision, so the call can be a node of a captured graph (`GraphedSampler(..., modes=...)`).  The distance is the
mean squared xy distance over the waypoints from `h0` on, in the units of the trajectories handed in.  The mode rows come back
mode-major (`[M, S, H, D]`), which is the candidate-major layout of an M-candidate set: they go into `TrajectorySelector`,
`OpenLoopMetrics.update` and `Guide.cost` as they are.  A greedy cover and not k-means: it is exact, deterministic and needs no
convergence test.  No reference counterpart: the reference's `train.evaluate` draws many trajectories for one image only to
paint them (train.py:62-90).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import torch

from .. import _lib as L

MAX_CANDIDATES = 64
MAX_MODES = 64
MAX_HORIZON = 64
OUTLIER, NON_FINITE = -1, -2          # `assign` of a candidate no mode took, and of one with a non-finite scored xy


class ModeSet(NamedTuple):
    modes: torch.Tensor                # [M, S, H, D]: the representatives' rows bit for bit; slots past `count` repeat mode 0
    index: torch.Tensor                # [S, M] int32: which candidate represents mode m, -1 past `count`
    mass: torch.Tensor                 # [S, M] int32: how many candidates the mode took, non-increasing, 0 past `count`
    assign: torch.Tensor               # [S, K] int32: every candidate's mode; -1 an outlier, -2 not finite
    count: torch.Tensor                # [S] int32: the modes formed
    dist2: Optional[torch.Tensor] = None      # [S, K, K]: the pairwise distances (a call with dist2=True only)

    def prob(self) -> torch.Tensor:
        """[S, M] float32: mass over the scene's number of finite candidates (0 everywhere in a scene that has none).  Device
        arithmetic alone: nothing is read."""
        finite = (self.assign != NON_FINITE).sum(dim=1, keepdim=True).clamp(min=1)
        return self.mass.to(torch.float32) / finite.to(torch.float32)


class TrajectoryModes:
    """Up to `max_modes` modes per scene; two candidates are near when the mean squared xy distance of their waypoints `h0`..H-1
    is at most `radius`^2 (include/adx.h, trajectory modes v1).  `radius` is in the units of the trajectories: the default is the
    open-loop metrics' 2 m miss radius in model units (2 / `model.magic_num`).  `h0` = 1: waypoint 0 is the ego pose the sampling
    loops zero.  `last`: the ModeSet of the last tick this object ran in (`generate_traj(..., modes=...)`), in model units."""

    def __init__(self, max_modes: int = 6, radius: float = 2.0 / 23.315, h0: int = 1):
        max_modes, radius, h0 = int(max_modes), float(radius), int(h0)
        if not 1 <= max_modes <= MAX_MODES:
            raise ValueError(f"TrajectoryModes: max_modes must be 1..{MAX_MODES}, got {max_modes}")
        if not (math.isfinite(radius) and radius >= 0.0):
            raise ValueError(f"TrajectoryModes: radius must be finite and >= 0, got {radius}")
        if not 0 <= h0 < MAX_HORIZON:
            raise ValueError(f"TrajectoryModes: h0 must be 0..{MAX_HORIZON - 1}, got {h0}")
        self.max_modes, self.radius, self.h0 = max_modes, radius, h0
        self.last: Optional[ModeSet] = None

    def key(self) -> tuple:
        """What a captured graph bakes: every setting (they are by-value arguments of the node)."""
        return ("modes_v1", self.max_modes, self.radius, self.h0)

    def __call__(self, trajs: torch.Tensor, scenes: int, dist2: bool = False) -> ModeSet:
        """trajs [K * scenes, H, D] in candidate-major order (candidate k of scene s is row k * scenes + s), or
        [K, scenes, H, D]; `dist2`: also return the [scenes, K, K] distances.  One launch on the current stream."""
        if not torch.is_tensor(trajs):
            raise TypeError(f"TrajectoryModes: trajs must be a tensor, got {type(trajs).__name__}")
        scenes = int(scenes)
        if trajs.dim() == 4:
            if trajs.shape[1] != scenes:
                raise ValueError(f"trajs {tuple(trajs.shape)} is not [K, {scenes}, H, D]")
            trajs = trajs.reshape(-1, trajs.shape[2], trajs.shape[3])
        if trajs.dim() != 3 or scenes < 1 or trajs.shape[0] == 0 or trajs.shape[0] % scenes != 0:
            raise ValueError(f"trajs must be [K * {scenes}, H, D], got {tuple(trajs.shape)}")
        rows, H, D = (int(v) for v in trajs.shape)
        K = rows // scenes
        if K > MAX_CANDIDATES:
            raise ValueError(f"TrajectoryModes: {K} candidates per scene, supported 1..{MAX_CANDIDATES}")
        if not 1 <= H <= MAX_HORIZON:
            raise ValueError(f"TrajectoryModes: horizon {H}, supported 1..{MAX_HORIZON}")
        if self.h0 > H - 1:
            raise ValueError(f"TrajectoryModes: h0 = {self.h0} leaves no waypoint of a horizon of {H} to score")
        trajs = L.require_gpu_f32(trajs, "trajs")
        dev, M = trajs.device, self.max_modes
        modes = torch.empty((M, scenes, H, D), dtype=torch.float32, device=dev)
        index = torch.empty((scenes, M), dtype=torch.int32, device=dev)
        mass = torch.empty((scenes, M), dtype=torch.int32, device=dev)
        assign = torch.empty((scenes, K), dtype=torch.int32, device=dev)
        count = torch.empty((scenes,), dtype=torch.int32, device=dev)
        d2 = torch.empty((scenes, K, K), dtype=torch.float32, device=dev) if dist2 else None
        cfg = L.ModesCfg(scenes, K, H, D, M, self.h0, self.radius)
        L.check(L.lazy("adx_traj_modes")(C.byref(cfg), trajs.data_ptr(), modes.data_ptr(), index.data_ptr(), mass.data_ptr(),
                                         assign.data_ptr(), count.data_ptr(), L.ptr(d2), L.stream_ptr(dev)), "adx_traj_modes")
        return ModeSet(modes, index, mass, assign, count, d2)

    def __repr__(self):
        return f"TrajectoryModes(max_modes={self.max_modes}, radius={self.radius}, h0={self.h0})"
