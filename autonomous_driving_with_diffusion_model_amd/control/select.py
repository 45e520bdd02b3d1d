"""Best-of-K sampling: score K candidate trajectories per scene on the device and keep the best one.

`TrajectorySelector` is one launch of `adx_traj_select` (csrc/select.hip): the costs, the arg-min and the copy of the winning
row run on the GPU with no host decision, so the call can be a node of a captured graph (`GraphedSampler(..., candidates=K)`).
The cost is "selection cost v1" of include/adx.h -- goal distance, smoothness and consensus terms over the xy columns, in the
model's own units (the clamped trajectory before xy scaling).  No reference counterpart: the reference's `train.evaluate`
draws many trajectories for one image only to paint them (train.py:62-90).

Given a `Guide` the call is one launch of `adx_traj_select_guide` instead ("selection cost v2"): the same three terms plus
`w_guide` times what a candidate still violates of the scene's discs and planes -- and of every record the guide holds (guide.py,
RECORDS); a candidate one ulp into a violation is "not free", there is no separate tolerance -- (bit for bit `Guide.cost` of
its row), and, with `hard`, the rule that a candidate which violates nothing beats every candidate that violates something.  `Selection.active` then
holds every candidate's count of violated (waypoint, constraint) pairs and `Selection.blocked` says per scene whether the chosen
plan still violates something -- on the device, where a later node can read it.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from .. import _lib as L
from ..guide import Guide

MAX_CANDIDATES = 64


class Selection(NamedTuple):
    best: torch.Tensor                 # [S, H, D]: the chosen candidate of every scene, bit for bit
    index: torch.Tensor                # [S] int32: which candidate that is
    cost: torch.Tensor                 # [S, K]: every candidate's cost
    candidates: Optional[torch.Tensor] = None   # [K, S, H, D] (generate_traj(..., return_selection=True) only)
    active: Optional[torch.Tensor] = None       # [S, K] int32: violated (waypoint, constraint) pairs (a call with a guide only)
    blocked: Optional[torch.Tensor] = None      # [S] int32: 1 where the chosen candidate is not free (a call with a guide only)


class TrajectorySelector:
    """cost = w_goal * goal + w_smooth * smooth + w_consensus * consensus (include/adx.h, selection cost v1); the
    candidate with the smallest cost wins, ties go to the lowest index, a non-finite cost loses to every finite one.

    Called with a guide (selection cost v2): `+ w_guide * violation`; a candidate is free when it violates nothing and all its
    xy are finite, and with `hard` the search runs over the free candidates with a finite cost alone whenever there is one."""

    def __init__(self, w_goal: float = 1.0, w_smooth: float = 0.0, w_consensus: float = 0.0, w_guide: float = 0.0,
                 hard: bool = False):
        self.w_goal, self.w_smooth, self.w_consensus = float(w_goal), float(w_smooth), float(w_consensus)
        self.w_guide, self.hard = float(w_guide), bool(hard)

    @property
    def uses_guide(self) -> bool:
        """The selector asks for something only a guide can answer: it cannot run without one."""
        return self.w_guide != 0.0 or self.hard

    def __call__(self, trajs: torch.Tensor, scenes: int, target: Optional[torch.Tensor] = None,
                 guide: Optional[Guide] = None) -> Selection:
        """trajs [K * scenes, H, D] in candidate-major order (candidate k of scene s is row k * scenes + s), or
        [K, scenes, H, D]; target None or [scenes, 2] in the units of trajs; guide None (selection cost v1) or a Guide over
        `scenes` scenes on the device of trajs (selection cost v2)."""
        if guide is None and self.uses_guide:
            raise ValueError(f"{self!r} scores against a guide: pass guide=Guide(...)")
        if guide is not None and not isinstance(guide, Guide):
            raise TypeError(f"`guide` must be a Guide or None, got {type(guide).__name__}")
        scenes = int(scenes)
        if trajs.dim() == 4:
            if trajs.shape[1] != scenes:
                raise ValueError(f"trajs {tuple(trajs.shape)} is not [K, {scenes}, H, D]")
            trajs = trajs.reshape(-1, trajs.shape[2], trajs.shape[3])
        if trajs.dim() != 3 or scenes < 1 or trajs.shape[0] % scenes != 0:
            raise ValueError(f"trajs must be [K * {scenes}, H, D], got {tuple(trajs.shape)}")
        trajs = L.require_gpu_f32(trajs, "trajs")
        rows, H, D = trajs.shape
        K = rows // scenes
        if target is not None:
            target = L.require_gpu_f32(target, "target")
            if tuple(target.shape) != (scenes, 2):
                raise ValueError(f"target must be [{scenes}, 2], got {tuple(target.shape)}")
        dev = trajs.device
        cost = torch.empty((scenes, K), dtype=torch.float32, device=dev)
        index = torch.empty((scenes,), dtype=torch.int32, device=dev)
        best = torch.empty((scenes, H, D), dtype=torch.float32, device=dev)
        if guide is not None:
            return self._guided(trajs, scenes, K, target, guide, cost, index, best)
        cfg = L.SelectCfg(scenes, K, H, D, self.w_goal, self.w_smooth, self.w_consensus)
        L.check(L.lib().adx_traj_select(C.byref(cfg), trajs.data_ptr(), L.ptr(target), cost.data_ptr(), index.data_ptr(),
                                        best.data_ptr(), L.stream_ptr(dev)), "adx_traj_select")
        return Selection(best, index, cost)

    def _guided(self, trajs, scenes, K, target, guide, cost, index, best) -> Selection:
        dev = trajs.device
        if guide.scenes is not None and guide.scenes != scenes:
            raise ValueError(f"the guide holds {guide.scenes} scenes; the selection has {scenes}")
        _, H, D = trajs.shape
        active = torch.empty((scenes, K), dtype=torch.int32, device=dev)
        blocked = torch.empty((scenes,), dtype=torch.int32, device=dev)
        cfg = L.SelectGuideCfg(scenes, K, H, D, self.w_goal, self.w_smooth, self.w_consensus, self.w_guide, int(self.hard))
        # the guide's records ride in the same launch, through the export guide.py's `Guide.descs` chooses for them
        suffix, guides, _alive = guide.descs(trajs)      # device, float32 and D >= 2 as every guided launch checks them
        name = "adx_traj_select_guide" + ("" if suffix == "guide" else "_" + suffix)
        L.check(L.lazy(name)(C.byref(cfg), trajs.data_ptr(), L.ptr(target), *guides, cost.data_ptr(), active.data_ptr(),
                             index.data_ptr(), blocked.data_ptr(), best.data_ptr(), L.stream_ptr(dev)), name)
        return Selection(best, index, cost, None, active, blocked)

    def __repr__(self):
        tail = f", w_guide={self.w_guide}, hard={self.hard}" if self.uses_guide else ""
        return f"TrajectorySelector(w_goal={self.w_goal}, w_smooth={self.w_smooth}, w_consensus={self.w_consensus}{tail})"
