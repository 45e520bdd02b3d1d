"""Open-loop evaluation: how far sampled plans lie from logged waypoints, measured on the device.

`OpenLoopMetrics.update` is two launches (csrc/metrics.hip, "open-loop metrics v1" of include/adx.h): `adx_traj_metrics` scores
every candidate of every scene of a batch -- ADE / FDE per candidate, the best candidate, the record of the chosen one -- and
`adx_metrics_accumulate` folds the batch into a device-resident state of fp64 sums and int64 counts.  Neither decides anything on
the host, allocates outside torch's caching allocator or synchronises, so both can follow a sampling tick (or a GraphedSampler
replay, or be captured themselves); `compute()` is the one device-to-host copy, at the end.  No reference counterpart: the
reference's `train.evaluate` paints dots on a BEV image (train.py:62-90).

`evaluate_open_loop` walks a loader of the dataset reader (`dataset.get_loader`: frames, logged waypoints, target points) through
`generate_traj` and returns `compute()`: ADE / FDE of the plan that was chosen, minADE_K / minFDE_K over the candidates, the miss
rates, what the selector loses against the best candidate, the displacement per waypoint.  Distances are metres: `xy_scale` turns
the model's units into them (`model.magic_num`).  With `modes=TrajectoryModes(...)` the tick also clusters each scene's candidates
(control/modes.py) and a second `OpenLoopMetrics` scores the M modes as an M-candidate set whose chosen plan is mode 0, the
heaviest: minADE over M modes -- the figure motion-prediction work is compared on -- and the majority-vote plan beside the
selector's.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, NamedTuple, Optional

import torch

from . import _lib as L
from .control.modes import OUTLIER, TrajectoryModes
from .control.select import MAX_CANDIDATES, Selection
from .guide import Guide

MAX_HORIZON = 64
XY_SCALE = 23.315          # model.magic_num: metres per model unit
# the state's words (include/adx.h, "Accumulation")
_SCORED, _NONFINITE, _HEADING, _AGREE, _BLOCKED, _REC, _REGRET, _ALONG, _CROSS, _DISP, _DISP_COUNT = 0, 1, 2, 3, 4, 5, 13, 14, 15, 16, 80
REC_FIELDS = ("min_ade", "min_fde", "sel_ade", "sel_fde", "along", "cross", "miss_sel", "miss_any")
FLAG_SCORED, FLAG_HEADING, FLAG_FINITE = 1, 2, 4


class MetricsBatch(NamedTuple):
    """What one `adx_traj_metrics` launch wrote (device tensors; nothing has been read)."""
    ade: torch.Tensor          # [S, K] metres
    fde: torch.Tensor          # [S, K]
    best: torch.Tensor         # [S] int32: arg-min of ade
    rec: torch.Tensor          # [S, 8]: REC_FIELDS
    flags: torch.Tensor        # [S] int32: FLAG_SCORED | FLAG_HEADING | FLAG_FINITE | n << 8 | h0 << 16
    disp_sel: torch.Tensor     # [S, H]: the chosen candidate's displacement per waypoint


def _int32(t: Optional[torch.Tensor], name: str, scenes: int, dev) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = L.require_gpu_f32(t, name, torch.int32)
    if tuple(t.shape) != (scenes,) or t.device != dev:
        raise ValueError(f"{name} must be int32 [{scenes}] on {dev}, got {tuple(t.shape)} on {t.device}")
    return t


class OpenLoopMetrics:
    """Running open-loop metrics over batches of `(candidates, logged waypoints)`.

    `h0`: the first scored waypoint (1: waypoint 0 is the ego pose the sampling loops zero); `miss_radius` in metres; `xy_scale`:
    metres per unit of the trajectories handed to `update` (`model.magic_num` for a result before xy scaling, 1.0 for metres)."""

    def __init__(self, h0: int = 1, miss_radius: float = 2.0, xy_scale: float = XY_SCALE):
        self.h0, self.miss_radius, self.xy_scale = int(h0), float(miss_radius), float(xy_scale)
        self.state: Optional[torch.Tensor] = None          # int64 words on the device of the first update
        self.horizon: Optional[int] = None

    def _state_on(self, dev, H: int) -> torch.Tensor:
        if self.state is None:
            words = L.lib().adx_metrics_state_bytes() // 8
            self.state = torch.zeros(words, dtype=torch.int64, device=dev)       # all zero bytes: empty
        if self.horizon is None:
            self.horizon = H
        if self.state.device != dev or self.horizon != H:
            raise ValueError(f"OpenLoopMetrics: the state holds horizon {self.horizon} on {self.state.device}, this batch is horizon "
                             f"{H} on {dev}; reset() first, or use a metrics object of its own")
        return self.state

    def update(self, trajs: torch.Tensor, gt: torch.Tensor, valid: Optional[torch.Tensor] = None,
               selection: Optional[Selection] = None, index: Optional[torch.Tensor] = None,
               blocked: Optional[torch.Tensor] = None) -> MetricsBatch:
        """trajs [K * S, H, D] candidate-major (candidate k of scene s is row k * S + s) or [K, S, H, D], in the units `xy_scale`
        turns into metres; gt [S, H, 2] (or [S, H, D]: the first two columns) in the same units; valid None or int32 [S]: how many
        logged waypoints count; `selection`: a Selection whose `index` (and `blocked`, when it has one) name the chosen candidate,
        or `index` / `blocked` int32 [S] themselves; neither: candidate 0.  Two launches, no synchronisation."""
        gt = L.require_gpu_f32(gt, "gt")
        if gt.dim() != 3 or gt.shape[2] < 2:
            raise ValueError(f"gt must be [S, H, 2] (or [S, H, D]: x, y first), got {tuple(gt.shape)}")
        if gt.shape[2] != 2:
            gt = gt[:, :, :2].contiguous()
        S, H = int(gt.shape[0]), int(gt.shape[1])
        if trajs.dim() == 4:
            if trajs.shape[1] != S:
                raise ValueError(f"trajs {tuple(trajs.shape)} is not [K, {S}, H, D]")
            trajs = trajs.reshape(-1, trajs.shape[2], trajs.shape[3])
        if trajs.dim() != 3 or S < 1 or trajs.shape[0] % S != 0 or trajs.shape[1] != H:
            raise ValueError(f"trajs must be [K * {S}, {H}, D], got {tuple(trajs.shape)}")
        trajs = L.require_gpu_f32(trajs, "trajs")
        dev = trajs.device
        if gt.device != dev:
            raise ValueError(f"gt lives on {gt.device}, trajs on {dev}")
        K, D = trajs.shape[0] // S, int(trajs.shape[2])
        if selection is not None:
            if index is not None:
                raise ValueError("OpenLoopMetrics.update: pass `selection` or `index`, not both")
            index = selection.index
            blocked = selection.blocked if blocked is None else blocked
        valid, index, blocked = (_int32(t, n, S, dev) for t, n in ((valid, "valid"), (index, "index"), (blocked, "blocked")))
        state = self._state_on(dev, H)
        out = MetricsBatch(torch.empty((S, K), dtype=torch.float32, device=dev), torch.empty((S, K), dtype=torch.float32, device=dev),
                           torch.empty((S,), dtype=torch.int32, device=dev), torch.empty((S, len(REC_FIELDS)), dtype=torch.float32, device=dev),
                           torch.empty((S,), dtype=torch.int32, device=dev), torch.empty((S, H), dtype=torch.float32, device=dev))
        cfg = L.MetricsCfg(S, K, H, D, self.h0, self.miss_radius, self.xy_scale)
        stream = L.stream_ptr(dev)
        L.check(L.lib().adx_traj_metrics(C.byref(cfg), trajs.data_ptr(), gt.data_ptr(), L.ptr(valid), L.ptr(index), out.ade.data_ptr(),
                                         out.fde.data_ptr(), out.best.data_ptr(), out.rec.data_ptr(), out.flags.data_ptr(),
                                         out.disp_sel.data_ptr(), stream), "adx_traj_metrics")
        L.check(L.lib().adx_metrics_accumulate(state.data_ptr(), out.rec.data_ptr(), out.flags.data_ptr(), out.best.data_ptr(),
                                               L.ptr(index), out.disp_sel.data_ptr(), L.ptr(blocked), S, H, stream),
                "adx_metrics_accumulate")
        return out

    def reset(self) -> None:
        """An empty state (a capturable launch); the next update may have another horizon."""
        if self.state is not None:
            L.check(L.lib().adx_metrics_reset(self.state.data_ptr(), L.stream_ptr(self.state.device)), "adx_metrics_reset")
        self.horizon = None

    def words(self):
        """The state on the host, one device-to-host copy: `(counts, sums)`, two NumPy arrays over the state's words (int64 and
        float64 views of the same bytes; include/adx.h says which word is which)."""
        import numpy as np
        if self.state is None:
            raw = np.zeros(16 + 2 * MAX_HORIZON, dtype=np.int64)
        else:
            raw = self.state.cpu().numpy()
        return raw, raw.view(np.float64)

    def compute(self) -> dict:
        """The metrics so far.  `n` scenes enter the averages: the scored ones whose chosen plan is finite (`nonfinite` counts the
        others).  An average over nothing is NaN."""
        counts, sums = self.words()
        n = int(counts[_SCORED] - counts[_NONFINITE])
        n_heading = int(counts[_HEADING])
        mean = lambda v, d: float(v) / d if d > 0 else float("nan")      # noqa: E731
        rec = {name: mean(sums[_REC + i], n) for i, name in enumerate(REC_FIELDS)}
        H = self.horizon or 0
        return {"n": n, "scored": int(counts[_SCORED]), "nonfinite": int(counts[_NONFINITE]),
                "ade": rec["sel_ade"], "fde": rec["sel_fde"], "min_ade_k": rec["min_ade"], "min_fde_k": rec["min_fde"],
                "miss_rate": rec["miss_sel"], "miss_rate_any": rec["miss_any"],
                "selector_regret": mean(sums[_REGRET], n), "selector_agreement": mean(int(counts[_AGREE]), n),
                "along": rec["along"], "cross": rec["cross"],
                "along_abs": mean(sums[_ALONG], n_heading), "cross_abs": mean(sums[_CROSS], n_heading), "heading_valid": n_heading,
                "blocked_rate": mean(int(counts[_BLOCKED]), n),
                "disp_at": [mean(sums[_DISP + h], int(counts[_DISP_COUNT + h])) for h in range(H)],
                "units": {"distance": "m", "xy_scale": self.xy_scale, "miss_radius_m": self.miss_radius, "h0": self.h0}}


def evaluate_open_loop(model, scheduler, cfg, loader, *, candidates: int = 1, selector=None, noise=None, warm=None,
                       guide_fn: Optional[Callable] = None, graphed: bool = False, max_batches: Optional[int] = None,
                       metrics: Optional[OpenLoopMetrics] = None, modes: Optional[TrajectoryModes] = None) -> dict:
    """Open-loop metrics of `generate_traj` over `loader`, whose batches are `(image, waypoints [B, H, D], target [B, 2])` as
    `dataset.get_loader` yields them (uint8 HWC frames go through `ops.image_transform` on the device; float frames are taken as
    they are).  Per batch: one tick (`generate_traj(..., scale_xy=False, return_selection=True)`, or a `GraphedSampler` replay
    with `graphed=True`), then the two metrics launches on the K candidates against the logged waypoints; the chosen candidate
    and `blocked` are the Selection's where there is one, and `Guide.cost`'s `active > 0` of the plan where a guide ran without a
    selector that reads it.  `guide_fn(batch) -> Guide | None` supplies a batch's logged obstacles.  `metrics`: an OpenLoopMetrics
    to fold into (default: a fresh one, h0 = 1, miss radius 2 m, `model.magic_num`).  Nothing inside the loop reads the device;
    the call returns `metrics.compute()`.

    `modes`: a TrajectoryModes (K > 1) the tick runs with; each batch's mode set is folded into a second OpenLoopMetrics (the
    settings of `metrics`) with the M modes as the candidates and mode 0 as the chosen one.  The returned dict then has one more
    entry, `"modes"`: `m`; `min_ade_m`, `min_fde_m`, `miss_rate_any_m` over the modes; `top_ade`, `top_fde`, `top_miss_rate` of
    mode 0 (the majority-vote plan, to read beside `ade`); `mean_count` (modes formed per scene), `mean_top_prob` (mode 0's share
    of the finite candidates) and `outlier_rate` (candidates no mode took, over all candidates) -- means over every scene of the
    run, accumulated with device-side adds."""
    from . import ops
    from .misc.constant import GuidanceType
    from .sampling import GraphedSampler, generate_traj
    K = int(candidates)
    if not 1 <= K <= MAX_CANDIDATES:
        raise ValueError(f"candidates must be 1..{MAX_CANDIDATES}, got {K}")
    if metrics is None:
        metrics = OpenLoopMetrics(xy_scale=float(model.magic_num))
    if modes is not None and not isinstance(modes, TrajectoryModes):
        raise TypeError(f"evaluate_open_loop: `modes` must be a TrajectoryModes, got {type(modes).__name__}")
    dev = next(model.parameters()).device
    mode_metrics = None if modes is None else OpenLoopMetrics(metrics.h0, metrics.miss_radius, metrics.xy_scale)
    mode_sums = None if modes is None else torch.zeros(3, dtype=torch.float64, device=dev)   # count, top prob, outliers
    mode_scenes = 0
    with_target = GuidanceType[cfg.GUIDANCE.USE_COND] != GuidanceType.NO_GUIDANCE
    sampler = GraphedSampler(model, scheduler, cfg, scale_xy=False, noise=noise, candidates=K, selector=selector, warm=warm,
                             modes=modes) if graphed else None
    for i, batch in enumerate(loader):
        if max_batches is not None and i >= max_batches:
            break
        image, wps, target = batch[0], batch[1], batch[2]
        image = image.to(dev, non_blocking=True)
        if image.dtype == torch.uint8:
            image = ops.image_transform(image)
        gt = wps.to(dev, non_blocking=True).to(torch.float32)
        tgt = target.to(dev, non_blocking=True).to(torch.float32) if with_target else None
        guide = None if guide_fn is None else guide_fn(batch)
        if guide is not None and not isinstance(guide, Guide):
            raise TypeError(f"guide_fn must return a Guide or None, got {type(guide).__name__}")
        with torch.no_grad():
            if sampler is not None:
                traj = sampler(image, tgt, guide=guide)
                sel, cands = sampler.last_selection, sampler.last_candidates
                mset = sampler.last_modes
            else:
                traj, sel = generate_traj(model, scheduler, cfg, image, tgt, noise=noise, candidates=K, selector=selector,
                                          warm=warm, guide=guide, scale_xy=False, return_selection=True, modes=modes)
                cands = None if sel is None else sel.candidates
                mset = None if modes is None else modes.last
            index = None if sel is None else sel.index
            blocked = None if sel is None else sel.blocked
            if blocked is None and guide is not None:
                blocked = (guide.cost(traj)[1] > 0).to(torch.int32)      # a comparison on the device: no read
            metrics.update(traj if cands is None else cands, gt, index=index, blocked=blocked)
            if mset is not None:
                mode_metrics.update(mset.modes, gt)          # index None: candidate 0 = mode 0, the heaviest
                mode_scenes += int(gt.shape[0])
                mode_sums += torch.stack([t.sum().to(torch.float64) for t in (mset.count, mset.prob()[:, 0], mset.assign == OUTLIER)])
    out = metrics.compute()
    if modes is not None:
        m, sums = mode_metrics.compute(), mode_sums.cpu().tolist()
        per = lambda v, d: v / d if d > 0 else float("nan")      # noqa: E731
        out["modes"] = {"m": modes.max_modes, "min_ade_m": m["min_ade_k"], "min_fde_m": m["min_fde_k"],
                        "miss_rate_any_m": m["miss_rate_any"], "top_ade": m["ade"], "top_fde": m["fde"],
                        "top_miss_rate": m["miss_rate"], "mean_count": per(sums[0], mode_scenes),
                        "mean_top_prob": per(sums[1], mode_scenes), "outlier_rate": per(sums[2], mode_scenes * K)}
    return out
