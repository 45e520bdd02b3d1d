"""Pin: waypoints the caller has already decided, held through a sampling tick ("pinned waypoints v1", include/adx.h).

A pin is a known trajectory and a mask over the same `[S, H, D]` cells, in the model's own units (the units of `target` and of
the clamped result before xy scaling) and in THIS tick's ego frame: moving last tick's plan into this tick's frame is the
caller's job.  Every sampler step blends its finished `prev_sample` with the known values under the mask, inside the step
kernel; `[:, 0, :3] = 0` keeps the last word on waypoint 0.  Two modes of one arithmetic:

    clean    the known values themselves after every step -- what the reference's loops do to `[:, 0, :3]` (interact.py:164),
             Diffuser's apply_conditioning.  Needs no noise.
    repaint  the known values noised to the level the step lands on (RePaint's per-step replacement, the blend of the
             reference's Inpainting*Scheduler classes), with the step's own noise.

No reference counterpart as a caller-facing object: the reference constructs neither inpainting scheduler.  What a pin does to
driving quality is a property of trained weights and is not measured in this repository.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from . import _lib as L

MODES = ("clean", "repaint")
CLEAN_LEVEL = (1.0, 0.0, False)        # (c_known, c_known_noise, known_noise) of a `clean` step


class Pin:
    """`known`, `mask`: float32 tensors of one shape `[S, H, D]` on one device; mask 1 = pinned, 0 = free, values between blend
    linearly.  `mode`: "clean" or "repaint"; None reads EVAL.PIN_MODE where a config is at hand (`generate_traj`,
    `GraphedSampler`; an absent key means "clean") and means "clean" in a bare `scheduler.step(pin=...)`."""

    def __init__(self, known: torch.Tensor, mask: torch.Tensor, mode: Optional[str] = None):
        if not torch.is_tensor(known) or not torch.is_tensor(mask):
            raise TypeError(f"Pin: known and mask must be tensors, got {type(known).__name__} and {type(mask).__name__}")
        if known.dim() != 3 or known.shape != mask.shape:
            raise ValueError(f"Pin: known and mask must share one shape [S, H, D], got {tuple(known.shape)} and {tuple(mask.shape)}")
        if known.dtype != torch.float32 or mask.dtype != torch.float32:
            raise TypeError(f"Pin: known and mask must be float32, got {known.dtype} and {mask.dtype}")
        if known.device != mask.device:
            raise ValueError(f"Pin: known lives on {known.device}, mask on {mask.device}")
        if mode is not None and mode not in MODES:
            raise ValueError(f"Pin: mode must be one of {MODES} or None (EVAL.PIN_MODE), got {mode!r}")
        self.known, self.mask, self.mode = known.contiguous(), mask.contiguous(), mode

    @classmethod
    def points(cls, horizon: int, dim: int, index: Sequence[int], xy: torch.Tensor, mode: Optional[str] = None) -> "Pin":
        """Pin (x, y) of the waypoints `index` to `xy` [S, len(index), 2]; everything else is free.  Built on `xy`'s device."""
        index = [int(i) for i in index]
        if not torch.is_tensor(xy) or xy.dim() != 3 or tuple(xy.shape[1:]) != (len(index), 2):
            got = tuple(xy.shape) if torch.is_tensor(xy) else type(xy).__name__
            raise ValueError(f"Pin.points: xy must be [S, {len(index)}, 2] for {len(index)} waypoints, got {got}")
        if int(dim) < 2:
            raise ValueError(f"Pin.points: pinning (x, y) needs dim >= 2, got {dim}")
        if len(set(index)) != len(index) or any(not 0 <= i < int(horizon) for i in index):
            raise ValueError(f"Pin.points: index must name distinct waypoints in 0..{int(horizon) - 1}, got {index}")
        S = xy.shape[0]
        known = torch.zeros((S, int(horizon), int(dim)), dtype=torch.float32, device=xy.device)
        mask = torch.zeros_like(known)
        if index:
            known[:, index, :2] = xy.to(torch.float32)
            mask[:, index, :2] = 1.0
        return cls(known, mask, mode)

    def resolve(self, cfg=None) -> str:
        """The mode in force: the object's own, else EVAL.PIN_MODE of `cfg`, else "clean"."""
        mode = self.mode
        if mode is None:
            mode = "clean" if cfg is None else getattr(cfg.EVAL, "PIN_MODE", "clean")
        if mode not in MODES:
            raise ValueError(f"Pin: mode must be one of {MODES}, got {mode!r} (EVAL.PIN_MODE)")
        return mode

    def with_mode(self, mode: str) -> "Pin":
        """The same tensors under an explicit mode."""
        return self if mode == self.mode else Pin(self.known, self.mask, mode)

    def desc(self, x: torch.Tensor, level: Tuple[float, float, bool]) -> L.PinDesc:
        """The `adx_pin` of a launch on the sample `x` [B, H, D] at `level` = (c_known, c_known_noise, known_noise).  The struct
        holds addresses: keep this object alive until the launch is enqueued."""
        known = L.require_gpu_f32(self.known, "pin.known")
        mask = L.require_gpu_f32(self.mask, "pin.mask")
        R, H, D = known.shape
        if known.device != x.device or tuple(x.shape[1:]) != (H, D) or R < 1 or x.shape[0] % R != 0:
            raise ValueError(f"the pin is {tuple(known.shape)} on {known.device}; the sample is {tuple(x.shape)} on {x.device}: same "
                             "device, same [H, D], rows a multiple of the pin's")
        p = L.PinDesc()
        p.known, p.mask, p.known_rows = known.data_ptr(), mask.data_ptr(), R
        p.c_known, p.c_known_noise, p.known_noise = float(level[0]), float(level[1]), int(bool(level[2]))
        return p

    def __repr__(self):
        return f"Pin({tuple(self.known.shape)}, device={self.known.device}, mode={self.mode!r})"


def pin_apply(x: torch.Tensor, pin: Pin, level: Tuple[float, float, bool] = CLEAN_LEVEL, noise=None) -> torch.Tensor:
    """One launch of `adx_pin_apply`: the blend of "pinned waypoints v1" IN PLACE on `x` [B, H, D] (contiguous float32; row r
    reads pin row r % S).  `level` = (c_known, c_known_noise, known_noise); with known_noise the noise is `noise`'s (a DeviceNoise)
    INIT_SLOT draw of the rows `noise.row_offset + r` under the current tick.  Returns `x`."""
    if L.require_gpu_f32(x, "x") is not x or x.dim() != 3:
        raise ValueError(f"pin_apply works in place on a contiguous [B, H, D] sample, got {tuple(x.shape)} (contiguous: {x.is_contiguous()})")
    if noise is not None and noise.device != x.device:
        raise ValueError(f"the DeviceNoise lives on {noise.device}, the sample on {x.device}")
    p = pin.desc(x, level)
    B, H, D = x.shape
    L.check(L.lazy("adx_pin_apply")(x.data_ptr(), C.byref(p), None if noise is None else noise.state_ptr(),
                                    0 if noise is None else noise.row_offset, B, H, D, L.stream_ptr(x.device)), "adx_pin_apply")
    return x
