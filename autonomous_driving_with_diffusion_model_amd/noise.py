"""DeviceNoise: the counter-based noise stream of csrc/noise.h ("stream v1", DESIGN.md / include/adx.h) as an object.

Noise is a pure function of (seed, tick, slot, element): seed names the run, tick the sampling call (one `begin_tick()`
per `generate_traj` / graph replay), slot the integer timestep of the scheduler step (`INIT_SLOT` for the initial
trajectory) and element the flat index in the logical `[rows][H][D]` tensor.  Seed and tick live in four device words
that every kernel reads when it RUNS, so a captured HIP graph draws fresh noise on every replay, and a rank that holds
rows [a, b) of a batch draws -- through `shard(a)` -- exactly what the unsharded run draws on those rows.

No reference counterpart (the reference draws `torch.randn` from the global generator); the values differ from
`torch.randn`'s for the same seed, as torch's own differ between CPU and GPU.
"""
from __future__ import annotations

import math

import torch

from . import _lib as L

_M32, _M64 = (1 << 32) - 1, (1 << 64) - 1


def _i32(word: int) -> int:
    """A 32-bit word as the int32 that carries its bits."""
    word &= _M32
    return word - (1 << 32) if word >= (1 << 31) else word


class DeviceNoise:
    INIT_SLOT = 0xFFFFFFFF      # slot of the initial trajectory (scheduler steps use their integer timestep)

    def __init__(self, seed: int, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise L.AdxError(f"DeviceNoise lives on a GPU (got {device}); there is no CPU path")
        self._state = torch.zeros(4, dtype=torch.int32, device=device)   # {seed_lo, seed_hi, tick_lo, tick_hi}
        self._row_offset = 0
        self.reseed(seed)

    # -- state -------------------------------------------------------------------------------------
    @property
    def device(self):
        return self._state.device

    @property
    def row_offset(self) -> int:
        return self._row_offset

    def state_ptr(self) -> int:
        return self._state.data_ptr()

    def _host_write(self, first: int, value: int, what: str) -> None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"DeviceNoise.{what}() copies host words into the state: not while a graph capture is open")
        value = int(value)
        if not 0 <= value <= _M64:
            raise ValueError(f"DeviceNoise.{what}: {value} is not an unsigned 64-bit number")
        words = torch.tensor([_i32(value), _i32(value >> 32)], dtype=torch.int32)
        self._state[first:first + 2].copy_(words)

    def reseed(self, seed: int) -> None:
        """Set the seed words; the tick stays."""
        self._host_write(0, seed, "reseed")

    def seek(self, tick: int) -> None:
        """Set the tick: the n-th `begin_tick()` after `seek(k)` makes draws use tick k + n."""
        self._host_write(2, tick, "seek")

    def tick(self) -> int:
        """The current tick, read back from the device (a host synchronisation: for tests, logs and capture set-up)."""
        w = [int(v) & _M32 for v in self._state.cpu().tolist()]
        return w[2] | (w[3] << 32)

    def begin_tick(self) -> None:
        """tick += 1 by a one-thread kernel on the current stream (capturable)."""
        L.check(L.lib().adx_noise_advance(self._state.data_ptr(), L.stream_ptr(self.device)), "adx_noise_advance")

    def shard(self, row_offset: int) -> "DeviceNoise":
        """A view on the SAME state whose draws start `row_offset` rows further into the logical tensor."""
        row_offset = int(row_offset)
        if row_offset < 0:
            raise ValueError(f"DeviceNoise.shard: negative row_offset {row_offset}")
        v = object.__new__(DeviceNoise)
        v._state, v._row_offset = self._state, self._row_offset + row_offset
        return v

    # -- draws under the current tick --------------------------------------------------------------------
    def _fill(self, fn_name: str, dtype, slot: int, shape, row_offset: int) -> torch.Tensor:
        shape = tuple(int(s) for s in shape)
        if not shape or any(s < 0 for s in shape):
            raise ValueError(f"DeviceNoise: shape {shape} must be non-empty with sizes >= 0 (rows first)")
        if int(row_offset) < 0:
            raise ValueError(f"DeviceNoise: negative row_offset {row_offset}")
        first = (self._row_offset + int(row_offset)) * math.prod(shape[1:])
        out = torch.empty(shape, dtype=dtype, device=self.device)
        L.check(getattr(L.lib(), fn_name)(self._state.data_ptr(), _i32(int(slot)), first, out.data_ptr(), out.numel(),
                                          L.stream_ptr(self.device)), fn_name)
        return out

    def normal(self, slot: int, shape, row_offset: int = 0) -> torch.Tensor:
        """fp32 normals of the logical rows [row_offset, row_offset + shape[0]) of `slot`: bit for bit what a
        `step(..., generator=self)` at timestep `slot` draws inside its kernel."""
        return self._fill("adx_noise_normal", torch.float32, slot, shape, row_offset)

    def words(self, slot: int, shape, row_offset: int = 0) -> torch.Tensor:
        """The raw Philox words behind `normal` (int32 tensor carrying the uint32 bits)."""
        return self._fill("adx_noise_words", torch.int32, slot, shape, row_offset)

    def __repr__(self):
        return f"DeviceNoise(device={self.device}, row_offset={self._row_offset})"
