"""Test infrastructure: fp32 restatement of "pinned waypoints v1" (include/adx.h) -- the blend, one pinned step of each
sampler (csrc/sched.hip: step_kernel<.., PIN>, dpm_step_kernel<PIN>, pin_apply_kernel) and the per-step levels
(c_known, c_known_noise, known_noise) the schedulers hand to the kernel.

torch on the CPU, one rounded fp32 operation per operation of the contract, in its order; scalars are 0-dim fp32 tensors.  The
noise `z` is an argument: the GPU tests feed the values the device stream produced (`DeviceNoise.normal(slot, shape,
row_offset=...)`) or the tensor they handed to the step, so the restatement has no generator of its own.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

import dpm_ref
from oracle.diffusers_base import make_betas

CLEAN = (1.0, 0.0, False)
PRED = {0: "epsilon", 1: "sample", 2: "v_prediction"}


def _s(v) -> torch.Tensor:
    """A host scalar as the fp32 number the kernel receives by value."""
    return torch.tensor(float(v), dtype=torch.float32)


def rows(t: torch.Tensor, batch: int) -> torch.Tensor:
    """[known_rows, H, D] -> [batch, H, D]: row r reads known row r % known_rows (candidate-major)."""
    assert batch % t.shape[0] == 0
    return t.repeat(batch // t.shape[0], 1, 1)


def blend(prev: torch.Tensor, known: torch.Tensor, mask: torch.Tensor, level=CLEAN, z: Optional[torch.Tensor] = None) -> torch.Tensor:
    """kp = c_known * known + (known_noise ? c_known_noise * z : 0);  u = mask * kp;  v = (1 - mask) * prev;  prev = u + v."""
    c_known, c_known_noise, known_noise = level
    B = prev.shape[0]
    k, m = rows(known, B), rows(mask, B)
    k0 = _s(c_known) * k
    k1 = _s(c_known_noise) * z if known_noise else torch.zeros_like(k0)
    kp = k0 + k1
    u = m * kp
    v = (1.0 - m) * prev
    return u + v


def zero_first(prev: torch.Tensor) -> torch.Tensor:
    prev = prev.clone()
    prev[:, 0, :3] = 0.0
    return prev


def combine(mo: torch.Tensor, scale: float) -> torch.Tensor:
    """The classifier-free combine fused in front of a step: rows [0, B) cond, [B, 2B) uncond."""
    c, u = mo.chunk(2, dim=0)
    d = c - u
    sd = _s(scale) * d
    return u + sd


def coef(c) -> dict:
    """The fields of an adx_step_coef / adx_dpm_coef (ctypes) as a dict."""
    return {f[0]: getattr(c, f[0]) for f in c._fields_}


def _finish(prev, pin, level, z, zf):
    if pin is not None:
        prev = blend(prev, pin[0], pin[1], level, z)
    return zero_first(prev) if zf else prev


def step(ddpm: bool, c: dict, mo, x, z=None, *, pin=None, level=CLEAN, cfg_scale=None, zf=False):
    """One DDIM (ddpm=False) or DDPM step from the host scalars `c` (the package's `_ddim_coef` / `_ddpm_coef`, tested against
    the oracle elsewhere), then the blend on the finished prev_sample, then zero_first.  `pin` = (known, mask) on the CPU.
    -> (prev_sample, x0); x0 is never pinned."""
    m = combine(mo, cfg_scale) if cfg_scale is not None else mo
    sa, sb = _s(c["sqrt_alpha_t"]), _s(c["sqrt_beta_t"])
    pt = PRED[c["prediction_type"]]
    if pt == "epsilon":
        x0, eps = (x - sb * m) / sa, m
    elif pt == "sample":
        x0 = m
        eps = (x - sa * x0) / sb
    else:
        x0 = sa * x - sb * m
        eps = sa * m + sb * x
    if c["clip"]:
        x0 = x0.clamp(-c["clip_range"], c["clip_range"])
    if not ddpm:
        if c["use_clipped_model_output"]:
            eps = (x - sa * x0) / sb
        direction = _s(c["c_dir"]) * eps
        prev = _s(c["c_x0"]) * x0 + direction
    else:
        prev = _s(c["c_x0"]) * x0 + _s(c["c_x"]) * x
    if c["add_noise"]:
        prev = prev + _s(c["c_noise"]) * z
    return _finish(prev, pin, level, z, zf), x0


def dpm_step(co: dict, prediction_type: str, thresholding: bool, mo, x, prev_x0=None, z=None, *, pin=None, level=CLEAN,
             cfg_scale=None, zf=False):
    """One DPM-Solver++ step through dpm_ref.step (scalars: dpm_ref.coefficients), then the blend, then zero_first."""
    m = combine(mo, cfg_scale) if cfg_scale is not None else mo
    prev, x0 = dpm_ref.step(co, prediction_type, thresholding, m, x, prev_x0)
    return _finish(prev, pin, level, z, zf), x0


# -- the levels -----------------------------------------------------------------------------------------------------------------
def alphas_cumprod(n_train: int, beta_schedule="squaredcos_cap_v2", beta_start=1e-4, beta_end=0.02) -> torch.Tensor:
    return torch.cumprod(1.0 - make_betas(beta_schedule, n_train, beta_start, beta_end), dim=0)


def leading_timesteps(n_train: int, steps: int):
    return (np.arange(0, steps) * (n_train // steps)).round()[::-1].astype(np.int64).tolist()


def level_leading(ac: torch.Tensor, n_train: int, steps: int, t: int, mode: str):
    """DDIM and DDPM ('leading' spacing, set_alpha_to_one): the level of t - n_train // steps, clean below timestep 0."""
    if mode == "clean":
        return CLEAN
    prev_t = t - n_train // steps
    a_prev = ac[prev_t] if prev_t >= 0 else torch.tensor(1.0)
    return float(a_prev ** 0.5), float((1.0 - a_prev) ** 0.5), t > 0


def level_dpm(sigmas: torch.Tensor, i: int, mode: str):
    """DPM-Solver++: alpha and sigma * alpha of sigmas[i + 1]; the last step lands on sigma = 0."""
    if mode == "clean":
        return CLEAN
    sigma = sigmas[i + 1]
    alpha = 1 / ((sigma ** 2 + 1) ** 0.5)
    return float(alpha), float(sigma * alpha), i < sigmas.shape[0] - 2
