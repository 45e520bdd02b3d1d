"""Test infrastructure: "cost guidance v1" (include/adx.h) restated twice.

`cost_grad` is NumPy, one rounded operation per operation of the contract, in its order, in the dtype it is given: float32 is
the bit-for-bit restatement of the kernels' `guide_grad` (csrc/sched.hip), float64 the yardstick of `adx_guide_cost`.  `iterate`
is the per-step loop (gradient, lambda, cap, move, clip) on the clipped x0 of a whole [B, H, D] tensor, `step` / `dpm_step` one
guided step of each sampler: the guided x0 of a moved element enters the sampler's update, an unmoved element runs the unguided
arithmetic.  The samplers' own arithmetic, the pin blend and zero_first are the fp32 torch restatements the pin tests pinned
(tests/pin_ref.py, tests/dpm_ref.py); the noise `z` is an argument, as there.

A guide here is a dict: discs [S, M, 5] or None, planes [S, P, 3] or None (NumPy or torch, CPU), lam (the step's lambda as the
fp32 number the kernel receives), cap, iters.
"""
from __future__ import annotations

import numpy as np
import torch

import pin_ref as R

F32, F64 = np.float32, np.float64
U = 2.0 ** -24                 # unit roundoff of fp32
DISC_OPS, PLANE_OPS = 15, 6    # rounded operations from the inputs to one term of J (the contract's lines, counted)


def _np(t, dtype):
    if t is None:
        return None
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(dtype)


def scene_rows(t, batch):
    """[S, n, k] -> [batch, n, k]: row r reads scene r % S (candidate-major)."""
    if t is None:
        return None
    assert batch % t.shape[0] == 0
    return np.tile(t, (batch // t.shape[0], 1, 1))


def cost_grad(discs, planes, x, y, dtype=F32):
    """x, y [B, H]; discs [B, M, 5] / planes [B, P, 3] (per ROW: `scene_rows` first) or None.
    -> (J [B, H], gx, gy, active [B, H] int) in `dtype`, every operation rounded on its own."""
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    B, H = x.shape
    hf = np.arange(H).astype(dtype)[None, :]
    one, two = dtype(1), dtype(2)
    J, gx, gy = np.zeros((B, H), dtype), np.zeros((B, H), dtype), np.zeros((B, H), dtype)
    active = np.zeros((B, H), np.int64)
    with np.errstate(all="ignore"):
        for i in range(0 if discs is None else discs.shape[1]):
            cx, cy, vx, vy, r = (np.asarray(discs[:, i, k], dtype)[:, None] for k in range(5))
            ox = cx + hf * vx
            oy = cy + hf * vy
            dx = x - ox
            dy = y - oy
            d2 = dx * dx + dy * dy
            inv = one / (r * r)
            phi = one - d2 * inv
            on = (r > 0) & (phi > 0)                     # an empty slot; a NaN compares false
            k = (two * phi) * inv
            J = np.where(on, J + (phi * phi) / two, J)
            gx = np.where(on, gx - k * dx, gx)
            gy = np.where(on, gy - k * dy, gy)
            active += on
        for i in range(0 if planes is None else planes.shape[1]):
            nx, ny, b = (np.asarray(planes[:, i, k], dtype)[:, None] for k in range(3))
            psi = (nx * x + ny * y) - b
            on = psi > 0
            J = np.where(on, J + (psi * psi) / two, J)
            gx = np.where(on, gx + psi * nx, gx)
            gy = np.where(on, gy + psi * ny, gy)
            active += on
    return J, gx, gy, active


def _clamp(v, lo, hi):
    """v < lo ? lo : (v > hi ? hi : v): a NaN goes through."""
    return np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(v.dtype)


def iterate(px, py, discs, planes, lam, cap, iters, clip, clip_range):
    """The contract's inner loop from the clipped x0 (px, py) [B, H], fp32.  -> (px, py, moved_x, moved_y)."""
    px, py = np.asarray(px, F32), np.asarray(py, F32)
    lam, cap, cr = F32(lam), F32(cap), F32(clip_range)
    mx, my = np.zeros(px.shape, bool), np.zeros(px.shape, bool)
    with np.errstate(all="ignore"):
        for _ in range(int(iters)):
            _, gx, gy, _ = cost_grad(discs, planes, px, py, F32)
            sx, sy = _clamp(lam * gx, -cap, cap), _clamp(lam * gy, -cap, cap)
            mx |= sx != 0
            my |= sy != 0
            px, py = px - sx, py - sy
            if clip:
                px, py = _clamp(px, -cr, cr), _clamp(py, -cr, cr)
    return px, py, mx, my


def guide_x0(x0: torch.Tensor, guide: dict, clip, clip_range):
    """x0 [B, H, D] fp32 torch, clipped -> (the guided x0, moved [B, H, D] bool): columns 0, 1 where they moved, the rest as it was."""
    B = x0.shape[0]
    discs, planes = scene_rows(_np(guide.get("discs"), F32), B), scene_rows(_np(guide.get("planes"), F32), B)
    a = x0.numpy()
    px, py, mx, my = iterate(a[:, :, 0], a[:, :, 1], discs, planes, guide["lam"], guide["cap"], guide["iters"], clip, clip_range)
    out, moved = a.copy(), np.zeros(a.shape, bool)
    out[:, :, 0] = np.where(mx, px, a[:, :, 0])
    out[:, :, 1] = np.where(my, py, a[:, :, 1])
    moved[:, :, 0], moved[:, :, 1] = mx, my
    return torch.from_numpy(out), torch.from_numpy(moved)


def step(ddpm: bool, c: dict, mo, x, z=None, *, guide=None, pin=None, level=R.CLEAN, cfg_scale=None, zf=False):
    """pin_ref.step with the guide between the clip and the sampler's update.  -> (prev_sample, x0); x0 is the guided value
    where an element moved."""
    s = R._s
    m = R.combine(mo, cfg_scale) if cfg_scale is not None else mo
    sa, sb = s(c["sqrt_alpha_t"]), s(c["sqrt_beta_t"])
    pt = R.PRED[c["prediction_type"]]
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
    moved = torch.zeros_like(x0, dtype=torch.bool)
    if guide is not None:
        x0, moved = guide_x0(x0, guide, c["clip"], c["clip_range"])
    if not ddpm:
        clipped = (x - sa * x0) / sb
        eps = clipped if c["use_clipped_model_output"] else torch.where(moved, clipped, eps)
        prev = s(c["c_x0"]) * x0 + s(c["c_dir"]) * eps
    else:
        prev = s(c["c_x0"]) * x0 + s(c["c_x"]) * x
    if c["add_noise"]:
        prev = prev + s(c["c_noise"]) * z
    return R._finish(prev, pin, level, z, zf), x0


def dpm_step(co: dict, prediction_type: str, thresholding: bool, mo, x, prev_x0=None, z=None, *, guide=None, pin=None, level=R.CLEAN,
             cfg_scale=None, zf=False):
    """dpm_ref.step with the guide after the clamp.  `guide["lam"]` is the caller's (sigma_s based under `variance`)."""
    m = R.combine(mo, cfg_scale) if cfg_scale is not None else mo
    a, sg = co["alpha_s"], co["sigma_s"]
    if prediction_type == "epsilon":
        x0 = (x - sg * m) / a
    elif prediction_type == "sample":
        x0 = m
    else:
        x0 = a * x - sg * m
    if thresholding:
        x0 = x0.clamp(-1, 1)
    if guide is not None:
        x0, _ = guide_x0(x0, guide, thresholding, 1.0)
    prev = co["r"] * x - co["k"] * x0
    if co["second_order"]:
        prev = prev - co["half_k"] * (co["inv_r0"] * (x0 - prev_x0))
    return R._finish(prev, pin, level, z, zf), x0


def level(scale, schedule, sb):
    """lambda as the schedulers' `guide_level` forms it: fp32(scale), times (sb * sb) in fp32 under `variance`."""
    scale = F32(scale)
    if schedule == "constant":
        return float(scale)
    sb = F32(sb)
    return float(scale * F32(sb * sb))


# -- the cost of a plan -----------------------------------------------------------------------------------------------------------
def row_cost(traj, discs, planes, dtype=F64):
    """traj [rows, H, D], discs / planes [S, ..]: -> (cost [rows], active [rows], terms J [rows, H]) in `dtype`."""
    t = _np(traj, dtype)
    B = t.shape[0]
    J, _, _, act = cost_grad(scene_rows(_np(discs, dtype), B), scene_rows(_np(planes, dtype), B), t[:, :, 0], t[:, :, 1], dtype)
    return J.sum(axis=1), act.sum(axis=1), J


def row_cost_wave(traj, discs, planes):
    """The fp32 cost as `adx_guide_cost` sums it: lane h of a 64-lane wave holds waypoint h's J (0 for h >= H), then the xor
    butterfly v = v + v[lane ^ off] at off = 32, 16, .. 1.  -> cost [rows] float32, bit for bit the kernel's."""
    _, _, J = row_cost(traj, discs, planes, F32)
    v = np.zeros((J.shape[0], 64), F32)
    v[:, :J.shape[1]] = J
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ off]
    return v[:, 0]


def cost_bound(traj, discs, planes):
    """|fp32 cost - fp64 cost| per row, from the contract: every term of J carries at most DISC_OPS roundings of its own, the sum
    of a row's H * (M + P) terms one more per term; each is a relative 2^-24 of a nonnegative term, so the bound is
    2^-24 * (DISC_OPS + H * (M + P)) * (the fp64 sum of the terms' magnitudes), per row."""
    cost, _, J = row_cost(traj, discs, planes, F64)
    H = J.shape[1]
    n = (0 if discs is None else discs.shape[1]) + (0 if planes is None else planes.shape[1])
    return U * (DISC_OPS + H * n) * np.abs(J).sum(axis=1)


def hinge_margin(traj, discs, planes):
    """The smallest |phi| over live discs and |psi| over planes, in fp64: how far every hinge stands from its kink."""
    t = _np(traj, F64)
    B, H = t.shape[:2]
    x, y = t[:, :, 0], t[:, :, 1]
    hf = np.arange(H, dtype=F64)[None, :]
    least = np.inf
    d, p = scene_rows(_np(discs, F64), B), scene_rows(_np(planes, F64), B)
    for i in range(0 if d is None else d.shape[1]):
        cx, cy, vx, vy, r = (d[:, i, k][:, None] for k in range(5))
        live = np.broadcast_to(r > 0, x.shape)
        with np.errstate(all="ignore"):
            phi = 1 - ((x - (cx + hf * vx)) ** 2 + (y - (cy + hf * vy)) ** 2) / (r * r)
        if live.any():
            least = min(least, np.abs(phi[live]).min())
    for i in range(0 if p is None else p.shape[1]):
        nx, ny, b = (p[:, i, k][:, None] for k in range(3))
        least = min(least, np.abs(nx * x + ny * y - b).min())
    return least


# -- the fixture of the issue -----------------------------------------------------------------------------------------------------
FIX_H = 8
FIX_DISCS = np.array([[[0.4, 0.02, 0.0, 0.0, 0.15], [0.0, 0.0, 0.0, 0.0, 0.0]]], F32)      # one disc and one empty slot
FIX_PLANES = np.array([[[1.0, 0.0, 0.6]]], F32)
FIX = dict(scale=0.01, schedule="constant", cap=0.05, iters=8, clip=1, clip_range=1.0)


def fixture_x0(dim=2):
    """[1, 8, dim]: the straight line from (0, 0) to (0.7, 0); further columns zero."""
    x0 = np.zeros((1, FIX_H, dim), F32)
    x0[0, :, 0] = np.linspace(0.0, 0.7, FIX_H).astype(F32)
    return x0
