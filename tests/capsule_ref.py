"""Test infrastructure: "cost guidance v5" (include/adx.h) restated -- per-scene moving capsules: segments with a radius, and what a
waypoint pays for standing closer to one than its radius; and "capsules from boxes v1", the slots from oriented boxes.

`slot_terms` is NumPy, one rounded operation per operation of the contract, in its order, in the dtype it is given: float32 is
the bit-for-bit restatement of the capsule branch of the kernels' `guide_grad` (csrc/guide.h), float64 the yardstick of the cost.
Everything that is v1 to v4 is tests/guide_ref.py's, tests/field_ref.py's, tests/motion_ref.py's and tests/route_ref.py's own
function: `_capsuled` wraps guide_ref's `cost_grad` after field_ref's `_fielded` and route_ref's `_routed` wrapped it and before
motion_ref's `_motioned` does, so the order of the whole is discs, planes, field, route, capsules, motion -- the contract's -- for
as long as one call of `iterate`, `step`, `dpm_step`, `row_cost` or `row_cost_wave` runs.

Capsules here are a dict (`capsules(...)` makes one): slots [S, C, 7] float32 NumPy and weight as the fp32 number the kernel
receives.  A guide is guide_ref's dict with the keys "field", "route", "capsules" and "motion" (absent or None: v1 .. v4).
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

import field_ref as FR
import guide_ref as G
import motion_ref as MR
import route_ref as RR

F32, F64, U = G.F32, G.F64, G.U


def capsules(slots, weight=1.0) -> dict:
    s = slots.detach().cpu().numpy() if torch.is_tensor(slots) else np.asarray(slots)
    s = np.ascontiguousarray(s, F32)
    assert s.ndim == 3 and s.shape[2] == 7 and 1 <= s.shape[1] <= 32, s.shape
    return dict(slots=s, weight=F32(weight))


def _rows(c, B, dtype):
    """slots [B, C, 7] of a launch of B rows: row r reads scene r % S."""
    s = c["slots"]
    assert B % s.shape[0] == 0
    return np.tile(s, (B // s.shape[0], 1, 1)).astype(dtype)


def slot_terms(c, x, y, dtype=F32):
    """x, y [B, H] -> per slot i the arrays [C, B, H] of the contract's loop body, in `dtype`, every operation rounded on its own:
    on (the slot is live, phi > 0 and the weight is not 0), cost = (weight * (phi * phi)) / 2, (kx, ky) = (k * rx, k * ry), phi, d2,
    (rx, ry), the clamped t and the raw quotient, and ee, uu, the magnitudes |a| + |h v| per component (mx, my) and r for the
    bounds."""
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    B, H = x.shape
    s = _rows(c, B, dtype)
    hf = np.arange(H).astype(dtype)[None, :]
    zero, one, two, w = dtype(0), dtype(1), dtype(2), dtype(c["weight"])
    keys = ("on", "cost", "kx", "ky", "phi", "d2", "rx", "ry", "t", "raw", "ee", "uu", "mx", "my", "r")
    out = {k: [] for k in keys}
    with np.errstate(all="ignore"):
        for i in range(s.shape[1]):
            ax, ay, bx, by, vx, vy, r = (s[:, i, k][:, None] for k in range(7))
            hx, hy = hf * vx, hf * vy
            px, py = ax + hx, ay + hy
            ex, ey = bx - ax, by - ay                                                    # from the unmoved ends
            ux, uy = x - px, y - py
            ee = ex * ex + ey * ey
            ue = ux * ex + uy * ey
            raw = np.where(ee > 0, ue / np.where(ee > 0, ee, one), zero)
            t = np.where(raw < 0, zero, np.where(raw > 1, one, raw)).astype(dtype)      # a NaN passes through
            rx, ry = ux - t * ex, uy - t * ey
            d2 = rx * rx + ry * ry
            rr = r * r
            inv = one / rr
            sd = d2 * inv
            phi = one - sd
            on = (r > 0) & (phi > 0) & (w != 0)                                          # an empty slot; a NaN compares false
            cost = (w * (phi * phi)) / two
            k = w * ((two * phi) * inv)
            vals = (on, cost, k * rx, k * ry, phi, d2, rx, ry, t, raw, ee, ux * ux + uy * uy, np.abs(ax) + np.abs(hx),
                    np.abs(ay) + np.abs(hy), r)
            for key, v in zip(keys, vals):
                out[key].append(np.broadcast_to(v, x.shape))
    return {k: np.stack(v) for k, v in out.items()}


def capsule_share(c, x, y, J, gx, gy, active, dtype=F32):
    """The capsule term added to (J, gx, gy, active) [B, H], slot by slot in index order; nothing at all where a slot is inactive,
    not even a zero."""
    s = slot_terms(c, x, y, dtype)
    with np.errstate(all="ignore"):
        for i in range(s["on"].shape[0]):
            on = s["on"][i]
            J = np.where(on, J + s["cost"][i], J)
            gx = np.where(on, gx - s["kx"][i], gx)
            gy = np.where(on, gy - s["ky"][i], gy)
            active = active + on
    return J, gx, gy, active


def capsule_cost(c, x, y, dtype=F64):
    """The capsule term alone: per waypoint [B, H]."""
    s = slot_terms(c, x, y, dtype)
    return np.where(s["on"], s["cost"], dtype(0)).sum(axis=0)


def capsule_grad(c, x, y, dtype=F64):
    """The capsule term's gradient alone: (gx, gy) per waypoint [B, H]."""
    z = np.zeros(np.asarray(x).shape, dtype)
    _, gx, gy, _ = capsule_share(c, x, y, z, z.copy(), z.copy(), np.zeros(z.shape, np.int64), dtype)
    return gx, gy


@contextlib.contextmanager
def _capsuled(c):
    """guide_ref with `c` in its cost_grad, for the calls made inside the block (inside field_ref._fielded and route_ref._routed
    where there is a field or a route, outside motion_ref._motioned where there are limits)."""
    if c is None:
        yield
        return
    inner = G.cost_grad

    def wrapped(discs, planes, x, y, dtype=F32):
        return capsule_share(c, x, y, *inner(discs, planes, x, y, dtype), dtype=dtype)

    G.cost_grad = wrapped
    try:
        yield
    finally:
        G.cost_grad = inner


@contextlib.contextmanager
def _guided(f, r, c, m):
    with FR._fielded(f), RR._routed(r), _capsuled(c), MR._motioned(m):
        yield


def _of(guide):
    if guide is None:
        return (None, None, None, None)
    return (guide.get("field"), guide.get("route"), guide.get("capsules"), guide.get("motion"))


def cost_grad(discs, planes, f, r, c, m, x, y, dtype=F32):
    """v1's discs and planes, v2's field, v4's route, the capsules, then v3's motion terms, into the same J, gx, gy and active."""
    with _guided(f, r, c, m):
        return G.cost_grad(discs, planes, x, y, dtype)


def iterate(px, py, discs, planes, f, r, c, m, lam, cap, iters, clip, clip_range):
    with _guided(f, r, c, m):
        return G.iterate(px, py, discs, planes, lam, cap, iters, clip, clip_range)


def step(ddpm, co, mo, x, z=None, *, guide=None, **kw):
    with _guided(*_of(guide)):
        return G.step(ddpm, co, mo, x, z, guide=guide, **kw)


def dpm_step(co, prediction_type, thresholding, mo, x, prev_x0=None, z=None, *, guide=None, **kw):
    with _guided(*_of(guide)):
        return G.dpm_step(co, prediction_type, thresholding, mo, x, prev_x0, z, guide=guide, **kw)


def row_cost(traj, discs, planes, f, r, c, m, dtype=F64):
    with _guided(f, r, c, m):
        return G.row_cost(traj, discs, planes, dtype)


def row_cost_wave(traj, discs, planes, f, r, c, m):
    with _guided(f, r, c, m):
        return G.row_cost_wave(traj, discs, planes)


def _gamma(n):
    return n * U / (1 - n * U)


def phi_bound(c, x, y):
    """|fp32 phi - fp64 phi| per slot and waypoint [C, B, H], from the contract's lines, for fp32 inputs (exact in fp64).  With
    |u|, |e|, |r| the fp64 lengths of u = p - (a + h v), e = b - a and the residual:
      hx = hf * vx and px = ax + hx are two roundings of values of magnitude <= |ax| + |hx|, and ux = x - px one more of ux itself:
      per component |d ux| <= gamma_2 (|ax| + |hx|) + u |ux|; as a vector, |d u| <= gamma_2 * hypot(mx, my) + u |u| =: du -- this is
      absolute, the subtraction cancels;
      ex, ey carry one rounding each; ee = ex * ex + ey * ey is a sum of nonnegative terms with four roundings on each path,
      |d ee| <= gamma_4 ee; ue = ux * ex + uy * ey is signed: |d ue| <= gamma_4 |u| |e| + 2 du |e|;
      t = ue / ee one rounding more: |d t| |e| <= gamma_4 |u| + 2 du + gamma_5 |t| |e| before the clamp.  The clamp is a contraction,
      and a quotient beyond 2 in magnitude clamps to the same end in both, so |d t| |e| <= gamma_4 |u| + 2 du + gamma_5 * 2 |e| after
      it.  A degenerate capsule has t = 0 and e = 0 in both: the same formula with |e| = 0;
      rx = ux - t * ex: the moved ux, the moved t, two roundings in t * ex (ex's own and the product's, t <= 1) and the
      subtraction's: |d r| <= du + |d t| |e| + 2 u |e| + u |r| <= 3 du + gamma_4 |u| + gamma_7 * 2 |e| + u |r| =: dr;
      d2 = rx * rx + ry * ry: |d d2| <= 2 |r| dr + dr^2 + gamma_2 (|r| + dr)^2 =: dd2;
      rr = r * r, inv = 1 / rr and sd = d2 * inv are three roundings, relative to sd: |d sd| <= gamma_3 sd + (1 + gamma_3) dd2 / r^2;
      phi = 1 - sd one more, relative to phi: |d phi| <= |d sd| + u |phi|."""
    s = slot_terms(c, x, y, F64)
    with np.errstate(all="ignore"):
        lu, le, lr = np.sqrt(s["uu"]), np.sqrt(s["ee"]), np.sqrt(s["d2"])
        du = _gamma(2) * np.hypot(s["mx"], s["my"]) + U * lu
        dr = 3 * du + _gamma(4) * lu + _gamma(7) * 2 * le + U * lr
        dd2 = 2 * lr * dr + dr * dr + _gamma(2) * (lr + dr) ** 2
        r2 = s["r"] * s["r"]
        dsd = _gamma(3) * (s["d2"] / r2) + (1 + _gamma(3)) * dd2 / r2
        return dsd + U * np.abs(s["phi"])


def term_bound(c, x, y):
    """|fp32 term - fp64 term| per slot and waypoint [C, B, H] where the term is active: with dphi of `phi_bound`, the cost
    (w * (phi * phi)) / 2 moves by w * (|phi| * dphi + dphi^2 / 2) and carries three roundings of its own, gamma_3 * cost."""
    s = slot_terms(c, x, y, F64)
    dphi = phi_bound(c, x, y)
    with np.errstate(all="ignore"):
        return np.where(s["on"], F64(c["weight"]) * (np.abs(s["phi"]) * dphi + dphi * dphi / 2) + _gamma(3) * s["cost"], 0.0)


def cost_bound(traj, discs, planes, f, r, c, m):
    """|fp32 cost - fp64 cost| per row, derived as route_ref.cost_bound derives it.  That bound, taken over the terms with the
    capsules' among them, covers v1 to v4 and their summation.  A capsule term adds its own error, which is NOT relative to the
    term -- u = p - (a + h v) cancels where the capsule is far from the origin, and phi = 1 - sd cancels at the capsule's edge --
    and is absolute instead: `term_bound`, summed over the row's slots and waypoints.  One more rounding per capsule term for the
    summation into J and the butterfly: u * (H * C + 6) * sum |J|.  It presumes fp32 and fp64 agree on which terms are active:
    `hinge_margin` against `phi_bound` says whether they can differ."""
    if c is None:
        return RR.cost_bound(traj, discs, planes, f, r, m)
    with _capsuled(c):
        base = RR.cost_bound(traj, discs, planes, f, r, m)
        _, _, J = RR.row_cost(traj, discs, planes, f, r, m, F64)
    t = G._np(traj, F64)
    x, y = t[:, :, 0], t[:, :, 1]
    n = x.shape[1] * c["slots"].shape[1]
    return base + U * (n + 6) * np.abs(J).sum(axis=1) + term_bound(c, x, y).sum(axis=(0, 2))


def hinge_margin(c, x, y):
    """|phi| per slot and waypoint [C, B, H] in fp64 (inf where the slot is empty, phi is not finite or the weight is 0: no kink
    there)."""
    s = slot_terms(c, x, y, F64)
    with np.errstate(all="ignore"):
        live = (s["r"] > 0) & np.isfinite(s["phi"]) & (c["weight"] != 0)
    return np.where(live, np.abs(s["phi"]), np.inf)


# -- capsules from boxes v1 ---------------------------------------------------------------------------------------------------------
def from_boxes(boxes, inflate):
    """boxes [S, N, 8] = (cx, cy, vx, vy, ux, uy, length, width) -> slots [S, N, 7] float32, the contract in fp32 NumPy, every
    operation rounded on its own; a box that is not live (a size <= 0 or NaN) becomes seven zeros."""
    b = boxes.detach().cpu().numpy() if torch.is_tensor(boxes) else np.asarray(boxes)
    b = b.astype(F32)
    cx, cy, vx, vy, ux, uy, length, width = (b[..., k] for k in range(8))
    two, inflate = F32(2), F32(inflate)
    with np.errstate(all="ignore"):
        live = (length > 0) & (width > 0)
        lon = length >= width
        la, lb = np.where(lon, length, width), np.where(lon, width, length)
        s = la / two - lb / two
        dx, dy = np.where(lon, ux, -uy), np.where(lon, uy, ux)
        ox, oy = s * dx, s * dy
        out = np.stack([cx - ox, cy - oy, cx + ox, cy + oy, vx, vy, lb / two + inflate], axis=-1).astype(F32)
    return np.where(live[..., None], out, F32(0)).astype(F32)


# -- the fixtures of the issue ------------------------------------------------------------------------------------------------------
FIX_ROWS, FIX_H = 400, 50


def fixture_points(seed=0):
    """[400, 50, 2] float32: 20,000 uniform points in [-1, 1]^2."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (FIX_ROWS, FIX_H, 2)).astype(F32)


def fixture_slots(Sn, Cn, g):
    """[Sn, Cn, 7] torch float32 from the generator `g`.  Slot 0: a capsule of radius 3 with both ends in [-0.3, 0.3]^2 and a
    velocity within 1e-3 per waypoint: active at every point of [-1, 1]^2 at every h < 64 (the furthest such point is
    1.3 * sqrt(2) + 0.09 < 3 from either end).  The rest: ends in [-1, 1]^2, velocities within 0.01, radii in 0.2 .. 0.6.  Where
    there is room (Cn >= 3), the last of two scenes holds an empty slot (r = 0) at 1 and a degenerate one (a == b) at 2."""
    s = torch.zeros(Sn, Cn, 7)
    s[..., 0:4] = torch.rand(Sn, Cn, 4, generator=g) * 2 - 1
    s[..., 4:6] = (torch.rand(Sn, Cn, 2, generator=g) - 0.5) * 0.02
    s[..., 6] = 0.2 + 0.4 * torch.rand(Sn, Cn, generator=g)
    s[:, 0, 0:4] = torch.rand(Sn, 4, generator=g) * 0.6 - 0.3
    s[:, 0, 4:6] = (torch.rand(Sn, 2, generator=g) - 0.5) * 0.002
    s[:, 0, 6] = 3.0
    if Sn == 2 and Cn >= 3:
        s[1, 1, 6] = 0.0
        s[1, 2, 2:4] = s[1, 2, 0:2]
    return s
