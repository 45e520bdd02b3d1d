"""Test infrastructure: "cost guidance v4" (include/adx.h) restated -- a per-scene route corridor: a polyline, a half-width, and
what a waypoint pays for standing further from the polyline than that.

`route_term` is NumPy, one rounded operation per operation of the contract, in its order, in the dtype it is given: float32 is
the bit-for-bit restatement of the route branch of the kernels' `guide_grad` (csrc/guide.h), float64 the yardstick of the cost.
Everything that is v1, v2 or v3 is tests/guide_ref.py's, tests/field_ref.py's and tests/motion_ref.py's own function: `_routed`
wraps guide_ref's `cost_grad` after field_ref's `_fielded` wrapped it and before motion_ref's `_motioned` does, so the order of the
whole is discs, planes, field, route, motion -- the contract's -- for as long as one call of `iterate`, `step`, `dpm_step`,
`row_cost` or `row_cost_wave` runs.

A route here is a dict (`route(...)` makes one): points [S, R, 2] and half_width [S] float32 NumPy and weight as the fp32 number
the kernel receives.  A guide is guide_ref's dict with the keys "field", "route" and "motion" (absent or None: v1 / v2 / v3).
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

import field_ref as FR
import guide_ref as G
import motion_ref as MR

F32, F64, U = G.F32, G.F64, G.U


def route(points, half_width, weight=1.0) -> dict:
    p = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    p = np.ascontiguousarray(p, F32)
    assert p.ndim == 3 and p.shape[2] == 2 and 2 <= p.shape[1] <= 32, p.shape
    w = half_width.detach().cpu().numpy() if torch.is_tensor(half_width) else np.asarray(half_width)
    w = np.ascontiguousarray(np.broadcast_to(np.asarray(w, F32).reshape(-1), (p.shape[0],)), F32)
    return dict(points=p, half_width=w, weight=F32(weight))


def _rows(r, B, dtype):
    """(points [B, R, 2], W2 [B, 1]) of a launch of B rows: row r reads scene r % S; W2 one rounded product."""
    p, w = r["points"], r["half_width"]
    assert B % p.shape[0] == 0
    n = B // p.shape[0]
    w = np.tile(w, n).astype(dtype)
    with np.errstate(all="ignore"):
        return np.tile(p, (n, 1, 1)).astype(dtype), (w * w)[:, None]


def segments(r, x, y, dtype=F32):
    """x, y [B, H] -> per segment i the arrays [R-1, B, H] of the contract's loop body, in `dtype`, every operation rounded on
    its own: d2, (rx, ry), the clamped t, the raw quotient, and |e| and |u| for the bounds."""
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    pts, _ = _rows(r, x.shape[0], dtype)
    zero, one = dtype(0), dtype(1)
    out = dict(d2=[], rx=[], ry=[], t=[], raw=[], ee=[], uu=[])
    with np.errstate(all="ignore"):
        for i in range(pts.shape[1] - 1):
            ax, ay = pts[:, i, 0][:, None], pts[:, i, 1][:, None]
            ex, ey = pts[:, i + 1, 0][:, None] - ax, pts[:, i + 1, 1][:, None] - ay
            ux, uy = x - ax, y - ay
            ee = ex * ex + ey * ey
            ue = ux * ex + uy * ey
            raw = np.where(ee > 0, ue / np.where(ee > 0, ee, one), zero)
            t = np.where(raw < 0, zero, np.where(raw > 1, one, raw)).astype(dtype)      # a NaN passes through
            rx, ry = ux - t * ex, uy - t * ey
            d2 = rx * rx + ry * ry
            for k, v in (("d2", d2), ("rx", rx), ("ry", ry), ("t", t), ("raw", raw), ("ee", np.broadcast_to(ee, d2.shape)),
                         ("uu", ux * ux + uy * uy)):
                out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}


def nearest(r, x, y, dtype=F32):
    """-> (best [B, H], qx, qy, winner [B, H] int, -1 where nothing won): strict `<` in index order, so the first of equals wins
    and a NaN never does."""
    s = segments(r, x, y, dtype)
    shape = s["d2"].shape[1:]
    best = np.full(shape, np.inf, dtype)
    qx, qy = np.zeros(shape, dtype), np.zeros(shape, dtype)
    win = np.full(shape, -1, np.int64)
    with np.errstate(all="ignore"):
        for i in range(s["d2"].shape[0]):
            less = s["d2"][i] < best
            best = np.where(less, s["d2"][i], best)
            qx, qy = np.where(less, s["rx"][i], qx), np.where(less, s["ry"][i], qy)
            win = np.where(less, i, win)
    return best, qx, qy, win


def route_term(r, x, y, dtype=F32):
    """x, y [B, H] -> (on [B, H] bool, the cost (weight * (phi * phi)) / 2, k * qx, k * qy, best, phi) in `dtype`.  A weight of
    exactly 0: nothing is on."""
    best, qx, qy, _ = nearest(r, x, y, dtype)
    _, W2 = _rows(r, best.shape[0], dtype)
    w, two = dtype(r["weight"]), dtype(2)
    with np.errstate(all="ignore"):
        phi = best - W2
        on = (best < np.inf) & (phi > 0) & (w != 0)
        k = w * (two * phi)
        return on, (w * (phi * phi)) / two, k * qx, k * qy, best, phi


def route_share(r, x, y, J, gx, gy, active, dtype=F32):
    """The route term added to (J, gx, gy, active) [B, H]; nothing at all where it is inactive, not even a zero."""
    on, tj, tx, ty, _, _ = route_term(r, x, y, dtype)
    with np.errstate(all="ignore"):
        return np.where(on, J + tj, J), np.where(on, gx + tx, gx), np.where(on, gy + ty, gy), active + on


def route_cost(r, x, y, dtype=F64):
    """The route term alone: per waypoint [B, H]."""
    on, tj, _, _, _, _ = route_term(r, x, y, dtype)
    return np.where(on, tj, dtype(0))


@contextlib.contextmanager
def _routed(r):
    """guide_ref with `r` in its cost_grad, for the calls made inside the block (inside field_ref._fielded where there is a
    field, outside motion_ref._motioned where there are limits)."""
    if r is None:
        yield
        return
    inner = G.cost_grad

    def wrapped(discs, planes, x, y, dtype=F32):
        return route_share(r, x, y, *inner(discs, planes, x, y, dtype), dtype=dtype)

    G.cost_grad = wrapped
    try:
        yield
    finally:
        G.cost_grad = inner


@contextlib.contextmanager
def _guided(f, r, m):
    with FR._fielded(f), _routed(r), MR._motioned(m):
        yield


def _of(guide):
    return (None, None, None) if guide is None else (guide.get("field"), guide.get("route"), guide.get("motion"))


def cost_grad(discs, planes, f, r, m, x, y, dtype=F32):
    """v1's discs and planes, v2's field, the route, then v3's motion terms, into the same J, gx, gy and active count."""
    with _guided(f, r, m):
        return G.cost_grad(discs, planes, x, y, dtype)


def iterate(px, py, discs, planes, f, r, m, lam, cap, iters, clip, clip_range):
    with _guided(f, r, m):
        return G.iterate(px, py, discs, planes, lam, cap, iters, clip, clip_range)


def step(ddpm, c, mo, x, z=None, *, guide=None, **kw):
    with _guided(*_of(guide)):
        return G.step(ddpm, c, mo, x, z, guide=guide, **kw)


def dpm_step(co, prediction_type, thresholding, mo, x, prev_x0=None, z=None, *, guide=None, **kw):
    with _guided(*_of(guide)):
        return G.dpm_step(co, prediction_type, thresholding, mo, x, prev_x0, z, guide=guide, **kw)


def row_cost(traj, discs, planes, f, r, m, dtype=F64):
    with _guided(f, r, m):
        return G.row_cost(traj, discs, planes, dtype)


def row_cost_wave(traj, discs, planes, f, r, m):
    with _guided(f, r, m):
        return G.row_cost_wave(traj, discs, planes)


def _gamma(n):
    return n * U / (1 - n * U)


def best_bound(r, x, y):
    """|fp32 best - fp64 best| per waypoint [B, H], from the contract's lines, for fp32 inputs (exact in fp64).  Per segment, with
    |u|, |e|, |r| the fp64 lengths:
      ex, ey, ux, uy carry one rounding each; ee = ex * ex + ey * ey is a sum of nonnegative terms with four roundings on each
      path, |d ee| <= gamma_4 ee; ue = ux * ex + uy * ey likewise but signed: |d ue| <= gamma_4 |u| |e|;
      t = ue / ee one rounding more: |d t| |e| <= gamma_4 |u| + gamma_5 |t| |e| before the clamp.  The clamp is a contraction, and
      a quotient beyond 2 in magnitude clamps to the same end in both, so |d t| |e| <= gamma_4 |u| + gamma_5 * 2 |e| after it.
      A degenerate segment has t = 0 and e = 0 in both: the same formula with |e| = 0;
      rx = ux - t * ex: the rounding of ux, the moved t, two roundings in t * ex (ex's own and the product's, t <= 1) and the
      subtraction's: |d r| <= u |u| + |d t| |e| + 2 u |e| + u |r| <= gamma_5 |u| + gamma_7 * 2 |e| + u |r| =: dr;
      d2 = rx * rx + ry * ry: |d d2| <= 2 |r| dr + dr^2 + gamma_2 (|r| + dr)^2 =: b_i.
    The minimum: fp32's best is at most d2_w + b_w for fp64's winner w and at least min_i (d2_i - b_i), whichever segment fp32
    picks -- the cost depends on the minimum only, so a different winner needs no allowance beyond this."""
    s = segments(r, x, y, F64)
    rr = np.sqrt(s["d2"])
    dr = _gamma(5) * np.sqrt(s["uu"]) + _gamma(7) * 2 * np.sqrt(s["ee"]) + U * rr
    b = 2 * rr * dr + dr * dr + _gamma(2) * (rr + dr) ** 2
    best = s["d2"].min(axis=0)
    w = s["d2"].argmin(axis=0)
    upper = np.take_along_axis(b, w[None], axis=0)[0]
    lower = best - (s["d2"] - b).min(axis=0)
    return np.maximum(upper, lower)


def phi_bound(r, x, y):
    """|fp32 phi - fp64 phi| per waypoint: best's bound, one rounding of W2 and one of the subtraction."""
    _, _, _, _, best, phi = route_term(r, x, y, F64)
    _, W2 = _rows(r, best.shape[0], F64)
    with np.errstate(all="ignore"):
        return best_bound(r, x, y) + U * W2 + U * np.abs(phi)


def term_bound(r, x, y):
    """|fp32 term - fp64 term| per waypoint [B, H] where the term is active: with dphi of `phi_bound`, the cost
    (w * (phi * phi)) / 2 moves by w * (|phi| * dphi + dphi^2 / 2) and carries three roundings of its own, gamma_3 * cost."""
    on, tj, _, _, _, phi = route_term(r, x, y, F64)
    dphi = phi_bound(r, x, y)
    with np.errstate(all="ignore"):
        return np.where(on, F64(r["weight"]) * (np.abs(phi) * dphi + dphi * dphi / 2) + _gamma(3) * tj, 0.0)


def cost_bound(traj, discs, planes, f, r, m):
    """|fp32 cost - fp64 cost| per row, derived as motion_ref.cost_bound derives it.  That bound, taken over the terms with the
    route's among them, covers v1 to v3 and the summation.  The route term adds its own error, which is NOT relative to the term --
    phi = best - W2 cancels at the corridor's edge -- and is absolute instead: `term_bound`, summed over the row.  One
    more rounding per term for the summation into J and the butterfly: u * (H + 6) * sum |J|.  It presumes fp32 and fp64 agree
    on which terms are active: `hinge_margin` against `phi_bound` says whether they can differ."""
    if r is None:
        return MR.cost_bound(traj, discs, planes, f, m)
    with _routed(r):
        base = MR.cost_bound(traj, discs, planes, f, m)
        _, _, J = MR.row_cost(traj, discs, planes, f, m, F64)
    t = G._np(traj, F64)
    x, y = t[:, :, 0], t[:, :, 1]
    return base + U * (x.shape[1] + 6) * np.abs(J).sum(axis=1) + term_bound(r, x, y).sum(axis=1)


def hinge_margin(r, x, y):
    """|phi| per waypoint in fp64 (inf where the width is +inf or NaN, or the weight 0: no kink there)."""
    _, _, _, _, _, phi = route_term(r, x, y, F64)
    return np.where(np.isfinite(phi) & (r["weight"] != 0), np.abs(phi), np.inf)


def smooth(r, x, y, margin=1e-4):
    """[B, H] bool: waypoints where the fp64 term is smooth within `margin` -- away from the medial axis (every segment within
    `margin` of the best d2 has the winner's closest point), from the lines where a near-winner's closest point passes from the
    segment's inside to an end (t = 0, t = 1: the cost is C1 there, its second derivative jumps) and from the hinge phi = 0."""
    s = segments(r, x, y, F64)
    best, qx, qy, _ = nearest(r, x, y, F64)
    ok = hinge_margin(r, x, y) > margin
    with np.errstate(all="ignore"):
        for i in range(s["d2"].shape[0]):
            near = s["d2"][i] - best < margin
            same = (np.abs(s["rx"][i] - qx) < 1e-9) & (np.abs(s["ry"][i] - qy) < 1e-9)
            along = np.minimum(np.abs(s["raw"][i]), np.abs(s["raw"][i] - 1)) * np.sqrt(s["ee"][i])      # distance to t = 0 / t = 1
            ok &= ~near | (same & ((along > margin) | (s["ee"][i] == 0)))
    return ok


# -- the fixture of the issue -----------------------------------------------------------------------------------------------------
FIX_POINTS = np.array([[[-0.8, -0.5], [-0.4, -0.45], [0.0, -0.1], [0.3, 0.3], [0.35, 0.6], [0.8, 0.7]]], F32)      # a 6-point route
FIX_WIDTHS = (0.0, 0.1, 0.25)
FIX_ROWS, FIX_H = 400, 50


def fixture_points(seed=0):
    """[400, 50, 2] float32: 20,000 uniform points in [-1, 1]^2."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (FIX_ROWS, FIX_H, 2)).astype(F32)
