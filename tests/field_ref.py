"""Test infrastructure: "cost guidance v2" and "cost field from occupancy v1" (include/adx.h) restated.

`field_term` is NumPy, one rounded operation per operation of the contract, in its order, in the dtype it is given: float32 is
the bit-for-bit restatement of the field branch of the kernels' `guide_grad` (csrc/guide.h), float64 the yardstick of the cost.
Everything else is tests/guide_ref.py's own function with that term added to its `cost_grad`: `_fielded` swaps guide_ref's
`cost_grad` for one that evaluates v1's discs and planes first and the field after them -- the contract's order -- for as long as
one call of `iterate`, `step`, `dpm_step`, `row_cost` or `row_cost_wave` runs.  Nothing of those functions is copied here.

A field here is a dict (`field(...)` makes one): cells [S, Gy, Gx] float32 NumPy, and x_min, y_min, inv_dx, inv_dy, weight as the
fp32 numbers the kernel receives.  A guide is guide_ref's dict with one more key, "field" (absent or None: v1).
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

import guide_ref as G

F32, F64, U = G.F32, G.F64, G.U
# rounded operations from the inputs to one field term weight * C of J (the contract's lines, counted): u and v two each; a, b,
# fu * a, fu * b, top, bot, dv, fv * dv, C; weight * C
FIELD_OPS = 14


def field(cells, origin=(0.0, 0.0), cell=(1.0, 1.0), weight=1.0) -> dict:
    """The launch's view of CostField(cells, origin, cell, weight): inv_dx = fp32(1 / dx), formed in double as the host does."""
    c = cells.detach().cpu().numpy() if torch.is_tensor(cells) else np.asarray(cells)
    return dict(cells=np.ascontiguousarray(c, F32), x_min=F32(origin[0]), y_min=F32(origin[1]), inv_dx=F32(1.0 / float(cell[0])),
                inv_dy=F32(1.0 / float(cell[1])), weight=F32(weight))


def _locate(f, x, y, dtype):
    """-> (inside, i, j, fu, fv, u, v) of waypoints x, y [B, H]; i, j, fu, fv are of a safe stand-in where a waypoint is outside."""
    Gy, Gx = f["cells"].shape[1:]
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    u = (x - dtype(f["x_min"])) * dtype(f["inv_dx"])
    v = (y - dtype(f["y_min"])) * dtype(f["inv_dy"])
    inside = (u >= 0) & (u <= dtype(Gx - 1)) & (v >= 0) & (v <= dtype(Gy - 1))          # a NaN compares false
    us, vs = np.where(inside, u, dtype(0)), np.where(inside, v, dtype(0))
    j = np.minimum(us.astype(np.int64), Gx - 2)                                         # (int)u truncates; u >= 0 here
    i = np.minimum(vs.astype(np.int64), Gy - 2)
    return inside, i, j, us - j.astype(dtype), vs - i.astype(dtype), u, v


def field_term(f, x, y, dtype=F32):
    """x, y [B, H] -> (on [B, H] bool, weight * C, (weight * du) * inv_dx, (weight * dv) * inv_dy, C, du, dv) in `dtype`, every
    operation rounded on its own; row r reads cells[r % S]."""
    B = np.asarray(x).shape[0]
    cells = f["cells"]
    assert B % cells.shape[0] == 0
    cells = np.tile(cells, (B // cells.shape[0], 1, 1)).astype(dtype)
    w, inv_dx, inv_dy = dtype(f["weight"]), dtype(f["inv_dx"]), dtype(f["inv_dy"])
    with np.errstate(all="ignore"):
        inside, i, j, fu, fv, _, _ = _locate(f, x, y, dtype)
        r = np.arange(B)[:, None]
        c00, c01, c10, c11 = cells[r, i, j], cells[r, i, j + 1], cells[r, i + 1, j], cells[r, i + 1, j + 1]
        a = c01 - c00
        b = c11 - c10
        top = c00 + fu * a
        bot = c10 + fu * b
        dv = bot - top
        C = top + fv * dv
        on = inside & (C > 0)
        du = a + fv * (b - a)
        return on, w * C, (w * du) * inv_dx, (w * dv) * inv_dy, C, du, dv


def cost_grad(discs, planes, f, x, y, dtype=F32, plain=None):
    """guide_ref.cost_grad, then the field term into the same J, gx, gy and active count."""
    J, gx, gy, active = (plain or G.cost_grad)(discs, planes, x, y, dtype)
    if f is None:
        return J, gx, gy, active
    on, tj, tx, ty, _, _, _ = field_term(f, x, y, dtype)
    with np.errstate(all="ignore"):
        return np.where(on, J + tj, J), np.where(on, gx + tx, gx), np.where(on, gy + ty, gy), active + on


@contextlib.contextmanager
def _fielded(f):
    """guide_ref with `f` in its cost_grad, for the calls made inside the block."""
    if f is None:
        yield
        return
    plain = G.cost_grad
    G.cost_grad = lambda discs, planes, x, y, dtype=F32: cost_grad(discs, planes, f, x, y, dtype, plain)
    try:
        yield
    finally:
        G.cost_grad = plain


def iterate(px, py, discs, planes, f, lam, cap, iters, clip, clip_range):
    with _fielded(f):
        return G.iterate(px, py, discs, planes, lam, cap, iters, clip, clip_range)


def step(ddpm, c, mo, x, z=None, *, guide=None, **kw):
    with _fielded(None if guide is None else guide.get("field")):
        return G.step(ddpm, c, mo, x, z, guide=guide, **kw)


def dpm_step(co, prediction_type, thresholding, mo, x, prev_x0=None, z=None, *, guide=None, **kw):
    with _fielded(None if guide is None else guide.get("field")):
        return G.dpm_step(co, prediction_type, thresholding, mo, x, prev_x0, z, guide=guide, **kw)


def row_cost(traj, discs, planes, f, dtype=F64):
    with _fielded(f):
        return G.row_cost(traj, discs, planes, dtype)


def row_cost_wave(traj, discs, planes, f):
    with _fielded(f):
        return G.row_cost_wave(traj, discs, planes)


def _gamma(n):
    return n * U / (1 - n * U)


def cost_bound(traj, discs, planes, f):
    """|fp32 cost - fp64 cost| per row, derived as guide_ref.cost_bound derives it.  That bound, taken over the terms with the field's
    among them, covers v1's terms and the summation of H * (M + P) terms; the field adds one term per waypoint to the sum (one more
    rounding each: 2^-24 * H * the sum of magnitudes) and its own error, which is NOT relative to the term -- the interpolant
    cancels -- and is bounded from the contract's lines instead:
      u carries two roundings, |du| <= gamma_2 |u| (and v likewise); u - (float)j is exact, so fu carries that absolute error and C
      moves by |dC/du| = |du| (in cell units) times it;
      each of the nine interpolation operations (a, b, fu * a, fu * b, top, bot, dv, fv * dv, C) rounds a value of magnitude
      <= 2 m, m = the largest |corner| of the cell, and reaches C with a coefficient of magnitude <= 1 (fu, fv in [0, 1]); weight * C
      is one more rounding of a value <= weight * m;
    so |error of weight * C| <= weight * (gamma_2 * (|du * u| + |dv * v|) * (1 + gamma_FIELD_OPS) + gamma_10 * 2 m), summed over a
    row's active waypoints.  It presumes fp32 and fp64 agree on the cell and on the sign of C: `margins` says by how much."""
    if f is None:
        return G.cost_bound(traj, discs, planes)
    t = G._np(traj, F64)
    with _fielded(f):
        base = G.cost_bound(traj, discs, planes)
        _, _, J = G.row_cost(traj, discs, planes, F64)
    H = J.shape[1]
    on, _, _, _, _, du, dv = field_term(f, t[:, :, 0], t[:, :, 1], F64)
    _, i, j, _, _, u, v = _locate(f, t[:, :, 0], t[:, :, 1], F64)
    B = t.shape[0]
    cells = np.abs(np.tile(f["cells"], (B // f["cells"].shape[0], 1, 1)).astype(F64))
    r = np.arange(B)[:, None]
    m = np.maximum(np.maximum(cells[r, i, j], cells[r, i, j + 1]), np.maximum(cells[r, i + 1, j], cells[r, i + 1, j + 1]))
    own = F64(f["weight"]) * (_gamma(2) * (np.abs(du * u) + np.abs(dv * v)) * (1 + _gamma(FIELD_OPS)) + _gamma(10) * 2 * m)
    return base + U * H * np.abs(J).sum(axis=1) + np.where(on, own, 0.0).sum(axis=1)


def margins(traj, f, skip=None):
    """In fp64: (the smallest |C| over waypoints inside the raster, the smallest distance -- in cells -- of a waypoint to a cell edge
    or to the raster's border).  `skip` [rows, H] bool: designated waypoints, left out of both."""
    t = G._np(traj, F64)
    Gy, Gx = f["cells"].shape[1:]
    x, y = t[:, :, 0], t[:, :, 1]
    _, _, _, _, C, _, _ = field_term(f, x, y, F64)
    inside, _, _, _, _, u, v = _locate(f, x, y, F64)
    keep = np.ones(x.shape, bool) if skip is None else ~np.asarray(skip, bool)
    least_c = np.abs(C[inside & keep]).min() if (inside & keep).any() else np.inf

    def edge(w, n):           # distance to the nearest integer in [0, n - 1]: every node line is an edge of a cell or of the raster
        near = np.clip(np.rint(w), 0, n - 1)
        return np.abs(w - near)

    with np.errstate(all="ignore"):
        d = np.minimum(edge(u, Gx), edge(v, Gy))
    # a waypoint far outside is only near the border line it is beyond: its distance to the raster is what matters
    return least_c, d[keep & np.isfinite(d)].min()


def hinge_margin(traj, discs, planes, f, skip=None):
    """guide_ref.hinge_margin and the field's |C|: how far every hinge of the cost stands from its kink, in fp64."""
    return min(G.hinge_margin(traj, discs, planes), np.inf if f is None else margins(traj, f, skip)[0])


# -- cost field from occupancy v1 ---------------------------------------------------------------------------------------------------
def from_occupancy(occ, dx, dy, inv_m2, ry, rx):
    """occ [S, Gy, Gx] -> cells float32, the contract in fp32 NumPy: d2 = the minimum over the window's occupied nodes of
    ((float)dj * dx)^2 + ((float)di * dy)^2, each product and the sum rounded on its own; phi = 1 - d2 * inv_m2."""
    occ = occ.detach().cpu().numpy() if torch.is_tensor(occ) else np.asarray(occ)
    with np.errstate(all="ignore"):
        full = occ.astype(F32) > F32(0.5)                                                # a NaN is free
    S, Gy, Gx = full.shape
    dx, dy, inv_m2 = F32(dx), F32(dy), F32(inv_m2)
    pad = np.zeros((S, Gy + 2 * ry, Gx + 2 * rx), bool)
    pad[:, ry:ry + Gy, rx:rx + Gx] = full
    best = np.full((S, Gy, Gx), np.inf, F32)
    with np.errstate(all="ignore"):
        for di in range(-ry, ry + 1):
            sy = F32(di) * dy
            yy = F32(sy * sy)
            for dj in range(-rx, rx + 1):
                sx = F32(dj) * dx
                xx = F32(sx * sx)
                d2 = F32(xx + yy)
                there = pad[:, ry + di:ry + di + Gy, rx + dj:rx + dj + Gx]               # node (i + di, j + dj)
                best = np.where(there & (d2 < best), d2, best)
        phi = F32(1) - best * inv_m2
        return np.where(phi > 0, (phi * phi) / F32(2), F32(0)).astype(F32)
