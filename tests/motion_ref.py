"""Test infrastructure: "cost guidance v3" (include/adx.h) restated -- per-scene limits on the length of a segment and of a second
difference of a row of waypoints.

`motion_share` is NumPy, one rounded operation per operation of the contract, in its order, in the dtype it is given: float32 is
the bit-for-bit restatement of `motion_grad` (csrc/guide.h), float64 the yardstick of the cost.  It works on whole rows [B, H]:
the terms couple neighbours, which is what guide_ref's functions already hand to `cost_grad` (an iteration of guide_ref.iterate
moves every waypoint of the array at once: Jacobi).  Everything that is v1 or v2 is tests/guide_ref.py's and tests/field_ref.py's
own function: `_motioned` wraps guide_ref's `cost_grad` -- after field_ref's `_fielded` wrapped it, so the order is discs, planes,
field, motion, the contract's -- for as long as one call of `iterate`, `step`, `dpm_step`, `row_cost` or `row_cost_wave` runs.

Motion limits here are a dict (`motion(...)` makes one): limits [S, 2] float32 NumPy and w_speed, w_accel as the fp32 numbers the
kernel receives.  A guide is guide_ref's dict with the keys "field" and "motion" (absent or None: v1 / v2).
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

import field_ref as FR
import guide_ref as G

F32, F64, U = G.F32, G.F64, G.U
# rounded operations from the waypoints to one term of J (the contract's lines, counted).  Segment: ex, ey, two squares, s2, phi,
# phi * phi, w * , / 2 and S2.  Curvature: four first differences more than that, the rest alike.
SEG_OPS, CURV_OPS = 10, 14


def motion(limits, w_speed=1.0, w_accel=1.0) -> dict:
    l = limits.detach().cpu().numpy() if torch.is_tensor(limits) else np.asarray(limits)
    return dict(limits=np.ascontiguousarray(l, F32).reshape(-1, 2), w_speed=F32(w_speed), w_accel=F32(w_accel))


def _rows(m, B, dtype):
    """(S2, A2) [B, 1] of a launch of B rows: row r reads scene r % S; one rounded product each."""
    l = m["limits"]
    assert B % l.shape[0] == 0
    l = np.tile(l, (B // l.shape[0], 1)).astype(dtype)
    with np.errstate(all="ignore"):
        return (l[:, 0] * l[:, 0])[:, None], (l[:, 1] * l[:, 1])[:, None]


def terms(m, x, y, dtype=F32):
    """x, y [B, H] -> the segments [B, H-1] and the curvatures [B, H-2] of every row, each a dict: on (active), arg (phi or psi),
    vx, vy (e or c), k (w * (2 * arg)) and cost ((w * (arg * arg)) / 2), in `dtype`, every operation rounded on its own.  A zero
    weight: nothing is on.  H < 2 (or 3): empty arrays."""
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    B, H = x.shape
    S2, A2 = _rows(m, B, dtype)
    two = dtype(2)
    ws, wa = dtype(m["w_speed"]), dtype(m["w_accel"])
    with np.errstate(all="ignore"):
        ex, ey = x[:, 1:] - x[:, :-1], y[:, 1:] - y[:, :-1]
        phi = (ex * ex + ey * ey) - S2
        seg = dict(on=(phi > 0) & (ws != 0), arg=phi, vx=ex, vy=ey, k=ws * (two * phi), cost=(ws * (phi * phi)) / two)
        cx, cy = ex[:, 1:] - ex[:, :-1], ey[:, 1:] - ey[:, :-1]
        psi = (cx * cx + cy * cy) - A2
        curv = dict(on=(psi > 0) & (wa != 0), arg=psi, vx=cx, vy=cy, k=wa * (two * psi), cost=(wa * (psi * psi)) / two)
    return seg, curv


def _at(t, key, first, H, fill=0):
    """A term array [B, n] as seen from the waypoints: out[:, h] = t[key][:, h - first] where that term exists."""
    a = t[key]
    out = np.full((a.shape[0], H), fill, a.dtype)
    lo, hi = max(first, 0), min(first + a.shape[1], H)
    if hi > lo:
        out[:, lo:hi] = a[:, lo - first:hi - first]
    return out


def motion_share(m, x, y, J, gx, gy, active, dtype=F32):
    """Waypoint h's share added to (J, gx, gy, active) [B, H] in the contract's order: J and active take segment h-1, then
    curvature h; the gradient takes segment h-1, segment h, curvature h-1, curvature h, curvature h+1; nothing at all where a term
    is absent or inactive, and no motion gradient at h = 0."""
    H = np.asarray(x).shape[1]
    seg, curv = terms(m, x, y, dtype)
    free = np.arange(H)[None, :] >= 1                                   # the anchor
    two = dtype(2)
    with np.errstate(all="ignore"):
        # term index i seen from waypoint h: segment h-1 -> first = 1, segment h -> 0, curvature i lives at i = 1..H-2 so its
        # array index 0 is curvature 1: curvature h-1 -> first = 2, curvature h -> 1, curvature h+1 -> 0
        on = _at(seg, "on", 1, H, False)
        J = np.where(on, J + _at(seg, "cost", 1, H), J)
        active = active + on
        gx = np.where(on & free, gx + _at(seg, "k", 1, H) * _at(seg, "vx", 1, H), gx)
        gy = np.where(on & free, gy + _at(seg, "k", 1, H) * _at(seg, "vy", 1, H), gy)
        on = _at(seg, "on", 0, H, False) & free
        gx = np.where(on, gx - _at(seg, "k", 0, H) * _at(seg, "vx", 0, H), gx)
        gy = np.where(on, gy - _at(seg, "k", 0, H) * _at(seg, "vy", 0, H), gy)
        on = _at(curv, "on", 2, H, False) & free
        gx = np.where(on, gx + _at(curv, "k", 2, H) * _at(curv, "vx", 2, H), gx)
        gy = np.where(on, gy + _at(curv, "k", 2, H) * _at(curv, "vy", 2, H), gy)
        on = _at(curv, "on", 1, H, False)
        J = np.where(on, J + _at(curv, "cost", 1, H), J)
        active = active + on
        q2 = two * _at(curv, "k", 1, H)
        gx = np.where(on & free, gx - q2 * _at(curv, "vx", 1, H), gx)
        gy = np.where(on & free, gy - q2 * _at(curv, "vy", 1, H), gy)
        on = _at(curv, "on", 0, H, False) & free
        gx = np.where(on, gx + _at(curv, "k", 0, H) * _at(curv, "vx", 0, H), gx)
        gy = np.where(on, gy + _at(curv, "k", 0, H) * _at(curv, "vy", 0, H), gy)
    return J, gx, gy, active


def cost_grad(discs, planes, f, m, x, y, dtype=F32):
    """v1's discs and planes, v2's field, then the motion terms, into the same J, gx, gy and active count."""
    J, gx, gy, active = FR.cost_grad(discs, planes, f, x, y, dtype)
    return (J, gx, gy, active) if m is None else motion_share(m, x, y, J, gx, gy, active, dtype)


@contextlib.contextmanager
def _motioned(m):
    """guide_ref with `m` in its cost_grad, for the calls made inside the block (inside field_ref._fielded where there is a field)."""
    if m is None:
        yield
        return
    inner = G.cost_grad

    def wrapped(discs, planes, x, y, dtype=F32):
        return motion_share(m, x, y, *inner(discs, planes, x, y, dtype), dtype=dtype)

    G.cost_grad = wrapped
    try:
        yield
    finally:
        G.cost_grad = inner


@contextlib.contextmanager
def _guided(f, m):
    with FR._fielded(f), _motioned(m):
        yield


def _of(guide):
    return (None, None) if guide is None else (guide.get("field"), guide.get("motion"))


def iterate(px, py, discs, planes, f, m, lam, cap, iters, clip, clip_range):
    with _guided(f, m):
        return G.iterate(px, py, discs, planes, lam, cap, iters, clip, clip_range)


def step(ddpm, c, mo, x, z=None, *, guide=None, **kw):
    with _guided(*_of(guide)):
        return G.step(ddpm, c, mo, x, z, guide=guide, **kw)


def dpm_step(co, prediction_type, thresholding, mo, x, prev_x0=None, z=None, *, guide=None, **kw):
    with _guided(*_of(guide)):
        return G.dpm_step(co, prediction_type, thresholding, mo, x, prev_x0, z, guide=guide, **kw)


def row_cost(traj, discs, planes, f, m, dtype=F64):
    with _guided(f, m):
        return G.row_cost(traj, discs, planes, dtype)


def row_cost_wave(traj, discs, planes, f, m):
    with _guided(f, m):
        return G.row_cost_wave(traj, discs, planes)


def row_grad(traj, discs, planes, f, m, dtype=F64):
    """(gx, gy) [rows, H] of the row cost: what one iteration steps along."""
    t = G._np(traj, dtype)
    B = t.shape[0]
    _, gx, gy, _ = cost_grad(G.scene_rows(G._np(discs, dtype), B), G.scene_rows(G._np(planes, dtype), B), f, m, t[:, :, 0], t[:, :, 1], dtype)
    return gx, gy


def motion_cost(m, x, y, dtype=F64):
    """The motion terms alone, every term once: [B]."""
    seg, curv = terms(m, x, y, dtype)
    return np.where(seg["on"], seg["cost"], 0).sum(axis=1) + np.where(curv["on"], curv["cost"], 0).sum(axis=1)


def cost_bound(traj, discs, planes, f, m):
    """|fp32 cost - fp64 cost| per row, derived as field_ref.cost_bound derives it.  That bound, taken over the terms with the
    motion terms among them, covers v1, v2 and the summation.  A motion term adds its own error, which is NOT relative to the
    term -- phi = s2 - S2 cancels -- and is bounded from the contract's lines instead:
      s2 = ex * ex + ey * ey carries the roundings of ex, ey (relative 2u on each square), the two squares and the sum:
      |d s2| <= gamma_4 * s2;  S2 one rounding: |d S2| <= u * S2;  the subtraction one more: |d phi| <= gamma_4 s2 + u S2 + u |phi|
      =: dphi, and a2 likewise with gamma_6 (cx is a difference of two rounded differences: relative to |fx| + |bx|, so a2's bound
      uses (|f| + |b|)^2 in place of a2);
      the cost w * phi^2 / 2 moves by w * |phi| * dphi (to first order; the second-order term w * dphi^2 / 2 is added) and carries
      three more roundings of its own: gamma_3 * cost.
    The sum over a row's terms; one more rounding per term for the summation into J and the butterfly: u * (H + 6) * sum |J|.
    It presumes fp32 and fp64 agree on which terms are active: `hinge_margin` says by how much."""
    base = FR.cost_bound(traj, discs, planes, f) if m is None else None
    if m is None:
        return base
    with _motioned(m):
        base = FR.cost_bound(traj, discs, planes, f)
        _, _, J = FR.row_cost(traj, discs, planes, f, F64)
    t = G._np(traj, F64)
    x, y = t[:, :, 0], t[:, :, 1]
    B, H = x.shape
    S2, A2 = _rows(m, B, F64)
    seg, curv = terms(m, x, y, F64)
    g = FR._gamma
    own = np.zeros(B)
    with np.errstate(all="ignore"):
        s2 = seg["arg"] + S2
        dphi = g(4) * s2 + U * S2 + U * np.abs(seg["arg"])
        w = F64(m["w_speed"])
        own += np.where(seg["on"], w * (np.abs(seg["arg"]) * dphi + dphi * dphi / 2) + g(3) * seg["cost"], 0.0).sum(axis=1)
        ex, ey = np.abs(x[:, 1:] - x[:, :-1]), np.abs(y[:, 1:] - y[:, :-1])
        big = (ex[:, 1:] + ex[:, :-1]) ** 2 + (ey[:, 1:] + ey[:, :-1]) ** 2
        dpsi = g(6) * big + U * A2 + U * np.abs(curv["arg"])
        w = F64(m["w_accel"])
        own += np.where(curv["on"], w * (np.abs(curv["arg"]) * dpsi + dpsi * dpsi / 2) + g(3) * curv["cost"], 0.0).sum(axis=1)
    return base + U * (H + 6) * np.abs(J).sum(axis=1) + own


def hinge_margin(traj, discs, planes, f, m, skip=None):
    """field_ref.hinge_margin and the motion terms' |phi| and |psi| (terms whose limit is +inf or NaN, or whose weight is 0, have
    no kink): how far every hinge of the cost stands from its kink, in fp64."""
    least = FR.hinge_margin(traj, discs, planes, f, skip)
    if m is None:
        return least
    t = G._np(traj, F64)
    seg, curv = terms(m, t[:, :, 0], t[:, :, 1], F64)
    for term, w in ((seg, m["w_speed"]), (curv, m["w_accel"])):
        a = term["arg"][np.isfinite(term["arg"])]
        if w != 0 and a.size:
            least = min(least, np.abs(a).min())
    return least


def hinge_slack(traj, f, m):
    """How far fp32's hinge arguments can stand from fp64's: the largest dphi / dpsi of cost_bound over the rows, so that a margin
    above it means fp32 and fp64 agree on every motion term's activity."""
    t = G._np(traj, F64)
    x, y = t[:, :, 0], t[:, :, 1]
    S2, A2 = _rows(m, x.shape[0], F64)
    seg, curv = terms(m, x, y, F64)
    g = FR._gamma
    worst = 0.0
    with np.errstate(all="ignore"):
        fin = lambda a: a[np.isfinite(a)]  # noqa: E731
        d = fin(g(4) * (seg["arg"] + S2) + U * S2 + U * np.abs(seg["arg"]))
        worst = max(worst, d.max() if d.size else 0.0)
        ex, ey = np.abs(x[:, 1:] - x[:, :-1]), np.abs(y[:, 1:] - y[:, :-1])
        big = (ex[:, 1:] + ex[:, :-1]) ** 2 + (ey[:, 1:] + ey[:, :-1]) ** 2
        d = fin(g(6) * big + U * A2 + U * np.abs(curv["arg"]))
        worst = max(worst, d.max() if d.size else 0.0)
    return worst


# -- the fixture of the issue -----------------------------------------------------------------------------------------------------
FIX_S_MAX, FIX_A_MAX = 0.03, 0.02
FIX_HS = (2, 3, 5, 8, 16, 64)


def fixture_rows(H, rows=20, seed=0):
    """[rows, H, 2] float64: x drifts 0.03 per waypoint, Gaussian scatter 0.02 on x and y, p_0 = 0."""
    g = np.random.default_rng(seed + H)
    t = g.normal(0.0, 0.02, (rows, H, 2))
    t[:, :, 0] += 0.03 * np.arange(H)[None, :]
    t[:, 0, :] = 0.0
    return t
