"""Test infrastructure: "stop-short fallback v1" (include/adx.h) restated in NumPy -- re-time a plan so that it brakes to a halt
before its first conflicting waypoint.

`stop_short` is one rounded operation per operation of the contract, in its order, in the dtype it is given: float32 is the
bit-for-bit restatement of `stop_short_kernel` (csrc/fallback.hip), float64 the yardstick of the contract's properties.  It is
vectorised over rows and sequential over waypoints, as the contract is.  Whether a waypoint conflicts is tests/capsule_ref.py's
`cost_grad` -- discs, planes, field, route and capsules in the contract's order, without motion limits -- and nothing of it is
restated here.

A guide here is a dict (`guide(...)` makes one): discs [S, M, 5] / planes [S, P, 3] float32 NumPy or None, and the dicts of
field_ref.field, route_ref.route and capsule_ref.capsules or None.
"""
from __future__ import annotations

import numpy as np

import capsule_ref as CR
import guide_ref as G

F32, F64 = G.F32, G.F64


def guide(discs=None, planes=None, field=None, route=None, capsules=None) -> dict:
    return dict(discs=G._np(discs, F32), planes=G._np(planes, F32), field=field, route=route, capsules=capsules)


def active(g: dict, x, y, dtype=F32):
    """The active count per waypoint [B, H] of x, y [B, H] (waypoint h at time h), row r against scene r % S."""
    B = x.shape[0]
    d, p = G.scene_rows(G._np(g["discs"], dtype), B), G.scene_rows(G._np(g["planes"], dtype), B)
    with np.errstate(all="ignore"):
        return CR.cost_grad(d, p, g["field"], g["route"], g["capsules"], None, x, y, dtype)[3]


def stop_short(traj, g: dict, params, dtype=F32) -> dict:
    """traj [B, H, D], params [P, 2] = (gap, decel): the contract's outputs `out` [B, H, D], `first`, `status`, `active_after`
    [B] int32 and `stop_at` [B], and what the property tests read: seg, s, q, u, w, d [B, H], L and the limit switch [B]."""
    t = G._np(traj, dtype)
    B, H, D = t.shape
    x, y = t[:, :, 0], t[:, :, 1]
    prm = np.asarray(G._np(params, dtype)).reshape(-1, 2)
    prm = prm[np.arange(B) % prm.shape[0]]
    gap, a = prm[:, 0], prm[:, 1]
    zero, half, eight, inf = dtype(0), dtype(0.5), dtype(8), dtype(np.inf)
    hidx = np.arange(H)[None, :]
    rows = np.arange(B)
    with np.errstate(all="ignore"):
        # 1. conflicts
        conflict = (active(g, x, y, dtype) > 0) | ~np.isfinite(x) | ~np.isfinite(y)
        first = np.where(conflict.any(axis=1), conflict.argmax(axis=1), H)
        blocked = first < H
        # 3. arc length, in index order
        seg = np.zeros((B, H), dtype)
        dx, dy = x[:, 1:] - x[:, :-1], y[:, 1:] - y[:, :-1]
        seg[:, 1:] = np.sqrt(dx * dx + dy * dy)
        seg = np.where((hidx >= 1) & (hidx < first[:, None]), seg, zero).astype(dtype)
        s = np.zeros((B, H), dtype)
        for h in range(1, H):
            s[:, h] = s[:, h - 1] + seg[:, h]
        # 4. the stop point
        gp = np.where(gap >= 0, gap, zero).astype(dtype)
        tl = s[rows, np.maximum(first - 1, 0)] - gp
        L = np.where(first >= 1, np.where(tl > 0, tl, zero), zero).astype(dtype)
        # 5. the speed profile
        limited = np.isfinite(a) & (a >= 0)
        aa, a8 = a * a, eight * a
        q, u, w, d = (np.zeros((B, H), dtype) for _ in range(4))
        w[:, 0], d[:, 0] = inf, L
        for h in range(1, H):
            d[:, h] = L - q[:, h - 1]
            w[:, h] = np.where(h < first, seg[:, h], inf)
            uh = np.where(d[:, h] < w[:, h], d[:, h], w[:, h]).astype(dtype)
            e = (np.sqrt(aa + a8 * d[:, h]) - a) * half
            uh = np.where(limited & (e < uh), e, uh).astype(dtype)
            u[:, h] = uh
            q[:, h] = q[:, h - 1] + uh
        late = (first > 1) & limited & (seg[:, 1] - u[:, 1] > a) if H > 1 else np.zeros(B, bool)
        status = np.where(blocked, np.where(late, 2, 1), 0).astype(np.int32)
        # 6. resample
        j = np.zeros((B, H), np.int64)
        s_j = np.zeros((B, H), dtype)
        for k in range(H):
            m = (k < first)[:, None] & (s[:, k:k + 1] <= q)
            j = np.where(m, k, j)
            s_j = np.where(m, s[:, k:k + 1], s_j).astype(dtype)
        jn = np.minimum(j + 1, H - 1)
        jx, jy = np.take_along_axis(x, j, 1), np.take_along_axis(y, j, 1)
        nx, ny = np.take_along_axis(x, jn, 1), np.take_along_axis(y, jn, 1)
        s_n = np.take_along_axis(s, jn, 1)
        lerp = (first[:, None] != 0) & (j != first[:, None] - 1) & ~(q == s_j)
        tt = ((q - s_j) / (s_n - s_j)).astype(dtype)
        ox = np.where(lerp, jx + tt * (nx - jx), jx).astype(dtype)
        oy = np.where(lerp, jy + tt * (ny - jy), jy).astype(dtype)
        # 7. the residual
        after = np.where(blocked, active(g, ox, oy, dtype).sum(axis=1), 0).astype(np.int32)
    out = t.copy()
    out[:, :, 0] = np.where(blocked[:, None], ox, x)
    out[:, :, 1] = np.where(blocked[:, None], oy, y)
    return dict(out=out, first=first.astype(np.int32), status=status, stop_at=np.where(blocked, L, inf).astype(dtype), active_after=after,
                seg=seg, s=s, q=q, u=u, w=w, d=d, t=np.where(lerp, tt, zero), L=L, limited=limited, blocked=blocked, a=a)
