"""NumPy restatement of "expert v1" (include/adx.h), line by line: fp64, every product, sum, division and square root rounded on
its own in the header's order, no library call but sqrt.  The contract has none either, so the device must EQUAL this in every
bit of `plan`, `leader` and `info`.

`expert_plan(cfg, window, velocity, boxes, discs, planes)` takes what `adx_expert_plan` takes (host arrays, fp32) and returns the
three outputs plus, per scene, `clearance`: the smallest distance of any decision the evaluation made from its threshold --
corridor membership, ahead-or-behind, the arg-min leader (the runner-up's r minus the winner's), a plane's sign at the points it
is evaluated at, and the curve vertices against the look-ahead range.  A world whose clearance is tiny is one where a rounding
could flip a decision; the device is exact, so it would still agree, but random tests redraw such worlds to keep every case
robust against anything but a real defect.  `decisions` holds the same per kind, for the hand scenarios.

`defect=` plants a mistake ("swap_extents", "largest_r", "plane_side", "frozen_leader", "curve_behind") so that the CPU tests can
show that their scenarios catch it.
"""
import numpy as np

F = np.float64
INF = F(np.inf)
DISC, PLANE, END = 64, 128, 136
DEFECTS = ("swap_extents", "largest_r", "plane_side", "frozen_leader", "curve_behind")
CFG_DEFAULT = dict(xy_scale=20.0, waypoint_dt=0.5, desired_v=8.0, accel=1.5, brake=2.0, brake_max=8.0, headway=1.5, jam=2.0,
                   gap_min=0.25, corridor_half=1.75, lat_accel=2.0, look_time=2.0, ego_front=2.25, end_margin=1.0, look_min=10.0)


def word32(v):
    """Round fp64 to fp32 once; a NaN is the word 0x7fc00000."""
    with np.errstate(all="ignore"):
        f = np.asarray(v, dtype=F).astype(np.float32)
    return np.where(np.isnan(f), np.array(0x7fc00000, dtype=np.uint32).view(np.float32), f).astype(np.float32)


class Path:
    def __init__(self, win, xs):
        P = np.asarray(win, dtype=np.float32).astype(F) * F(xs)                    # [R, 2]
        e = P[1:] - P[:-1]
        exx, eyy = e[:, 0] * e[:, 0], e[:, 1] * e[:, 1]
        l2 = exx + eyy
        good = l2 > 0.0                                                            # a NaN is not
        ln = np.where(good, np.sqrt(np.where(good, l2, 1.0)), 0.0)
        safe = np.where(good, ln, 1.0)
        self.P, self.e, self.l2, self.good, self.len = P, e, l2, good, ln
        self.tau = np.stack([np.where(good, e[:, 0] / safe, 0.0), np.where(good, e[:, 1] / safe, 0.0)], axis=1)
        cum = np.zeros(len(P), dtype=F)
        c = F(0.0)
        for j in range(len(P) - 1):
            c = c + ln[j]
            cum[j + 1] = c
        self.cum, self.R = cum, len(P)
        self.ends = not bool(good[-1])

    def project(self, q):
        """`project` for points q [n, 2] in metres: (s, d, j, c) arrays."""
        q = np.asarray(q, dtype=F).reshape(-1, 2)
        n = len(q)
        bs, bd, bj, bc = np.zeros(n), np.full(n, INF), np.zeros(n, dtype=np.int64), np.zeros((n, 2))
        for j in range(self.R - 1):
            ax, ay, ex, ey = self.P[j, 0], self.P[j, 1], self.e[j, 0], self.e[j, 1]
            t = np.zeros(n)
            if self.good[j]:
                rx, ry = q[:, 0] - ax, q[:, 1] - ay
                m0, m1 = rx * ex, ry * ey
                f = (m0 + m1) / self.l2[j]
                t = np.where(f > 0.0, np.where(f < 1.0, f, 1.0), 0.0)
                if j == 0:
                    t = np.where(f < 0.0, f, t)                                    # the path begins with a ray
            ox, oy = t * ex, t * ey
            cx, cy = ax + ox, ay + oy
            dx, dy = q[:, 0] - cx, q[:, 1] - cy
            dxx, dyy = dx * dx, dy * dy
            dd = np.sqrt(dxx + dyy)
            d = np.where(np.isnan(dd), INF, dd)
            take = (d < bd) if j else np.ones(n, dtype=bool)
            along = t * self.len[j]
            bs = np.where(take, self.cum[j] + along, bs)
            bd = np.where(take, d, bd)
            bj = np.where(take, j, bj)
            bc = np.where(take[:, None], np.stack([cx, cy], axis=1), bc)
        return bs, bd, bj, bc


def _scene(c, win, vel, boxes, discs, planes, H, D, defect):
    xs, wdt = F(c["xy_scale"]), F(c["waypoint_dt"])
    p = Path(win, xs)
    vin = F(np.float32(vel))
    v0 = vin if vin > 0.0 else F(0.0)
    s_e, d_e, j_e, c_e = (a[0] for a in p.project(np.zeros((1, 2))))
    j_e = int(j_e)
    dec = dict(corridor=[], ahead=[], plane=[], curve=[], leader=INF)
    cands = []                                                                     # (r, u, code) in the contract's order

    def slots(rec, code0, is_box):
        rec = np.asarray(rec, dtype=np.float32)
        size_ok = (rec[:, 6] > 0) & (rec[:, 7] > 0) if is_box else rec[:, 4] > 0
        r64 = rec.astype(F)
        ctr = r64[:, 0:2] * xs
        vel_ = (r64[:, 2:4] * xs) / wdt
        s, d, j, _ = p.project(ctr)
        tau = p.tau[j]
        if is_box:
            hl, hw = (r64[:, 6] * xs) / 2.0, (r64[:, 7] * xs) / 2.0
            d0, d1 = r64[:, 4] * tau[:, 0], r64[:, 5] * tau[:, 1]
            c0, c1 = r64[:, 4] * tau[:, 1], r64[:, 5] * tau[:, 0]
            dt_, cr = np.abs(d0 + d1), np.abs(c0 - c1)
            if defect == "swap_extents":
                dt_, cr = cr, dt_
            l0, l1 = hl * dt_, hw * cr
            lon = l0 + l1
            w0, w1 = hl * cr, hw * dt_
            lat = w0 + w1
        else:
            lon = lat = r64[:, 4] * xs
        ahead = s - s_e
        lim = F(c["corridor_half"]) + lat
        u0, u1 = vel_[:, 0] * tau[:, 0], vel_[:, 1] * tau[:, 1]
        us = u0 + u1
        u = np.where(us > 0.0, us, 0.0)
        r = (ahead - lon) - F(c["ego_front"])
        for i in np.nonzero(size_ok)[0]:
            dec["corridor"].append(abs(d[i] - lim[i]))
            dec["ahead"].append(abs(ahead[i]))
            if d[i] <= lim[i] and ahead[i] > 0.0:
                cands.append((r[i], u[i], code0 + int(i)))

    with np.errstate(all="ignore"):
        if boxes is not None and len(boxes):
            slots(boxes, 0, True)
        if discs is not None and len(discs):
            slots(discs, DISC, False)
        for k, pl in enumerate(() if planes is None else np.asarray(planes, dtype=np.float32)):
            nx, ny = F(pl[0]), F(pl[1])
            bm = F(pl[2]) * xs
            beyond = -bm
            if nx == 0.0 and ny == 0.0:
                continue
            dec["plane"].append(abs(bm))
            if beyond > 0.0:
                continue
            ax, ay, arc_a = c_e[0], c_e[1], s_e
            g0, g1 = nx * ax, ny * ay
            ga = (g0 + g1) - bm
            dec["plane"].append(abs(ga))
            arc = None
            for j in range(j_e, p.R - 1):
                bx, by, arc_b = p.P[j + 1, 0], p.P[j + 1, 1], p.cum[j + 1]
                h0, h1 = nx * bx, ny * by
                gb = (h0 + h1) - bm
                dec["plane"].append(abs(gb))
                cross = (ga >= 0.0 and gb < 0.0) if defect == "plane_side" else (ga <= 0.0 and gb > 0.0)
                if arc is None and cross:
                    fr = ga / (ga - gb)
                    span = arc_b - arc_a
                    part = fr * span
                    arc = arc_a + part
                ax, ay, arc_a, ga = bx, by, arc_b, gb
            if arc is not None:
                cands.append(((arc - s_e) - F(c["ego_front"]), F(0.0), PLANE + k))
        if p.ends:
            cands.append((((p.cum[-1] - s_e) - F(c["ego_front"])) - F(c["end_margin"]), F(0.0), END))
        best_r, best_u, code = INF, F(0.0), -1
        for r, u, cd in cands:
            better = (r > best_r or code < 0) and r < INF if defect == "largest_r" else r < best_r
            if better:
                best_r, best_u, code = F(r), F(u), cd
        rs = sorted(float(r) for r, _, _ in cands if r < INF)
        if len(rs) >= 2:
            dec["leader"] = rs[1] - rs[0]

        # ---- the curve limit ----
        lt = v0 * F(c["look_time"])
        look = F(c["look_min"]) + lt
        lim = INF
        for i in range(1, p.R - 1):
            if not (p.good[i - 1] and p.good[i]):
                continue
            ah = p.cum[i] - s_e
            dec["curve"].append(min(abs(ah), abs(ah - look)))
            in_range = (ah <= look) if defect == "curve_behind" else (ah >= 0.0 and ah <= look)
            if not in_range:
                continue
            chx, chy = p.P[i + 1, 0] - p.P[i - 1, 0], p.P[i + 1, 1] - p.P[i - 1, 1]
            cxx, cyy = chx * chx, chy * chy
            lc = np.sqrt(cxx + cyy)
            x0, x1 = p.e[i - 1, 0] * p.e[i, 1], p.e[i - 1, 1] * p.e[i, 0]
            x = abs(x0 - x1)
            num = F(2.0) * x
            ll = p.len[i - 1] * p.len[i]
            den = ll * lc
            kappa = num / den
            if kappa > 0.0:
                q = F(c["lat_accel"]) / kappa
                cand = np.sqrt(q)
                if cand < lim:
                    lim = cand
        desired = lim if lim < F(c["desired_v"]) else F(c["desired_v"])

        # ---- the law, rolled out ----
        accel, brake, bmax = F(c["accel"]), F(c["brake"]), F(c["brake_max"])
        ab = accel * brake
        den2 = F(2.0) * np.sqrt(ab)
        v, arc, arcs, acc0 = v0, F(0.0), [], F(0.0)
        for k in range(H):
            arcs.append(arc)
            f = v / desired
            f2 = f * f
            f4 = f2 * f2
            free = F(1.0) - f4
            inter = F(0.0)
            if code >= 0:
                tk = F(k) * wdt
                mv = F(0.0) if defect == "frozen_leader" else best_u * tk
                rk = best_r + mv
                gap = rk - arc
                t0 = v * F(c["headway"])
                dv = v - best_u
                t1 = v * dv
                t2 = t1 / den2
                dyn = t0 + t2
                star = F(c["jam"]) + (dyn if dyn > 0.0 else F(0.0))
                g = gap if gap > F(c["gap_min"]) else F(c["gap_min"])
                ratio = star / g
                inter = ratio * ratio
            acc = accel * (free - inter)
            if acc < -bmax:
                acc = -bmax
            if acc > accel:
                acc = accel
            if k == 0:
                acc0 = acc
            dvv = acc * wdt
            v1 = v + dvv
            v = v1 if v1 > 0.0 else F(0.0)
            ds = v * wdt
            arc = arc + ds

        # ---- the rows ----
        plan = np.zeros((H, D), dtype=np.float32)
        goods = np.nonzero(p.good)[0]
        for k in range(H):
            A = s_e + arcs[k]
            sel = -1
            for j in goods:
                if p.cum[j] <= A:
                    sel = int(j)
            if sel < 0 and len(goods):
                sel = int(goods[0])
            x, y = p.P[0, 0], p.P[0, 1]
            if sel >= 0:
                al = A - p.cum[sel]
                ox, oy = al * p.tau[sel, 0], al * p.tau[sel, 1]
                x, y = p.P[sel, 0] + ox, p.P[sel, 1] + oy
            plan[k, 0], plan[k, 1] = word32(x / xs), word32(y / xs)
        info = word32(np.array([s_e, d_e, desired, best_r, best_u, acc0, v, arc], dtype=F))
    flat = dec["corridor"] + dec["ahead"] + dec["plane"] + dec["curve"] + [dec["leader"]]
    finite = [float(x) for x in flat if np.isfinite(x)]
    return plan, code, info, (min(finite) if finite else float("inf")), dec


def expert_plan(cfg, window, velocity, boxes=None, discs=None, planes=None, *, horizon, dim, defect=None):
    """`cfg`: the contract's fp64 parameters (CFG_DEFAULT's keys).  window [S, R, 2], velocity [S], boxes [S, N, 8] or None,
    discs [S, M, 5] or None, planes [S, K, 3] or None: fp32 host arrays.  Returns dict(plan [S, H, D] fp32, leader [S] int32,
    info [S, 8] fp32, clearance [S] fp64, decisions [S] dicts)."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(defect)
    window = np.asarray(window, dtype=np.float32)
    S = window.shape[0]
    velocity = np.asarray(velocity, dtype=np.float32).reshape(S)
    plan = np.zeros((S, horizon, dim), dtype=np.float32)
    leader = np.zeros((S,), dtype=np.int32)
    info = np.zeros((S, 8), dtype=np.float32)
    clearance, decisions = np.zeros((S,), dtype=F), []
    for s in range(S):
        plan[s], leader[s], info[s], clearance[s], dec = _scene(cfg, window[s], velocity[s], None if boxes is None else boxes[s],
                                                                None if discs is None else discs[s],
                                                                None if planes is None else planes[s], horizon, dim, defect)
        decisions.append(dec)
    return dict(plan=plan, leader=leader, info=info, clearance=clearance, decisions=decisions)


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint8) == b.view(np.uint8)).all())


# ---- worlds for the tests: ego-frame inputs in model units -------------------------------------------------------------------
def straight_window(R, spacing=2.0, xy_scale=20.0, back=1, pad=0, lateral=0.0):
    """A straight path along +y (the ego frame's forward), `spacing` m apart, starting `back` points behind the ego; the last
    `pad` points repeat the one before them (a window at the end of a route).  fp32 [1, R, 2] model units."""
    ys = (np.arange(R) - back) * spacing
    if pad:
        ys[R - pad:] = ys[R - pad - 1]
    w = np.zeros((1, R, 2), dtype=np.float32)
    w[0, :, 0] = lateral / xy_scale
    w[0, :, 1] = ys / xy_scale
    return w


def box(s_m, d_m=0.0, speed=0.0, length=4.5, width=2.0, heading=(0.0, 1.0), xy_scale=20.0, dt=0.5):
    """A box on the straight window's frame: `s_m` m ahead of the ego along +y, `d_m` m to its right, moving along +y."""
    return np.array([d_m / xy_scale, s_m / xy_scale, 0.0, speed * dt / xy_scale, heading[0], heading[1], length / xy_scale,
                     width / xy_scale], dtype=np.float32)


def disc(s_m, d_m=0.0, speed=0.0, radius=1.0, xy_scale=20.0, dt=0.5):
    return np.array([d_m / xy_scale, s_m / xy_scale, 0.0, speed * dt / xy_scale, radius / xy_scale], dtype=np.float32)


def random_world(rng, S, R, N, M, K, cfg=CFG_DEFAULT, min_clearance=1e-9, max_draws=50):
    """Random ego-frame worlds whose every decision is at least `min_clearance` from its threshold: a scene below it is REDRAWN
    (never dropped).  Returns (window, velocity, boxes, discs, planes, draws): `draws` counts the redraws, so a test can check
    that the loop terminates early."""
    xs = cfg["xy_scale"]
    out = [np.zeros((S, R, 2), np.float32), np.zeros((S,), np.float32), np.zeros((S, N, 8), np.float32) if N else None,
           np.zeros((S, M, 5), np.float32) if M else None, np.zeros((S, K, 3), np.float32) if K else None]
    draws = 0
    for s in range(S):
        for attempt in range(max_draws):
            # a gently winding path from a little behind the ego, sometimes padded at its end
            step = rng.uniform(1.0, 4.0, size=R)
            turn = np.cumsum(rng.normal(0.0, 0.12, size=R)) + rng.normal(0.0, 0.1)
            pts = np.zeros((R, 2))
            pts[0] = (rng.normal(0.0, 0.8), -rng.uniform(0.5, 3.0))
            for i in range(1, R):
                pts[i] = pts[i - 1] + step[i] * np.array([np.sin(turn[i]), np.cos(turn[i])])
            pad = int(rng.integers(0, max(R - 2, 0) + 1)) if rng.random() < 0.4 else 0
            if pad:
                pts[R - pad:] = pts[R - pad - 1]
            win = (pts / xs).astype(np.float32)[None]
            vel = np.array([rng.uniform(0.0, 10.0) if rng.random() < 0.9 else 0.0], dtype=np.float32)
            bx = dc = pl = None
            if N:
                bx = np.zeros((1, N, 8), np.float32)
                for i in range(N):
                    at = pts[rng.integers(0, R)] + rng.normal(0.0, 2.5, size=2)
                    yaw = rng.uniform(-np.pi, np.pi)
                    v = rng.uniform(0.0, 8.0) * cfg["waypoint_dt"] / xs
                    kind = rng.random()
                    size = (rng.uniform(2.0, 6.0), rng.uniform(1.0, 2.5))
                    if kind < 0.15:
                        size = [(0.0, 2.0), (4.0, 0.0), (-1.0, 2.0), (np.nan, 2.0)][int(rng.integers(0, 4))]      # every kind of empty slot
                    bx[0, i] = (at[0] / xs, at[1] / xs, v * np.cos(yaw), v * np.sin(yaw), np.cos(yaw), np.sin(yaw), size[0] / xs, size[1] / xs)
            if M:
                dc = np.zeros((1, M, 5), np.float32)
                for i in range(M):
                    at = pts[rng.integers(0, R)] + rng.normal(0.0, 2.5, size=2)
                    yaw = rng.uniform(-np.pi, np.pi)
                    v = rng.uniform(0.0, 3.0) * cfg["waypoint_dt"] / xs
                    rad = rng.uniform(0.3, 1.5) if rng.random() > 0.15 else [0.0, -1.0, np.nan][int(rng.integers(0, 3))]
                    dc[0, i] = (at[0] / xs, at[1] / xs, v * np.cos(yaw), v * np.sin(yaw), rad / xs)
            if K:
                pl = np.zeros((1, K, 3), np.float32)
                for k in range(K):
                    if rng.random() < 0.4:
                        pl[0, k] = (0.0, 0.0, 1.0)                                 # the inert plane
                        continue
                    i = int(rng.integers(0, R - 1))
                    n = pts[i + 1] - pts[i]
                    n = n / np.linalg.norm(n) if np.linalg.norm(n) > 0 else np.array([0.0, 1.0])
                    at = pts[i] + rng.uniform(0.0, 1.0) * (pts[i + 1] - pts[i])
                    pl[0, k] = (n[0], n[1], (n @ at) / xs)
            ref = expert_plan(cfg, win, vel, bx, dc, pl, horizon=2, dim=2)
            if ref["clearance"][0] >= min_clearance:
                break
            draws += 1
        else:
            raise RuntimeError(f"random_world: scene {s} stayed within {min_clearance} of a threshold for {max_draws} draws")
        out[0][s], out[1][s] = win[0], vel[0]
        for dst, src in ((out[2], bx), (out[3], dc), (out[4], pl)):
            if dst is not None:
                dst[s] = src[0]
    return (*out, draws)
