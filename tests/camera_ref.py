"""The restatement of "camera v1" (include/adx.h) in NumPy, following the contract's operation order.

`stage(...)`   float64: the primitive table a render reads, each word rounded to float32 once, and per word the bound by which a
               device table may differ.  The bound follows ego frame v1's argument (tests/nav_ref.py derives its 8): the device's
               cos and sin are within 4 ulp of NumPy's, so a rotated vector differs by at most D(v) = 8 * 2^-52 * (|dx| + |dy|) per
               component; a word that is a rotated coordinate differs by one float32 ulp (the rounding may fall the other way) plus
               D; a word that is a product of such coordinates carries D through the product rule, plus the float64 roundings of
               its own terms (4 * 2^-52 of their magnitudes, generously).  A word with no cos or sin on its way (a height, r * r)
               is the same number: bound 0.  The pixel rectangles (words 1..4 of an object) are not part of the comparison: they
               may be any rectangle that loses no pixel, which the render test decides.
`render(...)`  float32 (or, for the CPU tests, float64 on the same float32 table): ids, depth, frames, and `near_threshold`, true
               where any comparison the pixel's verdict passed through had its two sides within 8 float32 ulps of the larger
               magnitude: hit or miss, t > near, nearest-of, far, road or marking, stop line, cap or side, the entered face.
               The plain loop over all primitives: the rectangles are not read.
`bias`         +1 decides every such near comparison as true, -1 as false: the ids of the three runs are the candidates on either
               side of a flagged comparison.
`defect`       plants one deliberate mistake; tests/test_camera_cpu.py shows that the closed-form scenes catch each.
"""
import math
from dataclasses import dataclass, field

import numpy as np

HDR, OBJ, GND = 16, 16, 8
SKY, GROUND, ROAD, MARK, LINE, BOX, DISC, LAMP, POLE = range(9)
EPS = 2.0 ** -52
HALF_PI = 1.57079632679489661923
DEFECTS = ("mirror", "nearest", "noclamp", "faces", "lamp_near")
PALETTE = ((135, 190, 235), (96, 128, 72), (120, 140, 110), (70, 70, 74), (230, 230, 225), (250, 250, 250),
           (200, 40, 40), (40, 80, 200), (230, 200, 40), (240, 240, 240), (30, 30, 30), (40, 160, 80), (150, 90, 170),
           (230, 130, 40), (150, 110, 70), (60, 60, 60), (30, 220, 60), (250, 210, 30), (240, 30, 30), (250, 120, 20))
SHADE = (200, 232, 168, 184, 255)


@dataclass
class Cfg:
    width: int = 900
    height: int = 256
    fov: float = math.radians(100.0)
    mount_back: float = -1.5
    cam_height: float = 2.0
    near: float = 0.1
    far: float = 150.0
    half_width: float = 1.75
    mark: float = 0.15
    line_half: float = 0.2
    box_height: float = 1.6
    disc_height: float = 1.8
    lamp_radius: float = 0.35
    lamp_height: float = 4.0
    lamp_setback: float = 12.0
    pole_radius: float = 0.1
    n_boxes: int = 0
    n_discs: int = 0
    n_signals: int = 0
    n_paths: int = 0
    n_points: int = 0
    palette: tuple = PALETTE
    shade: tuple = SHADE
    mean: tuple = (0.485, 0.456, 0.406)
    std: tuple = (0.229, 0.224, 0.225)
    extra: dict = field(default_factory=dict)

    @property
    def k(self):
        return np.float32(2.0 * math.tan(self.fov / 2.0) / float(self.width))

    @property
    def n_obj(self):
        return self.n_boxes + self.n_discs + 2 * self.n_signals

    @property
    def n_gnd(self):
        return self.n_signals + self.n_paths * max(self.n_points - 1, 0)

    @property
    def scene_words(self):
        return HDR + OBJ * self.n_obj + GND * self.n_gnd


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def _rot(c, s, dx, dy):
    a0, a1 = c * dx, s * dy
    r0 = a0 + a1
    b0, b1 = s * dx, c * dy
    r1 = -b0 + b1
    return r1, -r0, 8.0 * EPS * (np.abs(dx) + np.abs(dy))


def stage(cfg: Cfg, pose, boxes=None, discs=None, signals=None, phase=None, roads=None, road_len=None, defect=None):
    """(table float32 [S, scene_words], bound float64 [S, scene_words]); bound is +inf on the rectangle words of a live object."""
    pose = np.asarray(pose, dtype=np.float64)
    S = pose.shape[0]
    tab = np.zeros((S, cfg.scene_words), dtype=np.float32)
    bnd = np.zeros((S, cfg.scene_words), dtype=np.float64)
    itab = tab.view(np.int32)
    itab[:, 0], itab[:, 1], itab[:, 2] = 1, cfg.n_obj, cfg.n_gnd
    comp = np.where(np.isnan(pose[:, 2]), 0.0, pose[:, 2])
    th = comp + HALF_PI
    c, s = np.cos(th)[:, None], np.sin(th)[:, None]
    px, py = pose[:, 0:1], pose[:, 1:2]
    zg = -cfg.cam_height

    def point(X, Y):
        x, y, d = _rot(c, s, X - px, Y - py)
        return x, y - cfg.mount_back, d + 2.0 * EPS * (np.abs(y) + abs(cfg.mount_back))

    def put(base, words, live, vals, bounds, key=None):
        """vals / bounds: lists of [S, N] arrays for consecutive words from `first`."""
        for (w, v, b) in zip(words, vals, bounds):
            col = base + w
            v32 = np.asarray(v, dtype=np.float64).astype(np.float32)
            tab[:, col] = np.where(live, v32, np.float32(0))
            bnd[:, col] = np.where(live, b, 0.0)
        if key is not None:
            itab[:, base] = np.where(live, key, 0)
            for w in (1, 2, 3, 4):      # the rectangle: the whole image here, anything safe on the device
                itab[:, base + w] = np.where(live, -1 if w % 2 else 1 << 20, 0)
                bnd[:, base + w] = np.where(live, np.inf, 0.0)

    def cylinder(base, key, cx, cy, dpos, r, zlo, zhi):
        c0, c1 = cx * cx, cy * cy
        r2 = r * r
        cc = (c0 + c1) - r2
        inside = (cc <= 0.0) & (zlo <= 0.0) & (zhi >= 0.0)
        live = (r > 0.0) & (zhi > zlo) & ~inside & ~np.isnan(cc)
        zero = np.zeros_like(cc)
        put(base, (5, 6, 7, 8, 9), live, (cx, cy, r2 + zero, zlo + zero, zhi + zero),
            (_ulp32(cx) + dpos, _ulp32(cy) + dpos, zero, zero, zero), key)

    with np.errstate(all="ignore"):
        o = HDR
        if cfg.n_boxes:
            g = np.asarray(boxes, dtype=np.float64)
            hl, hw = g[..., 5] / 2.0, g[..., 6] / 2.0
            bx, by, db = point(g[..., 0], g[..., 1])
            ax, ay, da = _rot(c, s, np.cos(g[..., 4]), np.sin(g[..., 4]))
            da = da + 8.0 * EPS      # the two library calls of the yaw, each within 4 ulp of a value <= 1
            m0, m1 = bx * ax, by * ay
            el = -(m0 + m1)
            m2, m3 = bx * ay, by * ax
            ew = m2 - m3
            zhi = zg + cfg.box_height
            inside = (el >= -hl) & (el <= hl) & (ew >= -hw) & (ew <= hw) & (zg <= 0.0) & (zhi >= 0.0)
            live = (hl > 0.0) & (hw > 0.0) & ~inside & ~np.isnan(el) & ~np.isnan(ew)
            de = (np.abs(bx) + np.abs(by)) * da + (np.abs(ax) + np.abs(ay)) * db + 4.0 * EPS * (np.abs(m0) + np.abs(m1) + np.abs(m2) + np.abs(m3))
            zero = np.zeros_like(el)
            for j in range(cfg.n_boxes):
                sl = (slice(None), j)
                vals = (ax[sl], ay[sl], (-hl - el)[sl], (hl - el)[sl], (-hw - ew)[sl], (hw - ew)[sl], zero[sl] + zg, zero[sl] + zhi)
                dd = de[sl] + 2.0 * EPS * (np.abs(hl[sl]) + np.abs(el[sl]) + np.abs(hw[sl]) + np.abs(ew[sl]))
                bounds = (_ulp32(vals[0]) + da[sl], _ulp32(vals[1]) + da[sl]) + tuple(_ulp32(v) + dd for v in vals[2:6]) + (zero[sl], zero[sl])
                put(o + OBJ * j, range(5, 13), live[sl], vals, bounds, BOX << 8 | j)
        o += OBJ * cfg.n_boxes
        if cfg.n_discs:
            g = np.asarray(discs, dtype=np.float64)
            cx, cy, dpos = point(g[..., 0], g[..., 1])
            for j in range(cfg.n_discs):
                cylinder(o + OBJ * j, DISC << 8 | j, cx[:, j], cy[:, j], dpos[:, j], g[:, j, 4], zg, zg + cfg.disc_height)
        o += OBJ * cfg.n_discs
        gbase = HDR + OBJ * cfg.n_obj
        if cfg.n_signals:
            g = np.asarray(signals, dtype=np.float64)
            ph = np.asarray(phase, dtype=np.int64)
            ddx, ddy = g[..., 2] - g[..., 0], g[..., 3] - g[..., 1]
            L = np.sqrt(ddx * ddx + ddy * ddy)
            sig = (ph >= 1) & (ph <= 4) & (L > 0.0)
            tx, ty = ddx / L, ddy / L
            nx, ny = -ty, tx
            mx, my = g[..., 0] + 0.5 * ddx, g[..., 1] + 0.5 * ddy
            setback = -cfg.lamp_setback if defect == "lamp_near" else cfg.lamp_setback
            wx, wy = mx + setback * nx, my + setback * ny
            lx, ly, dl = point(wx, wy)
            lz, R = zg + cfg.lamp_height, cfg.lamp_radius
            q0, q1, q2 = lx * lx, ly * ly, lz * lz
            cc = ((q0 + q1) + q2) - R * R
            zero = np.zeros_like(cc)
            pax, pay, dpa = point(g[..., 0], g[..., 1])
            pbx, pby, dpb = point(g[..., 2], g[..., 3])
            for j in range(cfg.n_signals):
                sl = (slice(None), j)
                base = o + OBJ * j
                live = sig[sl] & (cc[sl] > 0.0)
                put(base, (5, 6, 7, 8), live, (lx[sl], ly[sl], zero[sl] + lz, zero[sl] + R * R),
                    (_ulp32(lx[sl]) + dl[sl], _ulp32(ly[sl]) + dl[sl], zero[sl], zero[sl]), LAMP << 8 | j)
                itab[:, base + 9] = np.where(live, ph[sl], 0)
                pole = o + OBJ * (cfg.n_signals + j)
                cylinder(pole, POLE << 8 | j, lx[sl], ly[sl], dl[sl], zero[sl] + cfg.pole_radius, zg, lz)
                dead = ~sig[sl]
                tab[dead, pole:pole + OBJ] = 0
                bnd[dead, pole:pole + OBJ] = 0
                _segment(tab, bnd, itab, gbase + GND * j, sig[sl], pax[sl], pay[sl], pbx[sl], pby[sl], dpa[sl], dpb[sl])
        if cfg.n_paths:
            r = np.asarray(roads, dtype=np.float64)
            n = np.clip(np.asarray(road_len, dtype=np.int64), 0, cfg.n_points)
            for q in range(cfg.n_paths):
                x, y, d = point(r[:, q, :, 0], r[:, q, :, 1])
                for g0 in range(cfg.n_points - 1):
                    base = gbase + GND * (cfg.n_signals + q * (cfg.n_points - 1) + g0)
                    _segment(tab, bnd, itab, base, g0 + 1 < n[:, q], x[:, g0], y[:, g0], x[:, g0 + 1], y[:, g0 + 1], d[:, g0], d[:, g0 + 1])
    return tab, bnd


def _segment(tab, bnd, itab, base, exists, ax, ay, bx, by, da, db):
    ex, ey = bx - ax, by - ay
    e0, e1 = ex * ex, ey * ey
    e2 = e0 + e1
    inv = np.where(e2 > 0.0, 1.0 / np.where(e2 > 0.0, e2, 1.0), 0.0)
    de = da + db + 2.0 * EPS * (np.abs(ax) + np.abs(ay) + np.abs(bx) + np.abs(by))
    de2 = 2.0 * (np.abs(ex) + np.abs(ey)) * de + 4.0 * EPS * e2
    dinv = np.where(e2 > 0.0, 2.0 * de2 * inv * inv, 0.0)
    for w, v, b in ((0, ax, _ulp32(ax) + da), (1, ay, _ulp32(ay) + da), (2, ex, _ulp32(ex) + de), (3, ey, _ulp32(ey) + de),
                    (4, inv, _ulp32(inv) + dinv)):
        tab[:, base + w] = np.where(exists, np.asarray(v, dtype=np.float64).astype(np.float32), np.float32(0))
        bnd[:, base + w] = np.where(exists, b, 0.0)
    itab[:, base + 5] = np.where(exists & ~np.isnan(e2), 1, 0)


class _Cmp:
    """Every comparison a verdict passes through: counts the near ones, and decides them as `bias` says."""

    def __init__(self, shape, bias):
        self.flag = np.zeros(shape, dtype=bool)
        self.bias = bias

    @staticmethod
    def close(a, b):
        a32, b32 = np.asarray(a).astype(np.float32), np.asarray(b).astype(np.float32)
        m = np.maximum(np.abs(a32), np.abs(b32))
        return np.abs(a32 - b32) <= np.float32(8) * np.spacing(m)

    def _decide(self, r, a, b, where):
        near = self.close(a, b) & where
        self.flag |= near
        return (r | near) if self.bias > 0 else ((r & ~near) if self.bias < 0 else r)

    def lt(self, a, b, where):
        return self._decide(a < b, a, b, where)

    def le(self, a, b, where):
        return self._decide(a <= b, a, b, where)


def render(prims, cfg: Cfg, dtype=np.float32, bias=0, defect=None):
    """dict(ids int32 [S, H, W], depth dtype [S, H, W], frames uint8 [S, H, W, 3], near_threshold bool [S, H, W]) of the float32
    table `prims` [S, scene_words]: the plain loop over every primitive."""
    prims = np.ascontiguousarray(prims, dtype=np.float32)
    S, W, H = prims.shape[0], cfg.width, cfg.height
    T = dtype
    ip = prims.view(np.int32)
    fp = prims.astype(T)
    k = T(cfg.k)
    u = np.arange(W, dtype=np.float32)
    v = np.arange(H, dtype=np.float32)
    dxr = (((u + np.float32(0.5)) - np.float32(W) * np.float32(0.5)).astype(T) * k)
    dzr = -(((v + np.float32(0.5)) - np.float32(H) * np.float32(0.5)).astype(T) * k)
    if defect == "mirror":
        dxr = -dxr
    dx = np.broadcast_to(dxr[None, :], (H, W)).reshape(1, H * W)
    dz = np.broadcast_to(dzr[:, None], (H, W)).reshape(1, H * W)
    A2 = dx * dx + T(1)
    A3 = A2 + dz * dz
    near, far, hgt = T(np.float32(cfg.near)), T(np.float32(cfg.far)), T(np.float32(cfg.cam_height))
    r_in2 = T(np.float32((cfg.half_width - cfg.mark) * (cfg.half_width - cfg.mark)))
    r_out2 = T(np.float32(cfg.half_width * cfg.half_width))
    line2 = T(np.float32(cfg.line_half * cfg.line_half))
    inf = T(np.inf)
    shape = (S, H * W)
    cmp = _Cmp(shape, bias)
    one = np.ones(shape, dtype=bool)

    with np.errstate(all="ignore"):
        # ---- the ground as the first candidate ----
        down = np.broadcast_to(dz < 0, shape)
        tg = np.broadcast_to(hgt / (-dz), shape)
        gvalid = down & cmp.lt(near, tg, down)
        best_t = np.where(gvalid, tg, inf).astype(T)
        best_id = np.where(gvalid, GROUND << 8, 0).astype(np.int32)
        best_aux = np.zeros(shape, dtype=np.int32)

        def consider(t, ident, aux, hit):
            nonlocal best_t, best_id, best_aux
            valid = hit & cmp.lt(near, t, hit)
            if defect == "nearest":
                better = t > best_t
            else:
                better = cmp.lt(t, best_t, valid) | ((t == best_t) & ((ident & 0xffff) < (best_id & 0xffff)))
            upd = valid & better
            best_t = np.where(upd, t, best_t).astype(T)
            best_id = np.where(upd, ident, best_id).astype(np.int32)
            best_aux = np.where(upd, aux, best_aux).astype(np.int32)

        def cyl(rec, key, live):
            cx, cy, r2, zlo, zhi = (rec[:, w:w + 1] for w in range(5, 10))
            B = dx * cx + cy
            cr = dx * cy - cx
            q = A2 * r2
            bb = cr * cr
            disc = q - bb
            pos = cmp.le(bb, q, live)      # disc >= 0: a difference is >= 0 exactly when its first term is >= its second
            sq = np.sqrt(np.where(pos, disc, T(0)))
            ts = (B - sq) / A2
            zs = ts * dz
            side = live & pos
            side = side & cmp.le(zlo, zs, side)
            side = side & cmp.le(zs, zhi, side)
            consider(ts, key, 0, side)
            capd = live & (dz < 0)
            tc = zhi / dz
            x, y = dx * tc - cx, tc - cy
            cap = capd & cmp.le(x * x + y * y, r2, capd)
            consider(tc, key, 0, cap)

        o = HDR
        for i in range(cfg.n_obj):
            rec = fp[:, o + OBJ * i: o + OBJ * (i + 1)]
            key = ip[:, o + OBJ * i][:, None]
            live = np.broadcast_to(key != 0, shape)
            if not live.any():
                continue
            if i < cfg.n_boxes:
                ax, ay = rec[:, 5:6], rec[:, 6:7]
                p = dx * ay
                dl, dw = dx * ax + ay, ax - p
                tn = np.full(shape, -inf, dtype=T)
                tf = np.full(shape, inf, dtype=T)
                face = np.zeros(shape, dtype=np.int32)
                ok = live.copy()
                for axis, d, n0, n1 in ((0, dl, rec[:, 7:8], rec[:, 8:9]), (1, dw, rec[:, 9:10], rec[:, 10:11]),
                                        (2, dz, rec[:, 11:12], rec[:, 12:13])):
                    d = np.broadcast_to(d, shape)
                    zero = d == 0
                    ok &= ~zero | ((n0 <= 0) & (n1 >= 0))
                    t1, t2 = n0 / d, n1 / d
                    up = d > 0
                    lo, hi = np.where(up, t1, t2), np.where(up, t2, t1)
                    fa = axis if defect != "faces" else (1, 0, 2)[axis]
                    f = np.where(up, 2 * fa, 2 * fa + 1) if axis < 2 else 4
                    upd = cmp.lt(tn, lo, ok & ~zero & (tn > -inf)) & ~zero
                    tn = np.where(upd, lo, tn).astype(T)
                    face = np.where(upd, f, face).astype(np.int32)
                    tf = np.where(~zero & (hi < tf), hi, tf).astype(T)
                hit = ok & cmp.le(tn, tf, ok)
                consider(tn, face << 16 | key, 0, hit)
            elif cfg.n_boxes + cfg.n_discs <= i < cfg.n_boxes + cfg.n_discs + cfg.n_signals:
                lx, ly, lz, R2 = (rec[:, w:w + 1] for w in range(5, 9))
                B = (dx * lx + ly) + dz * lz
                c0, c1, c2 = ly * dz - lz, lz * dx - lx * dz, lx - ly * dx
                bb = (c0 * c0 + c1 * c1) + c2 * c2
                q = A3 * R2
                disc = q - bb
                pos = live & cmp.le(bb, q, live)
                sq = np.sqrt(np.where(pos, disc, T(0)))
                consider((B - sq) / A3, key, ip[:, o + OBJ * i + 9][:, None], pos)
            else:
                cyl(rec, key, live)

        # ---- the ground's class, where the ground won ----
        gwin = best_id == GROUND << 8
        gcmp = _Cmp(shape, bias)
        gx, gy = dx * best_t, best_t

        def seg_d2(rec):
            ax, ay, ex, ey, inv = (rec[:, w:w + 1] for w in range(5))
            qx, qy = gx - ax, gy - ay
            dot = qx * ex + qy * ey
            uu = dot * inv
            if defect != "noclamp":
                uu = np.where(uu < 0, T(0), np.where(uu > 1, T(1), uu))
            cx, cy = qx - uu * ex, qy - uu * ey
            return cx * cx + cy * cy

        g0 = HDR + OBJ * cfg.n_obj
        is_far = gwin & gcmp.lt(far, best_t, gwin)
        todo = gwin & ~is_far
        cls = np.zeros(shape, dtype=np.int32)
        slot = np.zeros(shape, dtype=np.int32)
        for j in range(cfg.n_signals):
            live = np.broadcast_to(ip[:, g0 + GND * j + 5][:, None] != 0, shape)
            if not live.any():
                continue
            w = todo & live & (cls == 0)
            on = w & gcmp.le(seg_d2(fp[:, g0 + GND * j: g0 + GND * (j + 1)]), line2, w)
            cls = np.where(on, LINE, cls)
            slot = np.where(on, j, slot)
        dmin = np.full(shape, inf, dtype=T)
        for j in range(cfg.n_signals, cfg.n_gnd):
            live = np.broadcast_to(ip[:, g0 + GND * j + 5][:, None] != 0, shape)
            if not live.any():
                continue
            d2 = seg_d2(fp[:, g0 + GND * j: g0 + GND * (j + 1)])
            dmin = np.where(live & (d2 < dmin), d2, dmin).astype(T)
        w = todo & (cls == 0)
        road = w & gcmp.lt(dmin, r_in2, w)
        mark = w & ~road
        mark = mark & gcmp.le(dmin, r_out2, mark)
        cls = np.where(road, ROAD, np.where(mark, MARK, np.where(w, GROUND, cls)))
        gid = np.where(is_far, GROUND << 8 | 1, cls << 8 | slot)
        ids = np.where(gwin, gid, best_id).astype(np.int32)
        flag = cmp.flag | (gcmp.flag & gwin)

    # ---- the colour ----
    c, sl, face = (ids >> 8) & 0xff, ids & 0xff, ids >> 16
    row = np.select([c == SKY, c == GROUND, c == ROAD, c == MARK, c == LINE, c == BOX, c == DISC, c == POLE],
                    [0, 1 + sl, 3, 4, 5, 6 + (sl & 7), 14, 15], default=16 + ((best_aux - 1) & 3))
    pal = np.asarray(cfg.palette, dtype=np.int32)[row]
    sh = np.where(c == BOX, np.asarray(cfg.shade, dtype=np.int32)[np.clip(face, 0, 4)], 256)
    frames = ((pal * sh[..., None]) >> 8).astype(np.uint8)
    return dict(ids=ids.reshape(S, H, W), depth=best_t.reshape(S, H, W), frames=frames.reshape(S, H, W, 3),
                near_threshold=flag.reshape(S, H, W), phase_of=best_aux.reshape(S, H, W))


def render64(prims, cfg: Cfg, **kw):
    """The float64 render of the same float32 table, for the CPU tests."""
    return render(prims, cfg, dtype=np.float64, **kw)


def candidates(prims, cfg: Cfg):
    """ids int32 [3, S, H, W]: the verdict, and the verdicts with every near comparison decided true and decided false."""
    return np.stack([render(prims, cfg, bias=b)["ids"] for b in (0, 1, -1)])


def normalize(frames, mean, std):
    """adx_image_normalize's arithmetic in float32: [S, H, W, 3] uint8 -> [S, 3, H, W]."""
    f = frames.astype(np.float32) / np.float32(255.0)
    out = (f - np.asarray(mean, dtype=np.float32)) / np.asarray(std, dtype=np.float32)
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))
