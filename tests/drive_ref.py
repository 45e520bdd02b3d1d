"""fp64 restatement of "drive metrics v1" (include/adx.h: adx_drive_step, adx_drive_reset), written from the contract's text one
scene at a time in plain Python doubles, the hand-built drives whose verdicts are known in closed form, and the bound of a
kernel's fp64 accumulators.

Decisions.  Every comparison of the contract is made on numbers that both sides form by the same single IEEE operations, except
the contact tests, which pass through sin / cos of the compass and of a box's yaw.  `step` records in `clear` the smallest relative
distance from equality of every THRESHOLD comparison it makes (xtrack against offroad_min and offroad_max, the off-route share,
the stall clock, the speed, completion, every contact test); `build_drives` asserts it stays above 1e-9 on every drive that is not
marked `integer`, so no rounding can flip a verdict.  The integer drives meet their thresholds and ties exactly, on numbers that
are exact in fp64.

The accumulators.  xtrack_sum, xtrack_sq, distance, offroad, progress and the comfort sums are sums of T terms.  A term is a
distance d = sqrt(a^2 + b^2) to a projected point q = a + t u, t = ((p - a) . u) / L2.  If a kernel's division and square root were
each off by up to 2 ulp where the host's are correctly rounded (they are not expected to be: both are IEEE operations), t would be
off by 2.5 e t, q by 2.5 e |t u| <= 2.5 e |u|, d by that plus 2.5 e d; with R the largest coordinate difference the drive meets
(segment lengths, distances, speeds and their quotients by dt included) every term and its square is off by at most 8 e R
resp. 16 e R^2, and a sum of T of them by T times that plus T roundings of the sum itself, e T R (resp. e T R^2):
    accumulator_bound(T, R) = 9 e T R      squares_bound(T, R) = 17 e T R^2            e = 2^-52.
"""
import math

import numpy as np

E52 = 2.0 ** -52
INF = float("inf")
INTS = ("cursor", "ticks", "done", "flags", "contact", "events", "contact_ticks", "first_tick", "first_slot", "have")
F64 = ("px", "py", "v_prev", "a_prev", "progress", "progress_max", "xtrack", "xtrack_max", "xtrack_sum", "xtrack_sq", "distance",
       "offroad", "stall", "acc_max", "acc_sq", "jerk_max", "jerk_sq", "lat_max", "lat_sq")
SUMS = ("xtrack_sum", "distance", "offroad", "progress", "progress_max", "xtrack", "xtrack_max", "stall", "acc_max", "jerk_max", "lat_max",
        "px", "py", "v_prev", "a_prev")
SQUARES = ("xtrack_sq", "acc_sq", "jerk_sq", "lat_sq")
CFG = dict(dt=0.5, window=32, r_ego=1.0, offsets=(0.0,), offroad_min=15.0, offroad_max=30.0, max_route_percentage=0.3,
           speed_threshold=0.1, max_time=90.0, completion_tol=1.0, stop_on_collision=False, max_ticks=0)


def accumulator_bound(T, R):
    return 9.0 * E52 * T * R


def squares_bound(T, R):
    return 17.0 * E52 * T * R * R


def norm2(x, y):
    xx, yy = x * x, y * y
    return math.sqrt(xx + yy)


def cumulative(route):
    """cum [G] of one scene's route [G, 2]: the sequential sum in index order."""
    cum = [0.0]
    for i in range(1, len(route)):
        cum.append(cum[-1] + norm2(float(route[i][0] - route[i - 1][0]), float(route[i][1] - route[i - 1][1])))
    return np.array(cum)


def fresh():
    rec = {k: 0 for k in INTS}
    rec.update({k: 0.0 for k in F64})
    return rec


class Clear:
    """The smallest relative distance of a threshold comparison from equality."""

    def __init__(self):
        self.value = INF

    def __call__(self, a, b):
        if math.isfinite(a) and math.isfinite(b):
            self.value = min(self.value, abs(a - b) / max(abs(a), abs(b), 1e-300))


def nearest(route, length, cursor, window, px, py):
    """(j, t, d, |segment j|) of the contract's `progress`."""
    if length == 1:
        return 0, 0.0, norm2(px - route[0][0], py - route[0][1]), 0.0
    cursor = min(max(cursor, 0), length - 2)
    last = min(cursor + window - 1, length - 2)
    best = None
    for j in range(cursor, last + 1):
        ax, ay = float(route[j][0]), float(route[j][1])
        ux, uy = float(route[j + 1][0]) - ax, float(route[j + 1][1]) - ay
        uxx, uyy = ux * ux, uy * uy
        L2 = uxx + uyy
        t = 0.0
        if L2 > 0.0:
            rx, ry = px - ax, py - ay
            m0, m1 = rx * ux, ry * uy
            q = (m0 + m1) / L2
            t = (q if q < 1.0 else 1.0) if q > 0.0 else 0.0
        tx, ty = t * ux, t * uy
        qx, qy = ax + tx, ay + ty
        d = norm2(px - qx, py - qy)
        if d != d:
            d = INF
        if best is None or d < best[2]:      # the lower j keeps a tie
            best = (j, t, d, math.sqrt(L2))
    return best


def contact(cfg, px, py, compass, discs, boxes, clear):
    """(hit, lowest hit slot): disc j is slot j, box j slot 64 + j."""
    fx, fy = math.sin(compass), -math.cos(compass)
    hits = []
    centres = []
    for off in cfg["offsets"]:
        ox, oy = off * fx, off * fy
        centres.append((px + ox, py + oy))
    for j, o in enumerate(() if discs is None else discs):
        r = float(o[4])
        if not r > 0.0:
            continue
        reach = r + cfg["r_ego"]
        for ex, ey in centres:
            d = norm2(ex - float(o[0]), ey - float(o[1]))
            clear(d, reach)
            if d < reach:
                hits.append(j)
    for j, o in enumerate(() if boxes is None else boxes):
        length, width = float(o[5]), float(o[6])
        if not (length > 0.0 and width > 0.0):
            continue
        ux, uy = math.cos(float(o[4])), math.sin(float(o[4]))
        hl, hw = length / 2.0, width / 2.0
        for cx, cy in centres:
            ex, ey = cx - float(o[0]), cy - float(o[1])
            l0, l1 = ex * ux, ey * uy
            lx = l0 + l1
            w0, w1 = ex * uy, ey * ux
            ly = -w0 + w1
            qx, qy = max(abs(lx) - hl, 0.0), max(abs(ly) - hw, 0.0)
            d = norm2(qx, qy)
            clear(d, cfg["r_ego"])
            if d < cfg["r_ego"]:
                hits.append(64 + j)
    return bool(hits), (min(hits) if hits else 0)


def step(rec, cfg, pose, velocity, yaw_rate, route, length, cum, discs=None, boxes=None, clear=None):
    """One scene's record after one launch (`rec` is not modified).  velocity and yaw_rate are fp32 values."""
    clear = clear or Clear()
    if rec["done"] != 0:
        return dict(rec)
    n = dict(rec)
    G = len(route)
    length = min(max(int(length), 1), G)
    px, py = float(pose[0]), float(pose[1])
    compass = 0.0 if pose[2] != pose[2] else float(pose[2])
    dt = cfg["dt"]
    j, t, d, seg = nearest(route, length, rec["cursor"], cfg["window"], px, py)
    total = float(cum[length - 1])
    n["cursor"] = j
    along = t * seg
    n["progress"] = 0.0 if length == 1 else float(cum[j]) + along
    n["progress_max"] = max(rec["progress_max"], n["progress"])
    n["xtrack"] = d
    n["xtrack_max"] = max(rec["xtrack_max"], d)
    n["xtrack_sum"] = rec["xtrack_sum"] + d
    n["xtrack_sq"] = rec["xtrack_sq"] + d * d
    moved = norm2(px - rec["px"], py - rec["py"]) if rec["ticks"] > 0 else 0.0
    n["distance"] = rec["distance"] + moved
    n["px"], n["py"] = px, py
    hit, slot = contact(cfg, px, py, compass, discs, boxes, clear)
    n["events"] = rec["events"] + int(hit and rec["contact"] == 0)
    n["contact_ticks"] = rec["contact_ticks"] + int(hit)
    n["contact"] = int(hit)
    n["ticks"] = rec["ticks"] + 1
    if hit and rec["first_tick"] == 0:
        n["first_tick"], n["first_slot"] = n["ticks"], slot
    clear(d, cfg["offroad_max"])
    clear(d, cfg["offroad_min"])
    off = d > cfg["offroad_max"]
    if d > cfg["offroad_min"]:
        n["offroad"] = rec["offroad"] + moved
        share = n["offroad"] / total if total > 0.0 else (INF if n["offroad"] > 0.0 else float("nan"))      # IEEE x / 0
        clear(share, cfg["max_route_percentage"])
        off = off or share > cfg["max_route_percentage"]
    v = float(np.float32(velocity))
    clear(v, cfg["speed_threshold"])
    n["stall"] = rec["stall"] + dt if v < cfg["speed_threshold"] else 0.0
    clear(n["stall"], cfg["max_time"])
    blocked = n["stall"] > cfg["max_time"]
    acc = 0.0
    if rec["have"] >= 1:
        acc = (v - rec["v_prev"]) / dt
        n["acc_max"] = max(rec["acc_max"], abs(acc))
        n["acc_sq"] = rec["acc_sq"] + acc * acc
        n["a_prev"] = acc
    if rec["have"] >= 2:
        jk = (acc - rec["a_prev"]) / dt
        n["jerk_max"] = max(rec["jerk_max"], abs(jk))
        n["jerk_sq"] = rec["jerk_sq"] + jk * jk
    lat = v * float(np.float32(yaw_rate))
    n["lat_max"] = max(rec["lat_max"], abs(lat))
    n["lat_sq"] = rec["lat_sq"] + lat * lat
    n["v_prev"] = v
    n["have"] = min(rec["have"] + 1, 2)
    clear(n["progress_max"], total - cfg["completion_tol"])
    cond = (n["progress_max"] >= total - cfg["completion_tol"], hit and bool(cfg["stop_on_collision"]), off, blocked,
            cfg["max_ticks"] > 0 and n["ticks"] >= cfg["max_ticks"])
    n["done"] = next((i + 1 for i, c in enumerate(cond) if c), 0)
    n["flags"] = sum(1 << i for i, c in enumerate(cond) if c)
    return n


def pack(recs):
    """int32 [S, 48]: the contract's record words of a list of records."""
    w = np.zeros((len(recs), 48), dtype=np.int32)
    f = w.view(np.float64)
    for s, r in enumerate(recs):
        w[s, :10] = [r[k] for k in INTS]
        f[s, 5:] = [r[k] for k in F64]
    return w


def unpack(words):
    w = np.ascontiguousarray(words, dtype=np.int32)
    f = w.view(np.float64)
    return [dict({k: int(w[s, i]) for i, k in enumerate(INTS)}, **{k: float(f[s, 5 + i]) for i, k in enumerate(F64)}) for s in range(len(w))]


# ---- the hand-built drives -----------------------------------------------------------------------------------------------------------
def _straight(n, spacing=8.0):
    """n points along +x.  8 m apart: L2 = 64 is a power of two, so the projection of a point with dyadic coordinates is exact and
    a pose ON the route has xtrack 0.0, not 1e-15."""
    return np.stack([np.arange(n) * spacing, np.zeros(n)], axis=1)


def _poses_along_x(xs, y=0.0):
    """Poses heading along +x: the forward vector (sin c, -cos c) is (1, 6e-17) at compass pi / 2."""
    return np.stack([np.asarray(xs, dtype=np.float64), np.full(len(xs), y), np.full(len(xs), math.pi / 2)], axis=1)


STEP = 5.1875            # metres per tick of the standard drive: dyadic; x_k = 0.125 + STEP * k, x_20 = 103.875 on a 104 m route


def build_drives():
    """dict name -> dict(route [G, 2], length, cfg, poses [T, 3], velocity [T] fp32, yaw_rate [T] fp32, discs [T, M, 5] or None,
    boxes [T, N, 7] or None, integer: bool, cum, records: the restatement's record after every tick, expect: what the CPU test
    asserts in closed form)."""
    D = {}
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    T = 21
    xs = 0.125 + STEP * np.arange(T)
    base = dict(route=_straight(14), length=14, velocity=f32(np.full(T, STEP / 0.5)), yaw_rate=f32(np.zeros(T)), discs=None, boxes=None,
                integer=False)
    # driven exactly: progress reaches 103.875 >= 104 - 1 at k = 20, tick 21; every xtrack is 0.0
    D["exact"] = dict(base, cfg=dict(CFG), poses=_poses_along_x(xs), expect=dict(done=1, done_tick=21, xtrack_max=0.0))
    # parallel at 16 m: beyond offroad_min = 15, inside offroad_max = 30.  After tick n the off-route distance is STEP (n - 1); its
    # share of 104 m is 0.2993 at n = 7 and 0.3492 at n = 8: off route at tick 8
    D["offset_16"] = dict(base, cfg=dict(CFG), poses=_poses_along_x(xs, 16.0), expect=dict(done=3, done_tick=8, offroad=7 * STEP))
    D["offset_31"] = dict(base, cfg=dict(CFG), poses=_poses_along_x(xs, 31.0), expect=dict(done=3, done_tick=1, offroad=0.0))
    # a standstill: the clock adds 0.5 s per tick and exceeds max_time = 4.25 s first at 4.5 s: tick 9
    D["standstill"] = dict(base, cfg=dict(CFG, max_time=4.25), poses=_poses_along_x(np.full(T, 3.3)), velocity=f32(np.zeros(T)),
                           expect=dict(done=4, done_tick=9))
    # a disc of radius 1.5 on the route at x = 52.625, r_ego = 1: contact while |x - 52.625| < 2.5, which of the x_k only x_10 =
    # 52.0 meets: one event at tick 11.  From tick 13 on the disc stands at 68.1875 = x_13 + 0.625: left and re-entered, a second
    # event at tick 14.  Slot 1 is an empty slot in the ego's path
    discs = np.zeros((T, 2, 5))
    discs[:, 0] = [52.625, 0.0, 0.0, 0.0, 1.5]
    discs[12:, 0, 0] = 68.1875
    discs[:, 1] = [20.0, 0.0, 0.0, 0.0, -1.0]
    D["disc"] = dict(base, cfg=dict(CFG), poses=_poses_along_x(xs), discs=discs,
                     expect=dict(done=1, done_tick=21, events=2, first_tick=11, first_slot=0, contact_ticks=2))
    # a box 4 x 2 at (53, 0) turned by a quarter (its length across the route), so its half extent along x is 1: a disc of the ego
    # on y = 0 touches it while |x - 53| < 1 + r_ego = 2.  The ego is two discs at 0 and 4.5 m along its heading: the front one
    # is at 51.3125 at k = 9 (tick 10), one tick before the rear one arrives (52.0 at k = 10).  stop_on_collision ends the drive
    boxes = np.zeros((T, 1, 7))
    boxes[:, 0] = [53.0, 0.0, 0.0, 0.0, math.pi / 2, 4.0, 2.0]
    D["box_stop"] = dict(base, cfg=dict(CFG, offsets=(0.0, 4.5), stop_on_collision=True), poses=_poses_along_x(xs), boxes=boxes,
                         expect=dict(done=2, done_tick=10, events=1, first_tick=10, first_slot=64))
    # a route that doubles back: out along y = 0 for 104 m, over to y = 4 and back (28 points).  Driving out along y = 2.5 the far
    # leg (1.5 m away) is nearer than the near one (2.5 m); a window of 3 segments keeps the cursor on the outward leg
    back = np.concatenate([_straight(14), np.stack([104.0 - np.arange(14) * 8.0, np.full(14, 4.0)], axis=1)])
    D["doubled_back"] = dict(base, route=back, length=len(back), cfg=dict(CFG, window=3), poses=_poses_along_x(xs[:19], 2.5),
                             velocity=f32(np.full(19, STEP / 0.5)), yaw_rate=f32(np.zeros(19)),
                             expect=dict(done=0, cursor_last=11, xtrack_max=2.5))
    # ... and without it the cursor jumps to segment 26 at the first tick, 1.5 m away, where the route is all but over: "completed"
    D["doubled_back_wide"] = dict(D["doubled_back"], cfg=dict(CFG, window=64), expect=dict(done=1, done_tick=1, cursor_first=26, xtrack_first=1.5))
    # exact ties on integers along an L with a zero-length segment: (0,0) (10,0) (10,10) (10,10) (20,10).  (5, 5) is 5 from segment 0
    # and 5 from segment 1: the lower index wins.  (8, 12) is sqrt(8) from segments 1, 2 (zero length, t = 0) and 3: segment 1.
    # (12, 12) is 2 from segment 3
    ell = np.array([[0.0, 0.0], [10.0, 0.0], [10.0, 10.0], [10.0, 10.0], [20.0, 10.0]])
    D["ties"] = dict(route=ell, length=5, cfg=dict(CFG), poses=np.array([[5.0, 5.0, 0.0], [5.0, 5.0, 0.0], [8.0, 12.0, 0.0], [12.0, 12.0, 0.0]]),
                     velocity=f32([4.0] * 4), yaw_rate=f32([0.0, 0.5, 0.0, 0.0]), discs=None, boxes=None, integer=True,
                     expect=dict(done=0, cursors=[0, 0, 1, 3], xtracks=[5.0, 5.0, math.sqrt(8.0), 2.0]))
    # a one-point route: progress 0, xtrack the distance to the point; its length is 0, so "completed" holds at once
    D["one_point"] = dict(route=np.array([[3.0, 4.0]]), length=1, cfg=dict(CFG), poses=np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0]]),
                          velocity=f32([1.0, 1.0]), yaw_rate=f32([0.0, 0.0]), discs=None, boxes=None, integer=True,
                          expect=dict(done=1, done_tick=1, xtrack_max=5.0))
    # three conditions in one tick: 31 m off the route (off route, 3) at a standstill whose clock runs out in that tick (blocked, 4)
    # with max_ticks = 1 (timeout, 5): done is the first of them, the flags hold all three
    D["order"] = dict(base, cfg=dict(CFG, max_time=0.25, max_ticks=1), poses=_poses_along_x(np.full(3, 3.3), 31.0), velocity=f32(np.zeros(3)),
                      yaw_rate=f32(np.zeros(3)), expect=dict(done=3, done_tick=1, flags=4 | 8 | 16))
    # comfort: speeds 0, 2, 6, 6 at dt = 0.5: a = 4, 8, 0; jerk = 8, -16; lateral 6 * 0.5 = 3 on the last tick
    D["comfort"] = dict(base, cfg=dict(CFG), poses=_poses_along_x([0.125, 0.625, 2.625, 5.625]), velocity=f32([0.0, 2.0, 6.0, 6.0]),
                        yaw_rate=f32([0.0, 0.0, 0.0, 0.5]), expect=dict(done=0, acc_max=8.0, acc_sq=80.0, jerk_max=16.0, jerk_sq=320.0,
                                                                         lat_max=3.0, lat_sq=9.0, distance=5.5))
    for name, d in D.items():
        d["cum"] = cumulative(d["route"])
        d["records"], clear = run(d)
        if not d["integer"]:
            assert clear > 1e-9, (name, clear)
    return D


def run(d, upto=None):
    """The records after every tick of a drive, [T] dicts, and the smallest clearance."""
    clear = Clear()
    rec, out = fresh(), []
    T = len(d["poses"]) if upto is None else upto
    for t in range(T):
        rec = step(rec, d["cfg"], d["poses"][t], d["velocity"][t], d["yaw_rate"][t], d["route"], d["length"], d["cum"],
                   None if d["discs"] is None else d["discs"][t], None if d["boxes"] is None else d["boxes"][t], clear)
        out.append(rec)
    return out, clear.value


def scale_of(d):
    """R of the accumulator bounds: the largest coordinate difference, speed quotient and distance a drive meets."""
    pts = np.concatenate([d["route"][:d["length"]], d["poses"][:, :2]])
    v = np.abs(d["velocity"].astype(np.float64)).max()
    dt = d["cfg"]["dt"]
    return float(max(np.ptp(pts[:, 0]) + np.ptp(pts[:, 1]), d["cum"][d["length"] - 1], v, 2 * v / dt, 4 * v / dt / dt, 1.0))
