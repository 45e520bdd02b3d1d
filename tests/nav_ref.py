"""fp64 NumPy restatement of "ego frame v1" and "route planner v1" (include/adx.h: adx_world_to_ego, adx_ego_to_world,
adx_nav_step), written from the contract -- a head cursor into the plan, not the reference's deque --, the rounding bounds of a
kernel that evaluates them, and the loader of the fixture recorded from the reference's RoutePlanner (tests/golden/nav_v1.npz,
tests/golden/make_golden_nav.py).

The bound of `point` (and of every rotated vector).  Two evaluations of
    th = compass + pi/2;  c = cos th;  s = sin th;  dx = X - px;  dy = Y - py
    r0 = c * dx + s * dy;  r1 = -(s * dx) + c * dy;  x = r1 / k;  y = -r0 / k          (fp64, every operation rounded once)
that differ only in their cos and sin routines see the same th, dx and dy (the same single operations on the same numbers).  A
routine within 4 ulp (the OpenCL full profile, which the device library's sin and cos are written to) against one within 1 ulp
(the host's) differ by at most 5 ulp; |c|, |s| <= 1, where an ulp is at most 2^-52: |dc|, |ds| <= 5 * 2^-52.  With e = 2^-53 the
unit roundoff, and counting both sides:
    the products   |dc| |dx| + |ds| |dy|              <= 5 * 2^-52 (|dx| + |dy|)
                   their roundings, 2 sides            <= 2 e (|c dx| + |s dy|)   <= 2^-52 (|dx| + |dy|)
    the sum        rounded, 2 sides, |r| <= |dx| + |dy|                            <= 2^-52 (|dx| + |dy|)
    the division   rounded, 2 sides                                                <= 2^-52 (|dx| + |dy|) / k
so the fp64 results differ by at most C * 2^-52 * (|dx| + |dy|) / k with C = 5 + 1 + 1 + 1 = 8, and their roundings to fp32 by
that plus one fp32 ulp of the result (two numbers that close round to the same fp32 number or to neighbours).  The heading of a
box rotates (cos yaw, sin yaw), which carry 5 ulp of their own: 8 * 2 + 2 * 5 = 26 in place of 8 * (|dx| + |dy|).
"""
import os

import numpy as np

HALF_PI = np.pi / 2.0            # the double nearest to pi / 2, the contract's
C_POINT, C_HEADING = 8.0, 26.0
E52 = 2.0 ** -52
U32 = 2.0 ** -24                 # unit roundoff of fp32
POINTS, DISCS, PLANES, BOXES = 0, 1, 2, 3
WIDTH_IN, WIDTH_OUT = (2, 5, 3, 7), (2, 5, 3, 8)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nav_v1.npz")


# ---- ego frame v1 ------------------------------------------------------------------------------------------------------------------
def frame(pose):
    """(px, py, c, s), each [S]: pose [S, 3] fp64; a NaN compass counts as 0."""
    pose = np.asarray(pose, dtype=np.float64)
    compass = np.where(np.isnan(pose[..., 2]), 0.0, pose[..., 2])
    th = compass + HALF_PI
    return pose[..., 0], pose[..., 1], np.cos(th), np.sin(th)


def rotate(f, dx, dy):
    """The ego vector (r1, -r0) of a world vector; f's entries broadcast against dx, dy."""
    _, _, c, s = f
    a0, a1 = c * dx, s * dy
    r0 = a0 + a1
    b0, b1 = s * dx, c * dy
    r1 = -b0 + b1
    return r1, -r0


def point(f, X, Y, k):
    """(x, y) fp64 before the rounding to fp32, and |dx| + |dy| for the bound."""
    dx, dy = X - f[0], Y - f[1]
    ex, ey = rotate(f, dx, dy)
    return ex / k, ey / k, np.abs(dx) + np.abs(dy)


def _col(f):
    return tuple(v[:, None] for v in f)


def world_to_ego(kind, rec, pose, xy_scale, dt=None):
    """(out fp32 [S, N, w_out], bound fp64 [S, N, w_out]): the contract's table for `rec` fp64 [S, N, w_in]."""
    rec = np.asarray(rec, dtype=np.float64)
    k = float(xy_scale)
    f = _col(frame(pose))
    S, N, _ = rec.shape
    out = np.empty((S, N, WIDTH_OUT[kind]), dtype=np.float64)
    mag = np.zeros_like(out)          # what the fp64 part of the bound multiplies, per column
    if kind != PLANES:
        out[..., 0], out[..., 1], m = point(f, rec[..., 0], rec[..., 1], k)
        mag[..., 0] = mag[..., 1] = C_POINT * m / k
    if kind in (DISCS, BOXES):
        vs = float(dt) / k
        vx, vy = rotate(f, rec[..., 2], rec[..., 3])
        out[..., 2], out[..., 3] = vx * vs, vy * vs
        mag[..., 2] = mag[..., 3] = (C_POINT + 1.0) * (np.abs(rec[..., 2]) + np.abs(rec[..., 3])) * abs(vs)      # + the product's rounding
    if kind == DISCS:
        out[..., 4] = rec[..., 4] / k          # one division on both sides: the same double
    elif kind == PLANES:
        out[..., 0], out[..., 1] = rotate(f, rec[..., 0], rec[..., 1])
        mag[..., 0] = mag[..., 1] = C_POINT * (np.abs(rec[..., 0]) + np.abs(rec[..., 1]))
        t0, t1 = rec[..., 0] * f[0], rec[..., 1] * f[1]
        out[..., 2] = (rec[..., 2] - (t0 + t1)) / k      # no cos or sin: the same double on both sides
    elif kind == BOXES:
        out[..., 4], out[..., 5] = rotate(f, np.cos(rec[..., 4]), np.sin(rec[..., 4]))
        mag[..., 4] = mag[..., 5] = C_HEADING
        out[..., 6], out[..., 7] = rec[..., 5] / k, rec[..., 6] / k
    o32 = out.astype(np.float32)
    with np.errstate(invalid="ignore"):
        bound = np.where(np.isfinite(o32), np.spacing(np.abs(o32)).astype(np.float64), 0.0) + mag * E52
    return o32, bound


def ego_to_world(plans, pose, xy_scale):
    """fp64 [rows, H, 2] world metres: `back` of the contract; row r uses pose[r % S]."""
    p = np.asarray(plans, dtype=np.float32).astype(np.float64)
    pose = np.asarray(pose, dtype=np.float64)
    rows = p.shape[0]
    px, py, c, s = (v[np.arange(rows) % pose.shape[0], None] for v in frame(pose))
    a0, a1 = -(p[..., 1] * xy_scale), p[..., 0] * xy_scale
    m0, m1 = c * a0, s * a1
    n0, n1 = s * a0, c * a1
    return np.stack([(m0 - m1) + px, (n0 + n1) + py], axis=-1)


def roundtrip_bound(q32, xy_scale, world):
    """|to_world(points(p)) - p| per world coordinate, [..., 2], for q32 = points(p) [..., 2] and world = p.  The fp32 rounding of
    (x, y), half an ulp each, is scaled back by xy_scale and rotated (a coordinate of a rotated vector is at most the sum of the two
    magnitudes): xy_scale * (ulp(x) + ulp(y)) / 2.  The fp64 work of the two directions adds 2 * 8 * 2^-52 (|dx| + |dy|), and
    |dx| + |dy| <= 2 xy_scale (|x| + |y|) (the 1-norm of a rotated vector is at most sqrt(2) times its 2-norm, itself at most the
    1-norm): 32 * 2^-52 * xy_scale (|x| + |y|).  The last addition, of the position, rounds to the world coordinate's own fp64 ulp."""
    q = np.abs(np.asarray(q32, dtype=np.float32))
    x, y = q[..., 0:1], q[..., 1:2]
    half = 0.5 * (np.spacing(x).astype(np.float64) + np.spacing(y).astype(np.float64))
    return xy_scale * (half + 4.0 * C_POINT * E52 * (x.astype(np.float64) + y.astype(np.float64))) + np.spacing(np.abs(np.asarray(world, dtype=np.float64)))


def consistency_bound(q, t):
    """|warm start v1's fp32 re-base of q0 by the motion - q1| per coordinate, for a world-fixed point seen as q0 from pose 0 and
    as q1 from pose 1, with Q = max|q0| + max|t| (model units):
        the fp32 kernel on fp32 inputs, shift 0 (tests/warm_ref.py, error_bound: 2 E_q + (12 Q + 1) u with E_q = Q u)   (14 Q + 1) u
        q0 and t are rounded to fp32, u each relatively, and pass the rotation (a coordinate sums two)                  2 Q u
        phi is rounded to fp32, |phi| <= pi: the rotation moves by |dphi| |q0 - t|_1 <= pi u * 2 Q                      7 Q u
        q1 itself is rounded to fp32, |q1| <= |q0 - t|_1 <= 2 Q                                                          2 Q u
        sqrt_ab = 1 and sqrt_1mab = 0: 1 * w and 0 * z are exact; the fp64 work of the restatement, far below           u
    """
    Q = float(np.max(np.abs(q))) + float(np.max(np.abs(t)))
    return (25.0 * Q + 2.0) * U32


# ---- route planner v1 --------------------------------------------------------------------------------------------------------------
def norm2(x, y):
    xx, yy = x * x, y * y
    return np.sqrt(xx + yy)


def walk(route, head, length, pos, min_distance, max_distance):
    """The contract's walk for one scene: (pops, clear) with `clear` the smallest relative distance of any comparison from
    equality -- d against min_distance, cum against max_distance, a candidate d against the running far."""
    n = length - head
    clear = np.inf
    if n == 1:
        return 0, clear
    cum, far, to_pop = 0.0, -np.inf, 0
    for i in range(1, n):
        clear = min(clear, abs(cum - max_distance) / max_distance)
        if cum > max_distance:
            break
        a, b = route[head + i - 1], route[head + i]
        cum = cum + norm2(b[0] - a[0], b[1] - a[1])
        d = norm2(b[0] - pos[0], b[1] - pos[1])
        clear = min(clear, abs(d - min_distance) / min_distance)
        if d <= min_distance:
            if np.isfinite(far):
                clear = min(clear, abs(d - far) / max(d, far, 1e-300))
            if d > far:
                far, to_pop = d, i
    return min(to_pop, max(n - 2, 0)), clear


def fresh_state(S):
    return dict(head=np.zeros(S, dtype=np.int32), valid=np.zeros(S, dtype=np.int32), prev=np.zeros((S, 3), dtype=np.float64))


def nav_step(route, cmd, length, pose, state, *, min_distance=7.0, max_distance=50.0, xy_scale=23.315, R=16, first=0):
    """One launch of adx_nav_step.  route [S, G, 2] fp64, cmd [S, G], length [S], pose [S, 3]; `state` is not modified, the new
    one is out["state"].  Outputs as the contract names them, with `*_bound` beside every fp32 one and `clear` [S] from walk()."""
    route, pose = np.asarray(route, dtype=np.float64), np.asarray(pose, dtype=np.float64)
    S, G, _ = route.shape
    length = np.clip(np.asarray(length, dtype=np.int64), 1, G)
    head = np.clip(state["head"].astype(np.int64), 0, length - 1)
    compass = np.where(np.isnan(pose[:, 2]), 0.0, pose[:, 2])
    nxt, clear = np.zeros(S, dtype=np.int64), np.zeros(S)
    for s in range(S):
        pops, clear[s] = walk(route[s], head[s], length[s], pose[s, :2], min_distance, max_distance)
        head[s] += pops
        nxt[s] = head[s] if length[s] - head[s] == 1 else head[s] + 1
    sc = np.arange(S)
    target, target_bound = world_to_ego(POINTS, route[sc, nxt][:, None], pose, xy_scale)
    idx = np.minimum(head[:, None] + first + np.arange(R)[None], length[:, None] - 1)
    window, window_bound = world_to_ego(POINTS, route[sc[:, None], idx], pose, xy_scale)
    motion, motion_bound = np.zeros((S, 3), dtype=np.float32), np.zeros((S, 3))
    was = state["valid"] != 0
    if was.any():
        t, tb = world_to_ego(POINTS, pose[:, None, :2], state["prev"], xy_scale)
        d = compass - state["prev"][:, 2]
        phi = d - (2.0 * np.pi) * np.ceil((d - np.pi) / (2.0 * np.pi))
        full = np.concatenate([t[:, 0], phi.astype(np.float32)[:, None]], axis=1)
        motion[was] = full[was]
        motion_bound[was, :2] = tb[was, 0]      # phi has no cos or sin in it: the same double, the same float
    new = dict(head=head.astype(np.int32), valid=np.ones(S, dtype=np.int32), prev=np.stack([pose[:, 0], pose[:, 1], compass], axis=1))
    return dict(target=target[:, 0], target_bound=target_bound[:, 0], command=np.asarray(cmd)[sc, nxt].astype(np.int32), window=window,
                window_bound=window_bound, motion=motion, motion_bound=motion_bound, fresh=(~was).astype(np.int32),
                head=head.astype(np.int32), next=nxt, remaining=(length - head).astype(np.int32), clear=clear, state=new)


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def load_golden(path=GOLDEN):
    """The drives of tests/golden/nav_v1.npz: a list of dicts(name, integer, min_distance, max_distance, route [G, 2], cmd [G],
    pose [T, 3], ret_idx [T], ret_cmd [T], ret_len [T], ret_pt [T, 2])."""
    z = np.load(path)
    out = []
    for i, name in enumerate(z["names"]):
        g0, g1, t0, t1 = z["route_off"][i], z["route_off"][i + 1], z["tick_off"][i], z["tick_off"][i + 1]
        out.append(dict(name=str(name), integer=bool(z["integer"][i]), min_distance=float(z["min_distance"][i]),
                        max_distance=float(z["max_distance"][i]), route=z["routes"][g0:g1], cmd=z["cmds"][g0:g1], pose=z["poses"][t0:t1],
                        ret_idx=z["ret_idx"][t0:t1], ret_cmd=z["ret_cmd"][t0:t1], ret_len=z["ret_len"][t0:t1], ret_pt=z["ret_pt"][t0:t1]))
    return out


def pack(drives, S=3):
    """Launches of S scenes from the drives, taken S at a time in order (the last group wraps round): dicts(names, route [S, G, 2],
    cmd [S, G], length [S], poses [T, S, 3]) with G and T the group's largest; a shorter drive holds its last pose."""
    out = []
    for g in range(0, len(drives), S):
        grp = [drives[(g + j) % len(drives)] for j in range(S)]
        G, T = max(len(d["route"]) for d in grp), max(len(d["pose"]) for d in grp)
        route, cmd = np.zeros((S, G, 2)), np.full((S, G), -7, dtype=np.int32)
        poses = np.zeros((T, S, 3))
        for j, d in enumerate(grp):
            n = len(d["route"])
            route[j, :n], cmd[j, :n] = d["route"], d["cmd"]
            route[j, n:] = 1e6 + np.arange(G - n)[:, None]      # never read: a wrong index shows
            poses[:len(d["pose"]), j] = d["pose"]
            poses[len(d["pose"]):, j] = d["pose"][-1]
        out.append(dict(names=[d["name"] for d in grp], route=route, cmd=cmd, length=np.array([len(d["route"]) for d in grp], dtype=np.int32),
                        poses=poses, min_distance=grp[0]["min_distance"], max_distance=grp[0]["max_distance"]))
    return out
