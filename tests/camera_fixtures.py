"""The worlds the camera tests render, shared by tests/test_camera_cpu.py (which holds them to the 1 % cap on near-threshold pixels)
and tests/test_gpu_camera.py (which renders them on the device).  Everything is NumPy float64 in the formats of the contracts."""
import math

import numpy as np

import camera_ref as R


def to_world(pose, ex, ey):
    """World points of ego-frame points (ex lateral, ey forward, metres) under ego frame v1: +y is (sin compass, -cos compass),
    +x is (-cos compass, -sin compass)."""
    px, py, c = pose[..., 0], pose[..., 1], pose[..., 2]
    return px - np.cos(c) * ex + np.sin(c) * ey, py - np.sin(c) * ex - np.cos(c) * ey


def heading(pose):
    """The world angle of the ego's forward axis."""
    return pose[..., 2] - math.pi / 2.0


def line_records(pose, ex, ey, dyaw, width, kind=1.0):
    """signals v1 records [..., 10] of stop lines centred at ego (ex, ey) whose governed traffic heads the ego's way + dyaw."""
    cx, cy = to_world(pose, ex, ey)
    yaw = heading(pose) + dyaw
    hx, hy = width / 2.0 * np.sin(yaw), width / 2.0 * -np.cos(yaw)
    rec = np.zeros(np.broadcast(cx, hx).shape + (10,))
    rec[..., 0], rec[..., 1], rec[..., 2], rec[..., 3] = cx - hx, cy - hy, cx + hx, cy + hy
    rec[..., 4], rec[..., 5] = kind, 30.0
    rec[..., 7:10] = (10.0, 3.0, 10.0)
    return rec


def random_world(seed, S, W, H, nb, nd, ns, nq, ng, segs=None):
    """A dict(cfg, pose, boxes, discs, signals, phase, roads, road_len) with the given slot counts, objects scattered in front of
    and around the eye (none within 3 m of it), some slots empty."""
    rng = np.random.default_rng(seed)
    cfg = R.Cfg(width=W, height=H, n_boxes=nb, n_discs=nd, n_signals=ns, n_paths=nq, n_points=ng if nq else 0)
    pose = np.stack([rng.uniform(-200, 200, S), rng.uniform(-200, 200, S), rng.uniform(-math.pi, math.pi, S)], axis=1)
    out = dict(cfg=cfg, pose=pose, boxes=None, discs=None, signals=None, phase=None, roads=None, road_len=None)
    P = pose[:, None, :]

    def scatter(n):
        ex, ey = rng.uniform(-25, 25, (S, n)), rng.uniform(-12, 90, (S, n))
        close = np.hypot(ex, ey + 1.5) < 4.0
        return ex, np.where(close, ey + 12.0, ey)

    if nb:
        ex, ey = scatter(nb)
        x, y = to_world(P, ex, ey)
        b = np.zeros((S, nb, 7))
        b[..., 0], b[..., 1] = x, y
        b[..., 2:4] = rng.uniform(-3, 3, (S, nb, 2))
        b[..., 4] = rng.uniform(-math.pi, math.pi, (S, nb))
        b[..., 5], b[..., 6] = rng.uniform(3.5, 5.0, (S, nb)), rng.uniform(1.6, 2.2, (S, nb))
        if nb > 2:
            b[:, 1::7, 5] = 0.0      # empty slots
        out["boxes"] = b
    if nd:
        ex, ey = scatter(nd)
        x, y = to_world(P, ex, ey)
        d = np.zeros((S, nd, 5))
        d[..., 0], d[..., 1], d[..., 4] = x, y, rng.uniform(0.3, 0.8, (S, nd))
        if nd > 2:
            d[:, 2::9, 4] = -1.0
        out["discs"] = d
    if ns:
        ex, ey = rng.uniform(-8, 8, (S, ns)), rng.uniform(6, 70, (S, ns))
        out["signals"] = line_records(P, ex, ey, rng.uniform(-0.4, 0.4, (S, ns)), rng.uniform(3.5, 7.0, (S, ns)))
        out["phase"] = rng.integers(0, 5, (S, ns)).astype(np.int32) if ns > 1 else np.full((S, ns), 3, dtype=np.int32)
    if nq:
        n = ng if segs is None else segs + 1
        t = np.linspace(0.0, 1.0, ng)[None, None, :]
        off = rng.uniform(-12, 12, (S, nq, 1))
        curve = rng.uniform(-20, 20, (S, nq, 1))
        ey = -8.0 + 120.0 * t + 0.0 * off
        ex = off + curve * t * t
        x, y = to_world(pose[:, None, None, :], ex, ey)
        out["roads"] = np.stack([x, y], axis=-1)
        ln = np.full((S, nq), n, dtype=np.int32)
        if nq > 2:
            ln[:, 2] = 1      # a path with fewer than 2 counted points
        out["road_len"] = ln
    return out


def placed_world(W=129, H=65):
    """Hand-placed primitives at the edges the render kernel has: a box astride the 64-column tile edge and one astride the
    16-row tile edge, a box partly behind the eye, a box wholly left of the image, one wholly behind, a disc astride a tile
    corner, a lamp over a tile edge, and every kind of empty slot.  One pose with compass 0, one turned."""
    S = 2
    cfg = R.Cfg(width=W, height=H, n_boxes=8, n_discs=4, n_signals=3, n_paths=2, n_points=4)
    pose = np.array([[10.0, -4.0, 0.0], [-30.0, 55.0, 2.2]])
    P = pose[:, None, :]
    k = float(cfg.k)
    # a ground point seen at column u, row v:  t = h / ((v + .5 - H/2) k),  x = (u + .5 - W/2) k t
    def ground_at(u, v):
        t = cfg.cam_height / ((v + 0.5 - H / 2.0) * k)
        return (u + 0.5 - W / 2.0) * k * t, t + cfg.mount_back
    bex, bey = np.zeros((S, 8)), np.zeros((S, 8))
    bex[:, 0], bey[:, 0] = ground_at(64.3, 40.0)      # astride the column tile edge (tiles are 64 x 16)
    bex[:, 1], bey[:, 1] = ground_at(30.0, 47.6)      # its foot astride the row tile edge at 48
    bex[:, 2], bey[:, 2] = 2.5, -2.0                  # partly behind the eye's plane
    bex[:, 3], bey[:, 3] = -60.0, 12.0                # wholly left of the image
    bex[:, 4], bey[:, 4] = 0.5, -20.0                 # wholly behind
    bex[:, 5], bey[:, 5] = -6.0, 25.0
    bex[:, 6], bey[:, 6] = 0.0, 10.0                  # empty: no length
    bex[:, 7], bey[:, 7] = 0.0, 12.0                  # empty: a NaN width
    x, y = to_world(P, bex, bey)
    boxes = np.zeros((S, 8, 7))
    boxes[..., 0], boxes[..., 1] = x, y
    boxes[..., 4] = heading(P) + np.array([0.3, -1.1, 0.2, 0.0, 0.7, 1.5, 0.0, 0.0])
    boxes[..., 5], boxes[..., 6] = 4.4, 1.9
    boxes[:, 6, 5] = 0.0
    boxes[:, 7, 6] = np.nan
    dex, dey = np.zeros((S, 4)), np.zeros((S, 4))
    dex[:, 0], dey[:, 0] = ground_at(63.6, 47.8)      # astride a tile corner
    dex[:, 1], dey[:, 1] = 4.0, -6.0                  # behind
    dex[:, 2], dey[:, 2] = -3.0, 18.0                 # empty: radius 0
    dex[:, 3], dey[:, 3] = 3.0, 30.0                  # empty: a NaN radius
    x, y = to_world(P, dex, dey)
    discs = np.zeros((S, 4, 5))
    discs[..., 0], discs[..., 1], discs[..., 4] = x, y, 0.5
    discs[:, 2, 4] = 0.0
    discs[:, 3, 4] = np.nan
    signals = line_records(P, np.array([0.4, -5.0, 3.0]), np.array([14.0, 22.0, 9.0]), np.array([0.0, 0.2, 0.0]), 6.0)
    signals[:, 2, 2:4] = signals[:, 2, 0:2]      # a line of no length: empty whatever its phase says
    phase = np.array([[3, 0, 1], [1, 4, 2]], dtype=np.int32)
    t = np.array([0.0, 15.0, 40.0, 90.0])
    ex = np.stack([0.02 * t * t / 9.0, -3.5 + 0.0 * t])[None]
    ey = np.stack([-6.0 + t, -6.0 + t])[None]
    x, y = to_world(pose[:, None, None, :], ex, ey)
    roads = np.stack([x, y], axis=-1)
    road_len = np.array([[4, 3], [4, 1]], dtype=np.int32)
    return dict(cfg=cfg, pose=pose, boxes=boxes, discs=discs, signals=signals, phase=phase, roads=roads, road_len=road_len)


# name -> builder; the sizes, scene counts and primitive counts the GPU test sweeps
FIXTURES = {
    "empty_24x16_s1": lambda: random_world(1, 1, 24, 16, 0, 0, 0, 0, 0),
    "ones_70x33_s3": lambda: random_world(2, 3, 70, 33, 1, 1, 1, 1, 2),
    "full_129x65_s3": lambda: random_world(3, 3, 129, 65, 64, 64, 64, 8, 64),
    "full_24x16_s65": lambda: random_world(4, 65, 24, 16, 64, 64, 64, 8, 64),
    "placed_129x65_s2": placed_world,
    "frame_900x256_s1": lambda: random_world(5, 1, 900, 256, 8, 2, 2, 1, 64),
}


def staged(w, defect=None):
    """(table, bound) of a world dict by the restatement."""
    return R.stage(w["cfg"], w["pose"], w["boxes"], w["discs"], w["signals"], w["phase"], w["roads"], w["road_len"], defect=defect)
