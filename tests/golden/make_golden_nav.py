"""Record tests/golden/nav_v1.npz from the reference's own RoutePlanner (e2e_driving/planner.py, pure NumPy).

    python tests/golden/make_golden_nav.py /path/to/reference

Every drive sets a route, then calls `run_step(position)` tick by tick and records what the planner returned: the point (its index
in the route as set, and its coordinates), its command and `len(planner.route)` after the call.  The planner reads a route point
as `pos.location.x / .y`; a three-line stand-in supplies that.  Commands are small integers here (the planner stores and returns
them untouched).

What is NOT recorded: the ego-frame transform.  The reference applies it in `interact.py` and `e2e_driving/diffusion_agent.py`,
which import `carla` and cannot run without the simulator, so the transform is pinned to the fp64 restatement of its formula
(tests/nav_ref.py, from include/adx.h "ego frame v1") and not to a recorded reference output.  The compasses stored with the
positions are this script's own and are read only by that restatement and the kernels.

For every drive whose coordinates are not small integers the script asserts (through tests/nav_ref.py's `walk`) that every
comparison of every tick -- d against min_distance, cum against max_distance, a candidate d against the running far -- is clear of
equality by 1e-9 relative: a condition on the INPUTS, so that neither contraction inside NumPy's `dot` nor the order of a sum can
flip a decision.  tests/test_nav_cpu.py re-asserts it on the stored data.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import nav_ref as R  # noqa: E402

MIN_D, MAX_D, CLEAR = 7.0, 50.0, 1e-9


def _pos(x, y):
    return SimpleNamespace(location=SimpleNamespace(x=float(x), y=float(y)))


def polyline(points, spacing, G):
    """G points `spacing` apart along the polyline through `points` (straight on past its end)."""
    pts = np.asarray(points, dtype=np.float64)
    seg = np.diff(pts, axis=0)
    ln = np.hypot(seg[:, 0], seg[:, 1])
    out, k, at = [], 0, 0.0
    for i in range(G):
        s = i * spacing
        while k < len(ln) - 1 and s > at + ln[k]:
            at += ln[k]
            k += 1
        out.append(pts[k] + seg[k] * ((s - at) / ln[k]))
    return np.array(out)


def arc(radius, spacing, G):
    a = np.arange(G) * (spacing / radius)
    return np.stack([radius * np.sin(a), radius * (1.0 - np.cos(a))], axis=1)


def follow(route, step, ticks, offset=0.37, start=0.0):
    """Positions `step` metres of route length apart, `offset` metres to the left of it."""
    seg = np.diff(route, axis=0)
    ln = np.hypot(seg[:, 0], seg[:, 1])
    cum = np.concatenate([[0.0], np.cumsum(ln)])
    out = []
    for t in range(ticks):
        s = min(start + t * step, cum[-1] + 5.0)
        k = min(int(np.searchsorted(cum, s, side="right")) - 1, len(ln) - 1)
        d = seg[k] / ln[k]
        out.append(route[k] + d * (s - cum[k]) + offset * np.array([-d[1], d[0]]))
    return np.array(out)


def drives():
    rng = np.random.default_rng(2026)
    out = []

    def add(name, route, pos, integer=False):
        route, pos = np.asarray(route, dtype=np.float64), np.asarray(pos, dtype=np.float64)
        cmd = rng.integers(-1, 7, size=len(route)).astype(np.int32)
        head = np.arctan2(np.gradient(pos[:, 1]) if len(pos) > 1 else 0.0, np.gradient(pos[:, 0]) if len(pos) > 1 else 1.0)
        compass = head + rng.uniform(-0.2, 0.2, size=len(pos))
        out.append(dict(name=name, route=route, cmd=cmd, pose=np.concatenate([pos, compass[:, None]], axis=1), integer=integer))

    straight = polyline([[10.0, -4.0], [400.0, 90.0]], 3.0, 64)
    add("straight_3m_G64", straight, follow(straight, 2.3, 24))
    curve = arc(40.0, 3.0, 65)
    add("curve_3m_G65", curve, follow(curve, 2.9, 20, offset=-0.8))
    hairpin = polyline([[0.0, 0.0], [60.0, 0.3], [63.0, 2.1], [60.0, 4.2], [-200.0, 5.0]], 3.0, 200)
    add("hairpin_3m_G200", hairpin, follow(hairpin, 4.1, 30, offset=0.55))
    # 0.5 m apart up to 2 cm of jitter: a hundred segments of exactly 0.5 m would put cum on max_distance itself
    dense = polyline([[0.0, 0.0], [300.0, 17.0]], 0.5, 200) + rng.uniform(-0.02, 0.02, size=(200, 2))
    add("dense_0.5m_G200", dense, follow(dense, 1.7, 16))            # the max_distance stop falls past point 100
    mid = polyline([[0.0, 0.0], [300.0, -23.0]], 0.9, 200)
    add("dense_0.9m_G200", mid, follow(mid, 3.3, 16))                # ... and here before point 64
    sparse = polyline([[0.0, 0.0], [3000.0, 400.0]], 30.0, 64)
    add("sparse_30m_G64", sparse, follow(sparse, 6.1, 24))
    add("sparse_30m_G3", sparse[:3], follow(sparse[:3], 9.7, 10))
    add("one_point_G1", [[5.0, 6.0]], [[0.3, 0.2], [4.1, 5.5], [9.0, 9.0]])
    add("two_points_G2", [[0.0, 0.0], [3.0, 0.4]], follow(np.array([[0.0, 0.0], [3.0, 0.4]]), 1.3, 6))
    add("three_points_G3", straight[:3], follow(straight[:3], 1.9, 8))
    short = polyline([[0.0, 0.0], [40.0, 3.0]], 3.0, 5)
    # the second tick finds only the LAST of its three points in range: it asks for 2 pops where len - 2 = 1 may be given
    add("jump_past_len_minus_2", short, [short[0] + [0.2, 0.1], short[4] + [4.5, 0.4], short[4] + [4.7, 0.3]])
    add("route_ends", straight[:12], follow(straight[:12], 3.7, 16))
    add("stationary", curve[:40], np.repeat(follow(curve[:40], 2.9, 4)[3:], 5, axis=0))
    ties = np.array([[-1, 0], [3, 4], [4, 3], [5, 0], [0, 5], [-3, 4], [6, 8], [7, 0], [0, 7], [9, 9], [20, 20], [40, 40]], dtype=np.float64)
    add("integer_ties", ties, [[0, 0], [0, 0], [3, 4], [6, 8], [7, 7]], integer=True)
    return out


def record(planner_cls, d):
    planner = planner_cls(MIN_D, MAX_D)
    planner.set_route([(_pos(x, y), int(c)) for (x, y), c in zip(d["route"], d["cmd"])])
    G = len(d["route"])
    idx, cmd, ln, pt = [], [], [], []
    for pose in d["pose"]:
        p, c = planner.run_step(np.array([pose[0], pose[1]]))
        left = len(planner.route)
        i = G - left if left == 1 else G - left + 1
        assert np.array_equal(p, d["route"][i]) and c == d["cmd"][i]
        idx.append(i), cmd.append(c), ln.append(left), pt.append(p)
    return np.array(idx, dtype=np.int32), np.array(cmd, dtype=np.int32), np.array(ln, dtype=np.int32), np.array(pt)


def check_clear(d):
    head, G = 0, len(d["route"])
    for pose in d["pose"]:
        pops, clear = R.walk(d["route"], head, G, pose[:2], MIN_D, MAX_D)
        assert clear > CLEAR, (d["name"], clear)
        head += pops


def main(reference):
    sys.path.insert(0, reference)
    from e2e_driving.planner import RoutePlanner
    ds = drives()
    z = dict(names=np.array([d["name"] for d in ds]), integer=np.array([d["integer"] for d in ds]),
             min_distance=np.full(len(ds), MIN_D), max_distance=np.full(len(ds), MAX_D),
             route_off=np.cumsum([0] + [len(d["route"]) for d in ds]).astype(np.int32),
             tick_off=np.cumsum([0] + [len(d["pose"]) for d in ds]).astype(np.int32),
             routes=np.concatenate([d["route"] for d in ds]), cmds=np.concatenate([d["cmd"] for d in ds]),
             poses=np.concatenate([d["pose"] for d in ds]))
    rec = []
    for d in ds:
        if not d["integer"]:
            check_clear(d)
        rec.append(record(RoutePlanner, d))
    for j, key in enumerate(("ret_idx", "ret_cmd", "ret_len", "ret_pt")):
        z[key] = np.concatenate([r[j] for r in rec])
    path = os.path.join(HERE, "nav_v1.npz")
    np.savez_compressed(path, **z)
    print(f"{path}: {len(ds)} drives, {len(z['poses'])} ticks, {os.path.getsize(path)} bytes")
    for d, r in zip(ds, rec):
        print(f"  {d['name']:24s} G={len(d['route']):3d} ticks={len(d['pose']):2d} idx={r[0].tolist()}")


if __name__ == "__main__":
    main(sys.argv[1])
