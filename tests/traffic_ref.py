"""fp64 NumPy restatement of "traffic v1" (include/adx.h: adx_traffic_step, adx_traffic_reset), written from the contract's text one
operation per line in the contract's order, for every scene and every agent at once (the update is synchronous, so they are
independent); the candidates of a leader are taken one at a time in the contract's order.  Beside it: the parameters the hand-
derived scenarios share, a scalar drive of one path for them, and the random drives the device is compared on.

Decisions.  The contract has no library call: every number both sides compare is formed by the same single IEEE operations (+ - *
/ sqrt, all correctly rounded) on the same inputs, so the device is held to EQUALITY.  `step` still returns in `slack` the smallest
relative distance |a - b| / max(|a|, |b|, 1) of any comparison that DECIDES something from its threshold -- on_q, se > s_i, the
ordering of agents on a path and of a leader's candidates, front <= s_stop, the yellow test, the hard clamp, the overlap test,
arrival, and cum[j] <= s' for j >= 1 -- so that a test can assert that no rounding could flip a decision even if one word
differed.  The clamps that only bound a value (acc <= accel, v' >= 0, the floors under star and the gap) decide nothing: at their
threshold both branches give the same number.
"""
import numpy as np

INTS = ("ticks", "have", "arrived", "ego_yields", "ego_hard", "overlaps")
HEAD, MAXQ = 32, 8
YELLOW, RED, EGO = 2, 3, 64
# the parameters of the issue's numeric claims
LENGTH, WIDTH, HEADWAY, ACCEL, BRAKE = 4.5, 2.0, 1.5, 1.5, 2.0
CFG = dict(lane_half_width=1.75, ego_length=4.5, jam=2.0, gap_min=0.25, brake_max=8.0)
DTS = (0.05, 0.1, 0.5)
INF = np.inf


def words(N):
    return HEAD + 5 * N + (N & 1)


def fresh_state(S, N):
    st = {k: np.zeros(S, dtype=np.int32) for k in INTS}
    st.update(min_ego_gap=np.zeros(S), se_prev=np.zeros((S, MAXQ)), on_prev=np.zeros((S, MAXQ), dtype=np.int32), s=np.zeros((S, N)),
              v=np.zeros((S, N)), alive=np.zeros((S, N), dtype=np.int32))
    return st


def pack_state(st):
    """int32 [S, W]: the contract's record."""
    S, N = st["s"].shape
    w = np.zeros((S, words(N)), dtype=np.int32)
    for i, k in enumerate(INTS):
        w[:, i] = st[k]
    f = w.view(np.float64)
    f[:, 3] = st["min_ego_gap"]
    f[:, 4:12] = st["se_prev"]
    w[:, 24:32] = st["on_prev"]
    f[:, 16:16 + N] = st["s"]
    f[:, 16 + N:16 + 2 * N] = st["v"]
    w[:, HEAD + 4 * N:HEAD + 5 * N] = st["alive"]
    return w


def unpack_state(w):
    w = np.ascontiguousarray(w, dtype=np.int32)
    N = (w.shape[1] - HEAD) // 5
    f = w.view(np.float64)
    st = {k: w[:, i].copy() for i, k in enumerate(INTS)}
    st.update(min_ego_gap=f[:, 3].copy(), se_prev=f[:, 4:12].copy(), on_prev=w[:, 24:32].copy(), s=f[:, 16:16 + N].copy(),
              v=f[:, 16 + N:16 + 2 * N].copy(), alive=w[:, HEAD + 4 * N:HEAD + 5 * N].copy())
    return st


def path_tables(paths):
    """cum and heading [..., G] of paths [..., G, 2]: the caller's tables (Traffic.path_tables states the same)."""
    p = np.asarray(paths, dtype=np.float64)
    d = p[..., 1:, :] - p[..., :-1, :]
    xx, yy = d[..., 0] * d[..., 0], d[..., 1] * d[..., 1]
    cum = np.zeros(p.shape[:-1])
    cum[..., 1:] = np.cumsum(np.sqrt(xx + yy), axis=-1)
    heading = np.zeros(p.shape[:-1])
    heading[..., :-1] = np.arctan2(d[..., 1], d[..., 0])
    heading[..., -1] = heading[..., -2]
    return cum, heading


def _rel(a, b):
    with np.errstate(invalid="ignore"):
        r = np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1.0)
    return np.where(np.isnan(r), INF, r)


def _least(slack, r, where=None):
    r = np.asarray(r, dtype=np.float64)
    if where is not None:
        r = np.where(where, r, INF)
    return min(slack, float(r.min())) if r.size else slack


def slots(paths, plen, cum, agents):
    """"agents" of the contract: (valid bool [S, N], path int [S, N] (0 where not valid), plen clamped [S, Q], length [S, Q])."""
    S, Q, G = paths.shape[:3]
    pl = np.clip(np.asarray(plen, dtype=np.int64), 0, G)
    plength = np.take_along_axis(cum, np.maximum(pl - 1, 0)[..., None], axis=2)[..., 0]                # cum[plen-1]
    a = np.asarray(agents, dtype=np.float64)
    pf = a[..., 0]
    with np.errstate(invalid="ignore"):
        in_range = (pf >= 0.0) & (pf <= float(Q - 1))
        q = np.where(in_range, pf, 0.0).astype(np.int64)
        named = in_range & (q.astype(np.float64) == pf) & (np.take_along_axis(pl, q, axis=1) >= 2)
        q = np.where(named, q, 0)
        ok = (a[..., 4] > 0.0) & (a[..., 5] > 0.0) & (a[..., 3] > 0.0) & (a[..., 7] > 0.0) & (a[..., 8] > 0.0) & (a[..., 6] >= 0.0) & \
            (a[..., 1] >= 0.0) & (a[..., 2] >= 0.0) & (a[..., 1] < np.take_along_axis(plength, q, axis=1))
    return named & ok, q, pl, plength


def boxes_of(paths, pl, cum, heading, agents, path, live, s, v):
    """"boxes" of the contract for agents at (s, v); also the least distance of s from a cum[j], j >= 1, that it is compared with."""
    S, N = s.shape
    G = paths.shape[2]
    si = np.arange(S)[:, None]
    c = cum[si, path]                                                      # [S, N, G]
    last = pl[si, path] - 2                                                # [S, N]
    g = np.arange(G)[None, None, :]
    cand = (g >= 1) & (g <= last[..., None])
    with np.errstate(invalid="ignore"):
        below = cand & (c <= s[..., None])
    j = np.where(below, g, 0).max(axis=2)
    near = _least(INF, _rel(c, s[..., None]), cand & live[..., None])
    a = paths[si, path, j]                                                  # [S, N, 2]
    b = paths[si, path, np.minimum(j + 1, G - 1)]
    dx, dy = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1]
    dxx, dyy = dx * dx, dy * dy
    L = np.sqrt(dxx + dyy)
    with np.errstate(invalid="ignore", divide="ignore"):
        ux, uy = np.where(L > 0.0, dx / L, 0.0), np.where(L > 0.0, dy / L, 0.0)
    along = s - c[si, np.arange(N)[None, :], j]
    ox, oy = along * ux, along * uy
    out = np.zeros((S, N, 7))
    out[..., 0], out[..., 1] = a[..., 0] + ox, a[..., 1] + oy
    out[..., 2], out[..., 3] = v * ux, v * uy
    out[..., 4] = heading[si, path, j]
    out[..., 5], out[..., 6] = agents[..., 4], agents[..., 5]
    out[~live] = 0.0
    return out, near


def reset(state, paths, plen, cum, heading, agents, mask=None):
    """adx_traffic_reset: (state, boxes of the masked scenes (zeros elsewhere), the mask as bool)."""
    paths, cum, heading, agents = (np.asarray(x, dtype=np.float64) for x in (paths, cum, heading, agents))
    S, N = agents.shape[:2]
    m = np.ones(S, dtype=bool) if mask is None else np.asarray(mask) != 0
    valid, path, pl, _ = slots(paths, plen, cum, agents)
    new = {k: v.copy() for k, v in state.items()}
    for k in INTS:
        new[k][m] = 0
    new["have"][m] = 1
    new["min_ego_gap"][m] = INF
    new["se_prev"][m], new["on_prev"][m] = 0.0, 0
    new["s"][m] = np.where(valid, agents[..., 1], 0.0)[m]
    new["v"][m] = np.where(valid, agents[..., 2], 0.0)[m]
    new["alive"][m] = valid[m]
    boxes, _ = boxes_of(paths, pl, cum, heading, agents, path, valid, np.where(valid, agents[..., 1], 0.0), np.where(valid, agents[..., 2], 0.0))
    boxes[~m] = 0.0
    return new, boxes, m


def project(paths, pl, cum, pose):
    """"ego" of the contract without its memory: (se [S, Q], d [S, Q]) over all segments, +inf and 0 for an empty path."""
    S, Q, G = paths.shape[:3]
    px, py = pose[:, 0][:, None, None], pose[:, 1][:, None, None]
    ax, ay = paths[:, :, :-1, 0], paths[:, :, :-1, 1]
    ux, uy = paths[:, :, 1:, 0] - ax, paths[:, :, 1:, 1] - ay
    uxx, uyy = ux * ux, uy * uy
    L2 = uxx + uyy
    with np.errstate(invalid="ignore", divide="ignore"):
        rx, ry = px - ax, py - ay
        m0, m1 = rx * ux, ry * uy
        f = (m0 + m1) / L2
        t = np.where(L2 > 0.0, np.where(f > 0.0, np.where(f < 1.0, f, 1.0), 0.0), 0.0)
        tx, ty = t * ux, t * uy
        qx, qy = ax + tx, ay + ty
        ex, ey = px - qx, py - qy
        exx, eyy = ex * ex, ey * ey
        dd = np.sqrt(exx + eyy)
    d = np.where(np.isnan(dd), INF, dd)
    d = np.where(np.arange(G - 1)[None, None, :] <= (pl - 2)[..., None], d, INF)
    j = d.argmin(axis=2)                                                     # the first of the smallest: the lower j on a tie
    take = lambda x: np.take_along_axis(x, j[..., None], axis=2)[..., 0]     # noqa: E731
    along = take(t) * take(np.sqrt(L2))
    se = take(cum[:, :, :-1]) + along
    live = pl >= 2
    return np.where(live, se, 0.0), np.where(live, take(d), INF)


def step(state, paths, plen, cum, heading, agents, stops, phase, pose, hold=None, *, dt, lane_half_width, ego_length, jam, gap_min,
         brake_max):
    """One launch of adx_traffic_step; `state` is not modified.  Returns dict(state, boxes [S, N, 7], leader int32 [S, N] (of a
    held scene: -2, the launch does not write it), slack, acc [S, N] after its clamps, gap [S, N], hard bool [S, N], ue [S, 8] and
    on bool [S, 8]: the ego's speed along every path and whether it is on it)."""
    paths, cum, heading, agents, pose = (np.asarray(x, dtype=np.float64) for x in (paths, cum, heading, agents, pose))
    S, N = agents.shape[:2]
    Q = paths.shape[1]
    held = np.zeros(S, dtype=bool) if hold is None else np.asarray(hold) != 0
    valid, path, pl, plength = slots(paths, plen, cum, agents)
    fresh, _, _ = reset(state, paths, plen, cum, heading, agents)
    have = state["have"] != 0
    st = {k: np.where(have.reshape((S,) + (1,) * (v.ndim - 1)), v, fresh[k]) for k, v in state.items()}      # have == 0: the state a reset leaves
    s, v = st["s"], st["v"]
    live = (st["alive"] != 0) & valid
    a_des, a_len, a_head, a_acc, a_brk = (agents[..., i] for i in (3, 4, 6, 7, 8))
    si, slack = np.arange(S)[:, None], INF
    run = ~held[:, None]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # ---- the ego on every path ----
        se, d = project(paths, pl, cum, pose)
        se, d = np.pad(se, ((0, 0), (0, MAXQ - Q))), np.pad(d, ((0, 0), (0, MAXQ - Q)), constant_values=INF)
        on = d <= lane_half_width
        slack = _least(slack, _rel(d, lane_half_width), np.isfinite(d) & run)
        both = on & (st["on_prev"] != 0)
        rate = (se - st["se_prev"]) / dt
        ue = np.where(both & (rate > 0.0), rate, 0.0)
        # ---- the leader ----
        half = a_len / 2.0
        front, rear = s + half, s - half
        best_r, best_u, lead = np.full((S, N), INF), np.zeros((S, N)), np.full((S, N), -1, dtype=np.int32)
        idx = np.arange(N)[None, :]
        for k in range(N):
            same = live & live[:, k:k + 1] & (path == path[:, k:k + 1]) & (idx != k)
            ks, kv, kr = s[:, k:k + 1], v[:, k:k + 1], rear[:, k:k + 1]
            ahead = same & ((ks > s) | ((ks == s) & (k < idx)))
            slack = _least(slack, _rel(ks, s), same & (ks != s) & run)
            slack = _least(slack, _rel(kr, best_r), ahead & (kr != best_r) & run)
            take = ahead & (kr < best_r)
            best_r, best_u, lead = np.where(take, kr, best_r), np.where(take, kv, best_u), np.where(take, k, lead)
        e_se, e_on, e_ue = se[si, path], on[si, path], ue[si, path]
        slack = _least(slack, _rel(e_se, s), live & e_on & run)
        r = e_se - ego_length / 2.0
        cand = live & e_on & (e_se > s)
        slack = _least(slack, _rel(r, best_r), cand & run)
        take = cand & (r < best_r)
        best_r, best_u, lead = np.where(take, r, best_r), np.where(take, e_ue, best_u), np.where(take, EGO, lead)
        T = 0 if stops is None else np.asarray(stops).shape[1]
        b2, vv = 2.0 * a_brk, v * v
        for t in range(T):
            pf, ss, sf = (np.asarray(stops, dtype=np.float64)[:, t, i][:, None] for i in range(3))
            n_sig = phase.shape[1]
            ok = (sf >= 0.0) & (sf <= float(n_sig - 1))
            slot = np.where(ok, sf, 0.0).astype(np.int64)
            ok = ok & (slot.astype(np.float64) == sf)
            ph = np.take_along_axis(np.asarray(phase), slot, axis=1)
            mine = live & ok & (pf == path.astype(np.float64))
            before = mine & (front <= ss)
            room = (ss - front) * b2
            binds = before & ((ph == RED) | ((ph == YELLOW) & (room >= vv)))
            lit = mine & ((ph == RED) | (ph == YELLOW))
            slack = _least(slack, _rel(front, ss), lit & run)
            slack = _least(slack, _rel(room, vv), before & (ph == YELLOW) & run)
            slack = _least(slack, _rel(ss, best_r), binds & run)
            take = binds & (ss < best_r)
            best_r, best_u, lead = np.where(take, ss, best_r), np.where(take, 0.0, best_u), np.where(take, EGO + 1 + t, lead)
        # ---- the law ----
        f = v / a_des
        f2 = f * f
        f4 = f2 * f2
        free = 1.0 - f4
        led = lead >= 0
        gap = np.where(led, best_r - front, INF)
        ab = a_acc * a_brk
        den = 2.0 * np.sqrt(ab)
        t0 = v * a_head
        dv = v - best_u
        t1 = v * dv
        t2 = t1 / den
        dyn = t0 + t2
        star = jam + np.where(dyn > 0.0, dyn, 0.0)
        g = np.where(gap > gap_min, gap, gap_min)
        ratio = star / g
        inter = np.where(led, ratio * ratio, 0.0)
        acc = a_acc * (free - inter)
        hard = live & (acc < -brake_max)
        slack = _least(slack, _rel(acc, -brake_max), live & run)
        acc = np.where(acc < -brake_max, -brake_max, acc)
        acc = np.where(acc > a_acc, a_acc, acc)
        dvv = acc * dt
        v1 = v + dvv
        nv = np.where(v1 > 0.0, v1, 0.0)
        ds = nv * dt
        ns = s + ds
        mylen = plength[si, path]
        arrive = live & (ns >= mylen)
        slack = _least(slack, _rel(ns, mylen), live & run)
        by_ego = live & (lead == EGO)
        over = live & led & (lead < EGO) & (gap < 0.0)
        slack = _least(slack, _rel(best_r, front), live & led & (lead < EGO) & run)
        mg = np.where(by_ego & ~np.isnan(gap), gap, INF).min(axis=1)
    stays = live & ~arrive
    new = {k: x.copy() for k, x in st.items()}
    new["ticks"] = (st["ticks"] + 1).astype(np.int32)
    new["have"] = np.ones(S, dtype=np.int32)
    new["arrived"] = (st["arrived"] + arrive.sum(axis=1)).astype(np.int32)
    new["ego_yields"] = (st["ego_yields"] + by_ego.sum(axis=1)).astype(np.int32)
    new["ego_hard"] = (st["ego_hard"] + (by_ego & hard).sum(axis=1)).astype(np.int32)
    new["overlaps"] = (st["overlaps"] + over.sum(axis=1)).astype(np.int32)
    new["min_ego_gap"] = np.where(mg < st["min_ego_gap"], mg, st["min_ego_gap"])
    new["se_prev"], new["on_prev"] = se, on.astype(np.int32)
    new["s"], new["v"] = np.where(live, ns, s), np.where(live, nv, v)
    new["alive"] = stays.astype(np.int32)
    leader = np.where(live, lead, -1).astype(np.int32)
    boxes, near = boxes_of(paths, pl, cum, heading, agents, path, stays, new["s"], new["v"])
    slack = min(slack, _least(INF, near) if not held.all() else INF)
    # frozen scenes: the state as it was found, the boxes of that state, no leader
    boxes_held, _ = boxes_of(paths, pl, cum, heading, agents, path, live, s, v)
    for k in new:
        new[k] = np.where(held.reshape((S,) + (1,) * (new[k].ndim - 1)), state[k], new[k]).astype(new[k].dtype)
    boxes = np.where(held[:, None, None], boxes_held, boxes)
    leader = np.where(held[:, None], -2, leader).astype(np.int32)
    return dict(state=new, boxes=boxes, leader=leader, slack=slack, acc=acc, gap=gap, hard=hard, ue=ue, on=on)


# ---- one straight path and a handful of agents: the hand-derived scenarios ------------------------------------------------------

def straight(length=2000.0, points=3, S=1, Q=1, y=0.0):
    """paths [S, Q, points, 2] along +x from the origin, evenly spaced, path q at y + 10 q; plen; cum; heading."""
    x = np.linspace(0.0, length, points)
    paths = np.zeros((S, Q, points, 2))
    paths[..., 0] = x
    paths[..., 1] = y + 10.0 * np.arange(Q)[None, :, None]
    cum, heading = path_tables(paths)
    return paths, np.full((S, Q), points, dtype=np.int32), cum, heading


def agent(path=0.0, s=0.0, v=0.0, desired=8.0, length=LENGTH, width=WIDTH, headway=HEADWAY, accel=ACCEL, brake=BRAKE):
    return [path, s, v, desired, length, width, headway, accel, brake]


class Drive:
    """A scene stepped by the restatement, with the outputs of every step kept."""

    def __init__(self, tables, agents, dt, stops=None, **cfg):
        self.tables, self.agents, self.dt = tables, np.asarray(agents, dtype=np.float64), dt
        self.stops = None if stops is None else np.asarray(stops, dtype=np.float64)
        self.cfg = dict(CFG, **cfg)
        S, N = self.agents.shape[:2]
        self.state, self.boxes, _ = reset(fresh_state(S, N), *tables, self.agents)
        self.out, self.slack = None, INF

    def step(self, pose=None, phase=None, hold=None):
        S = self.agents.shape[0]
        pose = np.full((S, 3), 1e6) if pose is None else np.asarray(pose, dtype=np.float64)      # nowhere near a path
        self.out = step(self.state, *self.tables, self.agents, self.stops, phase, pose, hold, dt=self.dt, **self.cfg)
        self.state, self.boxes = self.out["state"], self.out["boxes"]
        self.slack = min(self.slack, self.out["slack"])
        return self.out


# ---- the hand-derived scenarios as scripts: tests/test_traffic_cpu.py derives their outcomes, tests/test_gpu_traffic.py steps the
# ---- device through every one of them beside `Drive` ----------------------------------------------------------------------------

HALF = LENGTH / 2.0
G_STAR = (CFG["jam"] + 6.0 * HEADWAY) / np.sqrt(1.0 - 0.6 ** 4)          # the gap at which a follower (desired 10) holds 6 m/s


def _script(tables, agents, dt, ticks, stops=None, n_signals=0, pose=None, phase=None, hold=None):
    """A scenario: the inputs of `Drive` and, per tick, (pose, phase, hold): a tuple holds one value per tick, anything else is
    the value of every tick."""
    def per_tick(v, dtype):
        if v is None:
            return [None] * ticks
        v = [np.asarray(x, dtype=dtype) for x in v] if isinstance(v, tuple) else [np.asarray(v, dtype=dtype)] * ticks
        assert len(v) == ticks
        return v
    return dict(tables=tables, agents=np.asarray(agents, dtype=np.float64), dt=dt, ticks=ticks,
                stops=None if stops is None else np.asarray(stops, dtype=np.float64), n_signals=n_signals,
                pose=per_tick(pose, np.float64), phase=per_tick(phase, np.int32), hold=per_tick(hold, np.int32))


def scenario_free_road(dt=0.5, seconds=200.0):
    """Four scenes: an agent from rest; one at exactly its desired speed; a follower at the closed-form gap behind a free leader
    that holds its own desired 6 m/s; the same follower started 5 m short of that gap and 2 m/s fast."""
    ag = np.zeros((4, 2, 9))
    ag[0, 0] = agent(s=0.0, v=0.0, desired=8.0)
    ag[1, 0] = agent(s=0.0, v=8.0, desired=8.0)
    ag[2, 0], ag[2, 1] = agent(s=100.0 + G_STAR + LENGTH, v=6.0, desired=6.0), agent(s=100.0, v=6.0, desired=10.0)
    ag[3, 0], ag[3, 1] = agent(s=100.0 + G_STAR - 5.0 + LENGTH, v=6.0, desired=6.0), agent(s=100.0, v=8.0, desired=10.0)
    return _script(straight(S=4), ag, dt, int(round(seconds / dt)))


def scenario_yellow(ticks=600):
    """Two agents at 10 m/s before a yellow line at 300 m, v^2 / (2 brake) = 25 m: agent 0's front is 10 m before it, agent 1's 80 m."""
    s_stop = 300.0
    return _script(straight(), [[agent(s=s_stop - 10.0 - HALF, v=10.0, desired=10.0), agent(s=s_stop - 80.0 - HALF, v=10.0, desired=10.0)]], 0.1,
                   ticks, stops=[[[0.0, s_stop, 0.0]]], n_signals=1, phase=[[YELLOW]])


def scenario_ego_rate():
    """The ego ahead of one agent: forward, forward, backward, off the path, on again twice, and a NaN pose."""
    x = [40.0, 42.5, 45.0, 44.0, 44.0, 46.0, 48.0, np.nan]
    y = [0.0, 0.0, 0.0, 0.0, 5.0, 0.0, 0.0, 0.0]
    return _script(straight(), [[agent(s=10.0, v=5.0, desired=10.0)]], 0.5, len(x), pose=tuple([[x[k], y[k], 0.0]] for k in range(len(x))))


def scenario_arrival_hold():
    """Two scenes of two agents on a 100 m path, the front one 10 m before its end at 8 m/s; scene 1 is held for three ticks."""
    return _script(straight(length=100.0, S=2), [[agent(s=90.0, v=8.0), agent(s=20.0, v=8.0)]] * 2, 0.5, 4, hold=([0, 1], [0, 1], [0, 1], [0, 0]))


def empty_slot_rows():
    """One agent and, behind it, every kind of empty slot (with path 1 of the scene empty)."""
    ok = agent(s=10.0, v=3.0)
    rows = [ok]
    for col, values in ((0, (-1.0, 0.5, 2.0, np.nan, 1.0)),            # no integer in 0..Q-1; path 1 is empty (one point)
                        (1, (-0.5, np.nan, 2000.0, 2500.0)),           # a negative, NaN or too large start
                        (2, (-1.0, np.nan)), (3, (0.0, -2.0, np.nan)), (4, (0.0, np.nan)), (5, (0.0, -1.0)), (6, (-0.1, np.nan)),
                        (7, (0.0, np.nan)), (8, (0.0, -3.0))):
        for v in values:
            rows.append(list(ok))
            rows[-1][col] = v
    return rows


def scenario_empty_slots():
    paths, plen, cum, heading = straight(Q=2)
    plen[0, 1] = 1
    return _script((paths, plen, cum, heading), [empty_slot_rows()], 0.1, 3)


def scenario_equal_s():
    """Agents 0 and 1 at the same arc length; agent 2 is 30 m long, so its rear (65) is nearer than agent 3's (67.75)."""
    return _script(straight(), [[agent(s=50.0, v=5.0), agent(s=50.0, v=5.0), agent(s=80.0, v=5.0, length=30.0), agent(s=70.0, v=5.0)]], 0.1, 3)


def scenario_kind_ties():
    """Candidates of different kinds with EQUAL rear positions, 67.75 m: agent 1 (s = 70), the parked ego (se = 70, its rear
    4.5 / 2 behind) and a red stop.  Scene 0 holds all three, scene 1 the ego and the stop, scene 2 the stop alone: the earlier kind
    wins, so agent 0 follows agent 1, then the ego (64), then the stop (65)."""
    ag = np.zeros((3, 2, 9))
    ag[:, 0] = agent(s=50.0, v=5.0)
    ag[0, 1] = agent(s=70.0, v=0.0)
    return _script(straight(S=3), ag, 0.1, 2, stops=[[[0.0, 70.0 - HALF, 0.0]]] * 3, n_signals=1, phase=[[RED]] * 3,
                   pose=[[70.0, 0.0, 0.0], [70.0, 0.0, 0.0], [1e6, 0.0, 0.0]])


def scenario_queue64(ticks=1200):
    """A full wave: 64 agents 8 m apart on ONE path of 64 points (a quarter circle of radius 400 m), a red line 20 m before its end."""
    G = N = 64
    paths = np.zeros((1, 1, G, 2))
    ang = np.linspace(0.0, 1.5, G)
    paths[0, 0] = 400.0 * np.stack([np.sin(ang), 1.0 - np.cos(ang)], axis=1)
    cum, heading = path_tables(paths)
    ag = np.zeros((1, N, 9))
    for i in range(N):
        ag[0, i] = agent(s=8.0 * (N - 1 - i), v=6.0, desired=9.0)               # agent 0 in front
    return _script((paths, np.full((1, 1), G, dtype=np.int32), cum, heading), ag, 0.25, ticks,
                   stops=[[[0.0, float(cum[0, 0, -1]) - 20.0, 0.0]]], n_signals=1, phase=[[RED]])


def play(sc, upto=None):
    """`Drive` over a scenario's script: (drive, the outputs of every tick)."""
    d = Drive(sc["tables"], sc["agents"], sc["dt"], stops=sc["stops"])
    outs = [d.step(pose=sc["pose"][t], phase=sc["phase"][t], hold=sc["hold"][t]) for t in range(sc["ticks"] if upto is None else upto)]
    return d, outs


# ---- the random drives the device is compared on --------------------------------------------------------------------------------

CASES =((1, 1, 1, 2, 0), (3, 5, 2, 7, 3), (65, 64, 8, 64, 16), (2, 33, 3, 33, 1))
STEPS = 6
FREE = (5, 12, 3, 9, 4, 40)


def random_drive(S, N, Q, G, T, steps, seed=0, dt=0.25):
    """Paths that wander from random origins with segments of 4..9 m, some shortened and one in eight empty; agents at random arc
    lengths and speeds on random paths, one in nine an empty slot of some kind; stops at random arc lengths on random signal
    slots of 6, their phases redrawn at every step (any of 0..4); an ego that walks along path 0 of each scene at 0..1.5 m to its
    side (so that it is on the path in most steps) and jumps away now and then; a hold on one scene in seven per step."""
    rng = np.random.default_rng([seed, S, N, Q, G, T])
    seg = rng.uniform(4.0, 9.0, (S, Q, G))
    turn = np.cumsum(rng.uniform(-0.08, 0.08, (S, Q, G)), axis=2) + rng.uniform(-3.0, 3.0, (S, Q, 1))
    step_xy = seg[..., None] * np.stack([np.cos(turn), np.sin(turn)], axis=-1)
    paths = rng.uniform(-100.0, 100.0, (S, Q, 1, 2)) + np.cumsum(step_xy, axis=2) - step_xy[:, :, :1]
    plen = np.where(rng.random((S, Q)) < 0.3, rng.integers(2, G + 1, (S, Q)), G).astype(np.int32)
    plen[rng.random((S, Q)) < 0.125] = rng.integers(0, 2)
    plen[0, 0] = G
    cum, heading = path_tables(paths)
    length = np.take_along_axis(cum, np.maximum(plen - 1, 0)[..., None].astype(np.int64), axis=2)[..., 0]
    path = rng.integers(0, Q, (S, N))
    agents = np.zeros((S, N, 9))
    agents[..., 0] = path
    agents[..., 1] = rng.uniform(0.0, 0.98, (S, N)) * np.take_along_axis(length, path, axis=1)
    agents[..., 2] = rng.uniform(0.0, 12.0, (S, N)) * (rng.random((S, N)) < 0.8)
    agents[..., 3] = rng.uniform(4.0, 14.0, (S, N))
    agents[..., 4], agents[..., 5] = rng.uniform(3.5, 6.0, (S, N)), rng.uniform(1.6, 2.4, (S, N))
    agents[..., 6] = rng.uniform(0.8, 2.0, (S, N))
    agents[..., 7], agents[..., 8] = rng.uniform(1.0, 2.5, (S, N)), rng.uniform(1.5, 3.0, (S, N))
    bad = rng.random((S, N)) < 1.0 / 9.0
    kind = rng.integers(0, 9, (S, N))
    poison = np.array([-1.0, 0.5, float(Q), np.nan])[rng.integers(0, 4, (S, N))]
    for col in range(9):
        value = poison if col == 0 else (np.where(rng.random((S, N)) < 0.5, np.nan, -1.0) if col in (1, 2, 6) else
                                         np.where(rng.random((S, N)) < 0.5, 0.0, np.nan))
        agents[..., col] = np.where(bad & (kind == col), value, agents[..., col])
    stops = None
    phases = [None] * steps
    n_sig = 6
    if T:
        sp = rng.integers(0, Q, (S, T))
        stops = np.zeros((S, T, 3))
        stops[..., 0] = sp
        stops[..., 1] = rng.uniform(0.05, 1.0, (S, T)) * np.take_along_axis(length, sp, axis=1)
        stops[..., 2] = rng.integers(0, n_sig, (S, T))
        stops[..., 2] = np.where(rng.random((S, T)) < 0.1, np.array([-1.0, 2.5, float(n_sig), np.nan])[rng.integers(0, 4, (S, T))], stops[..., 2])
        phases = [rng.integers(0, 5, (S, n_sig)).astype(np.int32) for _ in range(steps)]
    # the ego: along path 0, advancing 0..3 m a step from a random arc length
    poses, holds = [], []
    along = rng.uniform(0.0, 0.5, S) * length[:, 0]
    for t in range(steps):
        along = along + rng.uniform(0.0, 3.0, S)
        side = rng.uniform(-1.5, 1.5, S)
        j = np.clip((cum[:, 0] <= along[:, None]).sum(axis=1) - 1, 0, G - 2)
        a, h = paths[np.arange(S), 0, j], heading[np.arange(S), 0, j]
        rest = along - cum[np.arange(S), 0, j]
        xy = a + rest[:, None] * np.stack([np.cos(h), np.sin(h)], axis=1) + side[:, None] * np.stack([-np.sin(h), np.cos(h)], axis=1)
        away = rng.random(S) < 0.15
        xy = np.where(away[:, None], xy + rng.uniform(30.0, 60.0, (S, 2)), xy)
        poses.append(np.concatenate([xy, rng.uniform(-3.0, 3.0, (S, 1))], axis=1))
        holds.append((rng.random(S) < 1.0 / 7.0).astype(np.int32))
    cfg = dict(CFG, dt=dt)
    return dict(paths=paths, plen=plen, cum=cum, heading=heading, agents=agents, stops=stops, phases=phases, n_signals=n_sig if T else 0,
                poses=poses, holds=holds, velocities=[rng.uniform(0.0, 10.0, S).astype(np.float32) for _ in range(steps)], cfg=cfg)


def run(d, steps=None):
    """Free-running: every step from the step before.  Returns the list of `step` outputs."""
    S, N = d["agents"].shape[:2]
    state, outs = fresh_state(S, N), []
    for t in range(len(d["poses"]) if steps is None else steps):
        outs.append(step(state, d["paths"], d["plen"], d["cum"], d["heading"], d["agents"], d["stops"], d["phases"][t], d["poses"][t],
                         d["holds"][t], **d["cfg"]))
        state = outs[-1]["state"]
    return outs


# ---- the closed loop's discriminating scenario (tests/test_gpu_closed_loop_traffic.py) ----------------------------------------------

FOLLOW = dict(dt=0.25, ticks=60, line=12.0, halt=6.0, behind=14.0, speed=8.0, back=40.0, spacing=2.5, points=64,
              origin=((10.0, -5.0), (-40.0, 25.0)), heading=(0.3, -1.0))


def follow_scenario():
    """Two scenes, each a straight road: the ego's route of 60 points 2 m apart from `origin` along `heading`, and ONE traffic path
    on the same line that begins `back` metres behind the origin (64 points 2.5 m apart), so that an agent can start `behind`
    metres behind the ego at `speed` m/s.  A permanently red light lies `line` metres down the route (a stop of the path at the
    same place); the ego's plan is pinned onto the route until it is `halt` metres down it and onto its own position from then
    on, so it drives up to the light's plane and stands.  Arm A: the agent is `Traffic`'s.  Arm B: the same agent as a plain box
    of `World(boxes=)` that keeps its start velocity.  Returns a dict of what both tests build from."""
    f = FOLLOW
    origin, heading = np.array(f["origin"]), np.array(f["heading"])
    unit = np.stack([np.cos(heading), np.sin(heading)], axis=1)                                    # [S, 2]
    route = origin[:, None] + unit[:, None] * (2.0 * np.arange(60))[None, :, None]
    paths = (origin[:, None] + unit[:, None] * (f["spacing"] * np.arange(f["points"]) - f["back"])[None, :, None])[:, None]
    pose = np.concatenate([origin, np.arctan2(unit[:, 0], -unit[:, 1])[:, None]], axis=1)          # forward = (sin c, -cos c) = unit
    agents = np.array([[agent(s=f["back"] - f["behind"], v=f["speed"], desired=f["speed"])]] * 2)
    start = origin - f["behind"] * unit
    boxes = np.concatenate([start, f["speed"] * unit, heading[:, None], np.full((2, 1), LENGTH), np.full((2, 1), WIDTH)], axis=1)[:, None]
    stops = np.array([[[0.0, f["back"] + f["line"], 0.0]]] * 2)
    return dict(route=route, paths=paths, plen=np.full((2, 1), f["points"], dtype=np.int32), pose=pose, agents=agents, boxes=boxes,
                stops=stops, unit=unit, origin=origin, heading=heading, line_centre=origin + f["line"] * unit)
