"""fp64 NumPy restatement of "signals v1" (include/adx.h: adx_signals_step, adx_signals_reset), written from the contract's text
one operation per line in the contract's order: the geometry, the phases and the crossings for every slot at once (they are
independent), the stop sign machine and the emission one scene at a time.  The ego planes and their bound are `nav_ref`'s
("ego frame v1", kind 2).  Beside it: the hand-built scenarios whose records are known in closed form, and the random drives the
device is compared on.

Decisions.  Every comparison of the contract is made on numbers that both sides form by the same single IEEE operations on the
same inputs (fmod included: it is exact), except those whose operands pass through cos or sin of the compass: `head - min_cos`
and, with probe != 0, `l0`, `l1`, `mc` and `mc - L`.  `step` returns in `slack` the smallest distance of any of these from its
threshold over the live slots of every scene; two evaluations whose cos and sin differ by 5 ulp differ in these operands by less
than 1e-12 at coordinates within +-300 m (nav_ref's bound of a rotated vector: 8 * 2^-52 * 600, times |probe|), so a drive whose
slack stays above 1e-9 has the same verdicts on both sides.
"""
import numpy as np

import nav_ref

INTS = ("ticks", "have", "target", "stop_done", "red_runs", "stop_runs", "stops_met", "first_tick", "first_slot", "emitted", "flags", "pad")
F64 = ("qx", "qy")
WORDS = 16
LIGHT, STOP = 1.0, 2.0
EMPTY, GREEN, YELLOW, RED, SIGN = 0, 1, 2, 3, 4
INERT = (0.0, 0.0, 1.0)
CFG = dict(dt=0.5, xy_scale=23.315, planes=4, margin=3.0, probe=-2.0, min_cos=0.0, stop_on_yellow=False, speed_threshold=0.1)
E52 = 2.0 ** -52


def fresh_state(S):
    st = {k: np.zeros(S, dtype=np.int32) for k in INTS}
    st.update({k: np.zeros(S, dtype=np.float64) for k in F64})
    return st


def pack_state(st):
    """int32 [S, 16]: the contract's record."""
    S = len(st["ticks"])
    w = np.zeros((S, WORDS), dtype=np.int32)
    for i, k in enumerate(INTS):
        w[:, i] = st[k]
    w.view(np.float64)[:, 6] = st["qx"]
    w.view(np.float64)[:, 7] = st["qy"]
    return w


def unpack_state(words):
    w = np.ascontiguousarray(words, dtype=np.int32)
    st = {k: w[:, i].copy() for i, k in enumerate(INTS)}
    st["qx"], st["qy"] = w.view(np.float64)[:, 6].copy(), w.view(np.float64)[:, 7].copy()
    return st


def from_lines(centre, yaw, width, kind, reach, timing):
    """records [..., 10] from a centre [..., 2], the governed traffic's world heading, a width, a kind, a reach and
    timing [..., 4] = (offset, green, yellow, red): A = c - w/2 (sin yaw, -cos yaw), B = c + w/2 (sin yaw, -cos yaw)."""
    centre, timing = np.asarray(centre, dtype=np.float64), np.asarray(timing, dtype=np.float64)
    yaw, width = np.asarray(yaw, dtype=np.float64), np.asarray(width, dtype=np.float64)
    hx, hy = width / 2.0 * np.sin(yaw), width / 2.0 * -np.cos(yaw)
    rec = np.zeros(np.broadcast(centre[..., 0], yaw, width).shape + (10,))
    rec[..., 0], rec[..., 1] = centre[..., 0] - hx, centre[..., 1] - hy
    rec[..., 2], rec[..., 3] = centre[..., 0] + hx, centre[..., 1] + hy
    rec[..., 4], rec[..., 5] = kind, reach
    rec[..., 6:10] = timing
    return rec


def step(state, signals, pose, velocity, hold=None, *, dt, xy_scale, planes, margin, probe, min_cos, stop_on_yellow, speed_threshold):
    """One launch of adx_signals_step.  signals [S, N, 10] fp64, pose [S, 3] fp64, velocity [S] fp32, hold [S] or None; `state` is
    not modified.  Returns dict(state, planes fp32 [S, P, 3], planes_bound, phase int32 [S, N], slack, emit bool [S, N],
    red [S] (runs of this step), ran [S], completed [S] (stop-sign targets left with and without their stop), overflow [S])."""
    sig, pose = np.asarray(signals, dtype=np.float64), np.asarray(pose, dtype=np.float64)
    S, N, _ = sig.shape
    P = int(planes)
    vel = np.asarray(velocity, dtype=np.float32).astype(np.float64)
    held = np.zeros(S, dtype=bool) if hold is None else np.asarray(hold) != 0
    ax, ay, bx, by, kind, reach, offset, green, yellow, red = (sig[..., i] for i in range(10))
    with np.errstate(invalid="ignore", divide="ignore"):
        # ---- slots ----
        dx, dy = bx - ax, by - ay
        dxx, dyy = dx * dx, dy * dy
        L = np.sqrt(dxx + dyy)
        gy = green + yellow
        cycle = gy + red
        is_light, is_stop = kind == LIGHT, kind == STOP
        timed = (green >= 0.0) & (yellow >= 0.0) & (red >= 0.0) & (cycle > 0.0)
        live = (is_light | is_stop) & (L > 0.0) & (reach > 0.0) & (is_stop | timed)
        tx, ty = dx / L, dy / L
        nx, ny = -ty, tx
        # ---- the ego ----
        px, py, c, s = (v[:, None] for v in nav_ref.frame(pose))
        fx, fy = -c, -s
        rx, ry = px - ax, py - ay
        o0, o1 = nx * rx, ny * ry
        lon = o0 + o1
        a0, a1 = tx * rx, ty * ry
        lat = a0 + a1
        h0, h1 = nx * fx, ny * fy
        head = h0 + h1
        inside = (lat >= 0.0) & (lat <= L)
        gate = live & (lon <= 0.0) & (lon >= -reach) & inside & (head > min_cos)
        beyond = live & (lon > 0.0) & inside
        # ---- the clock ----
        have = state["have"] != 0
        ticks = np.where(have, state["ticks"] + 1, 0).astype(np.int32)
        tm = (ticks.astype(np.float64) * dt)[:, None]
        tau = np.fmod(tm + offset, cycle)
        tau = np.where(tau < 0.0, tau + cycle, tau)
        phase = np.where(tau < green, GREEN, np.where(tau < gy, YELLOW, RED))
        phase = np.where(live, np.where(is_stop, SIGN, phase), EMPTY).astype(np.int32)
        # ---- the red-light run ----
        e0, e1 = probe * fx, probe * fy
        qx, qy = px + e0, py + e1
        sx, sy = state["qx"][:, None] - ax, state["qy"][:, None] - ay
        p0, p1 = nx * sx, ny * sy
        l0 = p0 + p1
        ux, uy = qx - ax, qy - ay
        r0, r1 = nx * ux, ny * uy
        l1 = r0 + r1
        cross = have[:, None] & live & (l0 <= 0.0) & (l1 > 0.0)
        u = l0 / (l0 - l1)
        m00, m01 = tx * sx, ty * sy
        m0 = m00 + m01
        m10, m11 = tx * ux, ty * uy
        m1 = m10 + m11
        du = u * (m1 - m0)
        mc = m0 + du
        hit = cross & (mc >= 0.0) & (mc <= L)
        run = hit & (phase == RED)
    slack = np.inf
    if live.any():
        terms = [np.abs(head - min_cos)[live]]
        if probe != 0.0:
            lv = live & have[:, None]
            terms += [np.abs(l0)[lv], np.abs(l1)[lv], np.abs(mc)[cross], np.abs(mc - L)[cross]]
        slack = min([float(t.min()) for t in terms if t.size] + [np.inf])

    # ---- the world planes of every slot, then ego frame v1 kind 2 ----
    with np.errstate(invalid="ignore"):
        w0, w1 = nx * ax, ny * ay
        world = np.stack([nx, ny, (w0 + w1) - margin], axis=-1)
    ego, ego_bound = nav_ref.world_to_ego(nav_ref.PLANES, np.where(live[..., None], world, 0.0), pose, xy_scale)

    new = {k: v.copy() for k, v in state.items()}
    out_planes = np.tile(np.array(INERT, dtype=np.float32), (S, P, 1))
    out_bound = np.zeros((S, P, 3))
    emit = np.zeros((S, N), dtype=bool)
    red_now, ran, completed, overflow = (np.zeros(S, dtype=np.int32) for _ in range(4))
    for sc in range(S):
        if held[sc]:
            continue
        st = {k: state[k][sc] for k in state}
        red_runs = int(st["red_runs"]) + int(run[sc].sum())
        red_now[sc] = int(run[sc].sum())
        # ---- the stop sign machine ----
        target, stop_done = int(st["target"]), int(st["stop_done"])
        stop_runs, stops_met = int(st["stop_runs"]), int(st["stops_met"])
        gated_stop = gate[sc] & is_stop[sc]
        stop_slot = -1
        if target == 0:
            if gated_stop.any():
                target = int(np.argmax(gated_stop)) + 1
                stop_done = 0
                stops_met += 1
        else:
            if vel[sc] < speed_threshold:
                stop_done = 1
            j = target - 1
            if not (j < N and gate[sc, j]):
                if j < N and beyond[sc, j] and not stop_done:
                    stop_runs += 1
                    stop_slot = j
                    ran[sc] = 1
                elif j < N and beyond[sc, j]:
                    completed[sc] = 1
                target = 0
        # ---- the first infraction ----
        first_tick, first_slot = int(st["first_tick"]), int(st["first_slot"])
        if int(st["red_runs"]) + int(st["stop_runs"]) == 0:
            if run[sc].any():
                first_tick, first_slot = int(ticks[sc]), int(np.argmax(run[sc]))
            elif stop_slot >= 0:
                first_tick, first_slot = int(ticks[sc]), stop_slot
        # ---- emission ----
        lights = gate[sc] & is_light[sc] & ((phase[sc] == RED) | ((phase[sc] == YELLOW) & bool(stop_on_yellow)))
        signs = gated_stop & ~((np.arange(N) == target - 1) & (stop_done != 0))
        emit[sc] = lights | signs
        slots = np.flatnonzero(emit[sc])
        flags = int(st["flags"])
        if len(slots) > P:
            flags |= 1
            overflow[sc] = 1
            slots = slots[:P]
        out_planes[sc, :len(slots)] = ego[sc, slots]
        out_bound[sc, :len(slots)] = ego_bound[sc, slots]
        vals = dict(ticks=ticks[sc], have=1, target=target, stop_done=stop_done, red_runs=red_runs, stop_runs=stop_runs,
                    stops_met=stops_met, first_tick=first_tick, first_slot=first_slot, emitted=len(slots), flags=flags, pad=0,
                    qx=qx[sc, 0], qy=qy[sc, 0])
        for k, v in vals.items():
            new[k][sc] = v
    emit[held] = False
    return dict(state=new, planes=out_planes, planes_bound=out_bound, phase=phase, slack=slack, emit=emit, red=red_now, ran=ran,
                completed=completed, overflow=overflow)


def reset(state, mask=None):
    new = {k: v.copy() for k, v in state.items()}
    m = np.ones(len(state["ticks"]), dtype=bool) if mask is None else np.asarray(mask) != 0
    for k in new:
        new[k][m] = 0
    return new


def run(signals, poses, velocities, holds=None, state=None, **cfg):
    """Every step of a drive: poses [T, S, 3], velocities [T, S], holds [T, S] or None -> the list of `step` results."""
    S = np.asarray(signals).shape[0]
    state = fresh_state(S) if state is None else state
    outs = []
    for t in range(len(poses)):
        outs.append(step(state, signals, poses[t], velocities[t], None if holds is None else holds[t], **cfg))
        state = outs[-1]["state"]
    return outs


# ---- the scenarios with records known in closed form -----------------------------------------------------------------------------
def straight_drive(T, speed=3.0, y=0.0):
    """The ego at compass pi/2 (forward is +x) at x_k = 0.125 + 1.5 k: poses [T, 1, 3], velocities [T, 1] fp32."""
    k = np.arange(T, dtype=np.float64)
    poses = np.stack([0.125 + 1.5 * k, np.full(T, y), np.full(T, np.pi / 2.0)], axis=1)[:, None]
    return poses, np.full((T, 1), speed, dtype=np.float32)


def scenario_a():
    """Four lights of width 4: a timed one at x = 12, an always green one at x = 24, an always red one at x = 18 in another
    lane, an always red one at x = 30 that faces the other way."""
    rec = np.zeros((1, 4, 10))
    rec[0, 0] = from_lines([12.0, 0.0], 0.0, 4.0, LIGHT, 20.0, [0.0, 2.0, 1.0, 5.0])
    rec[0, 1] = from_lines([24.0, 0.0], 0.0, 4.0, LIGHT, 20.0, [0.0, 1.0, 0.0, 0.0])
    rec[0, 2] = [18.0, 10.0, 18.0, 6.0, LIGHT, 20.0, 0.0, 0.0, 0.0, 1.0]
    rec[0, 3] = from_lines([30.0, 0.0], np.pi, 4.0, LIGHT, 20.0, [0.0, 0.0, 0.0, 1.0])
    return rec, straight_drive(24)


def scenario_b(stop_at=None):
    """A stop sign at x = 12 with reach 10; `stop_at`: the step at which the reported velocity is 0.0."""
    rec = from_lines([12.0, 0.0], 0.0, 4.0, STOP, 10.0, [0.0, 0.0, 0.0, 0.0])[None, None]
    poses, vel = straight_drive(12)
    if stop_at is not None:
        vel[stop_at] = 0.0
    return rec, (poses, vel)


# ---- the random drives -----------------------------------------------------------------------------------------------------------
CASES = ((1, 1, 1), (3, 5, 3), (65, 64, 8), (2, 33, 2))      # (S, N, P) of the step-by-step comparison, 8 steps each
STEPS = 8
FREE = (5, 12, 3, 24)                                         # (S, N, P, T) of the free-running drive
EMPTY_KINDS = 6


def random_drive(S, N, P, T, seed=0):
    """dict(signals [S, N, 10], poses [T, S, 3], velocities [T, S] fp32, holds [T, S] int32, cfg): an ego per scene that drives
    2 to 3 m per step along a gently turning path from a start within +-200 m, and N lines across the path within the distance it
    covers: lights (a third of them always red) and stop signs, every fifth slot empty in one of the contract's ways.  The
    reported velocity is 0 on every seventh step (scene-shifted), which is what completes a stop; scene s with s % 5 == 3 is held
    from step 4 on.  Everything stays within +-300 m."""
    rng = np.random.default_rng([17, S, N, P, T, seed])
    cfg = dict(CFG, planes=P, stop_on_yellow=bool(seed % 2))
    start = rng.uniform(-200.0, 200.0, (S, 2))
    yaw0 = rng.uniform(-np.pi, np.pi, S)                                   # the world angle of the heading
    stride = rng.uniform(2.0, 3.0, (T, S))
    yaw = yaw0[None] + np.cumsum(rng.uniform(-0.02, 0.02, (T, S)), axis=0)
    xy = start[None] + np.cumsum(stride[..., None] * np.stack([np.cos(yaw), np.sin(yaw)], axis=-1), axis=0)
    # forward = (sin compass, -cos compass) = (cos yaw, sin yaw): compass = yaw + pi/2
    poses = np.concatenate([xy, (yaw + np.pi / 2.0)[..., None]], axis=-1)
    velocities = (stride / cfg["dt"]).astype(np.float32)
    velocities[(np.arange(T)[:, None] + np.arange(S)[None]) % 7 == 3] = 0.0
    holds = ((np.arange(S)[None] % 5 == 3) & (np.arange(T)[:, None] >= 4)).astype(np.int32)
    # lines across the straight continuation of the start heading
    dist = rng.uniform(1.0, 2.4 * T, (S, N))
    along = np.stack([np.cos(yaw0), np.sin(yaw0)], axis=-1)[:, None]
    across = np.stack([-np.sin(yaw0), np.cos(yaw0)], axis=-1)[:, None]
    centre = start[:, None] + dist[..., None] * along + rng.uniform(-1.0, 1.0, (S, N, 1)) * across
    line_yaw = yaw0[:, None] + rng.uniform(-0.3, 0.3, (S, N))
    kind = np.where(rng.uniform(size=(S, N)) < 0.6, LIGHT, STOP)
    timing = np.stack([rng.uniform(-5.0, 5.0, (S, N)), rng.uniform(0.5, 3.0, (S, N)), rng.uniform(0.0, 1.5, (S, N)),
                       rng.uniform(0.5, 4.0, (S, N))], axis=-1)
    always_red = rng.uniform(size=(S, N)) < 1.0 / 3.0
    timing[always_red, 1:3] = 0.0
    sig = from_lines(centre, line_yaw, rng.uniform(6.0, 12.0, (S, N)), kind, rng.uniform(4.0, 12.0, (S, N)), timing)
    idx = np.arange(S)[:, None] * N + np.arange(N)[None]
    for v in range(EMPTY_KINDS):
        m = (idx % 5 == 4) & ((idx // 5) % EMPTY_KINDS == v)
        if v == 0:
            sig[m, 4] = 0.0                    # no kind
        elif v == 1:
            sig[m, 4] = 3.0                    # not a kind
        elif v == 2:
            sig[m, 2:4] = sig[m, 0:2]          # L = 0
        elif v == 3:
            sig[m, 5] = 0.0                    # no reach
        elif v == 4:
            sig[m, 4], sig[m, 8] = LIGHT, -0.5  # a negative time
        else:
            sig[m, 4], sig[m, 7] = LIGHT, np.nan
    return dict(signals=sig, poses=poses, velocities=velocities, holds=holds, cfg=cfg)


def qxy_bound(q, probe):
    """|qx - ref|, |qy - ref| of two evaluations of q = p + probe * forward that differ only in cos and sin, for the restatement's
    q [S, 2]: cos and sin differ by at most 5 * 2^-52 and the product is rounded on both sides, within nav_ref's 8 * 2^-52 times
    |probe|; the sum is rounded on both sides: one ulp of the coordinate."""
    return abs(probe) * nav_ref.C_POINT * E52 + np.spacing(np.abs(np.asarray(q, dtype=np.float64)))
