"""fp64 NumPy restatement of "control v1" (include/adx.h: adx_control_step), the fp32 error bound of a kernel that evaluates it,
the margins of its three decisions, and the 80-tick fixture the CPU and GPU tests share.  Arithmetic only, written from the
contract; the settings are taken as the fp32 numbers the kernel is handed.

    wp[i]     (sign_x xy_scale traj[i][0], xy_scale traj[i][1]), i < W; tgt likewise from target (target_scale), or waypoint W
    desired   sum_i |wp[i+1] - wp[i]| 2 / (W - 1)
    aim       wp[i*], i* = the first arg-min of key_i = |AIM - |(wp[i+1] + wp[i]) / 2|| among key_i < |AIM - 1e5|; none: 0
    heading   degrees(pi/2 - atan2(v.y, v.x)) / 90 of aim (a), wp[W-1] - wp[W-2] (a_last), tgt (a_t)
    to_target |a_t| < |a| or (|a_t - a_last| > ANGLE_THRESH and tgt.y < DIST_THRESH)
    steer     clip(PID_turn(to_target ? a_t : a), -1, 1)
    brake     desired < BRAKE_SPEED or speed / desired > BRAKE_RATIO
    throttle  brake ? 0 : clip(PID_speed(clip(desired - speed, 0, CLIP_DELTA)), 0, MAX_THROTTLE)
    PID(e)    k_p e + k_i mean(last n samples, e included, zeros before the first) + k_d (e - previous); n = 1: k_p e
    post      "agent" / "interact": the two post_process_control variants; source "action": post(traj[0][D-3:])
"""
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32
# ASSUMPTION (not measurable without the device): the accuracy of the device library's single-precision atan2.  ROCm's device
# library documents its maths functions as meeting the OpenCL accuracy requirements, which give atan2 6 ulp.  The bound takes
# twice that, as ulps (2^-23 relative) of the largest result, pi.
ATAN2_ULPS = 6
ATAN2_ERR = 2 * ATAN2_ULPS * 2.0 ** -23 * np.pi
POSTS = ("none", "agent", "interact")


def gamma(n: int) -> float:
    """Higham's gamma_n = n u / (1 - n u): the relative error bound of n chained fp32 roundings."""
    return n * U / (1.0 - n * U)


def f32(v) -> float:
    return float(np.float32(v))


def params(cfg, waypoints=4, post="agent", source="pid", sign_x=-1.0, target_scale=1.0, xy_scale=1.0):
    p, c = cfg.PID, cfg.CONTROL
    return SimpleNamespace(
        W=int(waypoints), post=post, source=source, sign_x=f32(sign_x), target_scale=f32(target_scale), xy_scale=f32(xy_scale),
        n_turn=int(p.TURN_N), n_speed=int(p.SPEED_N),
        turn=(f32(p.TURN_KP), f32(p.TURN_KI), f32(p.TURN_KD)), speed=(f32(p.SPEED_KP), f32(p.SPEED_KI), f32(p.SPEED_KD)),
        aim_dist=f32(c.AIM_DIST), angle_thresh=f32(c.ANGLE_THRESH), dist_thresh=f32(c.DIST_THRESH), brake_speed=f32(c.BRAKE_SPEED),
        brake_ratio=f32(c.BRAKE_RATIO), clip_delta=f32(c.CLIP_DELTA), max_throttle=f32(c.MAX_THROTTLE))


def fresh(p):
    """The state of one scene: the two windows, oldest sample first."""
    return SimpleNamespace(turn=np.zeros(p.n_turn), speed=np.zeros(p.n_speed))


def clip(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)          # a NaN goes through


def heading(v) -> float:
    return float(np.degrees(np.pi / 2 - np.arctan2(v[1], v[0])) / 90.0)


def aim_index(keys, aim_dist) -> int:
    """The contract's rule: first arg-min among the keys strictly below |aim_dist - 1e5|; none (a NaN never qualifies): 0."""
    keys = np.asarray(keys, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = keys < abs(aim_dist - 1e5)
    return int(np.where(ok, keys, np.inf).argmin()) if ok.any() else 0


def aim_index_sequential(norms, aim_dist) -> int:
    """The reference's loop (control/controller.py:39-47): best = 1e5; segment i wins when it is strictly closer to aim_dist."""
    pick, best = 0, 1e5
    for i, norm in enumerate(norms):
        if abs(aim_dist - best) > abs(aim_dist - norm):
            pick, best = i, norm
    return pick


def post_process(post, throttle, steer, brake):
    if post == "none":
        return throttle, steer, brake
    if brake < f32(0.05):
        brake = 0.0
    if throttle > brake:
        brake = 0.0
    if brake > 0.5:
        throttle = 0.0
        if post == "interact":
            brake, steer = 1.0, 0.0
    return throttle, steer, brake


def pid(window, e, gains):
    """Pushes e; returns (output, the new window)."""
    kp, ki, kd = gains
    window = np.append(window[1:], e)
    if window.size < 2:
        return kp * e, window
    with np.errstate(invalid="ignore"):
        return (kp * e + ki * window.mean()) + kd * (e - window[-2]), window


def tick(p, state, traj, speed, target=None):
    """One scene, one tick.  traj [H, D] and target [2] hold fp32 numbers.  Returns (control [3], info); `state` is advanced.
    info: what the margins and the bound need (desired, q = speed / desired, keys, the three angles and their vectors' norms)."""
    t = np.asarray(traj, dtype=np.float64)
    H, D = t.shape
    if p.source == "action":
        return np.array(post_process(p.post, *t[0, D - 3:])), None
    W = p.W

    def scaled(row, scale):
        return np.array([p.sign_x * (scale * row[0]), scale * row[1] if len(row) > 1 else 0.0])

    wp = np.stack([scaled(t[i], p.xy_scale) for i in range(W)])
    tgt = scaled(t[W], p.xy_scale) if target is None else scaled(np.asarray(target, dtype=np.float64), p.target_scale)
    with np.errstate(invalid="ignore", divide="ignore"):
        desired = 0.0
        for i in range(W - 1):
            desired += np.linalg.norm(wp[i + 1] - wp[i]) * 2.0 / (W - 1)
        mids = np.array([np.linalg.norm((wp[i + 1] + wp[i]) / 2.0) for i in range(W - 1)])
        keys = np.abs(p.aim_dist - mids)
        idx = aim_index(keys, p.aim_dist)
        vecs = (wp[idx], wp[W - 1] - wp[W - 2], tgt)
        a, a_last, a_t = (heading(v) for v in vecs)
        c1, c2, c3 = abs(a_t) < abs(a), abs(a_t - a_last) > p.angle_thresh, tgt[1] < p.dist_thresh
        to_target = bool(c1 or (c2 and c3))
        out, state.turn = pid(state.turn, a_t if to_target else a, p.turn)
        steer = clip(out, -1.0, 1.0)
        q = speed / desired
        b1, b2 = desired < p.brake_speed, q > p.brake_ratio
        brake = bool(b1 or b2)
        delta = clip(desired - speed, 0.0, p.clip_delta)
        out, state.speed = pid(state.speed, delta, p.speed)
        throttle = 0.0 if brake else clip(out, 0.0, p.max_throttle)
    info = SimpleNamespace(idx=idx, to_target=to_target, brake=brake, desired=desired, q=q, keys=keys, mids=mids, a=a, a_last=a_last,
                           a_t=a_t, tgt_y=tgt[1], norms=tuple(float(np.linalg.norm(v)) for v in vecs), cmp_tt=(c1, c2, c3), cmp_b=(b1, b2),
                           scale=max(float(np.nanmax(np.abs(wp))), float(np.nanmax(np.abs(tgt)))))
    return np.array(post_process(p.post, throttle, steer, 1.0 if brake else 0.0)), info


# ---- the bound ----------------------------------------------------------------------------------------------------------------
def bound(p, M, V, r_min, has_target=True):
    """Absolute bounds on |fp32 evaluation - exact| for a run whose scaled waypoints and targets have |component| <= M, whose
    speeds have |speed| <= V and whose three heading vectors (aim point, last segment, target) all have norm >= r_min.  Every
    operation is rounded once (u = 2^-24; sqrt and division are correctly rounded), sums in any order; gamma_n as in Higham.

    waypoint   two products at most: per component within e_wp = gamma_2 M.
    segment    d = wp[i+1] - wp[i], |d| <= 2M per component: 2 e_wp + 2uM <= e_d = gamma_6 M.
    length     the norm is 1-Lipschitz in its vector (sqrt2 e_d for two components); two squares, their sum and the root are
               three roundings of a value <= 2 sqrt2 M:  e_len = sqrt2 e_d + gamma_3 2 sqrt2 M.
    desired    a term is len 2 / (W - 1) (the product is exact, the division one rounding); the W - 1 terms, each <= their
               largest, sum to at most D = 4 sqrt2 M:  e_des = 2 e_len + gamma_{W-1} D  (gamma_{W-2} for the additions, u for the
               divisions).
    key        the midpoint (wp[i+1] + wp[i]) / 2: e_wp + uM <= gamma_3 M per component, its norm <= sqrt2 M as above, then
               one subtraction of a value <= |AIM| + sqrt2 M:  e_key = sqrt2 gamma_3 M + gamma_3 sqrt2 M + u (|AIM| + sqrt2 M).
    angle      atan2 is (1 / r)-Lipschitz in its vector at norm r: a vector whose components are within e_v moves it by at most
               sqrt2 e_v / (r - sqrt2 e_v); the function itself adds ATAN2_ERR (see the top of this file).  theta in [-pi, pi]:
               pi/2 as an fp32 number (u pi/2), the subtraction (<= u 3pi/2), the product with 180/pi as an fp32 number (2u of
               <= 270) and the division by 90 (u of <= 3) turn that into  e_a = (2 / pi) e_theta + 16 u,  |a| <= 3.  e_v is
               e_wp for the aim point and for a stand-in target, e_d for the last segment, gamma_2 M for a given target.
               e_a below takes the largest, e_d, at r_min.
    PID        samples within e_in and of magnitude <= A: k_p e -> |k_p| e_in; the mean -> e_in + gamma_n A (n - 1 additions in
               any order and the division); e - previous -> 2 e_in + u 2A; three products and two sums, each one rounding of a
               value <= (|k_p| + |k_i| + 2 |k_d|) A:  e_pid = |k_p| e_in + |k_i| (e_in + gamma_n A) + |k_d| (2 e_in + 2uA) +
               gamma_3 (|k_p| + |k_i| + 2 |k_d|) A;  n = 1: |k_p| e_in + u |k_p| A.
    steer      e_pid(e_a, 3, n_turn, turn gains); clip is 1-Lipschitz.
    throttle   delta = clip(desired - speed): e_des + u (D + V), |delta| <= CLIP_DELTA; e_pid(that, CLIP_DELTA, n_speed, speed gains).
    Where the kernel takes another decision than the reference the controls are not comparable: the tests assert the margins."""
    r2 = np.sqrt(2.0)
    b = SimpleNamespace(M=M, V=V)
    b.e_wp = gamma(2) * M
    b.e_d = gamma(6) * M
    b.e_len = r2 * b.e_d + gamma(3) * 2 * r2 * M
    b.D = 4 * r2 * M
    b.e_des = 2 * b.e_len + gamma(p.W - 1) * b.D
    b.e_key = r2 * gamma(3) * M + gamma(3) * r2 * M + U * (abs(p.aim_dist) + r2 * M)

    def e_angle(e_v, r):
        return (2 / np.pi) * (r2 * e_v / (r - r2 * e_v) + ATAN2_ERR) + 16 * U
    b.e_angle = e_angle
    b.e_a = e_angle(b.e_d, r_min)

    def e_pid(e_in, A, n, gains):
        kp, ki, kd = (abs(g) for g in gains)
        if n < 2:
            return kp * e_in + U * kp * A
        return kp * e_in + ki * (e_in + gamma(n) * A) + kd * (2 * e_in + 2 * U * A) + gamma(3) * (kp + ki + 2 * kd) * A
    b.steer = e_pid(b.e_a, 3.0, p.n_turn, p.turn)
    b.e_delta = b.e_des + U * (b.D + V)
    b.throttle = e_pid(b.e_delta, abs(p.clip_delta), p.n_speed, p.speed)
    return b


def _or(x, y):
    """(truth, margin, allowance) of `x or y`: the comparison that decides it -- of two true ones the safer, of two false ones
    the closer."""
    rho = lambda c: c[1] / c[2]                      # noqa: E731
    if x[0] or y[0]:
        return max((c for c in (x, y) if c[0]), key=rho)
    return min((x, y), key=rho)


def _and(x, y):
    rho = lambda c: c[1] / c[2]                      # noqa: E731
    if x[0] and y[0]:
        return min((x, y), key=rho)
    return max((c for c in (x, y) if not c[0]), key=rho)


def margins(p, info, b, has_target=True):
    """Per decision (margin, allowance): how far the reference is from deciding otherwise at the comparison that decides, and the
    rounding the bound allows an fp32 evaluation on the two sides of that comparison.
      aim        two keys, each within e_key: 2 e_key against the gap to the runner-up (and to the qualifying threshold).
      to_target  |a_t| against |a|: e_a of each; |a_t - a_last| (<= 6: one more rounding, 6u) against the threshold; tgt.y (one
                 product: gamma_1 |tgt.y|; a stand-in: e_wp) against the threshold.
      brake      desired within e_des; q = speed / desired within q e_des / (desired - e_des) + u q."""
    thresh = abs(p.aim_dist - 1e5)
    ok = np.sort(info.keys[info.keys < thresh])
    gap = ok[1] - ok[0] if ok.size > 1 else np.inf
    aim = (min(gap, np.abs(info.keys - thresh).min()), 2 * b.e_key)
    e_v_t = gamma(2) * b.M if has_target else b.e_wp
    ea, el, et = b.e_angle(b.e_wp, info.norms[0]), b.e_angle(b.e_d, info.norms[1]), b.e_angle(e_v_t, info.norms[2])
    c1, c2, c3 = info.cmp_tt
    t1 = (c1, abs(abs(info.a_t) - abs(info.a)), et + ea)
    t2 = (c2, abs(abs(info.a_t - info.a_last) - p.angle_thresh), et + el + 6 * U)
    t3 = (c3, abs(info.tgt_y - p.dist_thresh), max(e_v_t, gamma(1) * abs(info.tgt_y)))
    tt = _or(t1, _and(t2, t3))
    b1, b2 = info.cmp_b
    e_q = abs(info.q) * b.e_des / (info.desired - b.e_des) + U * abs(info.q)
    br = _or((b1, abs(info.desired - p.brake_speed), b.e_des), (b2, abs(info.q - p.brake_ratio), e_q))
    return dict(aim=aim, to_target=tt[1:], brake=br[1:])


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
TICKS = 80


def fixture(P, horizon=16):
    """The 80 ticks of the controller parity run (utils/procedural.control_inputs): wp [80, H, 2], speed [80], target [80, 2]."""
    rows = [P.control_inputs(k, horizon) for k in range(TICKS)]
    return (np.stack([r[0].numpy() for r in rows]), np.array([float(r[1][0]) for r in rows], dtype=np.float32),
            np.stack([r[2].numpy() for r in rows]))


OFFSETS = (0, 7, 23)
MAGIC = 23.315          # model.magic_num


def scene_case(P, cfg, W, with_target, post="agent"):
    """The GPU tests' input: the 80 ticks as len(OFFSETS) scenes, scene s at tick k seeing tick (k + OFFSETS[s]) % 80 of the parity
    run, as the sampling loop would hand them over -- model units (metres / magic_num, rounded to fp32), x mirrored (sign_x = -1
    mirrors it back), xy_scale = magic_num; the target in the controller's units, x mirrored (target_scale = 1), or None: waypoint W
    stands in.  traj [80, S, H, 2], speed [80, S], target [80, S, 2] or None."""
    wps, speeds, targets = fixture(P)
    k = (np.arange(TICKS)[:, None] + np.array(OFFSETS)[None, :]) % TICKS
    mirror = np.array([-1.0, 1.0], dtype=np.float32)
    traj = (wps[k] * mirror / np.float32(MAGIC)).astype(np.float32)
    return SimpleNamespace(p=params(cfg, waypoints=W, post=post, sign_x=-1.0, xy_scale=MAGIC), S=len(OFFSETS), traj=traj, speed=speeds[k],
                           target=(targets[k] * mirror).astype(np.float32) if with_target else None)


def run(p, wps, speeds, targets=None, state=None):
    """A scene over its ticks: controls [T, 3], the per-tick info, the final state."""
    state = fresh(p) if state is None else state
    out, infos = [], []
    for k in range(len(wps)):
        c, info = tick(p, state, wps[k], float(speeds[k]), None if targets is None else targets[k])
        out.append(c)
        infos.append(info)
    return np.stack(out), infos, state


def run_bound(p, infos, speeds, has_target=True):
    """The bound of a run, from its own magnitudes: M and r_min over the ticks, V over the speeds."""
    M = max(i.scale for i in infos)
    r_min = min(min(i.norms) for i in infos)
    return bound(p, M, float(np.abs(speeds).max()), r_min, has_target)
