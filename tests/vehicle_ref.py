"""fp64 NumPy restatement of "vehicle v1" (include/adx.h: adx_vehicle_step, adx_vehicle_reset), written from the contract's text,
and the rounding bounds of a kernel that evaluates it.

What can differ.  Every operation of the contract is a single IEEE fp64 +, -, * or / on both sides, rounded once, EXCEPT the three
library calls: tan(delta) once per step, sin(compass) and cos(compass) once per sub-step.  So the speed never sees a library call:
it is the same double on both sides (bound 0), and so is everything a `hold` writes.  ROCm ships no accuracy table for its device
library (none under its share/ or doc trees), so the device's fp64 tan, sin and cos are ASSUMED to lie within DEVICE_ULP = 2 ulp
of the true value; the host's (glibc) lie within 1.  Two results of one call on one argument then differ by at most U = 3 ulp of
the value, i.e. by U e |value| with e = 2^-52.

The bound of one step from one state, first order in e, tracked along the sub-steps by `step`:
    k = fl(tan(delta) / wheelbase)          |dk| <= U e |k| + e |k|                     (the call; one rounding per side, half an ulp each)
    rate = fl(fl(sign * v) * k)             |d rate| <= |dk| |sv| + e |rate|            (sign * v is the same double)
    turn = fl(rate * h)                     |d turn| <= |d rate| h + e |turn|
    compass = fl(compass + turn)            bc <- bc + |d turn| + e |compass|
    sx = fl(dist * sin(compass))            |d sx| <= dist (U e + bc) + e |sx|          (|sin'| <= 1: the argument's error bc passes at most once)
    x = fl(x + sx)                          bx <- bx + |d sx| + e |x|;                  y likewise with cos
    yaw_rate = fl(fl(compass - c0) / dt)    <= (bc + e |compass - c0|) / dt + e |yaw_rate|, and one fp32 ulp on top when rounded to fp32
With U = 3 that is |d turn| <= (U + 1 + 1 + 1) e |turn| = 6 e |turn|.  SLACK = 1 + 2^-20 covers the second-order terms.

A free-running roll-out.  An error in x, y passes through a step unchanged (x' = x + ...); an error dc in the compass passes
unchanged into the next compass (the turn does not read it) and moves the step's displacement by at most dc times the distance
travelled.  After T steps the position is off by at most sum_t b_t + (sum_t travel_t) * sum_t bc_t <= T * b * (1 + path) with b the
largest per-step bound: tick count times per-step bound times the Lipschitz factor L = 1 + path length, which `rollout_bound` forms.
"""
import math

import numpy as np

# the host side of the comparison is glibc's libm (within 1 ulp), element by element: NumPy's own vector loops make no such promise
_sin, _cos, _tan = (np.vectorize(f, otypes=[np.float64]) for f in (math.sin, math.cos, math.tan))

DEVICE_ULP, HOST_ULP = 2.0, 1.0
U = DEVICE_ULP + HOST_ULP
E52 = 2.0 ** -52
SLACK = 1.0 + 2.0 ** -20
DEFAULTS = dict(dt=0.1, substeps=4, wheelbase=2.9, accel_max=3.0, brake_max=8.0, drag=0.05, roll=0.1, v_max=20.0, steer_max=0.6,
                steer_sign=1)


def fresh_state(S):
    return dict(x=np.zeros(S), y=np.zeros(S), compass=np.zeros(S), speed=np.zeros(S), valid=np.zeros(S, dtype=np.int32))


def reset(state, pose=None, speed=None, mask=None):
    """The contract's adx_vehicle_reset: a new state dict."""
    S = len(state["x"])
    m = np.ones(S, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    new = {k: v.copy() for k, v in state.items()}
    if pose is None:
        for k in ("x", "y", "compass", "speed"):
            new[k][m] = 0.0
        new["valid"][m] = 0
        return new
    pose = np.asarray(pose, dtype=np.float64)
    v = np.zeros(S) if speed is None else np.asarray(speed, dtype=np.float64).copy()
    v[~(v >= 0.0)] = 0.0
    new["x"][m], new["y"][m] = pose[m, 0], pose[m, 1]
    new["compass"][m] = np.where(np.isnan(pose[:, 2]), 0.0, pose[:, 2])[m]
    new["speed"][m] = v[m]
    new["valid"][m] = 1
    return new


def pedal(c, lo):
    c = np.asarray(c, dtype=np.float32)
    f = np.where(np.isfinite(c), c, np.float32(0.0))
    return np.clip(f, np.float32(lo), np.float32(1.0)).astype(np.float64)


def step(state, control, hold=None, **params):
    """One launch of adx_vehicle_step from `state` (not modified).  Returns dict(state, pose [S, 3] fp64, velocity and yaw_rate
    [S] fp32, pose_bound [S, 3], yaw_bound [S] (fp64 part plus one fp32 ulp), travel [S] metres)."""
    p = dict(DEFAULTS, **params)
    n, dt = int(p["substeps"]), float(p["dt"])
    h = dt / n
    control = np.asarray(control, dtype=np.float32)
    S = control.shape[0]
    held = np.zeros(S, dtype=bool) if hold is None else np.asarray(hold) != 0
    x, y, c, v = (state[k].astype(np.float64).copy() for k in ("x", "y", "compass", "speed"))
    throttle, steer, brake = pedal(control[:, 0], 0.0), pedal(control[:, 1], -1.0), pedal(control[:, 2], 0.0)
    delta = steer * p["steer_max"]
    k = _tan(delta) / p["wheelbase"]
    dk = (U + 1.0) * E52 * np.abs(k)
    c0 = c.copy()
    push, pull = throttle * p["accel_max"], brake * p["brake_max"]
    bx, by, bc, travel = np.zeros(S), np.zeros(S), np.zeros(S), np.zeros(S)
    for _ in range(n):
        dv = p["drag"] * v
        acc = (push - pull) - dv
        acc = np.where(v > 0.0, acc - p["roll"], acc)
        inc = acc * h
        v = v + inc
        v = np.where(v >= 0.0, v, 0.0)
        v = np.where(v > p["v_max"], p["v_max"], v)
        sv = float(p["steer_sign"]) * v
        rate = sv * k
        turn = rate * h
        d_rate = dk * np.abs(sv) + E52 * np.abs(rate)
        d_turn = d_rate * h + E52 * np.abs(turn)
        c = c + turn
        bc = bc + d_turn + E52 * np.abs(c)
        dist = v * h
        sx, sy = dist * _sin(c), dist * _cos(c)
        x = x + sx
        y = y - sy
        bx = bx + dist * (U * E52 + bc) + E52 * np.abs(sx) + E52 * np.abs(x)
        by = by + dist * (U * E52 + bc) + E52 * np.abs(sy) + E52 * np.abs(y)
        travel = travel + dist
    yaw = (c - c0) / dt
    b_yaw = (bc + E52 * np.abs(c - c0)) / dt + E52 * np.abs(yaw)
    # a held scene: speed 0, the pose kept, nothing computed
    x, y, c = np.where(held, state["x"], x), np.where(held, state["y"], y), np.where(held, state["compass"], c)
    v, yaw = np.where(held, 0.0, v), np.where(held, 0.0, yaw)
    zero = lambda b: np.where(held, 0.0, b * SLACK)  # noqa: E731
    yaw32 = yaw.astype(np.float32)
    new = dict(x=x, y=y, compass=c, speed=v, valid=np.ones(S, dtype=np.int32))
    return dict(state=new, pose=np.stack([x, y, c], axis=1), velocity=v.astype(np.float32), yaw_rate=yaw32,
                pose_bound=np.stack([zero(bx), zero(by), zero(bc)], axis=1),
                yaw_bound=zero(b_yaw) + np.where(held, 0.0, np.spacing(np.abs(yaw32)).astype(np.float64)),
                travel=np.where(held, 0.0, travel))


def rollout_bound(step_bounds, travels):
    """[S, 3]: the bound of the pose after the T free-running steps whose per-step `pose_bound` [T, S, 3] and `travel` [T, S] are
    given: T * (the largest per-step bound) * L, with L = 1 + path length for x and y and 1 for the compass."""
    step_bounds, travels = np.asarray(step_bounds), np.asarray(travels)
    T = step_bounds.shape[0]
    b = step_bounds.max(axis=(0, 2))                      # [S]
    lip = 1.0 + travels.sum(axis=0)
    return np.stack([T * b * lip, T * b * lip, T * step_bounds[..., 2].max(axis=0)], axis=1)


def pack_state(state):
    """The int32 [S, 10] words of the contract's record."""
    S = len(state["x"])
    w = np.zeros((S, 10), dtype=np.int32)
    w.view(np.float64)[:, 0:4] = np.stack([state["x"], state["y"], state["compass"], state["speed"]], axis=1)
    w[:, 8] = state["valid"]
    return w


def unpack_state(words):
    w = np.ascontiguousarray(words, dtype=np.int32)
    f = w.view(np.float64)
    return dict(x=f[:, 0].copy(), y=f[:, 1].copy(), compass=f[:, 2].copy(), speed=f[:, 3].copy(), valid=w[:, 8].copy())
