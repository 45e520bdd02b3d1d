"""NumPy restatement of "manoeuvre commitment v1" (include/adx.h: adx_traj_commit), one rounded operation per operation in a
`dtype` of the caller's choice (float32: the kernel's bits wherever each of its operations is a single correctly rounded one;
float64: the exact answer), the fp32 error bound of the distance when the prior is moved by the odometry, and the seeded fixtures
the CPU and GPU tests share.  Arithmetic only, written from the contract; the prior is warm start v1's own `advance` and `rebase`
(tests/warm_ref.py), imported and not restated.

    state      int32 [S][2 + 2H]: valid, held, then x and y (float32 bits) of the H waypoints of the last chosen plan
    prior      valid != 0: q = rebase(advance(stored, shift), stored[shift], motion) on the stored [H][2] plan; absent when valid == 0
               or a scored q_h is not finite
    dist2      d_k = (t_h0 + t_h0+1 + ... + t_H-1) / n, t_h = dx * dx + dy * dy, dx = x_k,h - qx_h, a missing y counts as 0
    finite     every scored xy of k finite;  near: finite and d_k <= r2 = fl32(radius * radius)
    eligible   near, cost[k] finite, and (no active, or active[k] == 0, or active[sel] != 0)
    decision   NO_PRIOR 0 | SAME 1 (sel near) | LOST 2 (nobody eligible) | HELD 3 (f = the cheapest eligible, lowest index first;
               cost[f] <= t = fl32(fl32(cost[sel] + margin) + fl32(ratio * |cost[sel]|)); max_hold == 0 or held < max_hold) |
               SWITCHED 4
    update     held' = held + 1 on HELD else 0; the chosen candidate finite: valid' = 1 and its xy of all H waypoints stored
               (y = 0 at D = 1); else valid' = 0 and the stored words stay
Rows are candidate-major: candidate k of scene s is row k * S + s.  The threshold t is fp32 arithmetic on fp32 numbers by
contract, whatever `dtype`: `dtype` governs the prior and the distance, the only places where the odometry's cos and sin enter.
"""
import numpy as np

import warm_ref as W
from modes_ref import r2_of
from select_ref import gamma

U = W.U
NO_PRIOR, SAME, LOST, HELD, SWITCHED = range(5)
RADIUS = 0.1                 # of every fixture
T_MAX = 0.05                 # the largest |tx|, |ty| of a fixture's odometry: what dist2_bound is evaluated at


def bits(a):
    return np.ascontiguousarray(a).view(np.int32) if np.asarray(a).dtype == np.float32 else np.ascontiguousarray(a)


def _rows(trajs, scenes):
    t = np.asarray(trajs)
    if t.ndim == 3:
        t = t.reshape(-1, scenes, t.shape[1], t.shape[2])
    assert t.ndim == 4 and t.shape[1] == scenes, t.shape
    return t


def fresh_state(S, H):
    return np.zeros((S, 2 + 2 * H), dtype=np.int32)


def stored_plan(state, H):
    """The [S, H, 2] float32 plan a state holds."""
    st = np.ascontiguousarray(state, dtype=np.int32)
    return st[:, 2:].view(np.float32).reshape(st.shape[0], H, 2)


def make_state(plan_xy, valid, held):
    """A state from a [S, H, 2] plan and per-scene valid / held words."""
    p = np.ascontiguousarray(plan_xy, dtype=np.float32)
    S, H, _ = p.shape
    st = fresh_state(S, H)
    st[:, 0], st[:, 1] = valid, held
    st[:, 2:] = p.reshape(S, 2 * H).view(np.int32)
    return st


def prior(state, H, shift, motion=None, dtype=np.float64):
    """q [S, H, 2] in `dtype`: warm start v1's advance and re-base of the stored plan (whatever `valid` says)."""
    p = stored_plan(state, H).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        return W.rebase(W.advance(p, shift, dtype), p[:, shift], motion, dtype)


def threshold(c_sel, margin, ratio):
    """t of the contract: fp32, every operation rounded on its own."""
    c, m, r = np.float32(c_sel), np.float32(margin), np.float32(ratio)
    with np.errstate(invalid="ignore", over="ignore"):
        t0 = np.float32(c + m)
        t1 = np.float32(r * np.float32(np.abs(c)))
        return np.float32(t0 + t1)


def commit(trajs, scenes, cost, selected, state, *, active=None, motion=None, h0=1, shift=1, max_hold=0, radius=RADIUS, margin=0.0,
           ratio=0.1, dtype=np.float64):
    """Everything the kernel writes, as a dict: best [S, H, D] (the dtype of trajs, copied bit for bit), index, status, follower
    [S] int32, blocked [S] int32 (None without `active`), dist2 [S, K] in `dtype`, state: the NEXT state; and, for the tests,
    finite / near / eligible [S, K] bool, prior_ok [S] bool, t [S] float32."""
    t = _rows(trajs, scenes)
    K, S, H, D = t.shape
    n = H - h0
    assert n >= 1 and H >= 2
    cost = np.asarray(cost, dtype=np.float32).reshape(S, K)
    state = np.ascontiguousarray(state, dtype=np.int32).reshape(S, 2 + 2 * H)
    r2 = dtype(r2_of(radius))
    q = prior(state, H, shift, motion, dtype)                                      # [S, H, 2]
    p = np.zeros((K, S, H, 2), dtype=dtype)
    p[..., :min(D, 2)] = t[..., :min(D, 2)].astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = None
        for h in range(h0, H):
            dx, dy = p[:, :, h, 0] - q[None, :, h, 0], p[:, :, h, 1] - q[None, :, h, 1]
            xx, yy = dx * dx, dy * dy
            th = xx + yy
            acc = th if acc is None else acc + th
        d = (acc / dtype(n)).T                                                     # [S, K]
        finite = np.isfinite(p[:, :, h0:]).all(axis=(2, 3)).T
        near = finite & (d <= r2)
    prior_ok = (state[:, 0] != 0) & np.isfinite(q[:, h0:]).all(axis=(1, 2))
    out = dict(best=np.empty((S, H, D), dtype=t.dtype), index=np.empty(S, dtype=np.int32), status=np.empty(S, dtype=np.int32),
               follower=np.empty(S, dtype=np.int32), blocked=None if active is None else np.empty(S, dtype=np.int32),
               dist2=np.ascontiguousarray(d), state=state.copy(), finite=finite, near=near, eligible=np.zeros((S, K), dtype=bool),
               prior_ok=prior_ok, t=np.empty(S, dtype=np.float32))
    if active is not None:
        active = np.asarray(active, dtype=np.int32).reshape(S, K)
    for s in range(S):
        sel = int(np.clip(int(np.asarray(selected).reshape(S)[s]), 0, K - 1))
        held = int(state[s, 1])
        elig = near[s] & np.isfinite(cost[s])
        if active is not None and active[s, sel] == 0:
            elig &= active[s] == 0
        out["eligible"][s] = elig
        tt = threshold(cost[s, sel], margin, ratio)
        out["t"][s] = tt
        chosen, f = sel, -1
        if not prior_ok[s]:
            status = NO_PRIOR
        elif near[s, sel]:
            status = SAME
        elif not elig.any():
            status = LOST
        else:
            f = int(np.where(elig, cost[s], np.float32(np.inf)).argmin())          # the first minimum: the lowest index
            if cost[s, f] <= tt and (max_hold == 0 or held < max_hold):
                status, chosen = HELD, f
            else:
                status = SWITCHED
        out["index"][s], out["status"][s], out["follower"][s] = chosen, status, f
        if active is not None:
            out["blocked"][s] = int(active[s, chosen] != 0)
        out["best"][s] = t[chosen, s]
        nxt = out["state"][s]
        nxt[1] = held + 1 if status == HELD else 0
        if finite[s, chosen]:
            xy = np.zeros((H, 2), dtype=np.float32)
            xy[:, :min(D, 2)] = t[chosen, s, :, :min(D, 2)]
            nxt[0] = 1
            nxt[2:] = xy.reshape(-1).view(np.int32)
        else:
            nxt[0] = 0
    return out


def dist2_bound(H, h0, shift, t_max=1.0):
    """Absolute bound on |fp32 d_k - exact d_k| WITH motion, for stored plans and candidates with |x|, |y| <= 1 and |tx|, |ty| <=
    t_max, every operation rounded once (u = 2^-24), sinf / cosf within 4 ulp (warm_ref.error_bound's stated assumption).

    the prior      q_h^ = q_h + e, |e| <= E_h: warm_ref.error_bound's E_w of a column d < 2 with motion, BEFORE its clamp and noise
                   (E_w = 2 E_q + (12 Q + 1) u, Q = 1 + 2k + t_max, k = max(0, h + shift - (H-1)); taken from that function with
                   z = 0 and its last line's (3 + 2 |z|) u of the noise stage subtracted, not restated).  |q_h| <= 2 Q (a sum of
                   two products of magnitude <= Q each).
    a difference   dx = x - q_h, |dx| <= A_h = 1 + 2 Q.  dx^ = fl(x - q_h^): |dx^ - dx| <= e_d = E_h + (A_h + E_h) u.
    a term         t_h = dx^2 + dy^2 <= 2 A_h^2.  With exact inputs its four roundings (difference, square, sum) give 2 A_h^2 gamma_4
                   as in modes_ref.bound.  The carried error: |(dx + e)^2 - dx^2| <= 2 A_h e_d + e_d^2 per component, two
                   components, through the square's and the sum's roundings: (4 A_h E_h + 2 E_h^2)(1 + gamma_4), the (A_h + E_h) u
                   part of e_d being the difference's own rounding that gamma_4 already counts.
                   tau_h = 2 A_h^2 gamma_4 + (4 A_h E_h + 2 E_h^2)(1 + gamma_4).
    the mean       the n computed terms are <= T_h = 2 A_h^2 + tau_h.  Their fp32 sum in the contract's order is within gamma_{n-1}
                   of sum T_h, the division by n (exact in fp32) adds a rounding: gamma_n * mean(T_h), as modes_ref.bound has it.
    Together mean(tau_h) + gamma_n mean(T_h) over the scored h.  The fp64 restatement it is compared with is itself within
    2^-45 of the exact value at these magnitudes, which the (1 + gamma_4) factors cover.  Nothing here is fitted to a device."""
    n = H - h0
    assert n >= 1
    z = np.zeros((1, H, 2))
    e_h = (W.error_bound(H, 2, shift, True, z, zero_first=False, t_max=t_max)[0] - 3.0 * U).max(axis=1)      # [H]: E_w, x and y alike
    k = np.maximum(0, np.arange(H) + shift - (H - 1)).astype(np.float64)
    a_h = 1.0 + 2.0 * ((1.0 + 2.0 * k) + t_max)
    g4 = gamma(4)
    tau = 2.0 * a_h ** 2 * g4 + (4.0 * a_h * e_h + 2.0 * e_h ** 2) * (1.0 + g4)
    big = 2.0 * a_h ** 2 + tau
    return float(tau[h0:].mean() + gamma(n) * big[h0:].mean())


def unclear(res64, bound, radius=RADIUS):
    """[S] bool: scenes in which some finite candidate's |d_k - r2| lies within `bound` (from the fp64 restatement's dict): the
    scenes whose decisions the rounding of dist2 may change."""
    r2 = r2_of(radius)
    with np.errstate(invalid="ignore"):
        close = np.abs(res64["dist2"] - r2) <= bound
    return (close & res64["finite"]).any(axis=1) & res64["prior_ok"]


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
def _motion(rng, S):
    """[S, 3] float32: a tick's odometry at model scale, |tx|, |ty| <= 0.05, |phi| <= 0.2."""
    return np.concatenate([rng.uniform(-0.05, 0.05, size=(S, 2)), rng.uniform(-0.2, 0.2, size=(S, 1))], axis=1).astype(np.float32)


def _plan(rng, S, H):
    """[S, H, 2] float32: a smooth stored plan that starts near 0 and stays within 0.25, so that its advance by any shift (at
    most twice as far), its re-base and a candidate 0.35 off it stay within [-1, 1]."""
    tau = np.linspace(0.0, 1.0, H)[None, :, None]
    xy = rng.uniform(-0.02, 0.02, size=(S, 1, 2)) + rng.uniform(-0.2, 0.2, size=(S, 1, 2)) * tau
    xy = xy + rng.uniform(-0.03, 0.03, size=(S, 1, 2)) * np.sin(np.pi * tau)
    return xy.astype(np.float32)


def _fill(rng, K, S, H, D, xy):
    """Candidates [K, S, H, D] float32: `xy` [K, S, H, 2] clipped to [-1, 1] in the first min(D, 2) columns, uniform elsewhere."""
    t = rng.uniform(-1.0, 1.0, size=(K, S, H, D)).astype(np.float32)
    t[..., :min(D, 2)] = np.clip(xy[..., :min(D, 2)], -1.0, 1.0).astype(np.float32)
    return t


def separated_case(S, K, H, D, shift, h0, motion=False, active=False, max_hold=0, first_kind=0, seed=2026):
    """A launch of two-manoeuvre scenes with known answers.  In every scene the candidates with an even index lie within
    0.5 * RADIUS (rms over the scored waypoints) of the prior, those with an odd index beyond 2 * RADIUS (asserted, in fp64).
    Scene s has kind (first_kind + s) % 5, arranged by its costs and its state to end in that status:
      0 NO_PRIOR  valid = 0 (the words behind it are not zero);  1 SAME  the selector picks a near one;  2 LOST  the near ones all
      have a non-finite cost;  3 HELD  the selector's far pick costs 1.0, the cheapest near one 1.05 <= 1.0 + 0.1 * 1.0;
      4 SWITCHED  the near ones cost 1.5 and more.
    K >= 2.  `want`: the statuses.  With `active`: zeros but for one violating far candidate that is not the selector's."""
    assert K >= 2
    rng = np.random.default_rng([seed, S, K, H, D, shift, h0, int(motion), int(active), max_hold, first_kind])
    plan = _plan(rng, S, H)
    kinds = (first_kind + np.arange(S)) % 5
    state = make_state(plan, valid=(kinds != NO_PRIOR).astype(np.int32), held=rng.integers(0, 2, size=S) if max_hold == 0 else 0)
    mo = _motion(rng, S) if motion else None
    q = prior(make_state(plan, 1, 0), H, shift, mo)                                # fp64 [S, H, 2]
    if D == 1:
        # a candidate's y counts as 0: the near group can only be near where the prior's y is 0 too
        plan[..., 1] = 0.0
        if mo is not None:
            mo[:, 1:] = 0.0
        state = make_state(plan, state[:, 0], state[:, 1])
        q = prior(make_state(plan, 1, 0), H, shift, mo)
    a = 0.35 * RADIUS                                                              # |dx|, |dy| <= a: the rms is at most a * sqrt(2) < 0.5 RADIUS
    xy = q[None] + rng.uniform(-a, a, size=(K, S, H, 2))
    far = np.arange(K) % 2 == 1
    side = np.where(rng.uniform(size=(K, S, 1)) < 0.5, -1.0, 1.0)
    xy[far, :, :, 0] += (3.0 * RADIUS * side)[far]
    trajs = _fill(rng, K, S, H, D, xy)
    cost = rng.uniform(2.0, 3.0, size=(S, K)).astype(np.float32)
    selected = np.empty(S, dtype=np.int32)
    near_k, far_k = np.flatnonzero(~far), np.flatnonzero(far)
    for s, kind in enumerate(kinds):
        pick_far = int(rng.choice(far_k))
        cost[s, pick_far] = 1.0
        selected[s] = pick_far
        if kind == SAME:
            selected[s] = int(rng.choice(near_k))
            cost[s, selected[s]] = 0.5
        elif kind == LOST:
            cost[s, near_k] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), size=near_k.size)
        elif kind == HELD:
            cost[s, rng.choice(near_k)] = 1.05
        elif kind == SWITCHED:
            cost[s, near_k] = rng.uniform(1.5, 2.0, size=near_k.size).astype(np.float32)
    act = None
    if active:
        act = np.zeros((S, K), dtype=np.int32)
        for s in range(S):
            others = far_k[far_k != selected[s]]
            if others.size:
                act[s, rng.choice(others)] = 3
    case = dict(S=S, K=K, H=H, D=D, shift=shift, h0=h0, max_hold=max_hold, trajs=trajs.reshape(K * S, H, D), cost=cost,
                selected=selected, active=act, motion=mo, state=state, want=kinds.astype(np.int32), separated=True)
    # the construction's promise, in fp64
    res = run(case, dtype=np.float64, state=make_state(plan, 1, 0))
    rms = np.sqrt(res["dist2"])
    assert (rms[:, ~far] <= 0.5 * RADIUS).all() and (rms[:, far] >= 2.0 * RADIUS).all(), (rms.min(), rms.max())
    return case


def random_case(S, K, H, D, shift, h0, motion=False, active=False, max_hold=0, odd=False, seed=2026):
    """A launch of random scenes: candidates scattered around the prior at scales from 0.2 to 5 RADIUS, random costs, a selector's
    pick that is the cheapest or any, valid words of both kinds, held counters 0..3, and with `active` counts 0, 0, 1, 2.  `odd`
    (never with motion: the test then compares bits, not distances) sprinkles NaN and inf over candidates, costs and stored
    plans and picks selectors' indices outside 0..K-1."""
    assert not (odd and motion)
    rng = np.random.default_rng([seed + 1, S, K, H, D, shift, h0, int(motion), int(active), max_hold, int(odd)])
    plan = _plan(rng, S, H)
    if D == 1:
        plan[..., 1] *= 0.1
    state = make_state(plan, valid=rng.integers(0, 4, size=S).clip(0, 1) * rng.integers(1, 9, size=S), held=rng.integers(0, 4, size=S))
    mo = _motion(rng, S) if motion else None
    q = prior(make_state(plan, 1, 0), H, shift, mo)
    scale = RADIUS * np.exp(rng.uniform(np.log(0.2), np.log(5.0), size=(K, S, 1, 1)))
    xy = q[None] + scale * rng.uniform(-1.0, 1.0, size=(K, S, H, 2))
    trajs = _fill(rng, K, S, H, D, xy)
    cost = rng.uniform(0.5, 1.5, size=(S, K)).astype(np.float32)
    cost[:, 0] = cost[:, -1]                                                       # a tie: the lowest index wins
    selected = np.where(rng.uniform(size=S) < 0.5, cost.argmin(axis=1), rng.integers(0, K, size=S)).astype(np.int32)
    act = rng.choice(np.array([0, 0, 1, 2], dtype=np.int32), size=(S, K)) if active else None
    if odd:
        bad = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
        hit = rng.uniform(size=trajs.shape) < 0.01
        trajs[hit] = rng.choice(bad, size=int(hit.sum()))
        hit = rng.uniform(size=cost.shape) < 0.1
        cost[hit] = rng.choice(bad, size=int(hit.sum()))
        stored = stored_plan(state, H)
        hit = rng.uniform(size=stored.shape) < 0.01
        stored[hit] = rng.choice(bad, size=int(hit.sum()))
        state = make_state(stored, state[:, 0], state[:, 1])
        selected[rng.uniform(size=S) < 0.2] = rng.choice(np.array([-3, K, K + 7], dtype=np.int32))
    return dict(S=S, K=K, H=H, D=D, shift=shift, h0=h0, max_hold=max_hold, trajs=trajs.reshape(K * S, H, D), cost=cost,
                selected=selected, active=act, motion=mo, state=state, want=None, separated=False)


def run(case, dtype=np.float64, state=None, **over):
    """`commit` on a fixture (RADIUS, margin 0, ratio 0.1)."""
    kw = dict(active=case["active"], motion=case["motion"], h0=case["h0"], shift=case["shift"], max_hold=case["max_hold"], dtype=dtype)
    kw.update(over)
    return commit(case["trajs"], case["S"], case["cost"], case["selected"], case["state"] if state is None else state, **kw)


def shifts(H):
    return sorted({0, 1, H - 1})


def grid_cases(motion: bool):
    """The GPU grid: a sparse cross of K in {1, 2, 5, 64}, H in {2, 3, 16, 64}, D in {1, 2, 7}, S in {1, 3, 5}, shift in {0, 1, H-1},
    h0 in {0, 1}, active given / NULL, max_hold in {0, 2} -- every value of every axis occurs, in separated and in random
    launches (K = 1 in random ones alone: a separated scene needs both groups).  Without motion the random launches come with and
    without non-finite values.  With motion shift = H-1 is kept at H <= 3 alone: warm start v1's bound of a waypoint extrapolated
    k steps grows with k for ANY stored plan within [-1, 1], and at k = 63 dist2_bound exceeds r2 itself -- no scene could stand
    clear of it, whatever the device computes."""
    out = []
    Ks, Hs, Ds, Ss = (1, 2, 5, 64), (2, 3, 16, 64), (1, 2, 7), (1, 3, 5)
    i = 0
    for K in Ks:
        for H in Hs:
            for sh in (shifts(H) if not motion or H <= 3 else (0, 1)):
                D, S, h0, act, mh = Ds[i % 3], Ss[(i // 2) % 3], i % 2, bool((i // 3) % 2), (0, 2)[(i // 5) % 2]
                h0 = min(h0, H - 1)
                if K >= 2:
                    out.append(separated_case(S, K, H, D, sh, h0, motion, act, mh, first_kind=i % 5))
                out.append(random_case(S, K, H, D, sh, h0, motion, act, mh, odd=(not motion) and i % 2 == 1))
                i += 1
    out.append(separated_case(5, 8, 16, 7, 1, 1, motion, True, 0, first_kind=0))         # all five statuses in one launch
    return out


def sequence_case(motion: bool, ticks=8, S=3, K=8, H=16, D=4, seed=2026):
    """`ticks` ticks of S two-manoeuvre scenes in the vehicle's frame: two straight centre lines from the ego pose that end
    3 RADIUS left and right of straight on (straight lines: a warm start's advance and re-base map them onto themselves), even
    candidates scattered 0.3 RADIUS around the one and odd ones around the other, the cheapest of each side within 3 % of the
    other and alternating from tick to tick; on tick 5 scene 1's other side is cheaper by half.  shift = 1, the step along the
    path 0.025; with `motion` a small odometry per tick.  A list of per-tick dicts (trajs, cost, selected, active, motion) and the
    settings."""
    rng = np.random.default_rng([seed + 2, int(motion), ticks, S, K, H, D])
    tau = np.arange(H)[None, :, None] * 0.025
    centre = np.stack([np.concatenate([tau, off * tau / tau.max()], axis=2) for off in (-3.0 * RADIUS, 3.0 * RADIUS)])      # [2, 1, H, 2]
    out = []
    for tick in range(ticks):
        side = np.arange(K) % 2
        xy = np.repeat(centre[side], S, axis=1) + rng.uniform(-0.3 * RADIUS, 0.3 * RADIUS, size=(K, S, H, 2))
        xy[:, :, 0] = 0.0
        trajs = _fill(rng, K, S, H, D, xy)
        cost = rng.uniform(1.2, 1.4, size=(S, K)).astype(np.float32)
        cheap = tick % 2
        cost[:, cheap] = 1.0
        cost[:, 1 - cheap] = 1.03
        if tick == 5:
            cost[1, cheap] = 0.5
        out.append(dict(trajs=trajs.reshape(K * S, H, D), cost=cost, selected=cost.argmin(axis=1).astype(np.int32), active=None,
                        motion=(_motion(rng, S) * np.float32(0.2)) if motion else None))
    return dict(S=S, K=K, H=H, D=D, shift=1, h0=1, max_hold=0, ticks=out)
