"""fp64 NumPy restatement of "selection cost v2" (include/adx.h: adx_traj_select_guide), the fp32 error bound of a kernel that
evaluates it, hand-built scenes for its rule and the seeded case generator the CPU and GPU tests share.  Written from the contract:

    goal, smooth, consensus   selection cost v1: tests/select_ref.py
    violation[s][k], active[s][k]   cost guidance v1 of candidate k under scene s's discs and planes: tests/guide_ref.py
    cost       ((w_goal goal + w_smooth smooth) + w_consensus consensus) + w_guide violation; a weight of exactly 0 is not evaluated
    free       active == 0 and every x and y of the candidate finite
    index      hard == 0: the smallest k among the smallest finite costs, none finite -> 0.  hard != 0: the same rule over the free
               candidates with a finite cost when there is one, else over all candidates
    blocked    1 where the chosen candidate is not free
Rows are candidate-major: candidate k of scene s is row k * S + s.
"""
import numpy as np

import guide_ref as G
import select_ref as R

U = R.U
F32, F64 = np.float32, np.float64


def _rows(trajs, scenes):
    t = np.asarray(trajs)
    return t.reshape(-1, t.shape[-2], t.shape[-1]) if t.ndim == 4 else t


def violation(trajs, scenes, discs, planes, dtype=F64):
    """(violation [S, K] in `dtype`, active [S, K] int): guide_ref.row_cost on the candidate-major rows (row r reads scene r % S)."""
    t = _rows(trajs, scenes)
    with np.errstate(all="ignore"):
        cost, act, _ = G.row_cost(t, discs, planes, dtype)
    K = t.shape[0] // scenes
    return cost.reshape(K, scenes).T, act.reshape(K, scenes).T


def free_of(trajs, scenes, active):
    """free [S, K]: nothing violated and every xy finite."""
    t = _rows(trajs, scenes)
    K = t.shape[0] // scenes
    fin = np.isfinite(t[:, :, :2].astype(F64)).all(axis=(1, 2)).reshape(K, scenes).T
    return (np.asarray(active) == 0) & fin


def pick(cost, free, hard):
    """The rule: (index [S] int32, blocked [S] int32) of cost [S, K] and free [S, K]."""
    cost, free = np.asarray(cost, F64), np.asarray(free, bool)
    finite = np.isfinite(cost)
    key = np.where(finite, cost, np.inf)
    if hard:
        sub = free & finite
        narrowed = sub.any(axis=-1, keepdims=True)
        key = np.where(narrowed & ~sub, np.inf, key)
    index = key.argmin(-1).astype(np.int32)                  # the first minimum; all +inf -> 0
    blocked = (~free[np.arange(cost.shape[0]), index]).astype(np.int32)
    return index, blocked


def select(trajs, scenes, target, weights, hard, discs, planes, v1_cost=None):
    """dict(cost [S, K] fp64, active, free, index, blocked).  `weights` = (w_goal, w_smooth, w_consensus, w_guide), taken as the
    fp32 numbers the kernel is handed.  `v1_cost`: the first three terms' sum computed elsewhere (the hand-built scene whose NaN
    is an fp32 overflow), in place of select_ref's fp64 one."""
    wv = float(F32(weights[3]))
    t = _rows(trajs, scenes)
    cost = R.select(t, scenes, target, weights[:3])[0] if v1_cost is None else np.asarray(v1_cost, F64)
    viol, active = violation(t, scenes, discs, planes)
    if wv != 0.0:
        with np.errstate(invalid="ignore", over="ignore"):
            cost = cost + wv * viol
    free = free_of(t, scenes, active)
    index, blocked = pick(cost, free, hard)
    return dict(cost=cost, violation=viol, active=active, free=free, index=index, blocked=blocked)


def cost_bound(trajs, scenes, weights, has_target, discs, planes):
    """[S, K]: |fp32 cost - exact cost| for inputs with |p| <= 1 and |g| <= 1.  With u = 2^-24:

    c1     the v1 sum: within B1 = select_ref.cost_bound(K, H, weights[:3], has_target) of its exact value, and of magnitude at
           most T1 = 8 |w_goal| + 32 |w_smooth| + 8 |w_consensus| (the largest values its terms take; select_ref says why).
    v      the violation: within Bv = guide_ref.cost_bound(row) of its exact value v (per row: it scales with the row's own terms).
    p      fl(w_guide * v^): |p^ - w v| <= |w| Bv + u |w| (v + Bv) =: Ep
    cost   fl(c1^ + p^): one more rounding of a sum of magnitude <= T1 + B1 + |w| v + Ep.
    So the bound is B1 + Ep + u (T1 + B1 + |w| v + Ep).  w_guide == 0: the term is not evaluated and the bound is B1."""
    t = _rows(trajs, scenes)
    K, H = t.shape[0] // scenes, t.shape[1]
    wg, ws, wc, wv = (abs(float(F32(w))) for w in weights)
    b1 = R.cost_bound(K, H, weights[:3], has_target)
    if wv == 0.0:
        return np.full((scenes, K), b1)
    t1 = 8.0 * (wg if has_target else 0.0) + 32.0 * (ws if H >= 3 else 0.0) + 8.0 * wc
    v, _ = violation(t, scenes, discs, planes)
    bv = G.cost_bound(t, discs, planes).reshape(K, scenes).T
    ep = wv * bv + U * wv * (v + bv)
    return b1 + ep + U * (t1 + b1 + wv * v + ep)


def searched(cost, free, hard):
    """[S, K] bool: the set the rule searches -- the free candidates with a finite cost under `hard` when there is one, else all
    candidates with a finite cost."""
    finite = np.isfinite(cost)
    if not hard:
        return finite
    sub = free & finite
    return np.where(sub.any(axis=-1, keepdims=True), sub, finite)


# ---- hand-built scenes: the rule, one decision each ------------------------------------------------------------------------------
def _line(a, b, H=4):
    tau = np.linspace(0.0, 1.0, H)[:, None]
    return (np.asarray(a, F64) * (1 - tau) + np.asarray(b, F64) * tau).astype(F32)


def v1_cost32(trajs, target, weights):
    """(w_goal goal + w_smooth smooth) of one scene's candidates [K, H, 2] in fp32 NumPy, every operation rounded on its own."""
    p = np.asarray(trajs, F32)
    g = np.asarray(target, F32).reshape(2)
    with np.errstate(all="ignore"):
        d = p - g
        goal = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).min(-1)
        a = (p[:, 2:] - F32(2) * p[:, 1:-1]) + p[:, :-2]
        sm = a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]
        smooth = sm.sum(-1, dtype=F32) / F32(p.shape[1] - 2)
        return (F32(weights[0]) * goal + F32(weights[1]) * smooth)[None, :]


def hand_scenes():
    """name -> dict(S, K, trajs [K * S, H, 2] fp32, target, discs, planes, weights, want = {hard: (index list, blocked list)}).
    One scene each, H = 4, D = 2; the target sits in the middle of the one disc (0.5, 0) r = 0.2."""
    tgt = np.array([[0.5, 0.0]], F32)
    disc = np.array([[[0.5, 0.0, 0.0, 0.0, 0.2]]], F32)
    wall = np.array([[[1.0, 0.0, -2.0]]], F32)                          # x <= -2: every waypoint in [-1, 1] violates it
    on = _line((0.0, 0.0), (0.5, 0.0))                                   # ends on the target, inside the disc: goal 0, blocked
    near = _line((0.0, 0.0), (0.5, 0.1))                                 # ends inside the disc too: goal 0.01, blocked
    far = _line((0.0, 0.0), (-0.5, 0.5))                                 # never near the disc: free, goal 0.25 (waypoint 0)
    huge = np.zeros((4, 2), F32)
    huge[:, 0] = (-3e38, 3e38, -3e38, 3e38)                              # finite, free (phi = -inf), goal inf, smooth inf
    nan_xy = far.copy()
    nan_xy[2, 1] = np.nan
    w = (1.0, 0.0, 0.0, 0.0)

    def scene(cands, weights=w, discs=disc, planes=None, want=None, overflow=False):
        t = np.stack(cands).astype(F32)
        return dict(S=1, K=len(cands), trajs=t, target=tgt, discs=discs, planes=planes, weights=weights, want=want, overflow=overflow)

    return {
        # the free candidate has the worst goal cost: it wins under `hard` and loses without
        "free beats blocked": scene([on, near, far], want={True: ([2], [0]), False: ([0], [1])}),
        # nothing is free: v1's winner, and the flag says so
        "all blocked": scene([on, near, far], planes=wall, want={True: ([0], [1]), False: ([0], [1])}),
        # candidate 0 is free but its cost is inf - inf = NaN (w_smooth < 0): the free candidate with a finite cost wins ...
        "free with a NaN cost": scene([huge, on, far], weights=(1.0, -1.0, 0.0, 0.0), overflow=True,
                                      want={True: ([2], [0]), False: ([1], [1])}),
        # ... and when it is the only free one the search falls back to all candidates
        "only free one has a NaN cost": scene([huge, on, near], weights=(1.0, -1.0, 0.0, 0.0), overflow=True,
                                              want={True: ([1], [1]), False: ([1], [1])}),
        # every weight 0: all costs are 0.0.  The NaN-xy candidate violates nothing by comparison, yet is not free: with `hard`
        # the search stays on all candidates (the tie goes to 0, which is blocked); counted as free it would win as index 1
        "a NaN waypoint is never free": scene([on, nan_xy, near], weights=(0.0, 0.0, 0.0, 0.0),
                                              want={True: ([0], [1]), False: ([0], [1])}),
        # with w_guide the blocked candidates pay for it: the free one wins on cost alone, `hard` or not
        "w_guide alone": scene([on, near, far], weights=(0.0, 0.0, 0.0, 1.0), want={True: ([2], [0]), False: ([2], [0])}),
    }


def hand_select(sc, hard):
    """The restatement on a hand-built scene.  The overflow scenes' v1 sum comes from fp32 NumPy: their NaN is 3e38^2 = inf and
    inf - inf in fp32, which fp64 does not reproduce."""
    v1 = v1_cost32(sc["trajs"], sc["target"], sc["weights"]) if sc["overflow"] else None
    return select(sc["trajs"], sc["S"], sc["target"], sc["weights"], hard, sc["discs"], sc["planes"], v1_cost=v1)


# ---- generated cases -------------------------------------------------------------------------------------------------------------
# (S, K, H, D, M, P): the minimum; K no multiple of the four waves, H < 3, per-scene obstacles that differ; every limit at once;
# one disc slot with r = 0 and one with a NaN radius
SHAPES = ((1, 1, 1, 2, 1, 0), (3, 5, 2, 7, 3, 2), (2, 64, 64, 16, 32, 8), (3, 7, 33, 4, 2, 1))
# (name, (w_goal, w_smooth, w_consensus, w_guide), hard): all four nonzero; w_guide alone; hard with w_guide = 0; all of it.  Dyadic:
# exact in fp32
WEIGHTS = (("all four", (1.0, 0.5, 0.25, 2.0), False), ("w_guide alone", (0.0, 0.0, 0.0, 1.0), False),
           ("hard", (1.0, 0.5, 0.25, 0.0), True), ("all four, hard", (1.0, 0.5, 0.25, 2.0), True))
GAP = 8.0


def _hinges(t, d, p):
    """Per live constraint of one scene -- t [K, H, D], d [1, M, 5] / p [1, P, 3] or None -- the fp64 hinge value phi or psi [K, H]
    and a first-order bound e [K, H] on the error of its fp32 evaluation, from the contract's operations (u = 2^-24):
      disc   ex = u (|h vx| + |ox| + |dx|) bounds the error of dx (three roundings: h * vx, cx + ., x - .), likewise ey;
             d2 = dx^2 + dy^2 is within 2 |dx| ex + 2 |dy| ey + 2 u d2; inv = 1 / (r * r) carries 2 u, the product one more:
             |phi^ - phi| <= inv (2 |dx| ex + 2 |dy| ey + 2 u d2) + 3 u d2 inv + u |phi|
      plane  |psi^ - psi| <= u (|nx x| + |ny y| + |nx x + ny y| + |psi|)"""
    x, y = t[:, :, 0].astype(F64), t[:, :, 1].astype(F64)
    hf = np.arange(t.shape[1], dtype=F64)[None, :]
    for q in (() if d is None else d[0].astype(F64)):
        cx, cy, vx, vy, r = q
        if not r > 0:
            continue
        ox, oy = cx + hf * vx, cy + hf * vy
        dx, dy = x - ox, y - oy
        ex, ey = U * (np.abs(hf * vx) + np.abs(ox) + np.abs(dx)), U * (np.abs(hf * vy) + np.abs(oy) + np.abs(dy))
        d2, inv = dx * dx + dy * dy, 1.0 / (r * r)
        phi = 1.0 - d2 * inv
        yield phi, inv * (2 * np.abs(dx) * ex + 2 * np.abs(dy) * ey + 2 * U * d2) + 3 * U * d2 * inv + U * np.abs(phi)
    for q in (() if p is None else p[0].astype(F64)):
        nx, ny, b = q
        psi = (nx * x + ny * y) - b
        yield psi, U * (np.abs(nx * x) + np.abs(ny * y) + np.abs(nx * x + ny * y) + np.abs(psi))


def hinges_clear(t, d, p):
    """True when fp32 finds every hinge of one scene on the side fp64 does: every phi and psi stands further from 0 than twice
    the first-order bound on its fp32 error (the factor holds the second-order terms)."""
    return all((np.abs(v) > 2.0 * e).all() for v, e in _hinges(t, d, p))


def violation_error(t, d, p):
    """[K]: a derived bound on |fp32 violation - exact violation| per candidate of one scene.  A term v^2 / 2 of a hinge value v
    known to e is within |v| e of its own value, its square adds one rounding (the halving none); a waypoint's a active terms
    are accumulated with a - 1 roundings (the first is added to 0) and the H lanes by ceil(log2 H) rounds of the butterfly (the
    rounds that add a lane >= H add 0); 5 % on top for what is second order."""
    K, H = t.shape[:2]
    E, J, A = np.zeros((K, H)), np.zeros((K, H)), np.zeros((K, H))
    for v, e in _hinges(t, d, p):
        on = v > 0
        j = np.where(on, v * v / 2.0, 0.0)
        E += np.where(on, np.abs(v) * e + 2.0 * U * j, 0.0)
        J += j
        A += on
    adds = np.maximum(A.max(axis=1) - 1, 0) + int(np.ceil(np.log2(H)))
    return 1.05 * (E.sum(axis=1) + U * adds * J.sum(axis=1))


def _obstacles(rng, t, M, P, keep_free):
    """One scene's discs [1, M, 5] and planes [1, P, 3] (None at a count of 0), fp32: centres in [-0.9, 0.9]^2 drifting by up to
    0.3 over the horizon, radii 0.2 .. 0.6, planes with a random normal.  `keep_free` = k: radii shrink and plane offsets grow
    until candidate k violates nothing (a disc left with r < 0.05 becomes an empty slot)."""
    K, H, _ = t.shape
    d = np.zeros((M, 5))
    d[:, :2] = rng.uniform(-0.9, 0.9, size=(M, 2))
    d[:, 2:4] = rng.uniform(-0.3, 0.3, size=(M, 2)) / H
    d[:, 4] = rng.uniform(0.2, 0.6, size=M)
    p = np.zeros((P, 3))
    p[:, :2] = rng.uniform(-1.0, 1.0, size=(P, 2))
    p[:, 2] = rng.uniform(-0.1, 0.8, size=P)
    d, p = d.astype(F32).astype(F64), p.astype(F32).astype(F64)
    if keep_free is not None:
        xy = t[keep_free, :, :2].astype(F64)
        hf = np.arange(H)[:, None]
        for i in range(M):
            dist = np.sqrt(((xy - (d[i, :2] + hf * d[i, 2:4])) ** 2).sum(-1)).min()
            d[i, 4] = min(d[i, 4], 0.8 * dist)
            if d[i, 4] < 0.05:
                d[i, 4] = 0.0
        for i in range(P):
            p[i, 2] = max(p[i, 2], (xy @ p[i, :2]).max() + 0.05)
    return (d[None].astype(F32) if M else None), (p[None].astype(F32) if P else None)


def make_case(shape, weights, hard, seed):
    """One case: dict(S, K, H, D, M, P, weights, hard, target [S, 2], trajs [K * S, H, D], discs, planes, bound [S, K],
    some_free [S]).  Every scene is redrawn -- candidates and obstacles, same stream, next draw -- until
      (a) every hinge stands clear of its kink (`hinges_clear`), so that `active` and `free` are what fp32 finds too;
      (b) every candidate's derived `violation_error` fits guide_ref.cost_bound.  That bound counts relative roundings per term,
          which a shallow hinge (phi near 0: 1 - d2 / r^2 cancels) does not keep; a case holds the scenes where it holds by
          derivation, so the cost bound below is one too;
      (c) the two smallest costs of the set the rule searches differ by more than GAP = 8 times the bound (a set of one is
          decided).
    Odd scenes keep a drawn candidate free; even scenes take their obstacles as drawn, dense enough that usually nothing is free.
    Under "w_guide alone" two free candidates would tie at exactly 0, so nothing is kept free there."""
    S, K, H, D, M, P = shape
    rng = np.random.default_rng([seed, S, K, H, D, M, P, int(hard)] + [int(w * 8) for w in weights])
    target = rng.uniform(-1.0, 1.0, size=(S, 2)).astype(F32)
    guide_alone = all(w == 0 for w in weights[:3])
    trajs = np.empty((K, S, H, D), F32)
    discs = np.zeros((S, M, 5), F32) if M else None
    planes = np.zeros((S, P, 3), F32) if P else None
    bound = np.empty((S, K))
    some_free = np.zeros(S, bool)
    for s in range(S):
        for _ in range(2000):
            t = R._scene(rng, K, H, D)
            keep = int(rng.integers(K)) if (s % 2 == 1 and not guide_alone) else None
            d, p = _obstacles(rng, t, M, P, keep)
            if (S, M) == (3, 2):                       # the shape of the special slots: r = 0 in scene 0, a NaN radius in scene 1
                if s == 0:
                    d[0, 0, 4] = 0.0
                if s == 1:
                    d[0, 1, 4] = np.nan
            if not hinges_clear(t, d, p) or (violation_error(t, d, p) > G.cost_bound(t, d, p)).any():
                continue
            got = select(t[:, None], 1, target[s:s + 1], weights, hard, d, p)
            b = cost_bound(t[:, None], 1, weights, True, d, p)
            c = np.sort(got["cost"][0][searched(got["cost"], got["free"], hard)[0]])
            if not np.isfinite(got["cost"]).all() or (len(c) > 1 and c[1] - c[0] <= GAP * b.max()):
                continue
            if keep is not None and not got["free"][0, keep]:
                continue
            if K == 1 and not got["active"].any():     # a lone candidate that violates nothing would compare zeros
                continue
            break
        else:
            raise AssertionError(("no scene with a decided winner", shape, weights, hard))
        trajs[:, s], bound[s], some_free[s] = t, b[0], got["free"][0].any()
        if M:
            discs[s] = d[0]
        if P:
            planes[s] = p[0]
    return dict(S=S, K=K, H=H, D=D, M=M, P=P, name=None, weights=weights, hard=hard, target=target,
                trajs=trajs.reshape(K * S, H, D), discs=discs, planes=planes, bound=bound, some_free=some_free)


_CASES = {}


def cases(seed: int = 2025):
    """Every shape under every weight setting, computed once per process and shared (callers leave the arrays unchanged)."""
    if seed not in _CASES:
        out = []
        for shape in SHAPES:
            for name, w, hard in WEIGHTS:
                c = make_case(shape, w, hard, seed)
                c["name"] = name
                out.append(c)
        _CASES[seed] = out
    return _CASES[seed]
