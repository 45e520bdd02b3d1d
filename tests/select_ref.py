"""fp64 NumPy restatement of "selection cost v1" (include/adx.h: adx_traj_select), the fp32 error bound of a kernel that
evaluates it, and the seeded fixture generator the CPU and GPU tests share.  Arithmetic only, written from the contract.

    points     p_h = the first min(D, 2) columns of waypoint h; a missing y column counts as 0
    goal       min over h of |p_h - g_s|^2                      (0 without a target; w_goal is then ignored)
    smooth     mean over h = 1..H-2 of |p_{h+1} - 2 p_h + p_{h-1}|^2        (0 when H < 3)
    consensus  mean over h of |p_h - m_h|^2, m_h = mean of p_h over the scene's K candidates
    cost       w_goal goal + w_smooth smooth + w_consensus consensus; a term whose weight is exactly 0 is not evaluated
    index      the smallest k with the smallest cost; a non-finite cost loses to every finite one; none finite -> 0
Rows are candidate-major: candidate k of scene s is row k * S + s.
"""
import itertools

import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32


def gamma(n: int) -> float:
    """Higham's gamma_n = n u / (1 - n u): the relative error bound of n chained fp32 roundings."""
    return n * U / (1.0 - n * U)


def _xy(trajs, scenes):
    t = np.asarray(trajs, dtype=np.float64)
    if t.ndim == 3:
        t = t.reshape(-1, scenes, t.shape[1], t.shape[2])
    K, S, H, D = t.shape
    assert S == scenes
    p = np.zeros((K, S, H, 2))
    p[..., :min(D, 2)] = t[..., :min(D, 2)]
    return p


def terms(trajs, scenes, target=None):
    """(goal, smooth, consensus), each [S, K] in fp64; goal is None without a target."""
    p = _xy(trajs, scenes)
    K, S, H, _ = p.shape
    goal = None
    if target is not None:
        g = np.asarray(target, dtype=np.float64).reshape(S, 2)
        goal = ((p - g[None, :, None, :]) ** 2).sum(-1).min(-1).T
    if H >= 3:
        a = p[:, :, 2:] - 2.0 * p[:, :, 1:-1] + p[:, :, :-2]
        smooth = (a ** 2).sum(-1).mean(-1).T
    else:
        smooth = np.zeros((S, K))
    m = p.mean(0, keepdims=True)
    cons = ((p - m) ** 2).sum(-1).mean(-1).T
    return goal, smooth, cons


def select(trajs, scenes, target=None, weights=(1.0, 0.0, 0.0)):
    """cost [S, K] (fp64) and index [S] (int32).  The weights are taken as the fp32 numbers the kernel is handed."""
    wg, ws, wc = (float(np.float32(w)) for w in weights)
    with np.errstate(invalid="ignore", over="ignore"):
        goal, smooth, cons = terms(trajs, scenes, target)
        cost = np.zeros_like(smooth)
        if goal is not None and wg != 0.0:
            cost = cost + wg * goal
        if ws != 0.0:
            cost = cost + ws * smooth
        if wc != 0.0:
            cost = cost + wc * cons
    return cost, pick(cost)


def pick(cost):
    key = np.where(np.isfinite(cost), cost, np.inf)
    return key.argmin(-1).astype(np.int32)        # argmin returns the first minimum; all +inf -> 0


def cost_bound(K: int, H: int, weights, has_target: bool) -> float:
    """Absolute bound on |fp32 cost - exact cost| for inputs with |p| <= 1 and |g| <= 1, every operation rounded once
    (u = 2^-24), whatever the order of the sums (gamma_{n-1} bounds an n-term sum of non-negative numbers in any order).

    goal       d^ = fl(p - g) = d (1 + e), |d| <= 2; squaring and adding the two components: 4 roundings on a term <= 8, so
               every per-waypoint term is within 8 gamma_4, and so is their minimum.
    smooth     a^ = fl(fl(p_{h+1} - 2 p_h) + p_{h-1}): 2 p_h is exact, |p_{h+1} - 2 p_h| <= 3 and |a| <= 4, so |a^ - a| <= 7u
               (8u with the second-order part); |a^2 - a^2| <= (8 + 8u) 8u <= 65u, its rounding adds <= 17u: 82u per component
               (taken as 96u), two components and their sum's rounding (<= 33u): 225u per term, taken as 256u.  The n = H - 2
               terms are <= 33 each: the sum is within gamma_{n-1} 33 n of theirs, the division adds u: 256u + 33 gamma_n.
    consensus  m^ = fl(sum / K): |m^ - m| <= gamma_{K-1} + u(1 + ..) <= gamma_K.  d^ = fl(p - m^): |d^ - d| <= gamma_K + 2.1u
               <= gamma_{K+3} =: e, |d| <= 2: |d^2 - d^2| <= (4 + e) e, the rounding adds 4.1u: <= 5 gamma_{K+4} per component, two
               components and the sum's rounding: <= 10 gamma_{K+5} per term.  H terms <= 8.1 each, summed and divided by H:
               + 8.1 gamma_H, taken as 9 gamma_H.
    weighted   three products and two sums, each one rounding of a partial sum of magnitude <= T = 8 |w_g| + 32 |w_s| + 8 |w_c|
               (the largest values the terms can take): gamma_4 T covers them with room for the terms' own errors.
    A term with weight 0 (or the goal term without a target) is not evaluated and contributes nothing."""
    wg, ws, wc = (abs(float(np.float32(w))) for w in weights)
    if not has_target:
        wg = 0.0
    e = wg * 8.0 * gamma(4)
    if H >= 3:
        e += ws * (256.0 * U + 33.0 * gamma(H - 2))
    else:
        ws = 0.0
    e += wc * (10.0 * gamma(K + 5) + 9.0 * gamma(H))
    return e + gamma(4) * (8.0 * wg + 32.0 * ws + 8.0 * wc)


# ---- fixtures -------------------------------------------------------------------------------------------------------------
SCENES, CANDIDATES, HORIZONS, DIMS = (1, 3), (2, 7, 16, 64), (8, 32, 64), (1, 2, 7, 16)
# (w_goal, w_smooth, w_consensus, with a target).  Every weight is a dyadic number: exact in fp32.  The consensus term never
# stands alone: at K = 2 both candidates are equally far from their mean, an exact tie by construction.
WEIGHTS = ((1.0, 0.0, 0.0, True), (0.0, 1.0, 0.0, False), (1.0, 0.5, 0.25, True), (2.0, 1.0, 1.0, True), (1.0, 0.5, 1.0, False),
           (0.0, 0.25, 2.0, True))


def _scene(rng, K, H, D):
    """K paths of one scene, fp32 [K, H, D] in [-1, 1]: per candidate a low-frequency curve (offset, drift, three sinusoids)
    plus a mild per-candidate jitter, so that the candidates differ in every term of the cost; xy rescaled to a random
    amplitude <= 1, the other columns uniform."""
    tau = np.linspace(0.0, 1.0, H)[None, :, None]
    j = np.arange(1, 4)[None, None, None, :]
    amp = rng.uniform(-0.5, 0.5, size=(K, 1, 2, 3))
    phase = rng.uniform(0.0, 2.0 * np.pi, size=(K, 1, 2, 3))
    xy = rng.uniform(-0.5, 0.5, size=(K, 1, 2)) + rng.uniform(-1.0, 1.0, size=(K, 1, 2)) * tau
    xy = xy + (amp * np.sin(np.pi * j * tau[..., None] + phase)).sum(-1)
    xy = xy + 0.2 * np.sqrt(rng.uniform(0.0, 1.0, size=(K, 1, 1))) * rng.uniform(-1.0, 1.0, size=(K, H, 2))
    xy *= rng.uniform(0.3, 1.0, size=(K, 1, 1)) / np.abs(xy).max(axis=(1, 2), keepdims=True)
    t = rng.uniform(-1.0, 1.0, size=(K, H, D))
    t[..., :min(D, 2)] = xy[..., :min(D, 2)]
    t = t.astype(np.float32)
    assert np.abs(t).max() <= 1.0
    return t


def gap(cost):
    """Per scene: second-smallest minus smallest cost."""
    s = np.sort(cost, axis=-1)
    return s[..., 1] - s[..., 0]


def make_case(S, K, H, D, weights, seed):
    """One fixture: dict(S, K, H, D, weights, target [S, 2] fp32 or None, trajs [K * S, H, D] fp32, bound).  Every scene is
    redrawn (same stream, next draw) until the reference's best and second-best costs are more than twice the fp32 bound apart,
    so that the index is decided by the contract and not by rounding: a test may compare the index of EVERY scene."""
    wg, ws, wc, with_target = weights
    rng = np.random.default_rng([seed, S, K, H, D, int(with_target), int(wg * 8), int(ws * 8), int(wc * 8)])
    target = rng.uniform(-1.0, 1.0, size=(S, 2)).astype(np.float32) if with_target else None
    bound = cost_bound(K, H, (wg, ws, wc), with_target)
    trajs = np.empty((K, S, H, D), dtype=np.float32)
    for s in range(S):
        for _ in range(1000):
            t = _scene(rng, K, H, D)
            c, _ = select(t[:, None], 1, None if target is None else target[s:s + 1], (wg, ws, wc))
            if gap(c)[0] > 4.0 * bound:       # twice what the tests need
                break
        else:
            raise AssertionError(("no scene with a decided winner", S, K, H, D, weights))
        trajs[:, s] = t
    return dict(S=S, K=K, H=H, D=D, weights=(wg, ws, wc), target=target, trajs=trajs.reshape(K * S, H, D), bound=bound)


def cases(seed: int = 2024):
    """Every (S, K, H, D) of the grid with two of the weight settings each, rotating so that every setting meets every K."""
    out = []
    for n, (S, K, H, D) in enumerate(itertools.product(SCENES, CANDIDATES, HORIZONS, DIMS)):
        for w in (WEIGHTS[n % len(WEIGHTS)], WEIGHTS[(n // len(DIMS) + 3) % len(WEIGHTS)]):
            out.append(make_case(S, K, H, D, w, seed))
    return out
