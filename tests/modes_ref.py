"""fp64 NumPy restatement of "trajectory modes v1" (include/adx.h: adx_traj_modes), the fp32 error bound of a kernel that
evaluates its distances, the seeded fixture generator and the hand-built scenes the CPU and GPU tests share.  Arithmetic only,
written from the contract.

    points     p_h = the first min(D, 2) columns of waypoint h; a missing y column counts as 0; h = h0 .. H-1 are scored
    finite     candidate k is finite when every scored xy of it is finite
    dist2      dist2[i][j] = mean over the scored h of |p_i,h - p_j,h|^2
    near       both finite and dist2 <= r2, r2 = fl32(radius * radius)
    cover      alive = the finite candidates; for m < M while alive is not empty: n_i = alive j near i; rep = the smallest i with
               the largest n_i; index[m] = rep, mass[m] = n_rep; the alive j near rep get assign = m and leave
    the rest   alive after M modes: assign -1; non-finite: assign -2; slots m >= count: index -1, mass 0
    modes      row m * S + s = row index[m] * S + s of trajs bit for bit; m >= count: mode 0's row; count 0: zeros
Rows are candidate-major: candidate k of scene s is row k * S + s.
"""
import itertools

import numpy as np

from select_ref import _scene, gamma

OUTLIER, NON_FINITE = -1, -2


def r2_of(radius) -> float:
    """radius * radius as the kernel forms it: the fp32 radius, one fp32 product."""
    r = np.float32(radius)
    return float(np.float32(r * r))


def _rows(trajs, scenes):
    t = np.asarray(trajs)
    if t.ndim == 3:
        t = t.reshape(-1, scenes, t.shape[1], t.shape[2])
    assert t.ndim == 4 and t.shape[1] == scenes, t.shape
    return t


def dist2(trajs, scenes, h0):
    """(dist2 [S, K, K] fp64, finite [S, K] bool).  Entries of a non-finite candidate are whatever fp64 gives: they enter nothing."""
    t = _rows(trajs, scenes)
    K, S, H, D = t.shape
    p = np.zeros((K, S, H - h0, 2))
    p[..., :min(D, 2)] = t[:, :, h0:, :min(D, 2)].astype(np.float64)
    finite = np.isfinite(p).all(axis=(2, 3)).T
    with np.errstate(invalid="ignore", over="ignore"):
        d = ((p[:, None] - p[None, :]) ** 2).sum(-1).mean(-1)       # [K, K, S]
    return np.ascontiguousarray(d.transpose(2, 0, 1)), finite


def cover(d, finite, M, r2):
    """The greedy cover of one scene from its [K, K] distances: index [M], mass [M], assign [K], count."""
    K = d.shape[0]
    with np.errstate(invalid="ignore"):
        near = (d <= r2) & finite[:, None] & finite[None, :]
    alive = finite.copy()
    index, mass = np.full(M, -1, dtype=np.int32), np.zeros(M, dtype=np.int32)
    assign = np.where(finite, OUTLIER, NON_FINITE).astype(np.int32)
    count = 0
    for m in range(M):
        if not alive.any():
            break
        n = np.where(alive, (near & alive[None, :]).sum(1), 0)
        rep = int(n.argmax())                     # the first maximum: the smallest i
        took = near[rep] & alive
        index[m], mass[m] = rep, n[rep]
        assert took.sum() == n[rep] and took[rep]
        assign[took] = m
        alive &= ~took
        count = m + 1
    assert K == (mass.sum() + (assign == OUTLIER).sum() + (assign == NON_FINITE).sum())
    return index, mass, assign, count


def modes(trajs, scenes, M, radius, h0):
    """Everything the kernel writes, as a dict: modes [M * S, H, D] (the dtype of trajs, copied bit for bit), index and mass
    [S, M] int32, assign [S, K] int32, count [S] int32, dist2 [S, K, K] fp64; and `finite` [S, K]."""
    t = _rows(trajs, scenes)
    K, S, H, D = t.shape
    r2 = r2_of(radius)
    d, finite = dist2(t, S, h0)
    out = dict(modes=np.zeros((M, S, H, D), dtype=t.dtype), index=np.empty((S, M), dtype=np.int32),
               mass=np.empty((S, M), dtype=np.int32), assign=np.empty((S, K), dtype=np.int32), count=np.empty(S, dtype=np.int32),
               dist2=d, finite=finite)
    for s in range(S):
        index, mass, assign, count = cover(d[s], finite[s], M, r2)
        out["index"][s], out["mass"][s], out["assign"][s], out["count"][s] = index, mass, assign, count
        for m in range(M):
            if count > 0:
                out["modes"][m, s] = t[index[m] if m < count else index[0], s]
    out["modes"] = out["modes"].reshape(M * S, H, D)
    return out


def bound(H: int, h0: int) -> float:
    """Absolute bound on |fp32 dist2 - exact dist2| for inputs with |p| <= 1, every operation rounded once (u = 2^-24), whatever
    the order of the sum (gamma_{n-1} bounds an n-term sum of non-negative numbers in any order).  n = H - h0.

    per waypoint   d^ = fl(p_i - p_j) = d (1 + e), |d| <= 2: the square carries (1 + e)^2 and its own rounding, the sum of the two
                   components one more: 4 roundings on a term t_h <= 8, so every t_h^ is within 8 gamma_4 of t_h -- and so is
                   the mean of the t_h^ of the mean of the t_h.
    the mean       the n terms t_h^ are <= 8 (1 + gamma_4) each.  Their fp32 sum is within gamma_{n-1} of n times that, the
                   division by n (n <= 64 is exact in fp32) adds one rounding: the quotient is within 8 (1 + gamma_4) gamma_n of
                   the exact mean of the t_h^, taken as 9 gamma_n.
    Together 8 gamma_4 + 9 gamma_n: about 3.6e-5 at n = 64."""
    n = H - h0
    assert n >= 1
    return 8.0 * gamma(4) + 9.0 * gamma(n)


def margins(trajs, scenes, radius, h0):
    """Per scene, the smallest |dist2[i][j] - r2| over the finite pairs i < j (inf where a scene has no such pair)."""
    d, finite = dist2(trajs, scenes, h0)
    r2 = r2_of(radius)
    S, K, _ = d.shape
    out = np.full(S, np.inf)
    iu = np.triu_indices(K, 1)
    for s in range(S):
        ok = finite[s][iu[0]] & finite[s][iu[1]]
        if ok.any():
            out[s] = np.abs(d[s][iu][ok] - r2).min()
    return out


# ---- fixtures -------------------------------------------------------------------------------------------------------------
SCENES, CANDIDATES, HORIZONS, DIMS = (1, 3), (1, 2, 33, 63, 64), ((1, 0), (2, 1), (32, 1), (64, 0)), (1, 2, 7, 16)
QUANTILE, WINDOW = 0.3, 8


def _radius(t, h0):
    """A radius for the scene t [K, H, D]: r2 at the midpoint of the widest gap between two neighbouring values of the sorted
    pair distances (0, the distance of a candidate to itself, in front) within WINDOW places of their QUANTILE: never on a value."""
    d, _ = dist2(t[:, None], 1, h0)
    K = t.shape[0]
    v = np.concatenate([[0.0], np.sort(d[0][np.triu_indices(K, 1)])])
    if len(v) == 1:
        return 0.1                                 # K = 1: nothing to separate
    q = int(QUANTILE * (len(v) - 1))
    lo, hi = max(0, q - WINDOW), min(len(v) - 1, q + WINDOW + 1)
    gaps = v[lo + 1:hi + 1] - v[lo:hi]
    i = lo + int(gaps.argmax())
    return float(np.sqrt(0.5 * (v[i] + v[i + 1])))


def make_case(S, K, H, D, M, h0, seed):
    """One fixture: dict(S, K, H, D, M, h0, radius, trajs [K * S, H, D] fp32, bound).  The radius comes from the first draw of
    scene 0 (`_radius`); every scene is then redrawn (same stream, next draw) until every pair's distance is more than FOUR times
    the fp32 bound away from r2 -- twice what the tests assert -- so that every integer output is decided by the contract and
    not by rounding: a test may compare EVERY scene."""
    rng = np.random.default_rng([seed, S, K, H, D, M, h0])
    b = bound(H, h0)
    trajs = np.empty((K, S, H, D), dtype=np.float32)
    radius = None
    for s in range(S):
        for _ in range(1000):
            t = _scene(rng, K, H, D)
            if radius is None:
                radius = float(np.float32(_radius(t, h0)))
            if margins(t[:, None], 1, radius, h0)[0] > 4.0 * b:
                break
        else:
            raise AssertionError(("no scene clear of the radius", S, K, H, D, M, h0))
        trajs[:, s] = t
    return dict(S=S, K=K, H=H, D=D, M=M, h0=h0, radius=radius, trajs=trajs.reshape(K * S, H, D), bound=b)


def cases(seed: int = 2025):
    """Every (S, K, (H, h0), D) of the grid with one M of (1, 6, K) each, rotating so that every M meets every K and every D."""
    out = []
    for n, (S, K, (H, h0), D) in enumerate(itertools.product(SCENES, CANDIDATES, HORIZONS, DIMS)):
        M = (1, 6, K)[(n + n // len(DIMS)) % 3]
        out.append(make_case(S, K, H, D, M, h0, seed))
    return out


# ---- hand-built scenes with known answers ---------------------------------------------------------------------------------
def _along_x(xs, H=4, D=3, h0=1):
    """One scene [K, H, D] fp32: candidate k is the straight path y = 0.1 h shifted by xs[k] in x on every waypoint, so that
    dist2[i][j] = (xs[i] - xs[j])^2; columns >= 2 and the waypoints below h0 hold values that differ per candidate (they must
    not matter)."""
    K = len(xs)
    t = np.zeros((K, H, D), dtype=np.float32)
    t[:, :, 0] = np.asarray(xs, dtype=np.float32)[:, None]
    if D > 1:
        t[:, :, 1] = 0.1 * np.arange(H, dtype=np.float32)[None, :]
    if D > 2:
        t[:, :, 2:] = np.linspace(-1.0, 1.0, K, dtype=np.float32)[:, None, None]
    t[:, :h0, :min(D, 2)] = np.linspace(-0.9, 0.9, K, dtype=np.float32)[:, None, None]
    return t


A, B, C = 0.0, 0.5, -0.5                          # three places far apart; members differ by multiples of 0.001
THREE = [A, B, A + .001, A + .002, C, B + .001, A + .003, B + .002, A + .004]       # A: 0 2 3 6 8, B: 1 5 7, C: 4


def hand_cases():
    """[(name, dict(trajs [K, H, D] fp32 of ONE scene, M, radius, h0), dict(index, mass, assign, count))].  `modes` follows from
    `index` and `count` by the contract's rule (tests check it with `expected_rows`)."""
    out = []
    three = _along_x(THREE)
    want3 = dict(index=[0, 1, 4, -1, -1, -1], mass=[5, 3, 1, 0, 0, 0], assign=[0, 1, 0, 0, 2, 1, 0, 1, 0], count=3)
    out.append(("three tight clusters of 5 / 3 / 1", dict(trajs=three, M=6, radius=0.1, h0=1), want3))
    # the bridge (0.165) is near A's 0.02 and 0.03 and B's 0.30 and 0.31 under radius 0.15: n = 5; A's 0.02 and 0.03 see all of A
    # and the bridge: n = 6, the smaller index (4) wins and takes the bridge; B is left with its three
    bridge = _along_x([0.165, 0.0, 0.005, 0.01, 0.02, 0.03, 0.30, 0.31, 0.32])
    out.append(("a bridge goes to the heavier cluster and is gone for the second", dict(trajs=bridge, M=6, radius=0.15, h0=1),
                dict(index=[4, 6, -1, -1, -1, -1], mass=[6, 3, 0, 0, 0, 0], assign=[0, 0, 0, 0, 0, 0, 1, 1, 1], count=2)))
    out.append(("equal counts go to the lowest index", dict(trajs=_along_x([B, A, A + .001, B + .001]), M=3, radius=0.1, h0=1),
                dict(index=[0, 1, -1], mass=[2, 2, 0], assign=[0, 1, 1, 0], count=2)))
    out.append(("M smaller than the number of clusters leaves outliers", dict(trajs=three, M=2, radius=0.1, h0=1),
                dict(index=[0, 1], mass=[5, 3], assign=[0, 1, 0, 0, -1, 1, 0, 1, 0], count=2)))
    out.append(("duplicates at radius 0", dict(trajs=_along_x([A, B, A, A, B, C]), M=4, radius=0.0, h0=1),
                dict(index=[0, 1, 5, -1], mass=[3, 2, 1, 0], assign=[0, 1, 0, 0, 1, 2], count=3)))
    bad = three.copy()
    bad[2, 2, 0] = np.nan                         # an A: a NaN x at a scored waypoint
    bad[7, 3, 1] = np.inf                         # a B: an infinite y
    out.append(("a non-finite scored xy takes the candidate out", dict(trajs=bad, M=6, radius=0.1, h0=1),
                dict(index=[0, 1, 4, -1, -1, -1], mass=[4, 2, 1, 0, 0, 0], assign=[0, 1, -2, 0, 2, 1, 0, -2, 0], count=3)))
    quiet = three.copy()
    quiet[0, 0, 0] = np.nan                       # below h0
    quiet[1, 0, 1] = np.inf
    quiet[3, 2, 2] = np.nan                       # a column >= 2
    quiet[4, 3, 2] = -np.inf
    out.append(("a NaN below h0 or in a column >= 2 has no effect", dict(trajs=quiet, M=6, radius=0.1, h0=1), want3))
    none = three.copy()
    none[:, 1, 0] = np.nan
    none[::2, 1, 0] = np.inf
    out.append(("no finite candidate: count 0 and zero rows", dict(trajs=none, M=3, radius=0.1, h0=1),
                dict(index=[-1, -1, -1], mass=[0, 0, 0], assign=[-2] * 9, count=0)))
    out.append(("one column: a missing y counts as 0", dict(trajs=_along_x(THREE, D=1), M=6, radius=0.1, h0=1), want3))
    return out


def expected_rows(trajs, index, count, M):
    """The contract's `modes` of one scene [M, H, D] from its index and count."""
    rows = np.zeros((M,) + trajs.shape[1:], dtype=trajs.dtype)
    for m in range(M):
        if count > 0:
            rows[m] = trajs[index[m] if m < count else index[0]]
    return rows


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
