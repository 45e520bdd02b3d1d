"""fp64 NumPy restatement of "open-loop metrics v1" (include/adx.h: adx_traj_metrics, adx_metrics_accumulate), the fp32 error bound
of a kernel that evaluates it, the inputs the CPU and GPU tests share, and the accumulation recomputed on the host in the
kernel's order.  Arithmetic only, written from the contract; xy_scale and miss_radius are taken as the fp32 numbers the kernel is
handed.

    n         clamp(valid[s], 0, H) (valid None: H); scored: n > h0 and 0 <= index[s] < K (index None: 0)
    disp      |((x, y) - (gx, gy)) xy_scale| for h0 <= h < n, 0 elsewhere
    ade       sum_h disp / (n - h0);  fde = disp[n - 1]
    search    the smallest k among the smallest finite values; none finite: 0
    rec       ade[best], fde[argmin fde], ade[index], fde[index], along, cross, sel_fde > R, min_fde > R
    heading   d = gt[n-1] - gt[n-2], valid when n - h0 >= 2 and 0 < |d| < inf; u = d / |d|; e = the chosen final error;
              along = e.x u.x + e.y u.y, cross = e.y u.x - e.x u.y
    flags     1 scored | 2 heading valid | 4 sel_ade finite | n << 8 | h0 << 16;  an unscored scene: zeros everywhere

The bound (u = 2^-24, gamma_n = n u / (1 - n u), every fp32 operation rounded once, no contraction; magnitudes far from fp32's
underflow threshold, as everything a planner produces is):
    ex        fl(fl(x - gx) * s) = (x - gx) s (1 + t2), |t2| <= gamma_2
    ex^2      one more rounding on two factors: gamma_5;  ex^2 + ey^2 (non-negative terms, one rounding): gamma_6
    disp      sqrt(v (1 + t6)) (1 + d): |sqrt(1 + t) - 1| <= |t| for |t| <= 1, so gamma_6 + u + gamma_6 u <= gamma_7:  E = gamma_7 disp
    fde       one disp: gamma_7 fde
    ade       m = n - h0 non-negative terms in ANY order: gamma_{m-1} on top (the lanes that hold 0 add exactly), (float)m is
              exact, the division rounds once: gamma_{7 + m - 1 + 1} ade = gamma_{m+7} ade
    u.x       d.x one rounding; |d|: d.x^2 gamma_3, the sum gamma_4, the root gamma_5; 1 / (1 + t5) <= 1 + gamma_6; the division one
              more: gamma_8
    along     ex u.x: gamma_2 + gamma_8 + one rounding = gamma_11, the sum one more: gamma_12 (|ex u.x| + |ey u.y|); cross likewise
    min_*     |min_k a_k - min_k b_k| <= max_k |a_k - b_k|: the largest bound among the finite candidates
On top of each: 2^-45 of the value for the fp64 evaluation's own rounding.
"""
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32
XY_SCALE = 23.315       # model.magic_num
MISS_RADIUS = 2.0
REC = ("min_ade", "min_fde", "sel_ade", "sel_fde", "along", "cross", "miss_sel", "miss_any")
SCORED, HEADING, FINITE = 1, 2, 4
# the state's words (include/adx.h, "Accumulation")
W_SCORED, W_NONFINITE, W_HEADING, W_AGREE, W_BLOCKED, W_REC, W_REGRET, W_ALONG, W_CROSS, W_DISP, W_DISP_COUNT, WORDS = \
    0, 1, 2, 3, 4, 5, 13, 14, 15, 16, 80, 144
SHAPES = [(1, 1, 2, 2), (3, 2, 16, 7), (5, 7, 24, 3), (2, 64, 64, 2)]      # (S, K, H, D)


def gamma(n: int) -> float:
    """Higham's gamma_n = n u / (1 - n u): the relative error bound of n chained fp32 roundings."""
    return n * U / (1.0 - n * U)


def f32(v) -> float:
    return float(np.float32(v))


def argmin_finite(v) -> int:
    """The smallest k among the smallest finite v_k; no finite v_k: 0."""
    v = np.asarray(v, dtype=np.float64)
    return int(np.where(np.isfinite(v), v, np.inf).argmin())


def _clamp_valid(valid, S, H):
    return np.full(S, H, dtype=np.int64) if valid is None else np.clip(np.asarray(valid, dtype=np.int64), 0, H)


def metrics(trajs, gt, valid=None, index=None, h0=1, miss_radius=MISS_RADIUS, xy_scale=XY_SCALE):
    """trajs [K * S, H, D] or [K, S, H, D], gt [S, H, 2] (fp32 numbers).  -> ade, fde [S, K], best [S], rec [S, 8], flags [S],
    disp_sel [S, H], and `e` [S, 2, 2] = (|ex u.x|, |ey u.y|), (|ey u.x|, |ex u.y|): the products the bound of along / cross needs."""
    gt = np.asarray(gt, dtype=np.float64)
    S, H = gt.shape[:2]
    t = np.asarray(trajs, dtype=np.float64).reshape(-1, S, H, np.shape(trajs)[-1])
    K = t.shape[0]
    scale, R = f32(xy_scale), f32(miss_radius)
    n_all = _clamp_valid(valid, S, H)
    idx_all = np.zeros(S, dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64)
    out = SimpleNamespace(ade=np.zeros((S, K)), fde=np.zeros((S, K)), best=np.zeros(S, dtype=np.int32), rec=np.zeros((S, 8)),
                          flags=np.zeros(S, dtype=np.int32), disp_sel=np.zeros((S, H)), e=np.zeros((S, 2, 2)), n=n_all)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            n, sel = int(n_all[s]), int(idx_all[s])
            if not (n > h0 and 0 <= sel < K):
                continue
            err = (t[:, s, h0:n, :2] - gt[s, h0:n]) * scale                       # [K, m, 2]
            disp = np.sqrt(err[..., 0] * err[..., 0] + err[..., 1] * err[..., 1])
            ade, fde = disp.sum(axis=1) / (n - h0), disp[:, -1]
            best, best_f = argmin_finite(ade), argmin_finite(fde)
            flags = SCORED | (n << 8) | (h0 << 16)
            along = cross = 0.0
            if n - h0 >= 2:
                d = gt[s, n - 1] - gt[s, n - 2]
                length = np.sqrt(d[0] * d[0] + d[1] * d[1])
                if 0.0 < length < np.inf:
                    ux, uy = d / length
                    ex, ey = err[sel, -1]
                    along, cross = ex * ux + ey * uy, ey * ux - ex * uy
                    out.e[s] = [[abs(ex * ux), abs(ey * uy)], [abs(ey * ux), abs(ex * uy)]]
                    flags |= HEADING
            if np.isfinite(ade[sel]):
                flags |= FINITE
            out.ade[s], out.fde[s], out.best[s], out.flags[s] = ade, fde, best, flags
            out.disp_sel[s, h0:n] = disp[sel]
            out.rec[s] = [ade[best], fde[best_f], ade[sel], fde[sel], along, cross, float(fde[sel] > R), float(fde[best_f] > R)]
    return out


def metrics_loops(trajs, gt, valid=None, index=None, h0=1, miss_radius=MISS_RADIUS, xy_scale=XY_SCALE):
    """The same contract as plain Python loops over scenes, candidates and waypoints: `(ade, fde, best, rec, flags, disp_sel)` as
    lists.  Written on its own from the header, to check the vectorised restatement."""
    import math
    gt = np.asarray(gt, dtype=np.float64)
    S, H = gt.shape[:2]
    t = np.asarray(trajs, dtype=np.float64).reshape(-1, S, H, np.shape(trajs)[-1])
    K = t.shape[0]
    scale, R = f32(xy_scale), f32(miss_radius)
    fin = lambda v: not (math.isnan(v) or math.isinf(v))      # noqa: E731

    def search(vals):
        pick, low = 0, math.inf
        for k, v in enumerate(vals):
            if fin(v) and v < low:
                pick, low = k, v
        return pick

    A, F, B, RC, FL, DS = [], [], [], [], [], []
    for s in range(S):
        n = H if valid is None else min(max(int(valid[s]), 0), H)
        sel = 0 if index is None else int(index[s])
        if n <= h0 or sel < 0 or sel >= K:
            A.append([0.0] * K); F.append([0.0] * K); B.append(0); RC.append([0.0] * 8); FL.append(0); DS.append([0.0] * H)
            continue
        ade, fde, rows, errs = [], [], [], []
        for k in range(K):
            row, total, e = [0.0] * H, 0.0, (0.0, 0.0)
            for h in range(h0, n):
                e = ((float(t[k, s, h, 0]) - float(gt[s, h, 0])) * scale, (float(t[k, s, h, 1]) - float(gt[s, h, 1])) * scale)
                sq = e[0] * e[0] + e[1] * e[1]
                row[h] = math.sqrt(sq) if sq == sq and sq >= 0 else math.nan
                total += row[h]
            ade.append(total / (n - h0)); fde.append(row[n - 1]); rows.append(row); errs.append(e)
        best, best_f = search(ade), search(fde)
        flags, along, cross = SCORED | (n << 8) | (h0 << 16), 0.0, 0.0
        if n - h0 >= 2:
            dx, dy = float(gt[s, n - 1, 0] - gt[s, n - 2, 0]), float(gt[s, n - 1, 1] - gt[s, n - 2, 1])
            length = math.sqrt(dx * dx + dy * dy) if fin(dx * dx + dy * dy) else math.nan
            if fin(length) and length > 0:
                ux, uy = dx / length, dy / length
                along, cross = errs[sel][0] * ux + errs[sel][1] * uy, errs[sel][1] * ux - errs[sel][0] * uy
                flags |= HEADING
        if fin(ade[sel]):
            flags |= FINITE
        A.append(ade); F.append(fde); B.append(best); FL.append(flags); DS.append(rows[sel])
        RC.append([ade[best], fde[best_f], ade[sel], fde[sel], along, cross, 1.0 if fde[sel] > R else 0.0, 1.0 if fde[best_f] > R else 0.0])
    return A, F, B, RC, FL, DS


def bound(ref, h0=1):
    """The fp32 error bounds of a kernel that evaluates the contract, from the restatement's own values (module docstring):
    ade, fde [S, K], disp_sel [S, H], along, cross [S] and rec [S, 8] (the miss fields: 0, they are exact or wrong)."""
    S, K = ref.ade.shape
    own = 2.0 ** -45
    m = np.maximum(ref.n - h0, 1)
    g_ade = np.array([gamma(int(v) + 7) for v in m])[:, None]
    b = SimpleNamespace(ade=(g_ade + own) * np.abs(ref.ade), fde=(gamma(7) + own) * np.abs(ref.fde),
                        disp_sel=(gamma(7) + own) * np.abs(ref.disp_sel),
                        along=(gamma(12) + own) * ref.e[:, 0].sum(axis=1), cross=(gamma(12) + own) * ref.e[:, 1].sum(axis=1))
    worst = lambda v: np.where(np.isfinite(v), v, 0.0).max(axis=1)      # noqa: E731
    finite = lambda v: np.abs(np.where(np.isfinite(v), v, 0.0))         # noqa: E731
    b.rec = np.zeros((S, 8))
    b.rec[:, 0], b.rec[:, 1] = worst(b.ade), worst(b.fde)
    b.rec[:, 2] = (g_ade[:, 0] + own) * finite(ref.rec[:, 2])
    b.rec[:, 3] = (gamma(7) + own) * finite(ref.rec[:, 3])
    b.rec[:, 4], b.rec[:, 5] = b.along, b.cross
    return b


def margins(ref, b, miss_radius=MISS_RADIUS):
    """Per scored scene what decides `best` and the two miss fields, each as (margin, allowed rounding): the gap between the two
    smallest finite ADEs against the largest ADE bound, and the distance of sel_fde and min_fde from the radius against their
    bounds.  A test demands margin > 2 * allowed before it asks a kernel for the exact decision."""
    R = f32(miss_radius)
    out = []
    for s in range(ref.ade.shape[0]):
        if not ref.flags[s] & SCORED:
            continue
        # equal values once: bit-identical rows give one value in any deterministic evaluation, and the tie rule picks among them
        a = np.unique(ref.ade[s][np.isfinite(ref.ade[s])])
        gap = np.inf if a.size < 2 else float(a[1] - a[0])
        m = {"best": (gap, float(b.rec[s, 0]))}
        if np.isfinite(ref.rec[s, 3]):
            m["miss_sel"] = (abs(float(ref.rec[s, 3]) - R), float(b.rec[s, 3]))
        if np.isfinite(ref.rec[s, 1]):
            m["miss_any"] = (abs(float(ref.rec[s, 1]) - R), float(b.rec[s, 1]))
        out.append((s, m))
    return out


def case(S, K, H, D, seed=0):
    """The construction the tests share: gt uniform in [-0.3, 0.3]; candidate k = gt + a constant offset of length
    0.008 (p(k) + 1) in direction (cos k, sin k), p a permutation drawn per scene, + noise within 1e-4 per coordinate; the other
    columns uniform in [-1, 1].  -> (trajs [K * S, H, D] float32 candidate-major, gt [S, H, 2] float32, p [S, K])."""
    rng = np.random.default_rng([seed, S, K, H, D])
    gt = rng.uniform(-0.3, 0.3, size=(S, H, 2)).astype(np.float32)
    p = np.stack([rng.permutation(K) for _ in range(S)])
    k = np.arange(K, dtype=np.float64)
    direction = np.stack([np.cos(k), np.sin(k)], axis=-1)                                       # [K, 2]
    t = rng.uniform(-1.0, 1.0, size=(K, S, H, D))
    offset = 0.008 * (p.T[:, :, None, None] + 1.0) * direction[:, None, None, :]                # [K, S, 1, 2]
    t[..., :2] = gt[None].astype(np.float64) + offset + rng.uniform(-1e-4, 1e-4, size=(K, S, H, 2))
    return t.astype(np.float32).reshape(K * S, H, D), gt, p


def accumulate(counts, sums, rec, flags, best, index, disp_sel, blocked, H):
    """adx_metrics_accumulate on the host, in place on the state's two views (`counts` int64 [144] and `sums` float64 [144]; only
    the words of their own kind are meaningful): every statistic walks the scenes in index order in fp64, as its thread does."""
    for s in range(len(flags)):
        f = int(flags[s])
        if not f & SCORED:
            continue
        counts[W_SCORED] += 1
        if not f & FINITE:
            counts[W_NONFINITE] += 1
            continue
        r = [np.float64(v) for v in rec[s]]
        counts[W_HEADING] += 1 if f & HEADING else 0
        counts[W_AGREE] += 1 if int(best[s]) == (0 if index is None else int(index[s])) else 0
        counts[W_BLOCKED] += 1 if blocked is not None and int(blocked[s]) != 0 else 0
        for i in range(8):
            sums[W_REC + i] = sums[W_REC + i] + r[i]
        sums[W_REGRET] = sums[W_REGRET] + (r[2] - r[0])
        if f & HEADING:
            sums[W_ALONG] = sums[W_ALONG] + abs(r[4])
            sums[W_CROSS] = sums[W_CROSS] + abs(r[5])
        n, h0 = (f >> 8) & 0x7F, (f >> 16) & 0x7F
        for h in range(max(h0, 0), min(n, H)):
            sums[W_DISP + h] = sums[W_DISP + h] + np.float64(disp_sel[s, h])
            counts[W_DISP_COUNT + h] += 1
    return counts, sums


def fresh_state():
    return np.zeros(WORDS, dtype=np.int64), np.zeros(WORDS, dtype=np.float64)


def summary(counts, sums, H):
    """The dict `OpenLoopMetrics.compute()` forms from the state, without `units`."""
    n, nh = int(counts[W_SCORED] - counts[W_NONFINITE]), int(counts[W_HEADING])
    mean = lambda v, d: float(v) / d if d > 0 else float("nan")      # noqa: E731
    r = {name: mean(sums[W_REC + i], n) for i, name in enumerate(REC)}
    return {"n": n, "scored": int(counts[W_SCORED]), "nonfinite": int(counts[W_NONFINITE]), "ade": r["sel_ade"], "fde": r["sel_fde"],
            "min_ade_k": r["min_ade"], "min_fde_k": r["min_fde"], "miss_rate": r["miss_sel"], "miss_rate_any": r["miss_any"],
            "selector_regret": mean(sums[W_REGRET], n), "selector_agreement": mean(int(counts[W_AGREE]), n),
            "along": r["along"], "cross": r["cross"], "along_abs": mean(sums[W_ALONG], nh), "cross_abs": mean(sums[W_CROSS], nh),
            "heading_valid": nh, "blocked_rate": mean(int(counts[W_BLOCKED]), n),
            "disp_at": [mean(sums[W_DISP + h], int(counts[W_DISP_COUNT + h])) for h in range(H)]}
