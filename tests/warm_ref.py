"""fp64 NumPy restatement of "warm start v1" (include/adx.h: adx_warm_init), the same operations in fp32 NumPy, the fp32 error
bound of a kernel that evaluates them, and the seeded fixture grid the CPU and GPU tests share.  Arithmetic only, written
from the contract.

    advance  j = h + shift.  j <= H-1: u[h][d] = prev[j][d].  Otherwise d < 2: u[h][d] = prev[H-1][d] + (j - (H-1)) *
             (prev[H-1][d] - prev[H-2][d]);  d >= 2: u[h][d] = prev[H-1][d]
    re-base  o = prev[shift].  No motion: w = u - o in columns d < min(D, 3), u unchanged in the others.  With motion
             (tx, ty, phi): qx = u[.][0] - tx, qy = u[.][1] - ty (a missing y column counts as 0), x' = c qx + s qy,
             y' = -(s qx) + c qy with c = cos(phi), s = sin(phi); column 2 is still u - o[2]
    clamp    to [-1, 1]
    noise    v = sqrt_ab * w + sqrt_1mab * z, z the caller's normals (the stream's INIT_SLOT draw of the logical element)
    zero_first: v = 0 where h == 0 and d < 3
Output row r reads prev[r % prev_rows].
"""
import itertools

import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32; also the spacing of fp32 numbers just below 1


def advance(prev, shift, dtype=np.float64):
    """u [P, H, D]: the plan `shift` waypoints on.  Every operation in `dtype`, rounded on its own."""
    p = np.asarray(prev, dtype=dtype)
    P, H, D = p.shape
    u = np.empty_like(p)
    for h in range(H):
        j = h + shift
        if j <= H - 1:
            u[:, h] = p[:, j]
            continue
        u[:, h] = p[:, H - 1]
        step = p[:, H - 1, :2] - p[:, H - 2, :2]
        run = dtype(j - (H - 1)) * step
        u[:, h, :2] = p[:, H - 1, :2] + run
    return u


def rebase(u, origin, motion=None, dtype=np.float64):
    """w [P, H, D] before the clamp.  origin [P, D] = prev[:, shift]; motion [P, 3] or None."""
    u = np.asarray(u, dtype=dtype)
    o = np.asarray(origin, dtype=dtype)
    P, H, D = u.shape
    w = u.copy()
    n = min(D, 3)
    if motion is None:
        w[..., :n] = u[..., :n] - o[:, None, :n]
        return w
    mo = np.asarray(motion, dtype=dtype)
    tx, ty, phi = mo[:, None, 0], mo[:, None, 1], mo[:, None, 2]
    c, s = np.cos(phi), np.sin(phi)          # on the fp32 angle; in `dtype`
    qx = u[..., 0] - tx
    qy = (u[..., 1] if D > 1 else np.zeros_like(qx)) - ty
    a0, a1 = c * qx, s * qy
    w[..., 0] = a0 + a1
    if D > 1:
        b0, b1 = s * qx, c * qy
        w[..., 1] = -b0 + b1
    if D > 2:
        w[..., 2] = u[..., 2] - o[:, None, 2]
    return w


def start(prev, shift, motion=None, dtype=np.float64):
    """clamp(rebase(advance(prev))): the tick's start before the re-noise, [P, H, D]."""
    p = np.asarray(prev, dtype=dtype)
    w = rebase(advance(p, shift, dtype), p[:, shift], motion, dtype)
    with np.errstate(invalid="ignore"):
        return np.where(w < -1, dtype(-1), np.where(w > 1, dtype(1), w))      # NaN passes, as torch.clamp


def warm_init(prev, rows, shift, sqrt_ab, sqrt_1mab, z, motion=None, zero_first=True, dtype=np.float64):
    """The whole contract: [rows, H, D].  z [rows, H, D]: the normals of the launch's elements.  sqrt_ab / sqrt_1mab are
    taken as the fp32 numbers the kernel is handed.  dtype=np.float32 is the same sequence with every operation rounded to
    fp32 on its own -- what the kernel computes wherever each of its operations is a single correctly rounded one."""
    w = start(prev, shift, motion, dtype)
    P = w.shape[0]
    assert rows % P == 0
    w = w[np.arange(rows) % P]
    sa, sb = dtype(np.float32(sqrt_ab)), dtype(np.float32(sqrt_1mab))
    m0, m1 = sa * w, sb * np.asarray(z, dtype=dtype)
    v = m0 + m1
    if zero_first:
        v[:, 0, :3] = 0
    return v


def error_bound(H, D, shift, has_motion, z, zero_first=True, t_max=1.0):
    """Absolute bound [rows, H, D] on |fp32 kernel - exact| for |prev| <= 1, |tx|, |ty| <= t_max, every operation rounded once
    (relative error <= u = 2^-24), sinf / cosf within 4 ulp.  First-order terms with every count rounded up by one u; the
    second-order terms are below 2^-40.

    advance   k = max(0, h + shift - (H-1)) <= 63 is exact in fp32.  k = 0 or d >= 2: a copy, exact, |u| <= 1.  Otherwise
              step^ = fl(last - before), |step| <= 2: error <= 2u; run^ = fl(k step^): <= 2ku carried + 2ku rounded;
              u^ = fl(last + run^), |u| <= A = 1 + 2k: + A u.  E_u = (6k + 2) u.
    re-base   no motion, d < 3: w^ = fl(u^ - o), |w| <= A + 1: E_w = E_u + (A + 2) u.  d >= 3: E_w = 0.
              motion, d < 2: q^ = fl(u^ - t), |q| <= Q = A + t_max: E_q = E_u + Q u.  The OpenCL full profile, which the device
              library's sin and cos are written to, allows 4 ulp; |cos|, |sin| <= 1, where an ulp is at most 2^-24 = u: 4u
              absolute.  One product: |c| E_q + Q 4u + Q u rounded = E_q + 5 Q u; the negation is exact; the sum of two, of
              magnitude <= 2 Q: E_w = 2 (E_q + 5 Q u) + 2 Q u + u = 2 E_q + (12 Q + 1) u.  Column 2: as without motion.
    clamp     1-Lipschitz: the error does not grow; |w| <= 1 after it.
    noise     sqrt_ab, sqrt_1mab <= 1 and z are the same fp32 numbers on both sides: fl(sa w^): E_w + u; fl(sb z): |z| u;
              their sum, |.| <= 1 + |z|: + (1 + |z|) u.  E_v = E_w + (2 + 2 |z|) u, + u for the second order.
    zero_first: exact zeros."""
    z = np.abs(np.asarray(z, dtype=np.float64))
    rows = z.shape[0]
    k = np.maximum(0, np.arange(H) + shift - (H - 1)).astype(np.float64)          # [H]
    e_w = np.zeros((H, D))
    for d in range(D):
        extr = (k > 0) & (d < 2)
        A = np.where(extr, 1.0 + 2.0 * k, 1.0)
        e_u = np.where(extr, (6.0 * k + 2.0) * U, 0.0)
        if has_motion and d < 2:
            Q = (1.0 + 2.0 * k) + t_max          # x' and y' both read columns 0 AND 1: the xy magnitudes, whichever d
            e_uxy = np.where(k > 0, (6.0 * k + 2.0) * U, 0.0)
            e_q = e_uxy + Q * U
            e_w[:, d] = 2.0 * e_q + (12.0 * Q + 1.0) * U
        elif d < 3:
            e_w[:, d] = e_u + (A + 2.0) * U
    e_v = e_w[None] + (3.0 + 2.0 * z) * U
    if zero_first:
        e_v[:, 0, :3] = 0.0
    assert e_v.shape == (rows, H, D)
    return e_v


# ---- fixtures -------------------------------------------------------------------------------------------------------------
SCENES, CANDIDATES, HORIZONS, DIMS, ROW_OFFSETS = (1, 3), (1, 4), (2, 8, 16), (1, 2, 3, 7, 16), (0, 5)
# a noise level in the middle of a schedule; both are fp32 numbers (sqrt(0.3), sqrt(0.7) rounded)
LEVEL = (float(np.float32(np.sqrt(0.3))), float(np.float32(np.sqrt(0.7))))


def shifts(H):
    return sorted({0, 1, H - 1})


def make_case(S, K, H, D, shift, has_motion, row_offset, seed=2025):
    """dict(S, K, H, D, shift, row_offset, prev [S, H, D] fp32 in [-1, 1], motion [S, 3] fp32 or None with |tx|, |ty| <= 1 and
    |phi| <= pi).  Uniform draws: neighbouring waypoints up to 2 apart, so extrapolated rows and re-based columns leave
    [-1, 1] and the clamp is exercised."""
    rng = np.random.default_rng([seed, S, K, H, D, shift, int(has_motion), row_offset])
    prev = rng.uniform(-1.0, 1.0, size=(S, H, D)).astype(np.float32)
    motion = None
    if has_motion:
        motion = np.concatenate([rng.uniform(-1.0, 1.0, size=(S, 2)), rng.uniform(-np.pi, np.pi, size=(S, 1))], axis=1).astype(np.float32)
        motion[:, 2] = np.clip(motion[:, 2], -np.float32(3.1415925), np.float32(3.1415925))
    assert np.abs(prev).max() <= 1.0
    return dict(S=S, K=K, H=H, D=D, shift=shift, row_offset=row_offset, prev=prev, motion=motion)


def cases(seed: int = 2025):
    out = []
    for S, K, H, D, mo, ro in itertools.product(SCENES, CANDIDATES, HORIZONS, DIMS, (False, True), ROW_OFFSETS):
        for sh in shifts(H):
            out.append(make_case(S, K, H, D, sh, mo, ro, seed))
    return out
