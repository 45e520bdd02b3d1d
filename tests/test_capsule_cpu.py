"""CPU: "cost guidance v5" and "capsules from boxes v1" (include/adx.h) without a device -- the restatement (tests/capsule_ref.py)
against finite differences of its own fp64 cost and on the cases the contract names (one capsule worked by hand, a degenerate
capsule against v1's disc, empty / NaN / zero-radius slots, a zero weight, a NaN end, a descent), the fp32 restatement against the
fp64 one within a derived bound, the `Capsules` object, `boxes_from_physical` and `Guide(capsules=...)`, the capsules in
`plan_tick` and `TickPlan.key()` (on the stubs of tests/test_tick_plan_cpu.py), the layout of the new ctypes record and every new
refusal of the C ABI by its whole text (placeholder addresses, never dereferenced: the checks run before any GPU work).  Nothing
here says what capsules do to driving quality."""
import ctypes
import math

import numpy as np
import pytest
import torch

import capsule_ref as CR
import guide_ref as G
import test_guide_cpu as TG
import test_tick_plan_cpu as T
from autonomous_driving_with_diffusion_model_amd.guide import Capsules, CostField, Guide, MotionLimits, Route

S, H, D = T.S, T.H, T.D
F32, F64 = np.float32, np.float64

# one scene: a long moving capsule, a degenerate (disc) one, a steep parked one and an empty slot
FIX_SLOTS = np.array([[[-0.5, -0.4, 0.3, -0.2, 0.004, 0.002, 0.45], [0.2, 0.5, 0.2, 0.5, -0.003, 0.0, 0.5],
                       [0.6, -0.7, 0.7, 0.6, 0.0, 0.0, 0.3], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]], F32)


def _fix(weight=1.0):
    return CR.capsules(FIX_SLOTS, weight)


def _share(c, x, y, dtype=F32):
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    z = np.zeros(x.shape, dtype)
    return CR.capsule_share(c, x, y, z, z.copy(), z.copy(), np.zeros(x.shape, np.int64), dtype)


def _smooth(c, x, y, margin=1e-4):
    """[B, H] bool: waypoints where the fp64 term is smooth within `margin` -- away from every live slot's hinge phi = 0 and, where
    the slot is active, from its axis and from the end normals (t = 0, t = 1: the cost is C1 there, its second derivative jumps)."""
    s = CR.slot_terms(c, x, y, F64)
    ok = (CR.hinge_margin(c, x, y) > margin).all(axis=0)
    with np.errstate(all="ignore"):
        along = np.minimum(np.abs(s["raw"]), np.abs(s["raw"] - 1)) * np.sqrt(s["ee"])      # distance to the lines t = 0 / t = 1
        fine = (s["d2"] > margin * margin) & ((along > margin) | (s["ee"] == 0))
    return ok & (~s["on"] | fine).all(axis=0)


# ---- 1. the restatement's gradient ------------------------------------------------------------------------------------------------
def test_the_fp64_gradient_is_the_central_difference_of_the_fp64_cost():
    """20,000 uniform points in [-1, 1]^2 (400 rows of 50 waypoints, so the capsules move) against FIX_SLOTS at weight 1.5.  The
    term is point-wise, so one perturbed evaluation differentiates every waypoint at once.  Waypoints within 1e-4 of a hinge, of
    an active slot's axis or of its end normals are left out (`_smooth`); on the rest every active slot's cost is a quartic
    polynomial of the waypoint, f = w * phi^2 / 2 with phi = 1 - d2 / r^2 quadratic, |grad phi| = 2 d / r^2 and |phi''| <= 2 / r^2,
    so |f'''| <= 3 w |phi'| |phi''| <= 12 w d / r^4.  A central difference at step e then errs, per active slot, by at most
      e^2 / 6 * 12 w d / r^4 = 2 w d e^2 / r^4    the truncation;
      2 * (2^-29 * term_bound) / (2 e)            the two evaluations' own rounding: `capsule_ref.term_bound` is linear in the
                                                  unit roundoff, and fp64's is 2^-29 of fp32's;
    and, for the sum, |g| * 2 * 2^-53 / (2 e): x + e and x - e are rounded to fp64, each by at most 2^-53 (|x| <= 1), and the
    cost follows with slope g.  The bound is formed per waypoint from its own slots, terms and gradient."""
    t = CR.fixture_points().astype(F64)
    x, y = t[:, :, 0], t[:, :, 1]
    eps, w = 1e-6, 1.5
    c = _fix(w)
    s = CR.slot_terms(c, x, y, F64)
    gx, gy = CR.capsule_grad(c, x, y)
    ok = _smooth(c, x, y, 1e-4)
    with np.errstate(all="ignore"):
        trunc = np.where(s["on"], 2 * w * np.sqrt(s["d2"]) * eps ** 2 / (s["r"] ** 4), 0.0).sum(axis=0)
    own = trunc + 2.0 ** -29 * CR.term_bound(c, x, y).sum(axis=0) / eps
    bx, by = own + np.abs(gx) * 2.0 ** -53 / eps, own + np.abs(gy) * 2.0 ** -53 / eps
    fdx = (CR.capsule_cost(c, x + eps, y) - CR.capsule_cost(c, x - eps, y)) / (2 * eps)
    fdy = (CR.capsule_cost(c, x, y + eps) - CR.capsule_cost(c, x, y - eps)) / (2 * eps)
    ex, ey = np.abs(gx - fdx), np.abs(gy - fdy)
    active = s["on"].any(axis=0)
    print("kept", int(ok.sum()), "of", ok.size, "active", int(active.sum()), "worst |g - fd|", ex[ok].max(), ey[ok].max(),
          "largest bound", bx[ok].max(), by[ok].max(), "largest |g|", np.abs(gx).max())
    assert (ex[ok] <= bx[ok]).all() and (ey[ok] <= by[ok]).all()
    assert active.sum() > 0.2 * active.size and np.abs(gx[ok]).max() > 1 and ok.sum() >= 0.95 * ok.size
    # on the axis itself the gradient is zero, as at a disc's centre: the midpoint of slot 2's (parked) axis, and slot 1's centre
    mx, my = (FIX_SLOTS[0, 2, 0] + FIX_SLOTS[0, 2, 2]) / F32(2), (FIX_SLOTS[0, 2, 1] + FIX_SLOTS[0, 2, 3]) / F32(2)
    only = CR.capsules(FIX_SLOTS[:, 2:3])
    J, ax_, ay_, act = _share(only, [[mx]], [[my]], F64)
    assert act[0, 0] == 1 and abs(ax_[0, 0]) < 1e-6 and abs(ay_[0, 0]) < 1e-6 and abs(J[0, 0] - 0.5) < 1e-6
    J, ax_, ay_, act = _share(CR.capsules(FIX_SLOTS[:, 1:2]), [[0.2]], [[0.5]])
    assert act[0, 0] == 1 and J[0, 0] == 0.5 and ax_[0, 0] == 0 and ay_[0, 0] == 0


# ---- 2. the restatement's behaviour -----------------------------------------------------------------------------------------------
def test_one_capsule_by_hand():
    """The capsule (0, 0) - (1, 0) of radius 0.5 moving by (0, 0.125) per waypoint, at weight 2: a waypoint beside the middle, one
    beyond each end, one outside, one on the axis.  Every number is a binary fraction, so every operation is exact."""
    c = CR.capsules([[[0.0, 0.0, 1.0, 0.0, 0.0, 0.125, 0.5]]], 2.0)
    J, gx, gy, act = _share(c, [[0.5, -0.25, 1.25, 0.5, 0.25]], [[0.25, 0.125, 0.5, 1.0, 0.5]])
    assert act.tolist() == [[1, 1, 1, 0, 1]] and J.dtype == F32
    # h = 0: t = 0.5, r = (0, 0.25), d2 = 0.0625, inv = 4, phi = 0.75: J = (2 * 0.5625) / 2, k = 2 * ((1.5) * 4) = 12
    assert (J[0, 0], gx[0, 0], gy[0, 0]) == (0.5625, 0.0, -3.0)
    # h = 1: the axis is at y = 0.125; t clamps to 0: r = u = (-0.25, 0), phi = 0.75
    assert (J[0, 1], gx[0, 1], gy[0, 1]) == (0.5625, 3.0, 0.0)
    # h = 2: the axis is at y = 0.25; t clamps to 1: r = (0.25, 0.25), d2 = 0.125, phi = 0.5: J = (2 * 0.25) / 2, k = 2 * (1 * 4) = 8
    assert (J[0, 2], gx[0, 2], gy[0, 2]) == (0.25, -2.0, -2.0)
    # h = 3: the axis is at y = 0.375, the waypoint 0.625 above it: outside, nothing
    assert (J[0, 3], gx[0, 3], gy[0, 3]) == (0.0, 0.0, 0.0)
    # h = 4: the axis is at y = 0.5 and the waypoint on it: the full potential and no gradient
    assert (J[0, 4], gx[0, 4], gy[0, 4]) == (1.0, 0.0, 0.0)
    # the gradient points toward the axis: a step against it leaves the capsule
    assert gy[0, 0] < 0 and gx[0, 1] > 0


def test_a_degenerate_capsule_at_weight_one_is_the_disc_bit_for_bit():
    """20,000 draws: a disc (cx, cy, vx, vy, r) per row of 50 waypoints, centres in [-1, 1]^2, velocities within 0.05, radii in
    0.05 .. 1.5, against the capsule (cx, cy, cx, cy, vx, vy, r) at weight 1: J, gx and gy equal guide_ref's on the int32 view,
    from accumulators that already hold something."""
    rng = np.random.default_rng(5)
    rows, Hn = 400, 50
    xy = rng.uniform(-1, 1, (rows, Hn, 2)).astype(F32)
    x, y = xy[:, :, 0], xy[:, :, 1]
    discs = np.zeros((rows, 1, 5), F32)
    discs[:, 0, :2] = rng.uniform(-1, 1, (rows, 2))
    discs[:, 0, 2:4] = rng.uniform(-0.05, 0.05, (rows, 2))
    discs[:, 0, 4] = rng.uniform(0.05, 1.5, rows)
    slots = np.concatenate([discs[:, :, :2], discs[:, :, :2], discs[:, :, 2:]], axis=2)
    want = G.cost_grad(discs, None, x, y)
    got = _share(CR.capsules(slots), x, y)
    assert want[3].sum() > 1000 and np.array_equal(got[3], want[3])
    for a, b in zip(got[:3], want[:3]):
        assert a.dtype == F32 and np.array_equal(a.view(np.int32), b.view(np.int32))
    planes = np.tile(np.array([[[1.0, 0.5, -0.2]]], F32), (rows, 1, 1))
    base = G.cost_grad(None, planes, x, y)
    after = CR.capsule_share(CR.capsules(slots), x, y, *base)                             # onto what a plane left: the same amounts
    alone = want
    on = alone[3] > 0
    assert np.array_equal(after[3], base[3] + alone[3])
    assert np.array_equal(after[0][~on].view(np.int32), base[0][~on].view(np.int32))
    assert np.array_equal(after[0][on].view(np.int32), (base[0] + alone[0])[on].view(np.int32))
    assert np.array_equal(after[1][on].view(np.int32), (base[1] + alone[1])[on].view(np.int32))


def test_empty_nan_and_zero_radius_slots_and_a_zero_weight_add_nothing():
    t = CR.fixture_points()[:8]
    x, y = t[:, :, 0], t[:, :, 1]
    for dtype in (F32, F64):
        for r in (0.0, -1.0, math.nan):
            off = FIX_SLOTS.copy()
            off[:, :, 6] = r
            J, gx, gy, act = _share(CR.capsules(off), x, y, dtype)
            assert not act.any() and not J.any() and not gx.any() and not gy.any(), r
        assert not _share(_fix(0.0), x, y, dtype)[3].any()                                 # weight 0: not evaluated
        J, gx, gy, act = _share(_fix(), x, y, dtype)
        assert act.any() and not (act > 0).all() and act.max() >= 2 and J.dtype == dtype and (J[act > 0] > 0).all()
        # an empty slot between live ones changes nothing: FIX_SLOTS without its last slot, and with an empty one in front
        J3, gx3, gy3, act3 = _share(CR.capsules(FIX_SLOTS[:, :3]), x, y, dtype)
        lead = np.concatenate([FIX_SLOTS[:, 3:], FIX_SLOTS[:, :3]], axis=1)
        J4, gx4, gy4, act4 = _share(CR.capsules(lead), x, y, dtype)
        for a, b, e in ((J, J3, J4), (gx, gx3, gx4), (gy, gy3, gy4), (act, act3, act4)):
            assert np.array_equal(a, b) and np.array_equal(a, e)
    # an inactive term adds nothing, not even a zero: the accumulators keep their bits (a -0.0 stays -0.0)
    neg = np.full(x.shape, -0.0, F32)
    off = FIX_SLOTS.copy()
    off[:, :, 6] = 0.0
    for c in (CR.capsules(off), _fix(0.0)):
        J, gx, gy, act = CR.capsule_share(c, x, y, neg.copy(), neg.copy(), neg.copy(), np.zeros(x.shape, np.int64))
        assert np.signbit(J).all() and np.signbit(gx).all() and np.signbit(gy).all()
    far = CR.capsules([[[5.0, 5.0, 6.0, 5.0, 0.0, 0.0, 0.5]]])                              # live, and nowhere near
    J, gx, gy, act = CR.capsule_share(far, x, y, neg.copy(), neg.copy(), neg.copy(), np.zeros(x.shape, np.int64))
    assert np.signbit(J).all() and np.signbit(gx).all() and not act.any()
    # row r reads scene r % S
    off = FIX_SLOTS.copy()
    off[:, :, 6] = 0.0
    big = FIX_SLOTS.copy()
    big[:, :, 6] = 4.0
    two = CR.capsules(np.concatenate([big, off]))
    assert _share(two, x[:4], y[:4])[3].sum(axis=1).tolist() == [4 * CR.FIX_H, 0, 4 * CR.FIX_H, 0]          # r = 4 makes the zero slot a disc too


def test_a_nan_end_stays_local_to_its_slot():
    t = CR.fixture_points()[:8]
    x, y = t[:, :, 0], t[:, :, 1]
    plain = _share(CR.capsules(FIX_SLOTS[:, 1:3]), x, y)
    for k in range(6):                                                                    # either end, either velocity
        holed = FIX_SLOTS[:, :3].copy()
        holed[0, 0, k] = np.nan
        got = _share(CR.capsules(holed), x, y)
        assert np.isfinite(got[0]).all() and all(np.array_equal(a, b) for a, b in zip(got, plain)), k
    assert plain[3].any()
    # a NaN waypoint is inactive too
    assert not _share(_fix(), [[np.nan, 0.2]], [[0.0, np.nan]])[3].any()


def test_eight_iterations_lower_the_cost_of_every_row():
    """The capsule term alone on 40 rows of 50 uniform points, FIX_SLOTS at weight 1, no cap, no clip.  The term is point-wise.
    The Hessian of w * phi^2 / 2 is w * (grad phi grad phi^T + phi * phi''): the first part is at most w * |grad phi|^2 =
    4 w d2 / r^4 <= 4 w / r^2 inside the capsule (d < r), the second is negative semidefinite and at least -2 w / r^2 (phi <= 1), so
    the gradient of the sum is Lipschitz with constant L = sum over the slots of 4 w / r^2, and the cost is C1 across the hinge
    and the end normals.  With lambda = 1 / L every step lowers the cost by at least |g|^2 / (2 L) in exact arithmetic; the fp64
    cost of the fp32 iterate is asserted per row, where the waypoints deep inside (whose decrease is many orders above fp32's
    rounding) decide."""
    t = CR.fixture_points()[:40]
    x, y = t[:, :, 0], t[:, :, 1]
    c = _fix()
    r = FIX_SLOTS[0, :3, 6].astype(F64)
    Lc = float((4.0 / (r * r)).sum())
    lam = 1.0 / Lc
    costs = [CR.capsule_cost(c, x, y).sum(axis=1)]
    px, py = x, y
    for _ in range(8):
        px, py, mx, my = CR.iterate(px, py, None, None, None, None, c, None, lam, math.inf, 1, 0, 1.0)
        costs.append(CR.capsule_cost(c, px, py).sum(axis=1))
    print("Lipschitz bound", Lc, "lambda", lam, "cost of row 0:", [float(v[0]) for v in costs])
    assert (costs[0] > 0).all()
    for before, after in zip(costs, costs[1:]):
        assert (after < before).all()
    eight = CR.iterate(x, y, None, None, None, None, c, None, lam, math.inf, 8, 0, 1.0)
    assert np.array_equal(eight[0], px) and np.array_equal(eight[1], py)
    # one iteration is one explicit step along the term's own gradient
    gx, _ = CR.capsule_grad(c, x, y, F32)
    one = CR.iterate(x, y, None, None, None, None, c, None, lam, math.inf, 1, 0, 1.0)[0]
    assert np.array_equal(one, x - F32(lam) * gx)


def test_the_restatement_goes_through_the_four_earlier_ones():
    """With neutral capsules the calls are route_ref's, bit for bit; the order is discs, planes, field, route, capsules, motion;
    the wrapper is gone after every call."""
    import field_fixtures as FX
    import field_ref as FR
    import motion_ref as MR
    import route_ref as RR
    plain = G.cost_grad
    rows, Sn, Hn, Dn, M, P, Gy, Gx, _ = FX.COST_CASES[0]
    traj, discs, planes, cells, geo, _ = FX.cost_case(*FX.COST_CASES[0])
    f = FR.field(cells, weight=0.6, **geo)
    m = MR.motion(np.full((Sn, 2), 0.01))
    r = RR.route(np.tile(RR.FIX_POINTS, (Sn, 1, 1)), np.zeros(Sn))
    slots = np.tile(FIX_SLOTS, (Sn, 1, 1))
    slots[:, 0, 6] = 3.0                                                                  # active everywhere on [-1, 1]^2
    empty = slots.copy()
    empty[:, :, 6] = 0.0
    a, b = CR.row_cost_wave(traj, discs, planes, f, r, CR.capsules(empty), m), RR.row_cost_wave(traj, discs, planes, f, r, m)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and G.cost_grad is plain
    on = CR.capsules(slots, 0.75)
    c, act, _ = CR.row_cost(traj, discs, planes, f, r, on, m)
    c0, act0, _ = RR.row_cost(traj, discs, planes, f, r, m)
    xy = traj.numpy().astype(F64)
    assert (c > c0).all() and (act >= act0 + Hn).all() and G.cost_grad is plain
    assert np.allclose(c - c0, CR.capsule_cost(on, xy[:, :, 0], xy[:, :, 1]).sum(axis=1), rtol=1e-9, atol=0)
    assert (CR.cost_bound(traj, discs, planes, f, r, on, m) > RR.cost_bound(traj, discs, planes, f, r, m)).all() and G.cost_grad is plain
    assert np.array_equal(CR.cost_bound(traj, discs, planes, f, r, None, m), RR.cost_bound(traj, discs, planes, f, r, m))
    # the order: J = ((((discs, planes) + field) + route) + capsules) + motion in fp32
    x32, y32 = traj.numpy()[:, :, 0], traj.numpy()[:, :, 1]
    d, p = G.scene_rows(discs.numpy(), rows), G.scene_rows(None if planes is None else planes.numpy(), rows)
    J, gx, gy, n = FR.cost_grad(d, p, f, x32, y32)
    J, gx, gy, n = RR.route_share(r, x32, y32, J, gx, gy, n)
    J, gx, gy, n = CR.capsule_share(on, x32, y32, J, gx, gy, n)
    J, gx, gy, n = MR.motion_share(m, x32, y32, J, gx, gy, n)
    got = CR.cost_grad(d, p, f, r, on, m, x32, y32)
    assert all(np.array_equal(u, v) for u, v in zip(got, (J, gx, gy, n))) and G.cost_grad is plain


def test_the_fp32_restatement_stays_within_the_derived_bound_of_the_fp64_one():
    """What tests/test_gpu_capsule.py asks of the kernel, asked of the fp32 restatement first, on the 20,000 fixture points against
    FIX_SLOTS and against 32 random capsules one of which covers everything: no slot's activity flips between fp32 and fp64 (so no
    waypoint is left out), every phi moves by less than `phi_bound`, and the row cost summed by the wave's butterfly stays within
    `cost_bound`.

    The bound is `capsule_ref.cost_bound`, derived there line by line from the contract's operation count: per slot, two roundings
    on the moved end and one on u (absolute: gamma_2 (|a| + |h v|) + u |u|), four on ee and ue, one on t, three on the residual, two
    on d2, three on sd and one on phi give `phi_bound`; the cost w * phi^2 / 2 moves by w (|phi| dphi + dphi^2 / 2) and carries three
    roundings of its own; the summation one per term.  Nothing in it was fitted to a kernel."""
    t = CR.fixture_points()
    x, y = t[:, :, 0], t[:, :, 1]
    many = CR.fixture_slots(1, 32, torch.Generator().manual_seed(11)).numpy()
    for name, c in (("FIX_SLOTS", _fix(1.5)), ("32 slots", CR.capsules(many, 0.75))):
        s32, s64 = CR.slot_terms(c, x, y, F32), CR.slot_terms(c, x, y, F64)
        dphi = CR.phi_bound(c, x, y)
        live = np.isfinite(s64["phi"]) & (s64["r"] > 0)
        with np.errstate(all="ignore"):
            worst = (np.abs(s32["phi"].astype(F64) - s64["phi"])[live] / dphi[live]).max()
        print(name, "active", int(s64["on"].sum()), "smallest |phi|", CR.hinge_margin(c, x, y).min(), "largest |d phi| / bound", worst)
        assert np.array_equal(s32["on"], s64["on"]) and worst <= 1
        got = CR.row_cost_wave(t, None, None, None, None, c, None).astype(F64)
        want, active, _ = CR.row_cost(t, None, None, None, None, c, None)
        bound = CR.cost_bound(t, None, None, None, None, c, None)
        print("largest |cost32 - cost64| / bound", (np.abs(got - want) / bound).max(), "largest bound", bound.max(), "largest cost", want.max())
        assert (np.abs(got - want) <= bound).all() and (bound < 1e-3 * want).all() and np.array_equal(active, s64["on"].sum(axis=(0, 2)))


def test_from_boxes_restated():
    """length > width, width > length (the axis turns), a square (a disc), zero / negative / NaN sizes and a slanted heading."""
    u = F32(0.6), F32(0.8)
    boxes = np.array([[[0.5, -0.25, 0.01, 0.02, 1.0, 0.0, 1.0, 0.5], [0.5, -0.25, 0.01, 0.02, 1.0, 0.0, 0.5, 1.0],
                       [0.1, 0.2, 0.0, 0.0, 0.0, 1.0, 0.5, 0.5], [0.1, 0.2, 0.3, 0.4, 1.0, 0.0, 0.0, 0.5],
                       [0.1, 0.2, 0.3, 0.4, 1.0, 0.0, 0.5, -1.0], [0.1, 0.2, 0.3, 0.4, 1.0, 0.0, math.nan, 0.5],
                       [0.0, 0.0, 0.0, 0.0, u[0], u[1], 1.5, 0.5]]], F32)
    out = CR.from_boxes(boxes, 0.125)
    assert out.dtype == F32 and out.shape == (1, 7, 7)
    assert out[0, 0].tolist() == [0.25, -0.25, 0.75, -0.25, float(F32(0.01)), float(F32(0.02)), 0.375]
    assert out[0, 1].tolist() == [0.5, -0.5, 0.5, 0.0, float(F32(0.01)), float(F32(0.02)), 0.375]      # along (-uy, ux) = (0, 1)
    assert out[0, 2].tolist() == [float(F32(0.1)), float(F32(0.2))] * 2 + [0.0, 0.0, 0.375]             # a == b: a disc
    assert not out[0, 3:6].any()
    ox, oy = F32(F32(0.5) * u[0]), F32(F32(0.5) * u[1])
    assert out[0, 6].tolist() == [float(-ox), float(-oy), float(ox), float(oy), 0.0, 0.0, 0.375]


# ---- 3. the objects ---------------------------------------------------------------------------------------------------------------
def _caps(C=3, scenes=S, **kw):
    return Capsules(torch.zeros(scenes, C, 7), **kw)


def test_capsules_and_their_refusals():
    c = _caps(weight=2.0)
    assert c.scenes == S and c.C == 3 and c.key() == (3, 2.0) and c.device == torch.device("cpu")
    other = c.like(torch.ones(3, 3, 7))
    assert other.key() == c.key() and other.scenes == 3 and other.slots.sum() == 63
    assert "Capsules(slots=(2, 3, 7), weight=2.0)" == repr(c)
    assert Capsules(torch.zeros(1, 32, 7)).C == 32 and Capsules(torch.zeros(1, 1, 7), 0.0).key() == (1, 0.0)
    for args, exc, text in (((None,), TypeError, "slots must be a tensor, got NoneType"),
                            ((torch.zeros(2, 7),), ValueError, r"slots must be \[S, C, 7\] = \(ax, ay, bx, by, vx, vy, r\) per slot, got \(2, 7\)"),
                            ((torch.zeros(2, 3, 5),), ValueError, r"slots must be \[S, C, 7\]"),
                            ((torch.zeros(0, 3, 7),), ValueError, r"slots must be \[S, C, 7\]"),
                            ((torch.zeros(2, 0, 7),), ValueError, r"0 slots per scene, supported 1..32"),
                            ((torch.zeros(2, 33, 7),), ValueError, r"33 slots per scene, supported 1..32"),
                            ((torch.zeros(2, 3, 7, dtype=torch.float64),), TypeError, "slots must be float32, got torch.float64"),
                            ((torch.zeros(2, 3, 7), -1.0), ValueError, "weight must be >= 0, got -1.0"),
                            ((torch.zeros(2, 3, 7), math.nan), ValueError, "weight must be >= 0, got nan")):
        with pytest.raises(exc, match=text):
            Capsules(*args)
    # from_boxes refuses before it touches the library
    good = torch.zeros(2, 3, 8)
    for args, exc, text in (((None,), TypeError, "boxes must be a tensor, got NoneType"),
                            ((torch.zeros(2, 3, 7),), ValueError, r"boxes must be \[S, N, 8\], got \(2, 3, 7\)"),
                            ((torch.zeros(2, 33, 8),), ValueError, "33 boxes per scene, supported 1..32"),
                            ((torch.zeros(2, 0, 8),), ValueError, "0 boxes per scene, supported 1..32"),
                            ((good.double(),), TypeError, "boxes must be float32, got torch.float64"),
                            ((good, -0.5), ValueError, "inflate must be finite and >= 0, got -0.5"),
                            ((good, math.inf), ValueError, "inflate must be finite and >= 0, got inf"),
                            ((good, math.nan), ValueError, "inflate must be finite and >= 0, got nan"),
                            ((good, 0.0, -1.0), ValueError, "weight must be >= 0, got -1.0")):
        with pytest.raises(exc, match=text):
            Capsules.from_boxes(*args)


def test_boxes_from_physical():
    yaw = 0.3
    boxes_m = [[[10.0, -2.0, 5.0, 0.5, yaw, 4.5, 2.0], [0.0, 0.0, 0.0, 0.0, math.pi / 2, 1.0, 1.0]]]
    b = Capsules.boxes_from_physical(boxes_m, 0.5, 23.315)
    assert b.dtype == torch.float32 and tuple(b.shape) == (1, 2, 8) and b.device == torch.device("cpu")
    want = [10.0 / 23.315, -2.0 / 23.315, 5.0 * (0.5 / 23.315), 0.5 * (0.5 / 23.315), math.cos(yaw), math.sin(yaw), 4.5 / 23.315,
            2.0 / 23.315]
    assert b[0, 0].tolist() == [float(F32(v)) for v in want]
    assert b[0, 1, 4].item() == float(F32(math.cos(math.pi / 2))) and b[0, 1, 5].item() == 1.0
    # formed in double and rounded once: not the fp32 quotient of fp32 operands
    third = Capsules.boxes_from_physical([[[0.1, 0.0, 0.0, 0.0, 0.0, 0.1, 0.1]]], 1.0, 3.0)
    assert third[0, 0, 0].item() == float(F32(0.1 / 3.0)) and third[0, 0, 6].item() == float(F32(0.1 / 3.0))
    # through the restated conversion: the car's capsule is 2.5 m of axis and 1 m of radius, in model units
    slots = CR.from_boxes(b, 0.0)
    axis = math.hypot(slots[0, 0, 2] - slots[0, 0, 0], slots[0, 0, 3] - slots[0, 0, 1])
    assert abs(axis * 23.315 - 2.5) < 1e-5 and abs(slots[0, 0, 6] * 23.315 - 1.0) < 1e-6
    assert slots[0, 1, 0] == slots[0, 1, 2] and slots[0, 1, 1] == slots[0, 1, 3]          # a square: a disc
    for args, text in (((boxes_m, 0.5, 0.0), "xy_scale must be finite and > 0"), ((boxes_m, 0.5, math.inf), "xy_scale must be finite and > 0"),
                       ((boxes_m, 0.0, 1.0), "dt must be finite and > 0"), ((boxes_m, math.nan, 1.0), "dt must be finite and > 0"),
                       ((boxes_m[0], 0.5, 1.0), r"boxes_m must be \[S, N, 7\] = \(cx, cy, vx, vy, yaw, length, width\), got \(2, 7\)"),
                       (([[[0.0] * 8]], 0.5, 1.0), r"boxes_m must be \[S, N, 7\]")):
        with pytest.raises(ValueError, match=text):
            Capsules.boxes_from_physical(*args)


def test_guide_with_capsules_and_its_refusals():
    d, p = torch.zeros(S, 3, 5), torch.zeros(S, 2, 3)
    f = CostField(torch.zeros(S, 3, 5), (-0.5, 0.25), (0.25, 0.5), 2.0)
    m = MotionLimits(torch.full((S, 2), 0.1), w_speed=2.0)
    r = Route(torch.zeros(S, 4, 2), 0.1, 3.0)
    c = _caps(weight=1.5)
    # a guide without capsules returns the key it returned before
    v1, v2 = Guide(d, p, scale=0.5, iters=2), Guide(d, p, scale=0.5, iters=2, field=f)
    v3, v4 = Guide(d, p, scale=0.5, iters=2, motion=m), Guide(d, p, scale=0.5, iters=2, field=f, motion=m, route=r)
    assert v1.key() == (3, 2, 0.5, "variance", math.inf, 2) and v2.key() == v1.key() + (f.key(),)
    assert v3.key() == v1.key() + (None, (2.0, 1.0)) and v4.key() == v1.key() + (f.key(), (2.0, 1.0), (4, 3.0))
    assert Guide(d, p, scale=0.5, iters=2, route=r).key() == v1.key() + (None, None, (4, 3.0)) and v1.capsules is None
    g = Guide(d, p, scale=0.5, iters=2, capsules=c)
    assert g.capsules is c and g.key() == v1.key() + (None, None, None, (3, 1.5))
    every = Guide(d, p, scale=0.5, iters=2, field=f, motion=m, route=r, capsules=c)
    assert every.key() == v1.key() + (f.key(), (2.0, 1.0), (4, 3.0), (3, 1.5))
    assert Guide(d, p, scale=0.5, iters=2, route=r, capsules=c).key() == v1.key() + (None, None, (4, 3.0), (3, 1.5))
    assert len({v1.key(), v2.key(), v3.key(), v4.key(), g.key(), every.key()}) == 6
    alone = Guide(capsules=c)
    assert alone.scenes == S and alone.device == torch.device("cpu") and (alone.M, alone.P) == (0, 0)
    again = every.like(d + 1, None, f.like(f.cells + 1), m.like(m.limits + 1), r.like(r.points + 1, r.half_width), c.like(c.slots + 1))
    assert again.key() == (3, 0) + every.key()[2:] and again.capsules is not c and again.capsules.slots.sum() == S * 3 * 7
    assert every.like(d, p).key() == v1.key()                                           # `like` without: a v1 guide
    with pytest.raises(TypeError):
        Guide(d, p, 1.0, "variance", math.inf, 1, None, None, None, c)                  # keyword only
    for kw, exc, text in ((dict(capsules=torch.zeros(S, 3, 7)), TypeError, "capsules must be a Capsules or None, got Tensor"),
                          (dict(discs=d, capsules=_caps(scenes=3)), ValueError, "discs hold 2 scenes, the capsules 3"),
                          (dict(planes=p, capsules=_caps(scenes=1)), ValueError, "planes hold 2 scenes, the capsules 1"),
                          (dict(field=f, capsules=_caps(scenes=3)), ValueError, "field hold 2 scenes, the capsules 3"),
                          (dict(motion=m, capsules=_caps(scenes=3)), ValueError, "motion limits hold 2 scenes, the capsules 3"),
                          (dict(route=r, capsules=_caps(scenes=3)), ValueError, "route hold 2 scenes, the capsules 3"),
                          (dict(discs=d.to("meta"), capsules=c), ValueError, "discs live on meta, the capsules on cpu"),
                          (dict(route=Route(torch.zeros(S, 4, 2, device="meta"), 0.1), capsules=c), ValueError,
                           "route live on meta, the capsules on cpu")):
        with pytest.raises(exc, match=text):
            Guide(**kw)
    assert Guide(torch.zeros(3, 0, 5), capsules=c).scenes == 3                           # no discs: nothing to agree with
    assert "capsules=Capsules(" in repr(g) and "capsules" not in repr(v4)


# ---- 4. the plan ------------------------------------------------------------------------------------------------------------------
_plan = TG._plan


def test_the_plan_carries_the_capsules_and_refuses_before_anything_is_touched():
    began = []
    sched = TG._Scheduler()
    sched.begin_index = 0
    c = _caps()
    before = c.slots.clone()
    plan = _plan(began, scheduler=sched, guide=Guide(capsules=c))
    assert plan.guide.capsules is c
    assert plan.key()[-1] == Guide(capsules=c).key() == (0, 0, 1.0, "variance", math.inf, 1, None, None, None, (3, 1.0))
    with pytest.raises(ValueError, match=r"guide.capsules.slots must hold 2 scenes \(image.shape\[0\]\) on cpu, got \(3, 3, 7\)"):
        _plan(began, scheduler=sched, guide=Guide(capsules=_caps(scenes=3)))
    with pytest.raises(ValueError, match=r"guide.capsules.slots must hold 2 scenes .* on meta"):
        _plan(began, scheduler=sched, guide=Guide(capsules=Capsules(torch.zeros(S, 3, 7, device="meta"))))
    cfg = T._cfg()
    cfg.MODEL.HORIZON = 65                                                                # capsules alone need no wave per row
    assert _plan(began, scheduler=sched, cfg=cfg, guide=Guide(capsules=c)).guide.capsules is c
    with pytest.raises(ValueError, match="need MODEL.HORIZON <= 64, got 65"):
        _plan(began, scheduler=sched, cfg=cfg, guide=Guide(capsules=c, motion=MotionLimits(torch.zeros(S, 2))))
    cfg.MODEL.TRANSITION_DIM = 1
    with pytest.raises(ValueError, match="needs MODEL.TRANSITION_DIM >= 2, got 1"):
        _plan(began, scheduler=sched, cfg=cfg, guide=Guide(capsules=c))
    with pytest.raises(ValueError, match="_Scheduler.step takes no guide"):
        T._plan(began, guide=Guide(capsules=c))
    assert dict(vars(sched)) == {"begin_index": 0} and torch.equal(c.slots, before)


def test_the_plans_key_bakes_presence_c_and_weight_and_not_the_values():
    base = dict(scale=0.5, schedule="variance", cap=0.1, iters=2)
    d = torch.zeros(S, 3, 5)
    f = CostField(torch.zeros(S, 3, 5))
    m = MotionLimits(torch.full((S, 2), 0.1))
    r = Route(torch.zeros(S, 4, 2), 0.1)
    variants = {"none": Guide(d, **base), "capsules": Guide(d, capsules=_caps(), **base), "alone": Guide(capsules=_caps(), **base),
                "C": Guide(d, capsules=_caps(C=5), **base), "weight": Guide(d, capsules=_caps(weight=2.0), **base),
                "field": Guide(d, field=f, **base), "field and capsules": Guide(d, field=f, capsules=_caps(), **base),
                "limits": Guide(d, motion=m, **base), "limits and capsules": Guide(d, motion=m, capsules=_caps(), **base),
                "route": Guide(d, route=r, **base), "route and capsules": Guide(d, route=r, capsules=_caps(), **base),
                "all": Guide(d, field=f, motion=m, route=r, capsules=_caps(), **base)}
    keys = {name: _plan(guide=g).key() for name, g in variants.items()}
    hash(tuple(keys.values()))
    names = list(keys)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert keys[a] != keys[b], (a, b)
    moved = Capsules(torch.ones(S, 3, 7))
    assert keys["capsules"] == _plan(guide=Guide(d + 1, capsules=moved, **base)).key()    # the values are buffers


# ---- 5. the C ABI -----------------------------------------------------------------------------------------------------------------
B = 6
(MO, X, PX0, PREV, X0, KNOWN, MASK, DISCS, PLANES, CELLS, LIMITS, POINTS, WIDTH, CAPS, COST, ACTIVE, INDEX, BLOCKED, BEST, TARGET, Z, STATE,
 BOXES, OUT) = (0x10000000 * (i + 1) for i in range(24))
GY, GX, RN, CN = 3, 5, 4, 3
STEP = ("adx_ddim_step_capsule", "adx_ddpm_step_capsule")
DPM = ("adx_dpm_step_capsule",)
COSTFN = ("adx_guide_cost_capsule",)
SELECT = ("adx_traj_select_guide_capsule",)
LAUNCH = STEP + DPM
EVERY = LAUNCH + COSTFN + SELECT
NAME = {**{n: "scheduler step" for n in STEP}, **{n: "dpm step" for n in DPM}, "adx_guide_cost_capsule": "guide cost",
        "adx_traj_select_guide_capsule": "traj select guide"}
BARE = dict(n_discs=0, n_planes=0)
OVERLAP = "%s: an output overlaps the capsules"
ALONE = dict(field=None, motion=None, route=None)

# (exports, the one defect as overrides of a good call, adx_last_error() in full; %s: the export's prefix)
TABLE = [
    (EVERY, dict(capsule=dict(capsules=None)), "%s: null capsules"),
    (EVERY, dict(capsule=dict(n_capsules=0)), "%s: n_capsules 0 outside 1..32"),
    (EVERY, dict(capsule=dict(n_capsules=33)), "%s: n_capsules 33 outside 1..32"),
    (EVERY, dict(capsule=dict(scene_rows=0)), "%s: batch 6 must be a positive multiple of the capsules' scene_rows 0"),
    (EVERY, dict(capsule=dict(scene_rows=4)), "%s: batch 6 must be a positive multiple of the capsules' scene_rows 4"),
    (EVERY, dict(capsule=dict(scene_rows=3), **ALONE), "%s: the capsules hold 3 scenes, the guide's discs and planes 2"),
    (EVERY, dict(capsule=dict(scene_rows=3), guide=BARE, motion=None, route=None), "%s: the capsules hold 3 scenes, the field 2"),
    (EVERY, dict(capsule=dict(scene_rows=3), guide=BARE, field=None, route=None), "%s: the capsules hold 3 scenes, the motion limits 2"),
    (EVERY, dict(capsule=dict(scene_rows=3), guide=BARE, field=None, motion=None), "%s: the capsules hold 3 scenes, the route 2"),
    (EVERY, dict(capsule=dict(weight=-1.0)), "%s: capsule weight -1 is negative or NaN"),
    (EVERY, dict(capsule=dict(weight=math.nan)), "%s: capsule weight nan is negative or NaN"),
    (EVERY, dict(capsule=dict(weight=-1.0), **ALONE), "%s: capsule weight -1 is negative or NaN"),      # NULL field, motion and route
    (LAUNCH, dict(prev=CAPS), OVERLAP),
    (LAUNCH, dict(x0=CAPS + 2 * CN * 7 * 4 - 4), OVERLAP),
    (COSTFN, dict(cost=CAPS + 4), OVERLAP),
    (COSTFN, dict(active=CAPS), OVERLAP),
    (SELECT, dict(cost=CAPS), OVERLAP),
    (SELECT, dict(active=CAPS + 4), OVERLAP),
    (SELECT, dict(index=CAPS + 8), OVERLAP),
    (SELECT, dict(blocked=CAPS), OVERLAP),
    (SELECT, dict(best=CAPS), OVERLAP),
    (LAUNCH, dict(guide=None, route=None), "%s: capsules without a guide: a step reads iters, lambda and cap from the guide"),
    (LAUNCH, dict(guide=None, **ALONE), "%s: capsules without a guide: a step reads iters, lambda and cap from the guide"),
    (SELECT, dict(capsule=dict(scene_rows=1), guide=BARE, **ALONE), "traj select guide: the capsules hold 1 scenes, the selection 2"),
    # whatever the _route export refuses, through the new exports
    (LAUNCH, dict(guide=None), "%s: a route without a guide: a step reads iters, lambda and cap from the guide"),
    (EVERY, dict(route=dict(points=None)), "%s: null route points"),
    (EVERY, dict(route=dict(n_points=33)), "%s: route of 33 points, supported 2..32"),
    (EVERY, dict(route=dict(weight=-1.0)), "%s: route weight -1 is negative or NaN"),
    (LAUNCH, dict(prev=POINTS), "%s: an output overlaps the route's points or half_width"),
    (EVERY, dict(motion=dict(limits=None)), "%s: null motion limits"),
    (EVERY, dict(motion=dict(w_speed=-1.0)), "%s: motion w_speed -1 is negative or NaN"),
    (LAUNCH, dict(H=65), "%s: motion limits give a row to a wave: horizon 65, supported 1..64"),
    (COSTFN, dict(H=65), "guide cost: horizon 65 outside 1..64"),
    (SELECT, dict(H=65), "traj select: horizon 65, supported 1..64"),
    (LAUNCH, dict(prev=LIMITS), "%s: an output overlaps the motion limits"),
    (LAUNCH, dict(route=None, capsule=None, guide=None), "%s: motion limits without a guide: a step reads iters, lambda and cap from the guide"),
    (EVERY, dict(field=dict(cells=None)), "%s: null field cells"),
    (EVERY, dict(guide=dict(n_discs=33)), "%s: n_discs 33 outside 0..32"),
    (LAUNCH + COSTFN, dict(D=1), "%s: cost guidance moves (x, y), dim is 1"),
    (SELECT, dict(D=1), "traj select guide: the guide scores (x, y), dim is 1"),
    (LAUNCH, dict(guide=dict(iters=9)), "%s: guide iters 9 outside 1..8"),
    (LAUNCH, dict(guide=dict(iters=9), motion=None), "%s: guide iters 9 outside 1..8"),
    (STEP, dict(coef=dict(inpaint=1)), "%s: c->inpaint (the inpainting schedulers' blend) and a guide do not compose"),
    (LAUNCH, dict(mo=None), "%s: null tensor"),
    (COSTFN, dict(guide=None, field=None), "guide cost: null traj, guide, cost or active"),
    (SELECT, dict(guide=None, field=None), "traj select guide: null guide"),
]

# (overrides of a good adx_capsules_from_boxes call, adx_last_error() in full)
BOX_TABLE = [
    (dict(boxes=None), "capsules from boxes: null boxes or out"),
    (dict(out=None), "capsules from boxes: null boxes or out"),
    (dict(n=0), "capsules from boxes: n_boxes 0 outside 1..32"),
    (dict(n=33), "capsules from boxes: n_boxes 33 outside 1..32"),
    (dict(scenes=0), "capsules from boxes: 0 scenes, supported 1..1048576"),
    (dict(scenes=-2), "capsules from boxes: -2 scenes, supported 1..1048576"),
    (dict(inflate=-1.0), "capsules from boxes: inflate -1 is negative or not finite"),
    (dict(inflate=math.inf), "capsules from boxes: inflate inf is negative or not finite"),
    (dict(inflate=math.nan), "capsules from boxes: inflate nan is negative or not finite"),
    (dict(out=BOXES), "capsules from boxes: out overlaps boxes"),
    (dict(out=BOXES + 2 * 3 * 8 * 4 - 4), "capsules from boxes: out overlaps boxes"),
    (dict(out=BOXES - 2 * 3 * 7 * 4 + 4), "capsules from boxes: out overlaps boxes"),
]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from autonomous_driving_with_diffusion_model_amd import _lib
    return _lib


def call(L, name, over):
    """One call of export `name`: a good call at [6][8][7] (the selection: 3 candidates of 2 scenes) on placeholder addresses,
    with the overrides of `over` applied."""
    a = dict(coef={}, mo=MO, x=X, z=None, state=None, slot=7, row_offset=0, pin=None, guide={}, field={}, motion={}, route={}, capsule={},
             prev=PREV, x0=X0, px0=PX0, cost=COST, active=ACTIVE, index=INDEX, blocked=BLOCKED, best=BEST, select={}, B=B, H=H, D=D)
    a.update(over)
    coef = L.DpmCoef() if name.startswith("adx_dpm") else L.StepCoef()
    coef.prediction_type = 1
    for k, v in a["coef"].items():
        setattr(coef, k, v)
    guide = field = motion = route = capsule = None
    if a["guide"] is not None:
        g = L.GuideDesc()
        g.discs, g.planes, g.scene_rows, g.n_discs, g.n_planes, g.iters, g.lambda_, g.cap = DISCS, PLANES, 2, 3, 2, 1, 0.5, math.inf
        for k, v in a["guide"].items():
            setattr(g, k, v)
        guide = ctypes.byref(g)
    if a["field"] is not None:
        f = L.FieldDesc()
        f.cells, f.scene_rows, f.gx, f.gy, f.x_min, f.y_min, f.inv_dx, f.inv_dy, f.weight = CELLS, 2, GX, GY, -0.5, 0.25, 4.0, 2.0, 1.0
        for k, v in a["field"].items():
            setattr(f, k, v)
        field = ctypes.byref(f)
    if a["motion"] is not None:
        m = L.MotionDesc()
        m.limits, m.scene_rows, m.w_speed, m.w_accel = LIMITS, 2, 1.0, 0.5
        for k, v in a["motion"].items():
            setattr(m, k, v)
        motion = ctypes.byref(m)
    if a["route"] is not None:
        r = L.RouteDesc()
        r.points, r.half_width, r.scene_rows, r.n_points, r.weight = POINTS, WIDTH, 2, RN, 1.5
        for k, v in a["route"].items():
            setattr(r, k, v)
        route = ctypes.byref(r)
    if a["capsule"] is not None:
        c = L.CapsuleDesc()
        c.capsules, c.scene_rows, c.n_capsules, c.weight = CAPS, 2, CN, 1.5
        for k, v in a["capsule"].items():
            setattr(c, k, v)
        capsule = ctypes.byref(c)
    shape = (a["B"], a["H"], a["D"], None)
    if name in STEP:
        return L.lazy(name)(ctypes.byref(coef), a["mo"], a["x"], a["z"], a["state"], a["slot"], a["row_offset"], None, guide, field, motion,
                            route, capsule, a["prev"], a["x0"], *shape)
    if name in DPM:
        return L.lazy(name)(ctypes.byref(coef), a["mo"], a["x"], a["px0"], a["state"], a["slot"], a["row_offset"], None, guide, field,
                            motion, route, capsule, a["prev"], a["x0"], *shape)
    if name in COSTFN:
        return L.lazy(name)(a["x"], guide, field, motion, route, capsule, a["cost"], a["active"], *shape)
    assert name in SELECT, name
    cfg = L.SelectGuideCfg(2, 3, a["H"], a["D"], 1.0, 0.0, 0.0, 1.0, 1)
    for k, v in a["select"].items():
        setattr(cfg, k, v)
    return L.lazy(name)(ctypes.byref(cfg), a["x"], TARGET, guide, field, motion, route, capsule, a["cost"], a["active"], a["index"],
                        a["blocked"], a["best"], None)


def test_the_abi_has_the_six_entries(built, monkeypatch):
    import os
    import re
    with open(os.path.join(T.__file__.rsplit(os.sep, 2)[0], "include", "adx.h")) as fh:
        header = fh.read()
    for title in ("Cost guidance v5", "Capsules from boxes v1", "Cost guidance v4", "Cost guidance v3", "Cost guidance v2", "Cost guidance v1"):
        assert title in header, title
    v5 = header[header.index("Cost guidance v5"):]
    assert "a change is a new version, never an edit" in v5[:v5.index("typedef struct adx_guide_capsules")]
    boxes = header[header.index("Capsules from boxes v1"):]
    assert "a change is a new version" in boxes[:boxes.index("int adx_capsules_from_boxes")] and "INSCRIBED stadium" in boxes
    assert "#define ADX_CAPSULE_MAX 32" in header
    handle = built.lib()
    for name in EVERY + ("adx_capsules_from_boxes",):
        assert re.search(r"\b" + name + r"\s*\(", header) and hasattr(handle, name) and name in built.EXPORTED_SYMBOLS, name
    R = built.CapsuleDesc
    assert [f[0] for f in R._fields_] == ["capsules", "scene_rows", "n_capsules", "weight"]
    assert ctypes.sizeof(R) == 24
    assert (R.capsules.offset, R.scene_rows.offset, R.n_capsules.offset, R.weight.offset) == (0, 8, 12, 16)
    # v1's to v4's records are what they were
    assert ctypes.sizeof(built.GuideDesc) == 40 and ctypes.sizeof(built.FieldDesc) == 40 and ctypes.sizeof(built.MotionDesc) == 24
    assert ctypes.sizeof(built.RouteDesc) == 32
    assert {name for row in TABLE for name in row[0]} == set(EVERY)
    c = _caps(weight=2.0)
    monkeypatch.setattr(built, "require_gpu_f32", lambda t, name, dtype=torch.float32: t)      # `desc` launches nothing
    d = c.desc(torch.zeros(S, H, D))
    assert (d.capsules, d.scene_rows, d.n_capsules, d.weight) == (c.slots.data_ptr(), S, 3, 2.0)
    suffix, refs, alive = Guide(capsules=c).descs(torch.zeros(S, H, D), 0.5)
    assert suffix == "capsule" and len(refs) == 5 and refs[1] is None and refs[2] is None and refs[3] is None and alive[0].lambda_ == 0.5
    r = Route(torch.zeros(S, 4, 2), 0.1)
    suffix, refs, alive = Guide(route=r, capsules=c).descs(torch.zeros(S, H, D))
    assert suffix == "capsule" and refs[2] is None and refs[3] is not None and alive[4].n_capsules == 3 and alive[3].n_points == 4
    assert Guide().descs(torch.zeros(S, H, D))[0] == "guide" and Guide(route=r).descs(torch.zeros(S, H, D))[0] == "route"
    assert Guide(motion=MotionLimits(torch.zeros(S, 2))).descs(torch.zeros(S, H, D))[0] == "motion"
    assert Guide(field=CostField(torch.zeros(S, 3, 5))).descs(torch.zeros(S, H, D))[0] == "field"


@pytest.mark.parametrize("row", TABLE, ids=lambda row: "%s-%s" % (row[0][0], ",".join(row[1])))
def test_refusal_text(built, row):
    for name in row[0]:
        got = call(built, name, row[1])
        want = row[2] % NAME[name] if "%s" in row[2] else row[2]
        assert (got, built.lib().adx_last_error().decode()) == (-1, want), (name, row[1])


@pytest.mark.parametrize("row", BOX_TABLE, ids=lambda row: ",".join("%s=%s" % kv for kv in row[0].items()))
def test_from_boxes_refusal_text(built, row):
    a = dict(boxes=BOXES, out=OUT, scenes=2, n=3, inflate=0.25)
    a.update(row[0])
    got = built.lazy("adx_capsules_from_boxes")(a["boxes"], a["out"], a["scenes"], a["n"], a["inflate"], None)
    assert (got, built.lib().adx_last_error().decode()) == (-1, row[1])
