"""CPU: "stop-short fallback v1" (include/adx.h).  The contract's consequences on its NumPy restatement (tests/fallback_ref.py): the
invariants of the resampling on a few thousand random rows in fp32, the braking property and the convexity property in fp64, the
`status` rule on hand-made rows; every refusal of `adx_stop_short` by its whole text (they fire on the host before any GPU work,
so placeholder addresses are enough); `StopShort` as an object; and `plan_tick` with a fallback: its refusals, the field's
default and the plan key, which without a fallback is the key it was."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import fallback_ref as FB                                                                                       # noqa: E402
import test_tick_plan_cpu as TT                                                                                 # noqa: E402
from autonomous_driving_with_diffusion_model_amd import Capsules, Guide, MotionLimits, StopResult, StopShort     # noqa: E402
from autonomous_driving_with_diffusion_model_amd.control import fallback as F                                   # noqa: E402
from autonomous_driving_with_diffusion_model_amd.sampling import TickPlan, plan_tick                            # noqa: E402

F32, F64 = np.float32, np.float64
HS = (1, 2, 3, 5, 16, 24, 64)
DECELS = (0.0, 1e-4, 3e-3, 0.02, math.inf, math.nan, -1.0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == F32 else np.int64)


def _rows(H, n, seed, D=3):
    """n rows of H waypoints walking mostly along +x from the origin with steps of 0 .. 0.12 (one step in five is a duplicate
    waypoint), the params (a gap of 0 .. 0.1, every tenth larger than any path; a decel of DECELS in turn), and a guide
    that stops them somewhere: a plane x <= 0.02 .. min(1.2, 0.05 H) per row, a disc ahead and one empty slot."""
    r = np.random.default_rng(seed)
    step = r.uniform(0.0, 0.12, (n, H, 2)) * np.array([1.0, 0.3]) * r.choice([1.0, 1.0, 1.0, 1.0, 0.0], (n, H, 1))
    step[:, :, 1] *= r.choice([-1.0, 1.0], (n, H))
    t = np.zeros((n, H, D), F32)
    t[:, :, :2] = (np.cumsum(step, axis=1) - step[:, :1]).astype(F32)                  # p_0 = (0, 0)
    t[::9, :, 0] += 2.0                                                                 # every ninth starts beyond its plane: first = 0
    t[:, :, 2:] = r.uniform(-1, 1, (n, H, D - 2)).astype(F32)
    gap = r.uniform(0.0, 0.1, n)
    gap[::10] = 100.0
    params = np.stack([gap, np.resize(np.array(DECELS), n)], axis=1).astype(F32)
    planes = np.zeros((n, 1, 3), F32)
    planes[:, 0, 0], planes[:, 0, 2] = 1.0, r.uniform(0.02, min(1.2, 0.05 * H), n)       # within reach of a short row too
    discs = np.zeros((n, 2, 5), F32)
    discs[:, 0] = np.stack([r.uniform(0.3, 1.5, n), r.uniform(-0.3, 0.3, n), r.uniform(-0.02, 0.0, n), np.zeros(n), r.uniform(0.05, 0.3, n)], 1)
    return t, params, FB.guide(discs, planes)


@pytest.mark.parametrize("H", HS)
def test_the_invariants_of_the_resampling_hold_in_fp32(H):
    """600 rows per horizon, 4,200 in all: q is non-decreasing and never beyond L, 0 <= t <= 1, every output is finite, out_0 is
    p_0 in bits, and while the plan's own speed governs q_h is s_h and out_h is p_h in bits; free rows come back in bits."""
    t, params, g = _rows(H, 600, 100 + H)
    o = FB.stop_short(t, g, params, F32)
    b, first = o["blocked"], o["first"]
    assert o["out"].dtype == F32 and o["first"].dtype == np.int32 and o["stop_at"].dtype == F32
    assert b.any() and (H <= 2 or ((first > 1) & b).sum() > 50), (b.sum(), H)
    assert np.array_equal(_bits(o["out"][~b]), _bits(t[~b])) and (o["status"][~b] == 0).all() and np.isinf(o["stop_at"][~b]).all()
    assert (o["active_after"][~b] == 0).all() and (o["status"][b] >= 1).all()
    q, s, L = o["q"][b], o["s"][b], o["L"][b]
    assert (np.diff(q, axis=1) >= 0).all() and (q <= L[:, None]).all() and (L >= 0).all() and (q[:, 0] == 0).all()
    assert np.array_equal(o["stop_at"][b], L)
    assert (o["t"] >= 0).all() and (o["t"] <= 1).all()
    assert np.isfinite(o["out"]).all()
    assert np.array_equal(_bits(o["out"][:, 0]), _bits(t[:, 0]))                        # the loop's [:, 0, :3] = 0 survives
    assert np.array_equal(_bits(o["out"][:, :, 2:]), _bits(t[:, :, 2:]))                # columns >= 2 are traj's
    hidx = np.arange(H)[None, :]
    own = np.logical_and.accumulate((o["u"] == o["w"]) | (hidx == 0), axis=1) & (hidx < first[:, None]) & b[:, None]
    assert H < 3 or own[:, 1:].sum() > 20, own.sum()                                    # the fixture reaches the case
    assert np.array_equal(_bits(o["q"][own]), _bits(o["s"][own]))
    assert np.array_equal(_bits(o["out"][own]), _bits(t[own]))
    # decel = 0 does not move, a gap beyond the path stops at once: every waypoint is p_0
    for still in (b & (o["a"] == 0), b & (params[:, 0] == 100.0)):
        assert still.any() and np.array_equal(_bits(o["out"][still][:, :, :2]), _bits(np.broadcast_to(t[still][:, :1, :2], o["out"][still][:, :, :2].shape)))
    # a limit that is off (inf, NaN, negative) keeps the plan's speed up to the stop point: u = min(w, d)
    off = b & ~o["limited"]
    assert off.any() and np.array_equal(o["u"][off][:, 1:], np.minimum(o["w"][off][:, 1:], o["d"][off][:, 1:]))


@pytest.mark.parametrize("H", [h for h in HS if h >= 3])
def test_a_binding_envelope_sheds_decel_per_step_in_fp64(H):
    """For every h >= 1: u_{h+1} >= min(w_{h+1}, u_h - a, d_{h+1}) within rounding -- no step is shorter than braking by `a` from
    the step before asks, unless the plan's own speed or the stop point asks.  The bound is rounding alone: e is five fp64 operations
    on magnitudes up to a + sqrt(8 a d), and d_{h+1} = L - (q_{h-1} + u_h) stands in for d_h - u_h with two roundings of
    magnitude L, which e passes on at most doubled (de/dd = 2a / sqrt(a^2 + 8 a d) <= 2): 16 * 2^-53 * (a + sqrt(8 a d) + u_h + L)
    covers both with room to spare."""
    t, params, g = _rows(H, 600, 300 + H)
    o = FB.stop_short(t.astype(F64), g, params.astype(F64), F64)
    lim = o["blocked"] & o["limited"]
    u, w, d, a = o["u"][lim], o["w"][lim], o["d"][lim], o["a"][lim][:, None]
    want = np.minimum(np.minimum(w[:, 2:], u[:, 1:-1] - a), d[:, 2:])
    tol = 16 * 2.0 ** -53 * (a + np.sqrt(8 * a * d[:, 2:]) + u[:, 1:-1] + o["L"][lim][:, None])
    short = want - u[:, 2:]
    print("H", H, "rows", int(lim.sum()), "largest shortfall / a", float(np.max(short / np.where(a > 0, a, 1.0))))
    assert lim.sum() > 100 and (short <= tol).all()
    assert (u >= 0).all()


def test_planes_alone_leave_nothing_active_in_fp64():
    """The free set of half-planes is convex and every output lies on the free part of the plan's polyline, so a re-timed row
    violates nothing whenever it has a free waypoint to stand on (first >= 1).  A property of the contract, not of rounding:
    fp64, and rows whose waypoints all keep 1e-6 from every plane's edge."""
    n, H = 3000, 16
    r = np.random.default_rng(7)
    t = np.zeros((n, H, 2))
    t[:, 1:] = np.cumsum(r.uniform(-0.03, 0.12, (n, H - 1, 2)), axis=1)
    ang = r.uniform(-1.2, 1.2, (n, 3))
    planes = np.stack([np.cos(ang), np.sin(ang), r.uniform(0.1, 1.0, (n, 3))], axis=2)
    psi = planes[:, None, :, 0] * t[:, :, None, 0] + planes[:, None, :, 1] * t[:, :, None, 1] - planes[:, None, :, 2]
    keep = (np.abs(psi) >= 1e-6).all(axis=(1, 2))
    t, planes = t[keep], planes[keep]
    params = np.stack([r.uniform(0, 0.05, len(t)), np.resize(np.array([0.0, 2e-3, 0.01, math.inf]), len(t))], axis=1)
    o = FB.stop_short(t, dict(discs=None, planes=planes, field=None, route=None, capsules=None), params, F64)
    stands = o["blocked"] & (o["first"] >= 1)
    print("rows", len(t), "blocked with a free waypoint", int(stands.sum()), "blocked at 0", int((o["first"] == 0).sum()))
    assert keep.sum() > 2500 and stands.sum() > 1000 and (o["first"][0:] >= 1).all()         # p_0 = (0, 0) is free of b >= 0.1
    assert (o["active_after"][stands] == 0).all()


def test_the_status_rule_on_hand_made_rows():
    """A plan advancing 0.1 per waypoint toward a wall at x <= 0.45 (first = 5, s_4 = 0.4): free of it -> 0; a decel that the
    plan's first step already meets -> 1; one it cannot -> 2; a limit that is off, a conflict at waypoint 0 or 1 -> 1."""
    H = 8
    t = np.zeros((6, H, 2), F32)
    t[:, :, 0] = np.float32(0.1) * np.arange(H, dtype=F32)
    t[3, :, 0] += 0.5                                                                   # starts beyond the wall: first = 0
    t[4, 1:, 0] += 0.4                                                                  # jumps beyond it: first = 1
    planes = np.array([[[1.0, 0.0, 0.45]]] * 6, F32)
    planes[0, 0, 2] = 5.0                                                               # no wall in reach
    params = np.array([[0, 0.01], [0, 0.05], [0, 0.005], [0, 0.005], [0, 0.005], [0, np.inf]], F32)
    o = FB.stop_short(t, FB.guide(None, planes), params, F32)
    assert o["first"].tolist() == [H, 5, 5, 0, 1, 5] and o["status"].tolist() == [0, 1, 2, 1, 1, 1]
    # row 1: e(0.4) = (sqrt(0.0025 + 0.16) - 0.05) / 2 > 0.1: the plan's own first step stands; row 2: e(0.4) < 0.1 - 0.005
    assert o["u"][1, 1] == o["seg"][1, 1] and o["seg"][2, 1] - o["u"][2, 1] > np.float32(0.005)
    assert np.isinf(o["stop_at"][0]) and o["stop_at"][3] == 0 and o["stop_at"][4] == 0 and abs(o["stop_at"][1] - 0.4) < 1e-6
    assert np.array_equal(o["out"][3, :, 0], np.full(H, t[3, 0, 0])) and np.array_equal(o["out"][4, :, 0], np.zeros(H, F32))
    # a NaN waypoint is a conflict of its own
    t[0, 3, 1] = np.nan
    o = FB.stop_short(t, FB.guide(None, planes), params, F32)
    assert o["first"][0] == 3 and o["status"][0] == 2 and np.isfinite(o["out"][0]).all() and abs(o["stop_at"][0] - 0.2) < 1e-6


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------------------------
B, H, D = 6, 8, 7
TRAJ, OUT, PARAMS, FIRST, STATUS, STOP, AFTER, DISCS, PLANES, CELLS, POINTS, WIDTH, SLOTS = (0x10000000 * (i + 1) for i in range(13))
NULLS = "stop short: null traj, out, params, first, status, stop_at or active_after"
OVER = "stop short: an output overlaps traj, params or another output (out == traj, the same pointer, is allowed)"
TABLE = [
    (dict(traj=None), NULLS), (dict(out=None), NULLS), (dict(params=None), NULLS), (dict(first=None), NULLS),
    (dict(status=None), NULLS), (dict(stop=None), NULLS), (dict(after=None), NULLS),
    (dict(guide=None), "stop short: null guide and null field"),
    (dict(H=0), "stop short: horizon 0 outside 1..64"), (dict(H=65), "stop short: horizon 65 outside 1..64"),
    (dict(D=1), "stop short: the fallback re-times (x, y), dim is 1"),
    (dict(param_rows=0), "stop short: param_rows 0, at least 1"),
    (dict(B=0), "stop short: empty shape"), (dict(B=-3), "stop short: empty shape"),
    (dict(B=1 << 25, H=64, D=16), "stop short: 34359738368 elements do not fit the kernel's 32-bit index"),
    # what guide_records_check (csrc/sched.h) refuses, under this launch's name
    (dict(guide=dict(n_discs=33)), "stop short: n_discs 33 outside 0..32"),
    (dict(guide=dict(n_planes=-1)), "stop short: n_planes -1 outside 0..8"),
    (dict(guide=dict(discs=None)), "stop short: null discs with n_discs 2"),
    (dict(guide=dict(planes=None)), "stop short: null planes with n_planes 1"),
    (dict(guide=dict(scene_rows=4)), "stop short: batch 6 must be a positive multiple of scene_rows 4"),
    (dict(out=DISCS), "stop short: an output overlaps discs or planes"),
    (dict(first=PLANES + 4), "stop short: an output overlaps discs or planes"),
    (dict(stop=DISCS + 8), "stop short: an output overlaps discs or planes"),
    (dict(after=PLANES), "stop short: an output overlaps discs or planes"),
    (dict(field=dict(cells=None)), "stop short: null field cells"),
    (dict(field=dict(gx=1)), "stop short: field of 4 x 1 nodes (gy x gx), supported 2..256 each"),
    (dict(field=dict(scene_rows=3)), "stop short: the field holds 3 scenes, the guide's discs and planes 2"),
    (dict(field={}, status=CELLS + 16), "stop short: an output overlaps the field's cells"),
    (dict(route=dict(points=None)), "stop short: null route points"),
    (dict(route=dict(n_points=1)), "stop short: route of 1 points, supported 2..32"),
    (dict(route=dict(scene_rows=3)), "stop short: the route holds 3 scenes, the guide's discs and planes 2"),
    (dict(route={}, after=WIDTH + 4), "stop short: an output overlaps the route's points or half_width"),
    (dict(route={}, status=POINTS + 2 * 3 * 2 * 4 - 4), "stop short: an output overlaps the route's points or half_width"),
    (dict(route={}, status=POINTS + 2 * 3 * 2 * 4, after=STOP), OVER),                 # one byte past the points: the next refusal
    (dict(capsules=dict(capsules=None)), "stop short: null capsules"),
    (dict(capsules=dict(n_capsules=33)), "stop short: n_capsules 33 outside 1..32"),
    (dict(capsules=dict(weight=-1.0)), "stop short: capsule weight -1 is negative or NaN"),
    (dict(capsules={}, stop=SLOTS), "stop short: an output overlaps the capsules"),
    (dict(guide=dict(n_discs=0, n_planes=0)), F.NO_POINTWISE_TERM),
    # the outputs against traj, params and each other; out == traj alone is allowed
    (dict(out=TRAJ + 4), OVER), (dict(first=TRAJ), OVER), (dict(status=TRAJ + B * H * D * 4 - 4), OVER), (dict(out=PARAMS - 4), OVER),
    (dict(stop=PARAMS + 8), OVER), (dict(first=OUT + 64), OVER), (dict(status=FIRST + 20), OVER), (dict(after=STOP), OVER),
    (dict(out=TRAJ, first=TRAJ + 8), OVER),
]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from autonomous_driving_with_diffusion_model_amd import _lib
    return _lib


def _call(L, over):
    """One call of adx_stop_short: a good call at [6][8][7] over 2 scenes on placeholder addresses (a guide of 2 discs and 1 plane;
    a field, a route or capsules when `over` names one), with the overrides applied."""
    a = dict(traj=TRAJ, out=OUT, params=PARAMS, param_rows=2, first=FIRST, status=STATUS, stop=STOP, after=AFTER, B=B, H=H, D=D,
             guide={}, field=None, route=None, capsules=None)
    a.update(over)
    recs = []
    for name, cls, base in (("guide", L.GuideDesc, dict(discs=DISCS, planes=PLANES, scene_rows=2, n_discs=2, n_planes=1, iters=1, cap=1.0)),
                            ("field", L.FieldDesc, dict(cells=CELLS, scene_rows=2, gy=4, gx=4, inv_dx=1.0, inv_dy=1.0, weight=1.0)),
                            ("route", L.RouteDesc, dict(points=POINTS, half_width=WIDTH, scene_rows=2, n_points=3, weight=1.0)),
                            ("capsules", L.CapsuleDesc, dict(capsules=SLOTS, scene_rows=2, n_capsules=3, weight=1.0))):
        if a[name] is None:
            recs.append(None)
            continue
        rec = cls()
        for k, v in dict(base, **a[name]).items():
            setattr(rec, k, v)
        recs.append(rec)
    refs = [None if r is None else ctypes.byref(r) for r in recs]
    return L.lazy("adx_stop_short")(a["traj"], *refs, a["params"], a["param_rows"], a["out"], a["first"], a["status"], a["stop"], a["after"],
                                    a["B"], a["H"], a["D"], None)


@pytest.mark.parametrize("row", TABLE, ids=lambda row: ",".join("%s=%s" % (k, v if not isinstance(v, dict) else ".".join(v) or "on")
                                                                 for k, v in row[0].items()))
def test_refusal_text(built, row):
    assert (_call(built, row[0]), built.lib().adx_last_error().decode()) == (-1, row[1]), row[0]


def test_the_export_is_declared_bound_and_listed(built):
    header = open(os.path.join(ROOT, "include", "adx.h")).read()
    assert "Stop-short fallback v1" in header and re.search(r"\badx_stop_short\s*\(", header)
    assert hasattr(ctypes.CDLL(built.LIB_PATH), "adx_stop_short") and "adx_stop_short" in built.EXPORTED_SYMBOLS
    assert "active_after" in header and "NOT promised to be 0" in header               # the header says what the number is
    srcs = open(os.path.join(os.path.dirname(built.LIB_PATH), "csrc", "build.sh")).read()
    assert " fallback.hip " in srcs


# ---- the object -------------------------------------------------------------------------------------------------------------------
def test_stop_short_the_object():
    import autonomous_driving_with_diffusion_model_amd as pkg
    from autonomous_driving_with_diffusion_model_amd import control
    assert pkg.StopShort is StopShort is control.StopShort and {"StopShort", "StopResult"} <= set(pkg.__all__) & set(control.__all__)
    assert StopResult._fields == ("traj", "first", "status", "stop_at", "active_after")
    fb = StopShort(torch.tensor([[0.05, 0.01], [0.0, math.inf]]))
    assert fb.scenes == 2 and fb.device == torch.device("cpu") and fb.last is None
    assert fb.key() == fb.like(torch.zeros(5, 2)).key() and fb.like(torch.zeros(5, 2)).scenes == 5       # the values are not baked
    assert repr(fb) == "StopShort(params=(2, 2))"
    for bad, err in (([[0.0, 0.0]], TypeError), (torch.zeros(2, 3), ValueError), (torch.zeros(2), ValueError),
                     (torch.zeros(0, 2), ValueError), (torch.zeros(2, 2, dtype=torch.float64), TypeError)):
        with pytest.raises(err, match="StopShort: params"):
            StopShort(bad)
    # from_physical: 2 m of gap and 3 m/s^2 at 0.5 s between waypoints and 40 m per unit; a number stands for every scene
    p = StopShort.from_physical(2.0, [3.0, math.inf, 0.0], 0.5, 40.0).params
    assert p.dtype == torch.float32 and p.shape == (3, 2)
    assert p[:, 0].tolist() == [np.float32(2.0 / 40.0)] * 3 and p[:, 1].tolist() == [np.float32(3.0 * 0.25 / 40.0), math.inf, 0.0]
    # a 0-dim tensor, a NumPy scalar and a one-element list are numbers too; a 1-D tensor or array is a sequence
    for one in (torch.tensor(2.0), np.float32(2.0), np.array(2.0), [2.0]):
        assert torch.equal(StopShort.from_physical(one, torch.tensor([3.0, math.inf, 0.0]), 0.5, 40.0).params, p)
        assert torch.equal(StopShort.from_physical(one, np.array([3.0, math.inf, 0.0]), 0.5, 40.0).params, p)
    with pytest.raises(TypeError, match="gap_m must be a number or a sequence of numbers, got NoneType"):
        StopShort.from_physical(None, 1.0, 0.5, 40.0)
    for kw, msg in ((dict(dt=0.0), "dt and xy_scale"), (dict(xy_scale=math.inf), "dt and xy_scale"), (dict(gap_m=-1.0), "gap_m must be >= 0"),
                    (dict(decel_mps2=[1.0, -2.0]), "decel_mps2 must be >= 0"), (dict(gap_m=[1.0, 2.0], decel_mps2=[1.0, 2.0, 3.0]), "holds 2 scenes")):
        with pytest.raises(ValueError, match=msg):
            StopShort.from_physical(**dict(dict(gap_m=1.0, decel_mps2=1.0, dt=0.5, xy_scale=40.0), **kw))
    with pytest.raises(TypeError, match="`guide` must be a Guide"):
        fb(torch.zeros(2, 8, 3), None)


# ---- plan_tick ----------------------------------------------------------------------------------------------------------------------
S = TT.S


class _Scheduler(TT._Scheduler):
    supports_guide = True


def _guide(**kw):
    return Guide(planes=torch.tensor([[[1.0, 0.0, 0.5]]] * S), **kw)


def _plan(cfg=None, **kw):
    return plan_tick(TT.MODEL, _Scheduler(), cfg or TT._cfg(), TT.IMG, None, None, noise=TT._Noise([]), **kw)


def _old_key(p):
    """TickPlan.key() as it was before the plan had a fallback."""
    sel, ctl, pin, guide = p.selector, p.controller, p.pin, p.guide
    weights = None if sel is None else (sel.w_goal, sel.w_smooth, sel.w_consensus)
    if sel is not None and sel.uses_guide:
        weights += (sel.w_guide, sel.hard)
    return (p.S, p.K, weights, p.rows, p.H, p.D, p.n, p.use, p.free_scale, p.fuse, p.hoisted, p.is_ddpm,
            "init" if p.start == "randn" else p.start, p.m_warm, p.shift, p.is_warm, p.motion is None,
            None if ctl is None else (id(ctl), ctl.state.data_ptr(), ctl.key(), p.velocity is None),
            None if pin is None else (pin.mode, tuple(pin.known.shape)), None if guide is None else guide.key())


def test_the_plan_with_and_without_a_fallback():
    assert TickPlan.__dataclass_fields__["fallback"].default is None
    assert list(TickPlan.__dataclass_fields__)[-1] == "fallback"                        # after every field the plan had
    fb = StopShort(torch.zeros(S, 2))
    ctl = TT._controller()
    for kw in (dict(), dict(guide=_guide()), dict(guide=_guide(), candidates=3, selector=TT.TrajectorySelector(1.0, 0.5, 0.0, 2.0, True)),
               dict(guide=_guide(), controller=ctl, velocity=torch.zeros(S)), dict(pin=TT._pin())):
        plain = _plan(**kw)
        assert plain.fallback is None and plain.key() == _old_key(plain), kw
        if "guide" in kw:
            with_fb = _plan(fallback=fb, **kw)
            assert with_fb.fallback is fb and with_fb.key() == plain.key() + (fb.key(),) and with_fb.key() != plain.key()
            # new params are a buffer's values: the same key
            assert _plan(fallback=StopShort(torch.ones(S, 2)), **kw).key() == with_fb.key()


def test_plan_tick_refuses_a_fallback_it_cannot_run():
    fb = StopShort(torch.zeros(S, 2))
    with pytest.raises(TypeError, match="`fallback` must be a StopShort, got tuple"):
        _plan(guide=_guide(), fallback=(0.0, 0.0))
    with pytest.raises(ValueError, match="a fallback re-times the plan against a guide; pass guide=Guide"):
        _plan(fallback=fb)
    limits_only = Guide(motion=MotionLimits(torch.ones(S, 2)))
    with pytest.raises(ValueError) as e:
        _plan(guide=limits_only, fallback=fb)
    assert str(e.value) == F.NO_POINTWISE_TERM == "stop short: the guide holds no point-wise term (discs, planes, a field, a route or capsules)"
    assert _plan(guide=Guide(capsules=Capsules(torch.zeros(S, 1, 7))), fallback=fb).fallback is fb
    long = TT._cfg()
    long.MODEL.HORIZON = 65
    with pytest.raises(ValueError, match="needs MODEL.HORIZON <= 64, got 65"):
        _plan(long, guide=_guide(), fallback=fb)
    flat = TT._cfg()
    flat.MODEL.TRANSITION_DIM = 1
    with pytest.raises(ValueError, match="TRANSITION_DIM >= 2, got 1"):                 # the guide's own refusal comes first
        _plan(flat, guide=_guide(), fallback=fb)
    with pytest.raises(ValueError, match=r"fallback.params must hold 2 scenes \(image.shape\[0\]\) on cpu, got \(3, 2\) on cpu"):
        _plan(guide=_guide(), fallback=StopShort(torch.zeros(3, 2)))
    with pytest.raises(ValueError, match="source='action' reads the model's action columns and would not see a re-timing"):
        _plan(guide=_guide(), fallback=fb, controller=TT._controller(source="action"))
    assert _plan(guide=_guide(), fallback=fb, controller=TT._controller(), velocity=torch.zeros(S)).fallback is fb
    assert fb.last is None                                                              # no refusal and no plan ran anything
