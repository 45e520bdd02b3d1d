"""GPU: "cost guidance v3" -- the row-wise step kernels against the fp32 restatement (tests/motion_ref.py) bit for bit, neutral
limits against the element-wise kernels bit for bit (which holds the row-wise kernel's whole step body to the existing one), the
C ABI's NULL motion record, `Guide.cost` with limits against the fp64 restatement within a bound derived from the contract, the
guided selection, generate_traj(guide=Guide(motion=...)) against the loop written out from public `scheduler.step(guide=...)`
calls, and GraphedSampler replays.  No timing is asserted anywhere (tools/guide_tick_probe.py --motion measures), and nothing here
says what limits do to driving quality.

Shapes are the smallest at which the row-wise kernel can go wrong: H in {1, 2, 3, 5, 24, 64} (no segment, no curvature, one
curvature, the first full five-point stencil, idle lanes, a full wave), D in {2, 3, 7}, rows in {1, 4, 5} (one wave, one full
workgroup, a ragged last workgroup), 6 rows over 2 scenes, iters in {1, 8}.  Every launch is at most a few thousand elements."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

import field_ref as FR
import guide_ref as G
import motion_ref as MR
import pin_ref as R
import test_gpu_guide as TG
import test_gpu_pin as TP
from autonomous_driving_with_diffusion_model_amd import (CostField, DeviceController, DeviceNoise, Guide, MotionLimits, TrajectorySelector,
                                                         WarmStart)
from autonomous_driving_with_diffusion_model_amd import _lib as L
from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler, generate_traj

pytestmark = pytest.mark.gpu
DEV = TP.DEV
_bits, _same = TP._bits, TP._same
FUSIONS, PREDS, STEP_CASES = TG.FUSIONS, TG.PREDS, TG.STEP_CASES
# (K, S, H, D, iters): every H, D, row count and iters of the docstring; K * S = 6 over S = 2 is `r % scene_rows`
GEOS = [(1, 1, 1, 2, 1), (4, 1, 2, 3, 8), (5, 1, 3, 7, 1), (3, 2, 5, 2, 8), (1, 1, 24, 3, 1), (4, 1, 64, 7, 8), (5, 1, 64, 2, 1),
        (3, 2, 24, 7, 8), (5, 1, 5, 3, 8), (1, 1, 64, 3, 8), (4, 1, 3, 2, 1), (3, 2, 2, 7, 1), (3, 2, 64, 3, 1), (3, 2, 1, 7, 8)]
GY, GX, WEIGHT = 3, 5, 0.6
GEO = dict(origin=(-1.0, -1.0), cell=(0.5, 1.0))                 # the raster covers the clipped x0's [-1, 1]^2
W_SPEED, W_ACCEL = 1.0, 0.5


class Inputs(TP.Inputs):
    """One step's operands (test_gpu_pin.Inputs) and one scene set's guide: a disc of radius 3 around the origin and a positive
    field over [-1, 1]^2, which no clipped x0 can miss, and limits (0.3, 0.2), (0.15, 0.4) that random waypoints a unit apart
    exceed -- both motion terms, the disc and the field are active at once wherever the terms exist (the step test asserts it)."""

    def __init__(self, K, Sn, H, D, seed, combine, field=True):
        super().__init__(K, Sn, H, D, seed, combine)
        g = torch.Generator().manual_seed(seed + 2000)
        self.discs = torch.zeros(Sn, 1, 5)
        self.discs[..., :2] = torch.rand(Sn, 1, 2, generator=g) * 0.2 - 0.1
        self.discs[..., 4] = 3.0
        self.cells = torch.rand(Sn, GY, GX, generator=g) + 0.1 if field else None
        self.limits = torch.tensor([[0.3, 0.2], [0.15, 0.4]])[:Sn].contiguous()
        self.d = {k: v.to(DEV) for k, v in vars(self).items() if torch.is_tensor(v)}

    def field(self):
        return None if self.cells is None else CostField(self.d["cells"], weight=WEIGHT, **GEO)

    def guide(self, limits="own", w=(W_SPEED, W_ACCEL), **kw):
        motion = None if limits is None else MotionLimits(self.d["limits"] if isinstance(limits, str) else limits.to(DEV), *w)
        return Guide(self.d["discs"], None, field=self.field(), motion=motion, **kw)

    def ref_field(self):
        return None if self.cells is None else FR.field(self.cells, weight=WEIGHT, **GEO)

    def ref_motion(self):
        return MR.motion(self.limits, W_SPEED, W_ACCEL)

    def ref(self, lam, cap, iters):
        return dict(discs=self.discs, planes=None, lam=lam, cap=cap, iters=iters, field=self.ref_field(), motion=self.ref_motion())


def _ref_step(inp, *a):
    with MR._guided(inp.ref_field(), inp.ref_motion()):          # test_gpu_guide's restated step, field and limits in its cost_grad
        return TG._ref_step(*a)


def _what_is_active(inp, x0):
    """(disc, field, segment, curvature) active anywhere on the clipped x0 [B, H, D] the guide starts from, by the restatement."""
    a = x0.cpu().numpy()
    x, y = a[:, :, 0], a[:, :, 1]
    B = a.shape[0]
    disc = G.cost_grad(G.scene_rows(inp.discs.numpy(), B), None, x, y)[3].any()
    field = FR.field_term(inp.ref_field(), x, y)[0].any()
    seg, curv = MR.terms(inp.ref_motion(), x, y)
    return bool(disc), bool(field), bool(seg["on"].any()), bool(curv["on"].any())


# ---- 1. the step against the restatement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_motion_guided_step_equals_the_restatement_bit_for_bit(case):
    """DDIM, DDPM and DPM (orders 1 and 2), tensor noise and DeviceNoise: the three prediction types x clip on and off x the
    classifier-free combine and zero_first x with and without a pin (`clean` or `repaint`, the case's); the geometry walks through
    all of GEOS, the schedule alternates `constant` and `variance`, the cap 0.03 and 0.25.  prev_sample and x0 equal
    tests/motion_ref.py on the int32 view, fed the z the step itself saw; disc, field and both motion terms are active on the x0
    the guide starts from; the limits are in the result; no column d >= 2 ever differs from the unguided step."""
    noise = DeviceNoise((11 << 32) | 3, DEV)
    noise.begin_tick()
    sampler, mode = case[1], case[4]
    n, seen, motion_any, moved_any = 0, set(), 0, 0
    for pred, clip in itertools.product(PREDS, (True, False)):
        q = TG._sched(sampler, pred, clip)
        for (cfg_scale, zf), pinned, w in itertools.product(FUSIONS, (False, True), case[5]):
            geo = GEOS[n % len(GEOS)]
            K, Sn, H, D, iters = geo
            seen.add(geo)
            schedule, scale = ("variance", 0.05) if n % 2 else ("constant", 0.02)
            cap = 0.25 if n % 3 else 0.03
            what = (case[0], pred, clip, cfg_scale, zf, pinned, w, geo, schedule, cap)
            inp = Inputs(K, Sn, H, D, 700 + n, cfg_scale is not None)
            guide = inp.guide(scale=scale, schedule=schedule, cap=cap, iters=iters)
            pin = inp.pin(mode) if pinned else None
            prev, x0, hist = TG._gpu_step(case, q, inp, w, pin, guide, cfg_scale, zf, noise)
            z = TG._z(case, inp, w, noise, (K * Sn, H, D))
            args = (case, q, inp, w, pred, clip, (scale, schedule, cap, iters), pinned, cfg_scale, zf, z, hist)
            want_prev, want_x0, lam = _ref_step(inp, *args)
            diff = (prev.cpu() - want_prev).abs().max().item()
            print(what, "lambda =", lam, "max |prev - ref| =", diff)
            assert torch.isfinite(want_x0).all(), what
            assert _same(x0, want_x0), (what, (x0.cpu() - want_x0).abs().max().item())
            assert _same(prev, want_prev), (what, diff)
            plain, x0_plain, _ = TG._gpu_step(case, q, inp, w, pin, None, cfg_scale, zf, noise)
            moved = _bits(x0.cpu()) != _bits(x0_plain.cpu())
            assert not moved[..., 2:].any(), what                                         # columns d >= 2 never move
            moved_any += int(moved.any())
            disc, field, seg, curv = _what_is_active(inp, x0_plain)
            assert seg == (H >= 2) and curv == (H >= 3), (what, seg, curv)
            assert (disc and field) or not clip, (what, disc, field)                      # an unclipped x0 may leave disc and raster
            without = TG._gpu_step(case, q, inp, w, pin, inp.guide(None, scale=scale, schedule=schedule, cap=cap, iters=iters), cfg_scale,
                                   zf, noise)[1]
            motion_any += int(not torch.equal(without, x0))
            assert H >= 2 or torch.equal(without, x0), what                               # H = 1: no motion term at all
            if zf:
                assert bool((prev[:, 0, :3] == 0).all()), what
            n += 1
    assert n == 6 * len(FUSIONS) * 2 * len(case[5]) and seen == set(GEOS)
    assert motion_any >= n // 2 and moved_any >= n // 2, (motion_any, moved_any, n)       # the limits are really in the results


# ---- 2. neutral limits are the old kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_neutral_limits_are_the_element_wise_kernel_bit_for_bit(case):
    """Every scene at +inf, and separately both weights 0 (over live limits): the `_motion` export -- the row-wise kernel -- gives
    the `_field` export's prev_sample and x0 (the `_guide` export's without a field) by torch.equal, on every geometry, fusion and
    pin of the step test.  A NaN limit is neutral too."""
    noise = DeviceNoise(47, DEV)
    noise.begin_tick()
    sampler, mode = case[1], case[4]
    n = 0
    for pred, clip in zip(PREDS, (True, False, True)):
        q = TG._sched(sampler, pred, clip)
        for (cfg_scale, zf), pinned, w in itertools.product(FUSIONS, (False, True), case[5]):
            for geo in (GEOS[n % len(GEOS)], GEOS[(n + 5) % len(GEOS)]):
                K, Sn, H, D, iters = geo
                what = (case[0], pred, clip, cfg_scale, zf, pinned, w, geo)
                inp = Inputs(K, Sn, H, D, 300 + n, cfg_scale is not None, field=bool(n % 2))
                pin = inp.pin(mode) if pinned else None
                kw = dict(scale=0.03, schedule="constant", cap=0.25, iters=iters)
                old, old_x0, _ = TG._gpu_step(case, q, inp, w, pin, inp.guide(None, **kw), cfg_scale, zf, noise)
                neutral = {"inf": inp.guide(torch.full((Sn, 2), math.inf), **kw), "nan": inp.guide(torch.full((Sn, 2), math.nan), **kw),
                           "weights 0": inp.guide("own", (0.0, 0.0), **kw)}
                for name, guide in neutral.items():
                    assert guide.descs(inp.d["x"])[0] == "motion"
                    got, got_x0, _ = TG._gpu_step(case, q, inp, w, pin, guide, cfg_scale, zf, noise)
                    assert torch.equal(_bits(got), _bits(old)) and torch.equal(_bits(got_x0), _bits(old_x0)), (what, name)
                if H >= 2:
                    live, _, _ = TG._gpu_step(case, q, inp, w, pin, inp.guide(**kw), cfg_scale, zf, noise)
                    assert not torch.equal(live, old), what
            n += 1


def test_a_null_motion_record_is_the_field_export_bit_for_bit():
    inp = Inputs(3, 2, 8, 7, 13, False)
    d = inp.d
    B, H, D = d["x"].shape
    noise = DeviceNoise(8, DEV)
    noise.begin_tick()
    st = L.stream_ptr(torch.device(DEV))
    pin = inp.pin("clean").desc(d["x"], R.CLEAN)
    guide = inp.guide(None, scale=0.05, schedule="constant", iters=2)
    g, f = guide.desc(d["x"], 0.05), guide.field_desc(d["x"])

    def outs():
        return torch.empty_like(d["x"]), torch.empty_like(d["x"])

    for name, coef in (("ddim", TG._sched("ddim")._ddim_coef(60, 0.5, False)), ("ddpm", TG._sched("ddpm")._ddpm_coef(60))):
        old, new = L.lazy(f"adx_{name}_step_field"), L.lazy(f"adx_{name}_step_motion")
        for p, fd in itertools.product((None, C.byref(pin)), (None, C.byref(f))):
            (p0, a0), (p1, a1), (p2, a2), (p3, a3) = outs(), outs(), outs(), outs()
            L.check(old(C.byref(coef), d["mo"].data_ptr(), d["x"].data_ptr(), d["z"].data_ptr(), None, 0, 0, p, C.byref(g), fd, p0.data_ptr(),
                        a0.data_ptr(), B, H, D, st))
            L.check(new(C.byref(coef), d["mo"].data_ptr(), d["x"].data_ptr(), d["z"].data_ptr(), None, 0, 0, p, C.byref(g), fd, None,
                        p1.data_ptr(), a1.data_ptr(), B, H, D, st))
            L.check(old(C.byref(coef), d["mo"].data_ptr(), d["x"].data_ptr(), None, noise.state_ptr(), 60, 5, p, C.byref(g), fd, p2.data_ptr(),
                        a2.data_ptr(), B, H, D, st))
            L.check(new(C.byref(coef), d["mo"].data_ptr(), d["x"].data_ptr(), None, noise.state_ptr(), 60, 5, p, C.byref(g), fd, None,
                        p3.data_ptr(), a3.data_ptr(), B, H, D, st))
            assert torch.equal(_bits(p0), _bits(p1)) and torch.equal(_bits(a0), _bits(a1)), name
            assert torch.equal(_bits(p2), _bits(p3)) and torch.equal(_bits(a2), _bits(a3)), name
            assert not torch.equal(p0, p2), name                                         # two noises, two results
    coef = TG._sched("dpm")._dpm_coef(1)
    for p, fd in itertools.product((None, C.byref(pin)), (None, C.byref(f))):
        (p0, a0), (p1, a1) = outs(), outs()
        L.check(L.lazy("adx_dpm_step_field")(C.byref(coef), d["mo"].data_ptr(), d["x"].data_ptr(), d["hx"].data_ptr(), None, 0, 0, p,
                                             C.byref(g), fd, p0.data_ptr(), a0.data_ptr(), B, H, D, st))
        L.check(L.lazy("adx_dpm_step_motion")(C.byref(coef), d["mo"].data_ptr(), d["x"].data_ptr(), d["hx"].data_ptr(), None, 0, 0, p,
                                              C.byref(g), fd, None, p1.data_ptr(), a1.data_ptr(), B, H, D, st))
        assert coef.second_order == 1 and torch.equal(_bits(p0), _bits(p1)) and torch.equal(_bits(a0), _bits(a1))
    # the cost and the selection
    c0, c1 = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    n0, n1 = torch.empty(B, dtype=torch.int32, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
    L.check(L.lazy("adx_guide_cost_field")(d["x"].data_ptr(), C.byref(g), C.byref(f), c0.data_ptr(), n0.data_ptr(), B, H, D, st))
    L.check(L.lazy("adx_guide_cost_motion")(d["x"].data_ptr(), C.byref(g), C.byref(f), None, c1.data_ptr(), n1.data_ptr(), B, H, D, st))
    assert torch.equal(_bits(c0), _bits(c1)) and torch.equal(n0, n1) and int(n0.sum()) > 0
    cfg = L.SelectGuideCfg(2, 3, H, D, 0.0, 0.5, 0.25, 1.0, 1)
    res = []
    for name, extra in (("adx_traj_select_guide_field", ()), ("adx_traj_select_guide_motion", (None,))):
        cost, act = torch.empty(2, 3, device=DEV), torch.empty(2, 3, dtype=torch.int32, device=DEV)
        idx, blk = torch.empty(2, dtype=torch.int32, device=DEV), torch.empty(2, dtype=torch.int32, device=DEV)
        best = torch.empty(2, H, D, device=DEV)
        L.check(L.lazy(name)(C.byref(cfg), d["x"].data_ptr(), None, C.byref(g), C.byref(f), *extra, cost.data_ptr(), act.data_ptr(),
                             idx.data_ptr(), blk.data_ptr(), best.data_ptr(), st))
        res.append((cost, act, idx, blk, best))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*res))


# ---- 3. the cost kernel -----------------------------------------------------------------------------------------------------------
COST_CASES = [(rows, Sn, H, D) for (rows, Sn), H, D in zip(itertools.cycle([(1, 1), (4, 1), (5, 1), (6, 2)]), (1, 2, 3, 5, 24, 64, 64, 24),
                                                           itertools.cycle([2, 3, 7]))]


def _cost_case(rows, Sn, H, D, seed=7):
    """A random walk from the origin, 0.05 +- 0.04 per waypoint in x and +- 0.03 in y: segments on both sides of s_max = 0.05 and
    second differences on both sides of a_max = 0.04; a disc the walk starts in; a field over [-2, 2]^2 the long walks leave."""
    g = torch.Generator().manual_seed(seed + 31 * H + rows)
    step = torch.zeros(rows, H, D)
    step[..., 0] = 0.05 + (torch.rand(rows, H, generator=g) - 0.5) * 0.08
    step[..., 1] = (torch.rand(rows, H, generator=g) - 0.5) * 0.06
    traj = step.cumsum(dim=1)
    traj[..., 2:] = torch.rand(rows, H, D - 2, generator=g)
    discs = torch.tensor([[[0.1, 0.0, 0.01, 0.0, 0.4]]]).repeat(Sn, 1, 1)
    cells = torch.rand(Sn, 4, 6, generator=g) - 0.3
    geo = dict(origin=(-2.0, -2.0), cell=(0.8, 4.0 / 3.0))
    limits = torch.tensor([[0.05, 0.04], [0.06, math.inf]])[:Sn].contiguous()
    return traj, discs, cells, geo, limits


@pytest.mark.parametrize("case", COST_CASES, ids=str)
def test_guide_cost_with_limits_against_the_fp64_restatement(case):
    """`active` exact; |cost - fp64 cost| within motion_ref.cost_bound, derived from the contract's lines; the very bits equal the
    fp32 restatement summed by the wave's butterfly; row r reads scene r % S.  The inputs keep every hinge argument further from 0
    than fp32 can move it: the motion terms' by ten times motion_ref.hinge_slack (the bound's own |d phi|, |d psi|), the others'
    by the 1e-5 of the field's tests; checked here, on every case."""
    rows, Sn, H, D = case
    traj, discs, cells, geo, limits = _cost_case(*case)
    f, m = FR.field(cells, weight=WEIGHT, **geo), MR.motion(limits, W_SPEED, W_ACCEL)
    margin, own, slack = FR.hinge_margin(traj, discs, None, f), MR.hinge_margin(traj, None, None, None, m), MR.hinge_slack(traj, f, m)
    edges = FR.margins(traj, f)[1]
    print("hinge margin of disc and field", margin, "of the motion terms", own, "their fp32 slack", slack, "distance to a cell edge", edges)
    assert margin > 1e-5 and edges > 1e-5 and own > 10 * slack
    guide = Guide(discs.to(DEV), None, field=CostField(cells.to(DEV), weight=WEIGHT, **geo), motion=MotionLimits(limits.to(DEV), W_SPEED, W_ACCEL))
    cost, active = guide.cost(traj.to(DEV))
    want, want_active, _ = MR.row_cost(traj, discs, None, f, m, np.float64)
    bound = MR.cost_bound(traj, discs, None, f, m)
    err = np.abs(cost.cpu().numpy().astype(np.float64) - want)
    print("cost", want, "|err|", err, "bound", bound)
    assert cost.dtype == torch.float32 and active.dtype == torch.int32 and cost.shape == active.shape == (rows,)
    assert np.array_equal(active.cpu().numpy(), want_active) and want_active.max() > 0
    assert (err <= bound).all() and (want > 0).all()
    assert np.array_equal(cost.cpu().numpy().view(np.int32), MR.row_cost_wave(traj, discs, None, f, m).view(np.int32))
    without = Guide(discs.to(DEV), None, field=guide.field).cost(traj.to(DEV))
    only = Guide(motion=guide.motion).cost(traj.to(DEV))                                  # the limits' share alone
    assert torch.equal(only[1], active - without[1])
    assert np.array_equal(only[0].cpu().numpy().view(np.int32), MR.row_cost_wave(traj, None, None, None, m).view(np.int32))
    seg, curv = MR.terms(m, traj[:, :, 0].numpy(), traj[:, :, 1].numpy(), np.float64)
    assert int(only[1].sum()) == int(seg["on"].sum() + curv["on"].sum())
    if H >= 5:                                                                            # both sides of both hinges are met
        assert seg["on"].any() and not seg["on"].all() and curv["on"].any() and not curv["on"].all()
    if Sn < rows and Sn > 1:                                                              # row r reads scene r % S
        lone = Guide(motion=MotionLimits(limits[1:].to(DEV), W_SPEED, W_ACCEL)).cost(traj[1::Sn].to(DEV))
        assert _same(lone[0], only[0][1::Sn]) and torch.equal(lone[1], only[1][1::Sn])


# ---- 4. the selection -------------------------------------------------------------------------------------------------------------
def _speed_scene():
    """K = 3, S = 2, H = 8, D = 3, straight rows from the origin; the target lies 0.7 ahead.  Candidate 0 drives 0.1 per waypoint
    and reaches the target, candidate 1 drives 0.02 per waypoint along y (slow, far from the target), candidate 2 drives 0.08 per
    waypoint.  Scene 0 allows 0.05 per waypoint: candidate 1 alone is inside the limits.  Scene 1 allows 0.01: nobody is."""
    K, Sn, H, D = 3, 2, 8, 3
    t = torch.zeros(K, Sn, H, D)
    h = torch.arange(H, dtype=torch.float32)
    t[0, :, :, 0], t[1, :, :, 1], t[2, :, :, 0] = 0.1 * h, 0.02 * h, 0.08 * h
    t[2, :, :, 1] = 0.01 * h
    t[..., 2] = 0.3
    limits = torch.tensor([[0.05, 0.1], [0.01, 0.1]])
    target = torch.tensor([[0.7, 0.0], [0.7, 0.0]])
    return t.reshape(K * Sn, H, D), limits, target


def test_the_guided_selection_sees_the_limits():
    trajs, limits, target = _speed_scene()
    K, Sn = 3, 2
    m = MR.motion(limits)
    guide = Guide(motion=MotionLimits(limits.to(DEV)))
    x = trajs.to(DEV)
    cost, active = guide.cost(x)
    # violation and active: adx_guide_cost_motion of the same rows, bit for bit (cost = 0 + 1 * violation)
    only = TrajectorySelector(0.0, 0.0, 0.0, w_guide=1.0, hard=True)(x, Sn, None, guide)
    assert torch.equal(_bits(only.cost), _bits(cost.view(K, Sn).t().contiguous()))
    assert torch.equal(only.active, active.view(K, Sn).t().contiguous())
    assert only.active.tolist() == [[7, 0, 7], [7, 7, 7]]
    # index and blocked against fp64: cost = 1 * goal + 1 * violation, goal = the least squared distance to the target
    viol, act64, _ = MR.row_cost(trajs, None, None, None, m, np.float64)
    t64 = trajs.numpy().astype(np.float64)
    goal = (((t64[:, :, :2] - np.tile(target.numpy().astype(np.float64), (K, 1))[:, None, :]) ** 2).sum(axis=2)).min(axis=1)
    c64 = (goal + viol).reshape(K, Sn).T                                                 # [S, K]
    # |fp32 - fp64|: the violation's derived bound, five roundings for the goal (two differences, two squares, a sum), two products
    # by the weights and one sum
    bound = (MR.cost_bound(trajs, None, None, None, m) + 8 * MR.U * (goal + viol)).reshape(K, Sn).T
    free = (act64 == 0).reshape(K, Sn).T
    gap = np.sort(c64, axis=1)
    assert ((gap[:, 1] - gap[:, 0]) > 2 * (bound.max(axis=1))).all(), (gap, bound)       # every scene qualifies
    for hard in (True, False):
        sel = TrajectorySelector(1.0, 0.0, 0.0, w_guide=1.0, hard=hard)(x, Sn, target.to(DEV), guide)
        want = [int(np.where(free[s], c64[s], np.inf).argmin()) if hard and free[s].any() else int(c64[s].argmin()) for s in range(Sn)]
        assert sel.index.tolist() == want and sel.blocked.tolist() == [int(not free[s, want[s]]) for s in range(Sn)], (hard, want)
        assert (np.abs(sel.cost.cpu().numpy().astype(np.float64) - c64) <= bound).all()
        assert torch.equal(sel.active, only.active)
        for s in range(Sn):
            assert torch.equal(_bits(sel.best[s]), _bits(x[want[s] * Sn + s]))
    # scene 0 has one candidate inside the limits: `hard` picks it, the plain rule does not
    hard_sel = TrajectorySelector(1.0, 0.0, 0.0, w_guide=1.0, hard=True)(x, Sn, target.to(DEV), guide)
    plain_sel = TrajectorySelector(1.0, 0.0, 0.0, w_guide=1.0, hard=False)(x, Sn, target.to(DEV), guide)
    assert hard_sel.index.tolist()[0] == 1 and hard_sel.blocked.tolist() == [0, 1]
    assert plain_sel.index.tolist()[0] != 1 and plain_sel.blocked.tolist() == [1, 1]
    with pytest.raises(ValueError, match="the guide holds 1 scenes; the selection has 2"):
        TrajectorySelector(hard=True)(x, Sn, None, Guide(motion=MotionLimits(limits[:1].to(DEV))))


# ---- 5. the loop and the graph ----------------------------------------------------------------------------------------------------
def _limit_guide(Sn, s_max=0.05, a_max=0.03, w=(4.0, 2.0), obstacles=False, **kw):
    kw = dict(dict(scale=0.5, schedule="variance", cap=0.1, iters=3), **kw)
    motion = MotionLimits(torch.tensor([[s_max, a_max]] * Sn, device=DEV), *w)
    if not obstacles:
        return Guide(motion=motion, **kw)
    o = TG._obstacles(Sn, 141)
    return Guide(o.discs, o.planes, motion=motion, **kw)


@pytest.mark.parametrize("sampler", ["ddim", "ddpm", "dpm"])
def test_generate_traj_is_the_loop_written_out(sampler):
    """S = 2, H = 8, 5 steps, every noise from one DeviceNoise.  Bit-equal to the loop of public scheduler.step(guide=...) calls;
    without the limits the result is another one; beside discs and planes the same holds."""
    m, cfg, q = TG._setup("FREE_GUIDANCE", sampler)
    img, tgt = TP._frame(2, 40, "FREE_GUIDANCE")
    seed = (6 << 32) | 4
    for obstacles in (False, True):
        guide = _limit_guide(2, obstacles=obstacles)
        got = generate_traj(m, q, cfg, img, tgt, noise=DeviceNoise(seed, DEV), guide=guide, scale_xy=False)
        want = TG._written_out(m, cfg, q, DeviceNoise(seed, DEV), img, tgt, guide)
        assert torch.equal(_bits(got), _bits(want)), (got - want).abs().max().item()
        assert torch.isfinite(got).all() and bool((got[:, 0, :3] == 0).all())
        without = guide.like(guide.discs, guide.planes)
        plain = generate_traj(m, q, cfg, img, tgt, noise=DeviceNoise(seed, DEV), guide=without if obstacles else None, scale_xy=False)
        assert not torch.equal(plain, got)
        print("cost of the plan without and with the limits:", guide.cost(plain)[0].tolist(), guide.cost(got)[0].tolist())


def test_graph_replays_read_the_limits_and_weights_capture_a_second_graph():
    """Three ticks with new limits every tick == the eager ticks bit for bit on one captured graph; other weights capture a second."""
    m, cfg, q = TG._setup("FREE_GUIDANCE", "ddim")
    seed = (2 << 32) | 10
    z, z2 = DeviceNoise(seed, DEV), DeviceNoise(seed, DEV)
    gs = GraphedSampler(m, q, cfg, noise=z, scale_xy=False)
    outs = []
    for k, s_max in enumerate((0.05, 0.0, math.inf)):
        img, tgt = TP._frame(2, 70, "FREE_GUIDANCE")
        guide = _limit_guide(2, s_max=s_max)
        got = gs(img, tgt, guide=guide)
        want = generate_traj(m, q, cfg, img, tgt, noise=z2, guide=guide, scale_xy=False)
        assert torch.equal(_bits(got), _bits(want)), (k, (got - want).abs().max().item())
        assert z.tick() == z2.tick() == k + 1, k
        outs.append(got.clone())
    assert gs.captured == 1 and not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    heavier = _limit_guide(2, w=(8.0, 2.0))
    got = gs(img, tgt, guide=heavier)
    assert gs.captured == 2 and torch.equal(_bits(got), _bits(generate_traj(m, q, cfg, img, tgt, noise=z2, guide=heavier, scale_xy=False)))
    gs(img, tgt, guide=Guide(scale=0.5, schedule="variance", cap=0.1, iters=3))          # no limits: a third graph
    assert gs.captured == 3


def test_a_full_tick_under_a_standstill_limit_moves_less():
    """Best-of-3, a warm start and the controller in one tick, eager: it runs, the selection's `active` is Guide.cost of the
    candidates, and under s_max = 0 ("do not move") the chosen plan's Guide.cost is lower than that of the same tick without
    limits on the same noise."""
    m, cfg, q = TG._setup("FREE_GUIDANCE", "ddim", horizon=16)
    img, tgt = TP._frame(2, 50, "FREE_GUIDANCE", 16)
    vel = torch.tensor([1.5, 0.25], device=DEV)
    stop = _limit_guide(2, s_max=0.0, a_max=math.inf, w=(4.0, 0.0))
    sel = TrajectorySelector(1.0, 0.0, 0.0, w_guide=1.0, hard=True)
    results = {}
    for name, guide in (("limits", stop), ("none", Guide(scale=0.5, schedule="variance", cap=0.1, iters=3))):
        z, w, ctl = DeviceNoise(77, DEV), WarmStart(3), DeviceController(cfg, 2, DEV)
        for k in range(2):                                                                # a cold tick, then a warm one
            out = generate_traj(m, q, cfg, img, tgt, noise=z, warm=w, controller=ctl, velocity=vel, guide=guide, candidates=3,
                                selector=sel, return_selection=True, scale_xy=False)
            best, s, control = out
            assert torch.isfinite(best).all() and control.shape == (2, 3) and w.valid
            rows = s.candidates.reshape(6, 16, -1)
            assert torch.equal(s.active, guide.cost(rows)[1].view(3, 2).t().contiguous())
        results[name] = best
    with_limits, without = stop.cost(results["limits"])[0], stop.cost(results["none"])[0]
    print("standstill cost with and without the limits in the tick:", with_limits.tolist(), without.tolist())
    assert bool((with_limits < without).all())


def test_refusals_come_before_any_launch_tick_or_capture():
    m, cfg, q = TG._setup("FREE_GUIDANCE", "ddim")
    img, tgt = TP._frame(2, 95, "FREE_GUIDANCE")
    z = DeviceNoise(1, DEV)
    gs = GraphedSampler(m, q, cfg, noise=z, scale_xy=False)
    three = _limit_guide(3)
    on_cpu = Guide(motion=MotionLimits(torch.zeros(2, 2)))
    for bad in (three, on_cpu):
        with pytest.raises(ValueError, match="guide.motion.limits must hold 2 scenes"):
            gs(img, tgt, guide=bad)
        with pytest.raises(ValueError, match="guide.motion.limits must hold 2 scenes"):
            generate_traj(m, q, cfg, img, tgt, noise=z, guide=bad)
    assert gs.captured == 0 and z.tick() == 0
    # a bare step refuses limits of another batch, and the C ABI's refusals surface as ValueError
    x = torch.zeros(2, 8, 7, device=DEV)
    with pytest.raises(ValueError, match="rows a multiple"):
        q.step(x, 60, x, guide=three)
    guide = _limit_guide(2)
    (g, _, mo), active = guide.descs(x)[2], torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="an output overlaps the motion limits"):        # cost written over the limits
        L.check(L.lazy("adx_guide_cost_motion")(x.data_ptr(), C.byref(g), None, C.byref(mo), guide.motion.limits.data_ptr(), active.data_ptr(),
                                                2, 8, 7, L.stream_ptr(x.device)), "adx_guide_cost_motion")
    with pytest.raises(ValueError, match="horizon 65, supported 1..64"):
        q.step(torch.zeros(2, 65, 7, device=DEV), 60, torch.zeros(2, 65, 7, device=DEV), guide=guide)
