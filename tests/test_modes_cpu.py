"""CPU: "trajectory modes v1" without a device -- the fp64 restatement (tests/modes_ref.py) on hand-built scenes with known answers
and on the generated fixtures' invariants; every refusal of `adx_traj_modes` (its checks run on the host before any GPU work, so
placeholder addresses that are never dereferenced are enough) and of `TrajectoryModes`; and what `plan_tick` makes of `modes`."""
import ctypes as C

import numpy as np
import pytest
import torch

import modes_ref as R
import test_tick_plan_cpu as TT
from autonomous_driving_with_diffusion_model_amd import _lib as L
from autonomous_driving_with_diffusion_model_amd import ModeSet, TrajectoryModes
from autonomous_driving_with_diffusion_model_amd.control import modes as MD
from autonomous_driving_with_diffusion_model_amd.control.fallback import StopShort
from autonomous_driving_with_diffusion_model_amd.guide import Guide
from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler, TickPlan, plan_tick


# ---- the restatement on scenes with known answers -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case,want", R.hand_cases(), ids=[c[0] for c in R.hand_cases()])
def test_hand_built_scenes(name, case, want):
    t, M = case["trajs"], case["M"]
    got = R.modes(t[:, None], 1, M, case["radius"], case["h0"])
    assert got["index"][0].tolist() == want["index"] and got["mass"][0].tolist() == want["mass"], name
    assert got["assign"][0].tolist() == want["assign"] and int(got["count"][0]) == want["count"], name
    rows = R.expected_rows(t, want["index"], want["count"], M)
    assert np.array_equal(R.bits(got["modes"]), R.bits(rows))                         # NaN payloads included
    if want["count"] == 0:
        assert not R.bits(got["modes"]).any()
    else:
        for m in range(want["count"], M):
            assert np.array_equal(R.bits(got["modes"][m]), R.bits(t[want["index"][0]]))


def test_the_hand_built_scenes_are_decided_far_from_rounding():
    """Every pair of every hand-built scene is either an exact duplicate under radius 0 or clears r2 by far more than the bound."""
    for name, case, _ in R.hand_cases():
        if case["radius"] == 0.0:
            d, finite = R.dist2(case["trajs"][:, None], 1, case["h0"])
            off = d[0][np.triu_indices(len(case["trajs"]), 1)]
            assert ((off == 0.0) | (off > 0.1)).all(), name
        else:
            assert R.margins(case["trajs"][:, None], 1, case["radius"], case["h0"])[0] > 100.0 * R.bound(4, 1), name


def test_bound_and_radius():
    assert 3.5e-5 < R.bound(64, 0) < 3.7e-5 and R.bound(1, 0) < R.bound(2, 0) < R.bound(64, 1) < R.bound(64, 0)
    assert R.r2_of(0.1) == float(np.float32(0.1) * np.float32(0.1)) and R.r2_of(0.0) == 0.0


# ---- invariants on the generated fixtures -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixtures():
    return R.cases()


def test_generated_cases_are_decided_and_keep_the_invariants(fixtures):
    shapes = {(c["S"], c["K"], c["H"], c["h0"], c["D"]) for c in fixtures}
    assert len(shapes) == len(fixtures) == len(R.SCENES) * len(R.CANDIDATES) * len(R.HORIZONS) * len(R.DIMS)
    for K in R.CANDIDATES:
        assert {c["M"] for c in fixtures if c["K"] == K} == {1, 6, K}                   # every M meets every K
    for c in fixtures:
        S, K, M = c["S"], c["K"], c["M"]
        assert np.abs(c["trajs"]).max() <= 1.0 and c["trajs"].dtype == np.float32
        assert (R.margins(c["trajs"], S, c["radius"], c["h0"]) > 4.0 * c["bound"]).all()
        d, _ = R.dist2(c["trajs"], S, c["h0"])
        assert not np.isin(R.r2_of(c["radius"]), d)                                     # never on a data value
        got = R.modes(c["trajs"], S, M, c["radius"], c["h0"])
        rows = got["modes"].reshape(M, S, c["H"], c["D"])
        cands = c["trajs"].reshape(K, S, c["H"], c["D"])
        for s in range(S):
            mass, index, assign, count = got["mass"][s], got["index"][s], got["assign"][s], int(got["count"][s])
            assert 1 <= count <= min(M, K) and (np.diff(mass) <= 0).all()               # non-increasing
            assert mass.sum() + (assign == R.OUTLIER).sum() + (assign == R.NON_FINITE).sum() == K
            assert (mass[:count] > 0).all() and (mass[count:] == 0).all() and (index[count:] == -1).all()
            assert [int((assign == m).sum()) for m in range(M)] == mass.tolist()
            assert (assign[index[:count]] == np.arange(count)).all()                    # a representative belongs to its own mode
            for m in range(M):
                assert np.array_equal(R.bits(rows[m, s]), R.bits(cands[index[m] if m < count else index[0], s]))
    big = [c for c in fixtures if c["K"] >= 33 and c["M"] == 6]
    assert big and all((R.modes(c["trajs"], c["S"], 6, c["radius"], c["h0"])["mass"][:, 1] > 0).all() for c in big)   # real covers


# ---- refusals of adx_traj_modes, by their complete text -----------------------------------------------------------------------------
S, K, H, D, M = 3, 8, 16, 7, 6
ROW = H * D * 4
TRAJS, MODES, INDEX, MASS, ASSIGN, COUNT, DIST2 = (0x10000000 * (i + 1) for i in range(7))
GOOD = dict(scenes=S, candidates=K, horizon=H, dim=D, max_modes=M, h0=1, radius=0.1, trajs=TRAJS, modes=MODES, index=INDEX, mass=MASS,
            assign=ASSIGN, count=COUNT, dist2=DIST2)
REFUSALS = [
    (dict(cfg=None), "traj modes: null configuration"),
    (dict(candidates=0), "traj modes: 0 candidates, supported 1..64"),
    (dict(candidates=65), "traj modes: 65 candidates, supported 1..64"),
    (dict(max_modes=0), "traj modes: max_modes 0, supported 1..64"),
    (dict(max_modes=65), "traj modes: max_modes 65, supported 1..64"),
    (dict(horizon=0, h0=0), "traj modes: horizon 0, supported 1..64"),
    (dict(horizon=65), "traj modes: horizon 65, supported 1..64"),
    (dict(dim=0), "traj modes: transition dim 0, supported 1..16"),
    (dict(dim=17), "traj modes: transition dim 17, supported 1..16"),
    (dict(scenes=0), "traj modes: 0 scenes, supported 1..65535"),
    (dict(scenes=65536), "traj modes: 65536 scenes, supported 1..65535"),
    (dict(h0=-1), "traj modes: h0 -1, supported 0..15 (horizon - 1)"),
    (dict(h0=16), "traj modes: h0 16, supported 0..15 (horizon - 1)"),
    (dict(radius=-0.5), "traj modes: radius -0.5 must be finite and >= 0"),
    (dict(radius=float("inf")), "traj modes: radius inf must be finite and >= 0"),
    (dict(radius=float("nan")), "traj modes: radius nan must be finite and >= 0"),
    (dict(trajs=None), "traj modes: null trajs"),
    (dict(modes=None), "traj modes: null modes"),
    (dict(index=None), "traj modes: null index"),
    (dict(mass=None), "traj modes: null mass"),
    (dict(assign=None), "traj modes: null assign"),
    (dict(count=None), "traj modes: null count"),
    (dict(modes=TRAJS + K * S * ROW - 4), "traj modes: modes aliases trajs"),
    (dict(index=TRAJS), "traj modes: index aliases trajs"),
    (dict(mass=TRAJS + 8), "traj modes: mass aliases trajs"),
    (dict(assign=TRAJS - S * K * 4 + 4), "traj modes: assign aliases trajs"),
    (dict(count=TRAJS + ROW), "traj modes: count aliases trajs"),
    (dict(dist2=TRAJS + 4), "traj modes: dist2 aliases trajs"),
    (dict(index=MODES + M * S * ROW - 4), "traj modes: modes and index alias each other"),
    (dict(mass=INDEX + S * M * 4 - 4), "traj modes: index and mass alias each other"),
    (dict(assign=MASS), "traj modes: mass and assign alias each other"),
    (dict(count=ASSIGN + 4), "traj modes: assign and count alias each other"),
    (dict(dist2=COUNT - S * K * K * 4 + 4), "traj modes: count and dist2 alias each other"),
    (dict(dist2=MODES), "traj modes: modes and dist2 alias each other"),
]


def _call(**over):
    a = dict(GOOD, **over)
    cfg = L.ModesCfg(a["scenes"], a["candidates"], a["horizon"], a["dim"], a["max_modes"], a["h0"], a["radius"])
    ref = None if "cfg" in over else C.byref(cfg)
    rc = L.lazy("adx_traj_modes")(ref, a["trajs"], a["modes"], a["index"], a["mass"], a["assign"], a["count"], a["dist2"], None)
    return rc, L.lib().adx_last_error().decode()


@pytest.mark.parametrize("over,text", REFUSALS, ids=[r[1][12:] + " / " + ",".join(r[0]) for r in REFUSALS])
def test_adx_traj_modes_refuses_before_any_gpu_work(over, text):
    assert _call(**over) == (-1, text)


def test_the_limits_of_the_contract_are_the_python_side_s():
    assert (MD.MAX_CANDIDATES, MD.MAX_MODES, MD.MAX_HORIZON, MD.OUTLIER, MD.NON_FINITE) == (64, 64, 64, R.OUTLIER, R.NON_FINITE)
    assert "adx_traj_modes" in L.EXPORTED_SYMBOLS and C.sizeof(L.ModesCfg) == 28


# ---- refusals of TrajectoryModes ----------------------------------------------------------------------------------------------------
def test_trajectory_modes_refuses_what_it_cannot_run():
    tm = TrajectoryModes()
    assert (tm.max_modes, tm.radius, tm.h0, tm.last) == (6, 2.0 / 23.315, 1, None)
    assert tm.key() == ("modes_v1", 6, 2.0 / 23.315, 1) and repr(tm) == f"TrajectoryModes(max_modes=6, radius={2.0 / 23.315}, h0=1)"
    for bad in (0, 65, -1):
        with pytest.raises(ValueError, match=f"max_modes must be 1..64, got {bad}"):
            TrajectoryModes(bad)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="radius must be finite and >= 0"):
            TrajectoryModes(radius=bad)
    for bad in (-1, 64):
        with pytest.raises(ValueError, match=f"h0 must be 0..63, got {bad}"):
            TrajectoryModes(h0=bad)
    with pytest.raises(TypeError, match="trajs must be a tensor, got list"):
        tm([[0.0]], 1)
    with pytest.raises(ValueError, match=r"trajs \(4, 2, 8, 7\) is not \[K, 3, H, D\]"):
        tm(torch.zeros(4, 2, 8, 7), 3)
    for shape, scenes in (((7, 8, 7), 2), ((8, 7), 2), ((0, 8, 7), 2), ((4, 8, 7), 0)):
        with pytest.raises(ValueError, match=r"trajs must be \[K \* -?\d+, H, D\]"):
            tm(torch.zeros(shape), scenes)
    with pytest.raises(ValueError, match="65 candidates per scene, supported 1..64"):
        tm(torch.zeros(130, 8, 7), 2)
    with pytest.raises(ValueError, match="horizon 65, supported 1..64"):
        tm(torch.zeros(4, 65, 7), 2)
    with pytest.raises(ValueError, match="h0 = 8 leaves no waypoint of a horizon of 8 to score"):
        TrajectoryModes(h0=8)(torch.zeros(4, 8, 7), 2)
    with pytest.raises(L.AdxError, match="trajs lives on cpu; the adx kernels only run on an MI355X"):      # no CPU path
        tm(torch.zeros(4, 8, 7), 2)


def test_mode_set_prob_is_mass_over_the_finite_candidates():
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    ms = ModeSet(torch.zeros(3, 2, 4, 2), i32([[0, 1, 4], [-1, -1, -1]]), i32([[4, 2, 1], [0, 0, 0]]),
                 i32([[0, 1, -2, 0, 2, 1, 0, -2, 0, -1], [-2] * 10]), i32([3, 0]))
    assert ms.dist2 is None
    p = ms.prob()
    assert p.dtype == torch.float32 and p.tolist() == [[0.5, 0.25, 0.125], [0.0, 0.0, 0.0]]


# ---- plan_tick --------------------------------------------------------------------------------------------------------------------
class _Scheduler(TT._Scheduler):
    supports_guide = True


def _plan(cfg=None, **kw):
    return plan_tick(TT.MODEL, _Scheduler(), cfg or TT._cfg(), TT.IMG, None, None, noise=TT._Noise([]), **kw)


def _old_key(p):
    """TickPlan.key() as it was before the plan had modes."""
    sel, ctl, pin, guide = p.selector, p.controller, p.pin, p.guide
    weights = None if sel is None else (sel.w_goal, sel.w_smooth, sel.w_consensus)
    if sel is not None and sel.uses_guide:
        weights += (sel.w_guide, sel.hard)
    key = (p.S, p.K, weights, p.rows, p.H, p.D, p.n, p.use, p.free_scale, p.fuse, p.hoisted, p.is_ddpm,
           "init" if p.start == "randn" else p.start, p.m_warm, p.shift, p.is_warm, p.motion is None,
           None if ctl is None else (id(ctl), ctl.state.data_ptr(), ctl.key(), p.velocity is None),
           None if pin is None else (pin.mode, tuple(pin.known.shape)), None if guide is None else guide.key())
    return key if p.fallback is None else key + (p.fallback.key(),)


def test_the_plan_with_and_without_modes():
    assert TickPlan.__dataclass_fields__["modes"].default is None
    tm = TrajectoryModes()
    guide = Guide(planes=torch.tensor([[[1.0, 0.0, 0.5]]] * TT.S))
    fb = StopShort(torch.zeros(TT.S, 2))
    for kw in (dict(candidates=3), dict(candidates=3, guide=guide), dict(candidates=3, guide=guide, fallback=fb),
               dict(candidates=2, pin=TT._pin()), dict(), dict(guide=guide, fallback=fb)):
        plain = _plan(**kw)
        assert plain.modes is None and plain.key() == _old_key(plain), kw             # the keys they have
        if "candidates" in kw:
            with_tm = _plan(modes=tm, **kw)
            assert with_tm.modes is tm and with_tm.key() == plain.key() + (tm.key(),) and with_tm.key() != plain.key()
            assert with_tm.key()[-1] == ("modes_v1", 6, 2.0 / 23.315, 1)
    base = _plan(candidates=3, modes=tm).key()
    others = [_plan(candidates=3, modes=TrajectoryModes(*a)).key() for a in ((5, tm.radius, 1), (6, 0.1, 1), (6, tm.radius, 0))]
    assert len({base, *others}) == 4                                                    # distinct per (M, radius, h0)
    assert _plan(candidates=3, modes=TrajectoryModes()).key() == base                  # and equal for equal settings


def test_plan_tick_refuses_modes_it_cannot_run():
    tm = TrajectoryModes()
    with pytest.raises(ValueError, match="`modes` clusters a scene's candidates and needs candidates > 1"):
        _plan(modes=tm)
    with pytest.raises(ValueError, match="needs candidates > 1"):
        _plan(modes=tm, candidates=1)
    with pytest.raises(TypeError, match="`modes` must be a TrajectoryModes, got int"):
        _plan(modes=6, candidates=3)
    with pytest.raises(ValueError, match="modes.h0 = 8 leaves no waypoint of MODEL.HORIZON = 8 to score"):
        _plan(modes=TrajectoryModes(h0=8), candidates=3)
    long = TT._cfg()
    long.MODEL.HORIZON = 128
    with pytest.raises(ValueError, match="need MODEL.HORIZON <= 64, got 128"):
        _plan(cfg=long, modes=tm, candidates=3)
    cfg = TT._cfg()
    cfg.EVAL.CANDIDATES = 4                                                             # the config's K counts
    assert _plan(cfg=cfg, modes=tm).modes is tm
    gs = GraphedSampler(TT.MODEL, _Scheduler(), TT._cfg(), noise=TT._Noise([]), candidates=3, modes=tm)
    assert gs.modes is tm and gs.last_modes is None


# ---- the tools ----------------------------------------------------------------------------------------------------------------------
def test_the_eval_tool_parses_modes_and_the_probe_imports():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import modes_probe  # noqa: F401  (its module level needs no device)
    import open_loop_eval as T
    assert T.parse_modes(None, 2.0) is None and T.parse_modes("6", 2.0) == (6, 2.0) and T.parse_modes("3:1.5", 2.0) == (3, 1.5)
    for bad in ("six", "6:", "6:2:1", ""):
        with pytest.raises(SystemExit, match=r"expected M\[:radius_m\]"):
            T.parse_modes(bad, 2.0)
