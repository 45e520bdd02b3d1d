"""GPU: the device-side controller -- the kernel (adx_control_step) against the fp64 restatement of "control v1"
(tests/control_ref.py) on the 80 ticks of the parity run, which the CPU test vets (tests/test_control_device_cpu.py: every
decision of these inputs stands clear of rounding); batch independence, repeatability, reset, NaN, the action source;
generate_traj(controller=...) against DeviceController.step on the returned trajectory; GraphedSampler(controller=...) replays
against the eager ticks.  No fault is provoked, no assembly is inspected and no timing is asserted anywhere
(tools/control_tick_probe.py measures)."""
import numpy as np
import pytest
import torch

import control_ref as R
from autonomous_driving_with_diffusion_model_amd import DeviceController, DeviceNoise, TrajectorySelector
from autonomous_driving_with_diffusion_model_amd import scheduler as S
from autonomous_driving_with_diffusion_model_amd.config import create_cfg
from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler, generate_traj
from autonomous_driving_with_diffusion_model_amd.utils import procedural as P
from helpers import IMG_SMALL, SCHED_KW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _cfg(n_turn=40, n_speed=40):
    cfg = create_cfg()
    cfg.PID.TURN_N, cfg.PID.SPEED_N = n_turn, n_speed
    return cfg


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rows(S_, H, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((S_, H, D), generator=g) * 2 - 1).to(DEV), (torch.rand((S_,), generator=g) * 2).to(DEV)


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
_REF = {}


def _reference(W, windows, with_target, post):
    """The restatement's run of a case, computed once and shared: (case, per scene (controls, infos, final state, bound))."""
    key = (W, windows, with_target, post)
    if key not in _REF:
        case = R.scene_case(P, _cfg(*windows), W, with_target, post)
        runs = []
        for s in range(case.S):
            out, infos, state = R.run(case.p, case.traj[:, s], case.speed[:, s], None if case.target is None else case.target[:, s])
            runs.append((out, infos, state, R.run_bound(case.p, infos, case.speed[:, s], with_target)))
        _REF[key] = (case, runs)
    return _REF[key]


WORST = {}


@pytest.mark.parametrize("post", ["agent", "interact"])
@pytest.mark.parametrize("windows", [(40, 40), (1, 3)])
@pytest.mark.parametrize("W,with_target", [(4, True), (16, True), (4, False)])
def test_kernel_against_the_restatement_over_80_ticks(W, with_target, windows, post):
    """H = 16, D = 2, S = 3 scenes that see the parity run at tick offsets 0, 7 and 23, 80 launches on one state.  Steer and throttle
    within `bound` on every tick of every scene; brake equal on every tick, and with it -- the margins are vetted on the CPU --
    the aim index and to_target, which show in the steer.  The final windows equal the restatement's within the bound of one
    sample.  (W = 16 = H without a target is a refusal, not a case: nothing stands in for the target.)"""
    case, runs = _reference(W, windows, with_target, post)
    ctl = DeviceController(_cfg(*windows), case.S, DEV, waypoints=W, post=post)
    traj, speed, target = _dev(case.traj), _dev(case.speed), _dev(case.target)
    got = torch.stack([ctl.step(traj[k], speed[k], None if target is None else target[k], xy_scale=R.MAGIC) for k in range(R.TICKS)])
    got = got.cpu().numpy().astype(np.float64)
    turn, spd = (w.numpy().astype(np.float64) for w in ctl.windows())
    worst = 0.0
    for s, (want, infos, state, b) in enumerate(runs):
        assert np.array_equal(got[:, s, 2], want[:, 2]), (s, np.nonzero(got[:, s, 2] != want[:, 2])[0])
        e_th, e_st = np.abs(got[:, s, 0] - want[:, 0]), np.abs(got[:, s, 1] - want[:, 1])
        worst = max(worst, e_th.max() / b.throttle, e_st.max() / b.steer)
        assert (e_st <= b.steer).all(), (s, int(e_st.argmax()), e_st.max(), b.steer)
        assert (e_th <= b.throttle).all(), (s, int(e_th.argmax()), e_th.max(), b.throttle)
        assert turn.shape == (case.S, windows[0]) and spd.shape == (case.S, windows[1])
        assert (np.abs(turn[s] - state.turn) <= b.e_a).all() and (np.abs(spd[s] - state.speed) <= b.e_delta).all(), s
    WORST[(W, with_target, windows, post)] = worst
    print(f"W = {W}, target {with_target}, windows {windows}, post {post}: largest |error| / bound = {worst:.4f} "
          f"(so far over all cases: {max(WORST.values()):.4f})")
    braking = got[..., 2] == 1.0
    assert braking.any() and not braking.all() and (got[..., 0][braking] == 0).all()
    if post == "interact":
        assert (got[..., 1][braking] == 0).all()


def test_a_scene_does_not_depend_on_its_launch_and_a_launch_repeats():
    """The same scene alone (S = 1) and as row 64 of S = 65 -- the last workgroup then holds one scene, not four --: bit-equal
    controls and windows over six ticks.  Two launches from a restored state: bit-equal controls and state."""
    cfg = _cfg()
    one, many = DeviceController(cfg, 1, DEV), DeviceController(cfg, 65, DEV)
    for k in range(6):
        traj, speed = _rows(65, 16, 2, 100 + k)
        tgt = _rows(65, 1, 2, 200 + k)[0][:, 0] * 8
        a = one.step(traj[64:], speed[64:], tgt[64:], xy_scale=R.MAGIC)
        snap = many.state_snapshot()
        b = many.step(traj, speed, tgt, xy_scale=R.MAGIC)
        after = many.state_snapshot()
        assert torch.equal(_bits(a[0]), _bits(b[64])), k
        many.state_restore(snap)
        again = many.step(traj, speed, tgt, xy_scale=R.MAGIC)
        assert torch.equal(_bits(again), _bits(b)) and torch.equal(many.state, after), k
        assert torch.isfinite(b).all()
    for w1, w65 in zip(one.windows(), many.windows()):
        assert torch.equal(_bits(w1[0]), _bits(w65[64]))
    assert bool((one.windows()[0][0, -6:] != 0).all()) and not one.windows()[0][0, :-6].any()
    assert not torch.equal(many.windows()[0][0], many.windows()[0][1])


def test_reset_clears_the_masked_scenes_only():
    cfg = _cfg(3, 5)
    ctl, fresh = DeviceController(cfg, 5, DEV), DeviceController(cfg, 5, DEV)
    for k in range(4):                                               # both rings have wrapped or are about to
        traj, speed = _rows(5, 8, 2, 300 + k)
        ctl.step(traj, speed, xy_scale=R.MAGIC)
    before = [w.clone() for w in ctl.windows()]
    mask = torch.tensor([True, False, True, False, False], device=DEV)
    ctl.reset(mask)
    for w, b in zip(ctl.windows(), before):
        assert not w[mask.cpu()].any() and torch.equal(_bits(w[~mask.cpu()]), _bits(b[~mask.cpu()])) and b[mask.cpu()].any()
    traj, speed = _rows(5, 8, 2, 310)
    got, new = ctl.step(traj, speed, xy_scale=R.MAGIC), fresh.step(traj, speed, xy_scale=R.MAGIC)
    assert torch.equal(_bits(got[mask]), _bits(new[mask])) and not torch.equal(got[~mask], new[~mask])
    ctl.reset()
    assert not ctl.state.any()
    with pytest.raises(ValueError, match="mask"):
        ctl.reset(mask[:4])


def test_a_nan_waypoint_follows_the_contract_and_stays_in_its_scene():
    """x of waypoint 1 of scene 1 is NaN at W = 4: segments 0 and 1 have NaN lengths and keys, so desired is NaN (no brake: both
    comparisons are false; the throttle is NaN) and the aim point comes from segment 2; the steer is finite.  The other scenes'
    bits are those of the launch without the NaN."""
    case, _ = _reference(4, (40, 40), True, "none")
    cfg = _cfg()
    clean, dirty = DeviceController(cfg, case.S, DEV, post="none"), DeviceController(cfg, case.S, DEV, post="none")
    traj, speed, target = _dev(case.traj[5]), _dev(case.speed[5]), _dev(case.target[5])
    bad = traj.clone()
    bad[1, 1, 0] = float("nan")
    want, got = clean.step(traj, speed, target, xy_scale=R.MAGIC), dirty.step(bad, speed, target, xy_scale=R.MAGIC)
    assert torch.equal(_bits(got[[0, 2]]), _bits(want[[0, 2]]))
    for w, d in zip(clean.windows(), dirty.windows()):
        assert torch.equal(_bits(w[[0, 2]]), _bits(d[[0, 2]]))
    state = R.fresh(case.p)
    p = R.params(cfg, waypoints=4, post="none", sign_x=-1.0, xy_scale=R.MAGIC)
    ref, info = R.tick(p, state, bad[1].cpu().numpy(), float(case.speed[5, 1]), case.target[5, 1])
    g = got[1].cpu().numpy()
    assert info.idx == 2 and np.isnan(ref[0]) and ref[2] == 0.0
    assert np.isnan(g[0]) and g[2] == 0.0 and abs(g[1] - ref[1]) <= R.run_bound(p, [info], case.speed[5, 1:2]).steer
    turn, spd = dirty.windows()
    assert torch.isnan(spd[1, -1]) and torch.isfinite(turn[1]).all()


@pytest.mark.parametrize("post", ["none", "agent", "interact"])
def test_the_action_source_is_the_post_processed_first_waypoint(post):
    """D = 7, S = 6: (throttle, steer, brake) = post(traj[:, 0, -3:]) bit for bit; rows on both sides of each rule of the post
    step.  No PID state is touched, and no velocity is needed."""
    traj = _rows(6, 8, 7, 400)[0]
    traj[:, 0, 4:] = torch.tensor([[0.6, 0.1, 0.04], [0.2, 0.1, 0.3], [0.4, -0.2, 0.3], [0.1, 0.5, 0.9], [-0.3, 0.7, 0.2],
                                   [0.0, -1.0, 1.0]], device=DEV)
    ctl = DeviceController(_cfg(), 6, DEV, post=post, source="action")
    got = ctl.step(traj, None)
    raw = traj[:, 0, 4:].cpu().numpy()
    want = np.array([R.post_process(post, *(float(v) for v in row)) for row in raw], dtype=np.float32)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert not ctl.state.any()
    assert torch.equal(_bits(ctl.step(traj, _rows(6, 8, 7, 401)[1])), _bits(got))          # a velocity is not read


# ---- the loop -----------------------------------------------------------------------------------------------------------------
N_STEPS = 4


_MODELS = {}


def _setup(D, sampler, use_cond="FREE_GUIDANCE"):
    """The small model at transition dim D (built once per (D, use_cond) and shared: the tests only run it) and a new scheduler."""
    from autonomous_driving_with_diffusion_model_amd.modeling import build_model
    cfg = create_cfg()
    cfg.MODEL.HORIZON, cfg.MODEL.TRANSITION_DIM = 16, D
    cfg.TRAIN.USE_COND = cfg.GUIDANCE.USE_COND = use_cond
    cfg.EVAL.SAMPLE_STEPS, cfg.GUIDANCE.FREE_SCALE = N_STEPS, 7.5
    if (D, use_cond) not in _MODELS:
        m = build_model(cfg)
        P.load_procedural(m, 0)
        _MODELS[(D, use_cond)] = m.to(DEV).eval()
    m = _MODELS[(D, use_cond)]
    sch = {"ddim": lambda: S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW),
           "dpm": lambda: S.GuidanceDPMSolverMultistepScheduler(cfg=cfg, thresholding=True, lambda_min_clipped=-5.1, **SCHED_KW)}[sampler]()
    return m, cfg, sch


def _frame(B, D, seed):
    d = {k: v.to(DEV) for k, v in P.synthetic_batch(B, 16, D, image_hw=IMG_SMALL, seed=seed).items()}
    g = torch.Generator().manual_seed(seed)
    return d, (torch.rand((B,), generator=g) * 3).to(DEV)


@pytest.mark.parametrize("D,sampler,source,use_cond", [(2, "ddim", "pid", "FREE_GUIDANCE"), (2, "dpm", "pid", "NO_GUIDANCE"),
                                                       (7, "ddim", "action", "NO_GUIDANCE"), (7, "dpm", "action", "FREE_GUIDANCE")])
def test_generate_traj_hands_its_unscaled_result_to_the_controller(D, sampler, source, use_cond):
    """S = 2, IMG_SMALL, H = 16, 4 steps.  The trajectory is bit-equal to the call without a controller; the control is bit-equal
    to DeviceController.step on that result in the model's units (scale_xy=False returns it as the controller saw it), with
    xy_scale = magic_num and the scenes' targets -- and, without a target, with waypoint 4 standing in."""
    m, cfg, sch = _setup(D, sampler, use_cond)
    d, vel = _frame(2, D, 50)
    tgt = d["target"] if use_cond == "FREE_GUIDANCE" else None
    plain = generate_traj(m, sch, cfg, d["imgs"], tgt, d["init_trajs"])
    ctl, twin = (DeviceController(cfg, 2, DEV, source=source) for _ in range(2))
    traj, control = generate_traj(m, sch, cfg, d["imgs"], tgt, d["init_trajs"], controller=ctl, velocity=vel)
    assert torch.equal(_bits(traj), _bits(plain)) and control.shape == (2, 3)
    raw = generate_traj(m, sch, cfg, d["imgs"], tgt, d["init_trajs"], scale_xy=False)
    want = twin.step(raw, vel, tgt, xy_scale=m.magic_num)
    assert torch.equal(_bits(control), _bits(want)) and torch.equal(ctl.state, twin.state)
    assert torch.isfinite(control).all() and bool(((raw.abs() <= 1).all()))
    assert bool(ctl.state.any()) == (source == "pid")
    t3 = generate_traj(m, sch, cfg, d["imgs"], tgt, d["init_trajs"], controller=ctl, velocity=vel, return_selection=True)
    assert len(t3) == 3 and t3[1] is None and torch.equal(_bits(t3[0]), _bits(plain))


@pytest.mark.parametrize("D,source", [(2, "pid"), (7, "action")])
def test_best_of_k_controls_the_winners(D, source):
    m, cfg, sch = _setup(D, "ddim")
    d, vel = _frame(2, D, 60)
    sel = TrajectorySelector(1.0, 0.5, 0.25)
    ctl, twin = (DeviceController(cfg, 2, DEV, source=source) for _ in range(2))
    kw = dict(noise=None, candidates=4, selector=sel)
    init = _rows(8, 16, D, 61)[0]
    best, s, control = generate_traj(m, sch, cfg, d["imgs"], d["target"], init, controller=ctl, velocity=vel, return_selection=True,
                                     scale_xy=False, **kw)
    assert torch.equal(_bits(best), _bits(s.best))
    want = twin.step(best, vel, d["target"], xy_scale=m.magic_num)
    assert torch.equal(_bits(control), _bits(want))
    loser = s.candidates[(s.index[0].item() + 1) % 4, 0]
    assert not torch.equal(loser, best[0])
    b2, c2 = generate_traj(m, sch, cfg, d["imgs"], d["target"], init, controller=DeviceController(cfg, 2, DEV, source=source),
                           velocity=vel, **kw)
    scaled = best.clone()
    scaled[..., :2] *= m.magic_num
    assert torch.equal(_bits(c2), _bits(control)) and torch.equal(_bits(b2), _bits(scaled))


@pytest.mark.parametrize("D,sampler,source,use_cond", [(2, "ddim", "pid", "NO_GUIDANCE"), (7, "dpm", "action", "FREE_GUIDANCE")])
def test_graph_replays_carry_the_windows_like_eager_ticks(D, sampler, source, use_cond):
    """Five replays with a new image and a new velocity each == five eager ticks from a fresh controller: controls, trajectories
    and the final windows bit for bit.  The capture's warm-up pass is a real tick; had it left its sample in the windows, the first
    replay's control (I and D terms) and the final windows would differ.  A second capture key -- the same sampler called without
    a target, which the unguided model does not read and the controller replaces by waypoint 4 -- leaves the state as it was, and
    the first key then replays on it."""
    m, cfg, sch = _setup(D, sampler, use_cond)
    cg, ce = DeviceController(cfg, 2, DEV, source=source), DeviceController(cfg, 2, DEV, source=source)
    gs = GraphedSampler(m, sch, cfg, controller=cg)
    assert gs.last_control is None
    frames = [_frame(2, D, 70 + k) for k in range(6)]
    init = frames[0][0]["init_trajs"]
    for k in range(5):
        d, vel = frames[k]
        got = gs(d["imgs"], d["target"], init, velocity=vel)
        want, control = generate_traj(m, sch, cfg, d["imgs"], d["target"], init, controller=ce, velocity=vel)
        assert torch.equal(_bits(got), _bits(want)), k
        assert torch.equal(_bits(gs.last_control), _bits(control)), (k, gs.last_control, control)
        assert torch.equal(cg.state, ce.state), k
    assert gs.captured == 1
    for a, b in zip(cg.windows(), ce.windows()):
        assert torch.equal(_bits(a), _bits(b))
    if source == "pid":
        assert bool((cg.windows()[0][:, -5:] != 0).all()) and not cg.windows()[0][:, :-5].any()    # five samples, not six
        d, vel = frames[5]
        got = gs(d["imgs"], None, init, velocity=vel)                                         # another key: capture, then replay
        want, control = generate_traj(m, sch, cfg, d["imgs"], None, init, controller=ce, velocity=vel)
        assert gs.captured == 2
        assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(gs.last_control), _bits(control))
        assert torch.equal(cg.state, ce.state)
        d, vel = frames[0]
        gs(d["imgs"], d["target"], init, velocity=vel)
        _, control = generate_traj(m, sch, cfg, d["imgs"], d["target"], init, controller=ce, velocity=vel)
        assert gs.captured == 2 and torch.equal(_bits(gs.last_control), _bits(control))
        assert torch.equal(cg.state, ce.state)
    else:
        assert not cg.state.any()


def test_refusals_come_before_any_launch():
    m, cfg, sch = _setup(2, "ddim")
    d, vel = _frame(2, 2, 80)
    z = DeviceNoise(1, DEV)
    ctl = DeviceController(cfg, 2, DEV)
    for kw, word in ((dict(velocity=vel), "velocity"), (dict(controller=DeviceController(cfg, 3, DEV), velocity=vel), "3 scenes"),
                     (dict(controller=ctl), "needs `velocity`"), (dict(controller=ctl, velocity=vel[:1]), "velocity must be"),
                     (dict(controller=ctl, velocity=vel.cpu()), "velocity must be"),
                     (dict(controller=DeviceController(cfg, 2, DEV, waypoints=17), velocity=vel), "horizon"),
                     (dict(controller=DeviceController(cfg, 2, DEV, source="action")), "last three columns")):
        with pytest.raises(ValueError, match=word):
            generate_traj(m, sch, cfg, d["imgs"], d["target"], noise=z, **kw)
    with pytest.raises(ValueError, match="stands in"):
        generate_traj(m, sch, cfg, d["imgs"], None, noise=z, controller=DeviceController(cfg, 2, DEV, waypoints=16), velocity=vel)
    gs = GraphedSampler(m, sch, cfg, noise=z, controller=ctl)
    with pytest.raises(ValueError, match="velocity must be"):
        gs(d["imgs"], d["target"], velocity=vel[:1])
    assert z.tick() == 0 and gs.captured == 0 and not ctl.state.any()
    with pytest.raises(ValueError, match="traj must be"):
        ctl.step(torch.zeros(3, 16, 2, device=DEV), vel)
    with pytest.raises(ValueError, match="velocity"):
        ctl.step(torch.zeros(2, 16, 2, device=DEV), None)
