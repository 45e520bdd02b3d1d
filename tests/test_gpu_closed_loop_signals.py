"""GPU: traffic lights and stop signs in the closed loop (`simulation.drive` with `World(signals=...)`) at the tiny model of
tests/test_gpu_closed_loop.py -- S = 2 scenes, horizon 16, two DDIM steps, a `GraphedSampler(navigator=, controller=, noise=)` --:
the runner against the same ticks written out by hand, T calls of one tick against one call of T, a world without signals against
the loop as it was, and a pinned plan that runs a red light.  The loop is blind and the weights are procedural: these are plumbing
checks, not driving results."""
import numpy as np
import pytest
import torch

from autonomous_driving_with_diffusion_model_amd import DriveMetrics, Guide, Navigator, Pin, Signals, drive, evaluate_closed_loop
from autonomous_driving_with_diffusion_model_amd.simulation import World
from test_gpu_closed_loop import DEV, DT, K, S, TICKS, _bits, _routes, _same, _stack
from test_gpu_select import _frame, _setup

pytestmark = pytest.mark.gpu
INTS = ("ticks", "have", "target", "stop_done", "red_runs", "stop_runs", "stops_met", "first_tick", "first_slot", "emitted", "flags", "pad")


@pytest.fixture(scope="module")
def model():
    m, cfg, sch = _setup("FREE_GUIDANCE", "ddim", steps=2)
    d, _ = _frame(S, 53, "FREE_GUIDANCE")
    return m, cfg, sch, d["imgs"]


def _lines(ahead, kinds, **kw):
    """One line per scene across its route, `ahead[s]` metres down the first segment from the start pose, 6 m wide, always red
    where it is a light; kind 0: an empty slot."""
    route, _ = _routes()
    d = route[:, 1] - route[:, 0]
    unit = d / np.linalg.norm(d, axis=1, keepdims=True)
    rec = Signals.from_lines(route[:, 0] + np.asarray(ahead)[:, None] * unit, np.arctan2(unit[:, 1], unit[:, 0]), 6.0, kinds, 20.0,
                             [0.0, 0.0, 0.0, 1.0])[:, None]
    return Signals(rec, device=DEV, dt=DT, xy_scale=K, **kw)


def _same_signals(a, b, where):
    assert torch.equal(a.state, b.state) and torch.equal(_bits(a.planes), _bits(b.planes)) and torch.equal(a.phase, b.phase), (where, "signals")
    assert a.primed and b.primed


def test_drive_with_signals_is_the_ticks_written_out_by_hand(model):
    """A red light 6 m down scene 0's route and a stop sign 5 m down scene 1's: both bind from the start pose on, so every tick's
    guide holds a live plane."""
    m, cfg, sch, img = model
    assert float(m.magic_num) == K
    run, hand = _stack(m, cfg, sch), _stack(m, cfg, sch)
    sig_run, sig_hand = _lines([6.0, 5.0], [1.0, 2.0]), _lines([6.0, 5.0], [1.0, 2.0])
    assert drive(run[0], run[3], run[4], ticks=TICKS, image=img, world=World(signals=sig_run)) == TICKS
    sampler, nav, ctl, veh, metrics = hand
    bound = []
    for t in range(TICKS):
        if t == 0:
            sig_hand.step(veh.pose, veh.velocity, hold=metrics.done)
        bound.append(int(sig_hand.state[:, 9].sum()))
        sampler(img, pose=veh.pose, velocity=veh.velocity, guide=Guide(planes=sig_hand.planes))
        veh.step(sampler.last_control, hold=metrics.done)
        sig_hand.step(veh.pose, veh.velocity, hold=metrics.done)
        metrics.step(veh.pose, veh.velocity, veh.yaw_rate)
    _same(run, hand, "drive with signals against the ticks by hand")
    _same_signals(sig_run, sig_hand, "by hand")
    f = Signals.fields(sig_hand.words())
    assert f["ticks"].tolist() == [TICKS] * S and f["have"].tolist() == [1] * S and f["stops_met"][0] == 0 and f["stops_met"][1] >= 1
    print("signals after the drive:", {k: f[k].tolist() for k in INTS}, "lines bound per tick", bound)
    assert bound[0] == 2, bound                                   # the first tick's guide already held both lines
    assert sig_hand.phase.tolist() == [[3], [4]]


def test_repeated_calls_of_one_tick_equal_one_call_of_all_ticks(model):
    m, cfg, sch, img = model
    one, many = _stack(m, cfg, sch), _stack(m, cfg, sch)
    sig_one, sig_many = _lines([6.0, 5.0], [1.0, 2.0]), _lines([6.0, 5.0], [1.0, 2.0])
    w_one, w_many = World(signals=sig_one), World(signals=sig_many)
    drive(one[0], one[3], one[4], ticks=TICKS, image=img, world=w_one)
    for t in range(TICKS):
        drive(many[0], many[3], many[4], ticks=1, image=img, world=w_many)
    _same(one, many, "one call against many")
    _same_signals(sig_one, sig_many, "one call against many")


def test_a_world_without_signals_and_a_bare_drive_give_the_loop_as_it_was(model):
    m, cfg, sch, img = model
    bare, empty, hand = _stack(m, cfg, sch), _stack(m, cfg, sch), _stack(m, cfg, sch)
    drive(bare[0], bare[3], bare[4], ticks=TICKS, image=img)
    world = World(signals=None)
    drive(empty[0], empty[3], empty[4], ticks=TICKS, image=img, world=world)
    sampler, nav, ctl, veh, metrics = hand
    for t in range(TICKS):
        sampler(img, pose=veh.pose, velocity=veh.velocity)
        veh.step(sampler.last_control, hold=metrics.done)
        metrics.step(veh.pose, veh.velocity, veh.yaw_rate)
    _same(bare, hand, "a bare drive")
    _same(empty, hand, "a world without signals")
    assert world.signals is None and "signals" not in evaluate_closed_loop(bare[0], bare[3], bare[4], ticks=1, image=img)


def test_a_pinned_plan_runs_a_permanent_red_light_and_the_report_says_so(model):
    """tests/test_gpu_closed_loop.py's pinned drive (its `pin_fn`; it leaves its first 2 m within the twelve ticks) with a
    permanently red light 1 m down scene 0's route and a probe 0.5 m behind the centre: the probe crosses the line once the ego
    has moved 1.5 m.  Without a guide the plan is the pinned one and the light is run; scene 1's only slot is empty.  With the
    default world guide the plane joins every tick: whether that stack stops depends on procedural weights and is printed."""
    m, cfg, sch, img = model
    route, _ = _routes()

    def pinned():
        scout = Navigator(torch.from_numpy(route), torch.zeros(S, 60, dtype=torch.int32), torch.full((S,), 60, dtype=torch.int32), xy_scale=K,
                          first=1, device=DEV)
        xy = torch.zeros(S, 4, 2, device=DEV)

        def pin_fn(t, pose):
            scout.step(pose)
            xy[:, 1:] = scout.window[:, :3]
            return Pin.points(16, 7, [0, 1, 2, 3], xy, "clean")
        return pin_fn

    sampler, nav, ctl, veh, metrics = _stack(m, cfg, sch)
    sig = _lines([1.0, 1.0], [1.0, 0.0], probe=-0.5)
    sig.step(veh.pose, veh.velocity)                              # evaluate_closed_loop resets this away
    report = evaluate_closed_loop(sampler, veh, metrics, ticks=TICKS, image=img, world=World(signals=sig), pin_fn=pinned(),
                                  guide_fn=lambda t, frame, world: None)
    f = DriveMetrics.fields(metrics.words())
    print("pinned through a red light: progress_max", f["progress_max"].tolist(), "signals", {k: np.asarray(v).tolist() for k, v in report["signals"].items()})
    assert (f["progress_max"] > 2.0).all()
    assert report["signals"]["red_runs"].tolist() == [1, 0] and report["signals"]["stop_runs"].tolist() == [0, 0]
    assert report["signals"]["ticks"].tolist() == [TICKS] * S and 1 <= report["signals"]["first_tick"][0] <= TICKS
    assert report["signals"]["penalty"].tolist() == [0.7, 1.0] and report["completion"].shape == (S,)
    g = Signals.fields(sig.words())
    assert {k: int(g[k][1]) for k in INTS} == dict({k: 0 for k in INTS}, ticks=TICKS, have=1)
    # the same drive with the default world guide, which now holds the light's plane
    sampler, nav, ctl, veh, metrics = _stack(m, cfg, sch)
    sig = _lines([1.0, 1.0], [1.0, 0.0], probe=-0.5)
    guided = evaluate_closed_loop(sampler, veh, metrics, ticks=TICKS, image=img, world=World(signals=sig), pin_fn=pinned())
    print("the guided stack at the same light: progress_max", DriveMetrics.fields(metrics.words())["progress_max"].tolist(), "red_runs",
          guided["signals"]["red_runs"].tolist(), "speed", veh.velocity.tolist())
    assert guided["signals"]["ticks"].tolist() == [TICKS] * S
