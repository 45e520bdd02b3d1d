"""CPU: `plan_tick` -- the one place a sampling tick is decided.  Stubs only, no device: the plan is pure (it consumes no tick of
the noise stream and writes nothing to the scheduler, the warm state or the controller), its fields say what `generate_traj` will
do, its `key()` tells apart everything a captured graph bakes into a node and nothing that travels through a static buffer, and
the refusals come in the order candidates, noise / step_noise, warm, control, pin."""
from types import SimpleNamespace

import pytest
import torch

from autonomous_driving_with_diffusion_model_amd import sampling
from autonomous_driving_with_diffusion_model_amd.config import create_cfg
from autonomous_driving_with_diffusion_model_amd.control.device import DeviceController
from autonomous_driving_with_diffusion_model_amd.control.select import TrajectorySelector
from autonomous_driving_with_diffusion_model_amd.misc.constant import GuidanceType
from autonomous_driving_with_diffusion_model_amd.noise import DeviceNoise
from autonomous_driving_with_diffusion_model_amd.pin import Pin
from autonomous_driving_with_diffusion_model_amd.sampling import TickPlan, WarmStart, plan_tick

S, H, D, N = 2, 8, 7, 5
IMG = torch.zeros(S, 3, 16, 16)
MODEL = SimpleNamespace(cache_perception=True, time_conditioning=None)       # enough of a model for the hoisted path's test


class _Noise(DeviceNoise):
    """A DeviceNoise without its device state: `begin_tick` is recorded, not launched."""

    def __init__(self, began):
        self._state, self._row_offset, self.began = torch.zeros(4, dtype=torch.int32), 0, began

    def begin_tick(self):
        self.began.append(1)


class _Scheduler:
    """What a plan may read of a scheduler; what it must not call raises."""
    supports_pin, _is_ddim, deterministic = True, True, False
    timesteps = tuple(range(N))

    def set_timesteps(self, *a, **kw):
        raise AssertionError("plan_tick called set_timesteps")

    def set_begin_index(self, *a, **kw):
        raise AssertionError("plan_tick called set_begin_index")


def _controller(scenes=S, source="pid"):
    """`_stub_controller` of tests/test_control_device_cpu.py, with the two things `TickPlan.key()` reads of a controller."""
    c = object.__new__(DeviceController)
    c.scenes, c.source, c.waypoints, c.device = scenes, source, 4, torch.device("cpu")
    c.state = SimpleNamespace(data_ptr=lambda: 0x1000)
    c.key = lambda: (scenes, source)
    return c


def _warm(valid=True, steps=3, shift=1):
    w = WarmStart(steps, shift)
    w.valid, w.prev = valid, torch.zeros(S, H, D)
    return w


def _pin(mode="clean", fill=0.0):
    return Pin(torch.full((S, H, D), fill), torch.ones(S, H, D), mode)


def _cfg(steps=N, use="NO_GUIDANCE", free_scale=7.5):
    cfg = create_cfg()
    cfg.GUIDANCE.FREE_SCALE = free_scale
    cfg.MODEL.HORIZON, cfg.MODEL.TRANSITION_DIM, cfg.EVAL.SAMPLE_STEPS, cfg.GUIDANCE.USE_COND = H, D, steps, use
    return cfg


@pytest.fixture(autouse=True)
def any_device(monkeypatch):
    """`motion` goes through `require_gpu_f32`, which refuses CPU tensors; the plan's own checks are what is under test here."""
    monkeypatch.setattr(sampling.L, "require_gpu_f32", lambda t, name, dtype=torch.float32: t)


def _plan(began=None, cfg=None, target=None, init_trajs=None, noise="stub", scheduler=None, **kw):
    noise = _Noise([] if began is None else began) if noise == "stub" else noise
    return plan_tick(MODEL, scheduler or _Scheduler(), cfg or _cfg(), IMG, target, init_trajs, noise=noise, **kw)


def test_the_plan_is_pure():
    began = []
    for kw in (dict(), dict(warm=_warm()), dict(warm=_warm(), motion=torch.zeros(S, 3)), dict(candidates=3),
               dict(pin=_pin("clean")), dict(pin=_pin("repaint")), dict(controller=_controller(), velocity=torch.zeros(S)),
               dict(warm=_warm(), set_timesteps=False), dict(pin=_pin("repaint"), graphed=True)):
        warm, ctl = kw.get("warm"), kw.get("controller")
        prev = None if warm is None else warm.prev
        held = None if ctl is None else dict(vars(ctl))
        sched = _Scheduler()
        sched.begin_index = 0
        sched_before = dict(vars(sched))
        plan = _plan(began, scheduler=sched, **kw)
        assert isinstance(plan, TickPlan), kw
        with pytest.raises(AttributeError):
            plan.K = 2                                                               # immutable
        assert not began, kw
        assert dict(vars(sched)) == sched_before == {"begin_index": 0}
        if warm is not None:
            assert warm.valid and warm.prev is prev and not prev.any() and (warm.steps, warm.shift) == (3, 1)
        if ctl is not None:
            assert dict(vars(ctl)) == held


def test_fields():
    cold = _plan()
    assert (cold.S, cold.K, cold.rows, cold.H, cold.D, cold.n) == (S, 1, S, H, D, N) and cold.selector is None
    assert cold.use is GuidanceType.NO_GUIDANCE and cold.fuse and cold.hoisted and cold.table_rows == S and not cold.pair_identity
    assert (cold.m_warm, cold.shift, cold.is_warm, cold.motion, cold.i0) == (0, 0, False, None, 0)
    assert cold.controller is None and cold.velocity is None and cold.pin is None and not cold.entry_blend
    assert not cold.is_ddpm and cold.free_scale is None
    # how a tick starts
    motion = torch.zeros(S, 3)
    assert cold.start == "stream" and _plan(noise=None).start == "randn"
    assert _plan(init_trajs=torch.zeros(5, H, D)).start == "init" and _plan(warm=_warm(), motion=motion).start == "warm"
    assert _plan(warm=_warm(valid=False), init_trajs=torch.zeros(S, H, D)).start == "init"
    # i0 == n - m exactly when the tick is warm
    for m in (1, 3, N):
        w, c = _plan(warm=_warm(steps=m, shift=2), motion=motion), _plan(warm=_warm(valid=False, steps=m, shift=2), motion=motion)
        assert (w.m_warm, w.shift, w.is_warm, w.i0) == (m, 2, True, N - m) and w.motion is motion
        assert (c.m_warm, c.shift, c.is_warm, c.i0) == (m, 2, False, 0) and c.motion is None and c.start == "stream"
    off = _plan(warm=_warm(steps=0), motion=motion)
    assert (off.m_warm, off.shift, off.is_warm, off.motion, off.i0) == (0, 0, False, None, 0)
    # rows, and the table's under classifier-free guidance
    assert _plan(candidates=3).rows == 3 * S and _plan(init_trajs=torch.zeros(5, H, D)).rows == 5
    k3 = _plan(candidates=3, init_trajs=torch.zeros(3 * S, H, D))
    assert (k3.K, k3.rows) == (3, 3 * S) and (k3.selector.w_goal, k3.selector.w_smooth, k3.selector.w_consensus) == (1.0, 0.0, 0.0)
    free = _cfg(use="FREE_GUIDANCE")
    free.GUIDANCE.FREE_SCALE = 7.5
    for kw, rows in ((dict(), S), (dict(candidates=3), 3 * S), (dict(init_trajs=torch.zeros(5, H, D)), 5)):
        assert _plan(**kw).table_rows == rows and _plan(cfg=free, **kw).table_rows == 2 * rows
    assert _plan(cfg=free).free_scale == 7.5 and _plan(cfg=free).use is GuidanceType.FREE_GUIDANCE
    one = plan_tick(MODEL, _Scheduler(), free, IMG[:1], noise=None)
    assert one.pair_identity and not plan_tick(MODEL, _Scheduler(), free, IMG[:1], noise=None, fuse=False).pair_identity
    assert not plan_tick(SimpleNamespace(), _Scheduler(), _cfg(), IMG).hoisted and not _plan(fuse=False).hoisted
    ddpm = SimpleNamespace(_is_ddim=False)
    assert plan_tick(MODEL, ddpm, _cfg(), IMG).is_ddpm and not plan_tick(MODEL, SimpleNamespace(deterministic=True), _cfg(), IMG).is_ddpm
    # the entry blend runs iff the pin is clean; an open mode is EVAL.PIN_MODE
    k, mk = torch.zeros(S, H, D), torch.ones(S, H, D)
    clean, repaint, by_key = _plan(pin=_pin("clean")), _plan(pin=_pin("repaint")), _plan(pin=Pin(k, mk))
    assert clean.entry_blend and clean.pin.mode == "clean" and not repaint.entry_blend and repaint.pin.mode == "repaint"
    assert by_key.entry_blend and by_key.pin.mode == "clean" and by_key.pin.known is k and by_key.pin.mask is mk
    cfg = _cfg()
    cfg.EVAL.PIN_MODE = "repaint"
    assert not _plan(cfg=cfg, pin=Pin(k, mk)).entry_blend and _plan(cfg=cfg, pin=Pin(k, mk)).pin.mode == "repaint"
    # the controller and its velocity
    ctl, vel = _controller(), torch.zeros(S)
    got = _plan(controller=ctl, velocity=vel)
    assert got.controller is ctl and got.velocity is vel
    assert _plan(controller=_controller(source="action"), target=torch.zeros(2)).velocity is None


def test_key_tells_baked_decisions_apart_and_nothing_else():
    ctl, vel, motion, tgt = _controller(source="action"), torch.zeros(S), torch.zeros(S, 3), torch.zeros(S, 2)
    base = dict(target=tgt, warm=_warm(), motion=motion, candidates=2, selector=TrajectorySelector(1.0, 0.5, 0.25))
    variants = {
        "K": dict(candidates=3),
        "selector weight": dict(selector=TrajectorySelector(1.0, 0.5, 0.5)),
        "m_warm": dict(warm=_warm(steps=2)),
        "shift": dict(warm=_warm(shift=2)),
        "warm valid": dict(warm=_warm(valid=False)),
        "motion present": dict(motion=None),
        "controller present": dict(controller=ctl),
        "velocity present": dict(controller=ctl, velocity=vel),
        "pin present": dict(pin=_pin("clean")),
        "pin mode": dict(pin=_pin("repaint")),
        "SAMPLE_STEPS": dict(cfg=_cfg(steps=N + 1)),
        "USE_COND": dict(cfg=_cfg(use="CLASSIFIER_GUIDANCE")),
        "FREE_GUIDANCE": dict(cfg=_cfg(use="FREE_GUIDANCE")),
        "FREE_SCALE": dict(cfg=_cfg(use="FREE_GUIDANCE", free_scale=3.0)),     # a kernel argument of every fused step node
    }
    keys = {"base": _plan(**base).key()}
    for name, kw in variants.items():
        keys[name] = _plan(**dict(base, **kw)).key()
    hash(tuple(keys.values()))
    names = list(keys)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert keys[a] != keys[b], (a, b)
    assert _plan(**base).key() == keys["base"]                                        # a fresh plan of the same arguments
    # two controllers are two keys, and so are two settings of one
    other = _controller(source="action")
    assert _plan(**dict(base, controller=other)).key() != keys["controller present"]
    # values that travel through static buffers: the pin's known and mask, target, motion, velocity
    full = dict(base, controller=ctl, velocity=vel, pin=_pin("clean"))
    moved = dict(full, target=tgt + 1.0, motion=motion + 1.0, velocity=vel + 1.0, pin=_pin("clean", fill=0.5))
    assert _plan(**full).key() == _plan(**moved).key()
    # torch.randn is drawn outside a graph and handed in: the two starts are one graph
    assert _plan(noise=None).key() == _plan(noise=None, init_trajs=torch.zeros(S, H, D)).key() != _plan().key()


def test_refusals_keep_their_order():
    """One argument set, two faults: a bad `velocity` and a bad pin shape.  The control refusal is raised; with the velocity mended,
    the pin's; and the refusals ahead of control's win over both."""
    bad_pin = Pin(torch.zeros(3, H, D), torch.ones(3, H, D))
    both = dict(controller=_controller(), velocity=torch.zeros(S + 1), pin=bad_pin)
    began = []
    with pytest.raises(ValueError, match="velocity must be"):
        _plan(began, **both)
    with pytest.raises(ValueError, match="MODEL.HORIZON"):
        _plan(began, **dict(both, velocity=torch.zeros(S)))
    with pytest.raises(ValueError, match="more than EVAL.SAMPLE_STEPS"):
        _plan(began, warm=_warm(steps=N + 1), **both)
    with pytest.raises(ValueError, match="not both"):
        _plan(began, warm=_warm(steps=N + 1), step_noise=lambda i, shape: torch.zeros(shape), **both)
    with pytest.raises(ValueError, match="candidates must be"):
        _plan(began, candidates=0, warm=_warm(steps=N + 1), step_noise=lambda i, shape: torch.zeros(shape), **both)
    assert not began


def test_refusals_of_a_graphed_tick_come_from_the_plan():
    """What used to surface inside a capture's warm-up pass, and the one refusal only a graph has."""
    sharded = _Noise([])
    sharded._row_offset = 4
    with pytest.raises(ValueError, match="sharded DeviceNoise"):
        _plan(noise=sharded, candidates=3, graphed=True)
    with pytest.raises(ValueError, match=r"candidates \* scenes = 6 rows"):
        _plan(candidates=3, init_trajs=torch.zeros(4, H, D), graphed=True)
    with pytest.raises(ValueError, match="hoisted conditioning path"):
        plan_tick(SimpleNamespace(), _Scheduler(), _cfg(), IMG, candidates=3, graphed=True)
    with pytest.raises(ValueError, match="GraphedSampler: a `repaint` pin"):
        _plan(noise=None, pin=_pin("repaint"), graphed=True)
    assert _plan(noise=None, pin=_pin("repaint")).pin.mode == "repaint"               # eager DDIM draws tensors for it
    # a warm tick on the caller's own timesteps reads them, and only then
    short = _Scheduler()
    short.timesteps = (3, 2, 1)
    with pytest.raises(ValueError, match="holds 3 timesteps"):
        plan_tick(MODEL, short, _cfg(), IMG, noise=_Noise([]), warm=_warm(), set_timesteps=False)
    assert plan_tick(MODEL, short, _cfg(), IMG, noise=_Noise([]), warm=_warm()).i0 == N - 3
    assert plan_tick(MODEL, None, _cfg(), IMG, noise=_Noise([]), warm=_warm()).is_warm          # no scheduler, none needed
