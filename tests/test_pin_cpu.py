"""CPU: "pinned waypoints v1" -- the Pin object and Pin.points, every pin refusal of `plan_tick` that needs no device, the per-step levels
(c_known, c_known_noise, known_noise) of the three guidance schedulers against the fp32 restatement (tests/pin_ref.py), and the
binding: the four exports declared, exported, prototyped, and refusing bad arguments on the host before any GPU work."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

import dpm_ref
import pin_ref as R
from helpers import SCHED_KW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("adx_ddim_step_pin", "adx_ddpm_step_pin", "adx_dpm_step_pin", "adx_pin_apply")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from autonomous_driving_with_diffusion_model_amd import _lib
    return _lib


# ---- the object -------------------------------------------------------------------------------------------------------------
def test_pin_validates_its_tensors_and_mode(built):
    import autonomous_driving_with_diffusion_model_amd as pkg
    from autonomous_driving_with_diffusion_model_amd.pin import Pin
    assert pkg.Pin is Pin and "Pin" in pkg.__all__
    k, m = torch.zeros(2, 8, 7), torch.ones(2, 8, 7)
    p = Pin(k, m)
    assert p.mode is None and p.known is k and p.mask is m and p.resolve() == "clean"
    assert Pin(k, m, "repaint").resolve() == "repaint" and Pin(k, m, "clean").mode == "clean"
    with pytest.raises(ValueError, match="mode"):
        Pin(k, m, "dirty")
    with pytest.raises(ValueError, match="shape"):
        Pin(k, torch.ones(2, 8, 6))
    with pytest.raises(ValueError, match="shape"):
        Pin(torch.zeros(8, 7), torch.zeros(8, 7))
    with pytest.raises(TypeError, match="float32"):
        Pin(k.double(), m.double())
    with pytest.raises(TypeError, match="float32"):
        Pin(k, m.bool())
    with pytest.raises(TypeError, match="tensors"):
        Pin(k, None)
    # the mode left open reads EVAL.PIN_MODE; an absent key means clean; the object's own mode wins
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    cfg = create_cfg()
    assert cfg.EVAL.PIN_MODE == "clean" and p.resolve(cfg) == "clean"
    cfg.EVAL.PIN_MODE = "repaint"
    assert p.resolve(cfg) == "repaint" and Pin(k, m, "clean").resolve(cfg) == "clean"
    assert p.resolve(SimpleNamespace(EVAL=SimpleNamespace())) == "clean"
    cfg.EVAL.PIN_MODE = "dirty"
    with pytest.raises(ValueError, match="PIN_MODE"):
        p.resolve(cfg)
    q = p.with_mode("repaint")
    assert q.mode == "repaint" and q.known is k and q.mask is m and p.with_mode(None) is p
    # a non-contiguous view is made contiguous once, at construction
    v = torch.zeros(2, 7, 8).transpose(1, 2)
    assert Pin(v, v).known.is_contiguous()


def test_points_pins_xy_of_the_chosen_waypoints(built):
    from autonomous_driving_with_diffusion_model_amd.pin import Pin
    xy = torch.arange(12, dtype=torch.float32).reshape(2, 3, 2) / 16 - 0.3
    p = Pin.points(8, 7, [1, 2, 5], xy, mode="repaint")
    assert p.mode == "repaint" and p.known.shape == p.mask.shape == (2, 8, 7) and p.known.dtype == torch.float32
    assert torch.equal(p.known[:, [1, 2, 5], :2], xy) and torch.equal(p.mask[:, [1, 2, 5], :2], torch.ones(2, 3, 2))
    assert p.mask.sum() == 12 and p.known[p.mask == 0].abs().sum() == 0 and p.known.device == xy.device
    assert torch.equal(Pin.points(8, 2, [7], xy[:, :1]).mask[:, 7], torch.ones(2, 2))
    assert Pin.points(8, 7, [], xy[:, :0]).mask.sum() == 0
    for bad_index, bad_xy in (([8], xy[:, :1]), ([-1], xy[:, :1]), ([1, 1], xy[:, :2]), ([1, 2], xy), ([1], xy[:, :1, :1]),
                              ([1], xy[0, :1])):
        with pytest.raises(ValueError):
            Pin.points(8, 7, bad_index, bad_xy)
    with pytest.raises(ValueError, match="dim"):
        Pin.points(8, 1, [1], xy[:, :1])


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def test_pin_plan_refuses_before_anything_runs(built):
    """`plan_tick` only looks: shapes, devices, dtypes, the mode, the scheduler, the noise source.  None of it needs a device or a
    model, so the image here is a CPU tensor (generate_traj would refuse that later, on its own)."""
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    from autonomous_driving_with_diffusion_model_amd.pin import Pin
    from autonomous_driving_with_diffusion_model_amd.sampling import plan_tick
    cfg = create_cfg()
    cfg.MODEL.HORIZON, cfg.MODEL.TRANSITION_DIM = 8, 7
    img = torch.zeros(2, 3, 16, 16)
    ddim, ddpm = S.GuidanceDDIMScheduler(cfg=cfg, **SCHED_KW), S.GuidanceDDPMScheduler(cfg=cfg, **SCHED_KW)
    dpm = S.GuidanceDPMSolverMultistepScheduler(cfg=cfg, **SCHED_KW)
    k, m = torch.zeros(2, 8, 7), torch.ones(2, 8, 7)

    def _pin_plan(cfg, pin, img, sch, noise, step_noise=None):
        return plan_tick(None, sch, cfg, img, pin=pin, noise=noise, step_noise=step_noise).pin

    assert _pin_plan(cfg, None, img, ddim, None) is None
    for sch in (ddim, ddpm, dpm):
        got = _pin_plan(cfg, Pin(k, m), img, sch, None)
        assert got.mode == "clean" and got.known is k and got.mask is m
    assert _pin_plan(cfg, Pin(k, m, "repaint"), img, ddim, None).mode == "repaint"       # DDIM draws a tensor, as the inpainting one
    assert _pin_plan(cfg, Pin(k, m, "repaint"), img, ddpm, None).mode == "repaint"
    cfg.EVAL.PIN_MODE = "repaint"
    assert _pin_plan(cfg, Pin(k, m), img, ddpm, None).mode == "repaint"                  # the config key
    with pytest.raises(ValueError, match="DeviceNoise"):
        _pin_plan(cfg, Pin(k, m), img, dpm, None)                                        # ... reaches the DPM refusal too
    cfg.EVAL.PIN_MODE = "clean"
    with pytest.raises(ValueError, match="DeviceNoise"):
        _pin_plan(cfg, Pin(k, m, "repaint"), img, dpm, None)
    with pytest.raises(ValueError, match="step_noise"):
        _pin_plan(cfg, Pin(k, m, "repaint"), img, ddpm, None, step_noise=lambda i, shape: torch.zeros(shape))
    assert _pin_plan(cfg, Pin(k, m, "clean"), img, ddpm, None, step_noise=lambda i, shape: torch.zeros(shape)).mode == "clean"
    for bad in (Pin(torch.zeros(3, 8, 7), torch.ones(3, 8, 7)), Pin(torch.zeros(2, 16, 7), torch.ones(2, 16, 7)),
                Pin(torch.zeros(2, 8, 6), torch.ones(2, 8, 6)), Pin(torch.zeros(2, 8, 7, device="meta"), torch.ones(2, 8, 7, device="meta"))):
        with pytest.raises(ValueError, match="MODEL.HORIZON"):
            _pin_plan(cfg, bad, img, ddim, None)
    with pytest.raises(TypeError, match="Pin"):
        _pin_plan(cfg, (k, m), img, ddim, None)
    cfg.EVAL.PIN_MODE = "dirty"
    with pytest.raises(ValueError, match="PIN_MODE"):
        _pin_plan(cfg, Pin(k, m), img, ddim, None)
    cfg.EVAL.PIN_MODE = "clean"
    with pytest.raises(ValueError, match="takes no pin"):
        _pin_plan(cfg, Pin(k, m), img, S.DDPMScheduler(**SCHED_KW), None)
    # a Pin's dtype is checked at construction; one whose tensors were swapped afterwards is caught by the plan
    p = Pin(k, m)
    p.mask = m.double()
    with pytest.raises(ValueError, match="float32"):
        _pin_plan(cfg, p, img, ddim, None)


def test_repaint_on_the_dpm_step_needs_a_device_noise(built):
    """Raised from the arguments alone, before the sample is looked at."""
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    from autonomous_driving_with_diffusion_model_amd.pin import Pin
    q = S.GuidanceDPMSolverMultistepScheduler(**SCHED_KW)
    q.set_timesteps(5)
    x = torch.zeros(2, 8, 7)
    with pytest.raises(ValueError, match="DeviceNoise"):
        q.step(x, q.timesteps[0], x, pin=Pin(x, x, "repaint"))
    with pytest.raises(built.AdxError):                                    # clean gets as far as the CPU tensors
        q.step(x, q.timesteps[0], x, pin=Pin(x, x))


# ---- the levels -------------------------------------------------------------------------------------------------------------
GRID = [(4, 100), (5, 100), (10, 100), (50, 100), (5, 1000), (20, 1000)]


@pytest.mark.parametrize("steps,n_train", GRID)
def test_ddim_and_ddpm_levels_are_the_level_the_step_lands_on(steps, n_train, built):
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    kw = dict(SCHED_KW, num_train_timesteps=n_train)
    ac = R.alphas_cumprod(n_train)
    for q in (S.GuidanceDDIMScheduler(cfg=_cfg(), **kw), S.GuidanceDDPMScheduler(cfg=_cfg(), **kw)):
        q.set_timesteps(steps)
        assert q.timesteps.tolist() == R.leading_timesteps(n_train, steps)
        for t in q.timesteps:
            assert q.pin_level(t, "clean") == (1.0, 0.0, False)
            got, want = q.pin_level(t, "repaint"), R.level_leading(ac, n_train, steps, int(t), "repaint")
            assert got == want and isinstance(got[0], float) and isinstance(got[2], bool), (int(t), got, want)
        # every step but the last lands on a noised level, the last on the clean one: (1, 0, no noise) in both modes
        levels = [q.pin_level(t, "repaint") for t in q.timesteps]
        assert all(lv[2] and 0 < lv[0] < 1 and 0 < lv[1] < 1 for lv in levels[:-1])
        assert levels[-1] == (1.0, 0.0, False) == q.pin_level(q.timesteps[-1], "clean")
        # the level a step lands on is the level `add_noise` gives the next timestep
        for t, t_next in zip(q.timesteps.tolist()[:-1], q.timesteps.tolist()[1:]):
            assert q.pin_level(t, "repaint")[:2] == q.noise_level(t_next)
        with pytest.raises(ValueError, match="mode"):
            q.pin_level(q.timesteps[0], "dirty")


@pytest.mark.parametrize("steps,n_train", GRID)
def test_dpm_levels_are_alpha_and_sigma_of_the_next_sigma(steps, n_train, built):
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    q = S.GuidanceDPMSolverMultistepScheduler(**dict(SCHED_KW, num_train_timesteps=n_train), lambda_min_clipped=-5.1)
    q.set_timesteps(steps)
    ts, sig = dpm_ref.schedule(R.alphas_cumprod(n_train), steps, -5.1)
    assert q.timesteps.tolist() == ts.tolist()
    sigmas = torch.from_numpy(sig)
    for i, t in enumerate(q.timesteps):
        assert q.pin_level(t, "clean") == (1.0, 0.0, False)
        got, want = q.pin_level(t, "repaint"), R.level_dpm(sigmas, i, "repaint")
        assert got == want, (i, got, want)
        c = q._dpm_coef(i)                     # ... as `_dpm_coef` forms alpha_t and sigma_t: r = sigma_t(i + 1) / sigma_t(i)
        if i < steps - 1:
            assert got[2] and torch.tensor(got[1]) / torch.tensor(c.sigma_s) == torch.tensor(c.r)
    assert q.pin_level(q.timesteps[-1], "repaint") == (1.0, 0.0, False)
    with pytest.raises(ValueError, match="not one of"):
        q.pin_level(10 ** 6, "repaint")


def _cfg():
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    return create_cfg()


# ---- the restatement itself ---------------------------------------------------------------------------------------------------
def test_the_restated_blend_has_the_contracts_neutral_elements():
    g = torch.Generator().manual_seed(3)
    prev, known, z = (torch.randn(6, 8, 7, generator=g) for _ in range(3))
    known = known[:2]
    one, zero = torch.ones(2, 8, 7), torch.zeros(2, 8, 7)
    level = (0.75, 0.5, True)
    kp = torch.tensor(0.75) * R.rows(known, 6) + torch.tensor(0.5) * z
    assert torch.equal(R.blend(prev, known, one, level, z).view(torch.int32), kp.view(torch.int32))
    assert torch.equal(R.blend(prev, known, zero, level, z).view(torch.int32), prev.view(torch.int32))
    assert torch.equal(R.blend(prev, known, one), R.rows(known, 6))                      # clean, pinned: the known values
    quarter = torch.full((2, 8, 7), 0.25)
    assert torch.equal(R.blend(prev, known, quarter), 0.25 * R.rows(known, 6) + 0.75 * prev)
    assert not torch.equal(R.rows(known, 6)[0], R.rows(known, 6)[1]) and torch.equal(R.rows(known, 6)[1], R.rows(known, 6)[5])


# ---- the binding ------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_prototyped(built):
    header = open(os.path.join(ROOT, "include", "adx.h")).read()
    assert "Pinned waypoints v1" in header and re.search(r"typedef struct adx_pin\s*\{", header)
    handle = ctypes.CDLL(built.LIB_PATH)
    for name, n_args in zip(EXPORTS, (14, 14, 14, 8)):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(handle, name) and name in built.EXPORTED_SYMBOLS, name
        fn = built.lazy(name)
        assert fn.restype is built.i32 and len(fn.argtypes) == n_args, name
    assert [f[0] for f in built.PinDesc._fields_] == ["known", "mask", "known_rows", "c_known", "c_known_noise", "known_noise"]
    assert ctypes.sizeof(built.PinDesc) == 32


def test_bad_arguments_come_back_as_error_codes_without_a_gpu(built):
    """The checks run on the host before any GPU work, so placeholder addresses (never dereferenced) are enough."""
    lib = built.lib()
    B, H, D = 6, 8, 7
    row = H * D * 4
    mo, x, z, px0, prev, x0, known, mask, state = (0x10000000 * (i + 1) for i in range(9))

    def pin(known=known, mask=mask, rows=2, known_noise=0):
        p = built.PinDesc()
        p.known, p.mask, p.known_rows, p.c_known, p.c_known_noise, p.known_noise = known, mask, rows, 1.0, 0.5, known_noise
        return p

    sc, dc = built.StepCoef(), built.DpmCoef()
    sc.prediction_type = dc.prediction_type = 1

    def step(name, p, c=None, z=None, state=None, prev=prev, x0=x0, B=B, H=H, D=D, row_offset=0):
        return built.lazy(name)(ctypes.byref(c or sc), mo, x, z, state, 7, row_offset, None if p is None else ctypes.byref(p), prev, x0,
                                B, H, D, None)

    def dpm(p, state=None, prev=prev, x0=x0, B=B, H=H, D=D, row_offset=0):
        return built.lazy("adx_dpm_step_pin")(ctypes.byref(dc), mo, x, px0, state, 7, row_offset, None if p is None else ctypes.byref(p),
                                              prev, x0, B, H, D, None)

    def apply(p, x=x, state=None, B=B, H=H, D=D, row_offset=0):
        return built.lazy("adx_pin_apply")(x, None if p is None else ctypes.byref(p), state, row_offset, B, H, D, None)

    inpaint = built.StepCoef()
    inpaint.prediction_type, inpaint.inpaint = 1, 1
    far = (1 << 34) // (H * D) - 3
    cases = []
    for name in EXPORTS[:2]:
        cases += [(lambda n=name: step(n, pin(known=None)), b"null known or mask"),
                  (lambda n=name: step(n, pin(mask=None)), b"null known or mask"),
                  (lambda n=name: step(n, pin(rows=0)), b"multiple"), (lambda n=name: step(n, pin(rows=4)), b"multiple"),
                  (lambda n=name: step(n, pin(rows=-2)), b"multiple"),
                  (lambda n=name: step(n, pin(), z=z, state=state), b"both given"),
                  (lambda n=name: step(n, None, z=z, state=state), b"both given"),
                  (lambda n=name: step(n, pin(known_noise=1)), b"known_noise"),
                  (lambda n=name: step(n, pin(), c=inpaint), b"inpaint"),
                  (lambda n=name: step(n, pin(), prev=known), b"overlaps known or mask"),
                  (lambda n=name: step(n, pin(), prev=mask + 2 * row - 4), b"overlaps known or mask"),
                  (lambda n=name: step(n, pin(), prev=known - B * row + 4), b"overlaps known or mask"),
                  (lambda n=name: step(n, pin(), x0=mask), b"overlaps known or mask"),
                  (lambda n=name: step(n, pin(rows=1), B=1 << 30, H=2, D=1), b"32-bit index"),
                  (lambda n=name: step(n, pin(), state=state, row_offset=far), b"2^34"),
                  (lambda n=name: step(n, pin(), state=state, row_offset=-1), b"row_offset"),
                  (lambda n=name: step(n, pin(), B=0), b"empty shape")]
    cases += [(lambda: dpm(pin(known=None)), b"null known or mask"), (lambda: dpm(pin(rows=4)), b"multiple"),
              (lambda: dpm(pin(known_noise=1)), b"known_noise"), (lambda: dpm(pin(), prev=known), b"overlaps known or mask"),
              (lambda: dpm(pin(), x0=mask + row), b"overlaps known or mask"),
              (lambda: dpm(pin(known_noise=1), state=state, row_offset=far), b"2^34"),
              (lambda: dpm(pin(), state=state, row_offset=-1), b"row_offset"),
              (lambda: dpm(pin(rows=1), B=1 << 30, H=2, D=1), b"32-bit index"),
              (lambda: dpm(None, prev=x0), b"alias"),                                    # a NULL pin: adx_dpm_step's own refusals
              (lambda: apply(None), b"null sample or pin"), (lambda: apply(pin(), x=None), b"null sample or pin"),
              (lambda: apply(pin(mask=None)), b"null known or mask"), (lambda: apply(pin(rows=5)), b"multiple"),
              (lambda: apply(pin(known_noise=1)), b"known_noise"), (lambda: apply(pin(), x=known + row), b"overlaps known or mask"),
              (lambda: apply(pin(known_noise=1), state=state, row_offset=far), b"2^34"),
              (lambda: apply(pin(), B=0), b"empty shape"), (lambda: apply(pin(rows=1), B=1 << 30, H=2, D=1), b"32-bit index")]
    for i, (call, word) in enumerate(cases):
        assert call() == -1, i
        assert word in lib.adx_last_error(), (i, word, lib.adx_last_error())
    with pytest.raises(ValueError, match="multiple"):
        built.check(apply(pin(rows=4)), "adx_pin_apply")


def test_python_surface_refuses_cpu_tensors(built):
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    from autonomous_driving_with_diffusion_model_amd.pin import Pin, pin_apply
    x = torch.zeros(2, 8, 7)
    with pytest.raises(built.AdxError):
        pin_apply(x, Pin(x, x))
    q = S.GuidanceDDIMScheduler(cfg=_cfg(), **SCHED_KW)
    q.set_timesteps(5)
    with pytest.raises(built.AdxError):
        q.step(x, q.timesteps[0], x, pin=Pin(x, x))
