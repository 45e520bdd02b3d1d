"""GPU: the in-kernel noise stream (csrc/noise.h, noise.DeviceNoise) against its numpy restatement (tests/noise_ref.py), and
every consumer against the injected-tensor path the golden tests pin to the reference:

    reference --(tests/test_gpu_model.py, golden loop.ddpm.* / loop.evaluate.cfg1)--> loop with injected noise tensors
              --(this file, bit for bit)--> loop / graph drawing the same values inside the step kernel
"""
import math

import numpy as np
import pytest
import torch

import noise_ref as NR
from autonomous_driving_with_diffusion_model_amd import DeviceNoise
from autonomous_driving_with_diffusion_model_amd import scheduler as S
from autonomous_driving_with_diffusion_model_amd.utils import procedural as P
from helpers import IMG_SMALL, SCHED_KW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INIT = DeviceNoise.INIT_SLOT


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def test_words_equal_the_restatement_exactly():
    """adx_noise_words, word for word: seeds and ticks on both sides of 2^32, INIT_SLOT, ranges that start and end off a
    multiple of four, a row offset (direct and through shard()), and the tick kernel's carry into the high word."""
    cases = [  # seed, tick, slot, first, n
        (0, 0, 0, 0, 64),
        (1, 1, 99, 0, 1000),
        (0x1234567_89ABCDEF, (5 << 32) | 17, 50, 3, 1021),
        ((1 << 64) - 1, (1 << 64) - 1, INIT, 1, 6),
        (42, 3, INIT, 4 * 777 + 2, 333),
        (1 << 32, 1 << 32, 1, (1 << 34) - 1030, 1030),
    ]
    for seed, tick, slot, first, n in cases:
        z = DeviceNoise(seed, DEV)
        z.seek(tick)
        assert z.tick() == tick
        assert np.array_equal(_u32(z.words(slot, (n,), row_offset=first)), NR.words(seed, tick, slot, first, n)), (seed, tick, slot)
    z = DeviceNoise(7, DEV)
    z.seek((1 << 32) - 2)
    for k in (1, 2, 3):                 # ... fffffffe -> ffffffff -> 1_00000000 -> 1_00000001
        z.begin_tick()
        assert z.tick() == (1 << 32) - 2 + k
        got = _u32(z.words(90, (3, 16, 7), row_offset=5))
        assert np.array_equal(got.reshape(-1), NR.words(7, (1 << 32) - 2 + k, 90, 5 * 112, 336))
        assert np.array_equal(_u32(z.shard(5).words(90, (3, 16, 7))), got)
        assert np.array_equal(_u32(z.shard(2).shard(1).words(90, (3, 16, 7), row_offset=2)), got)
    z.reseed(8)                         # the tick stays
    assert np.array_equal(_u32(z.words(0, (9,))), NR.words(8, (1 << 32) + 1, 0, 0, 9))
    with pytest.raises(ValueError):
        z.words(0, (16,), row_offset=1 << 34)


def test_normals_within_four_times_the_fp32_restatements_own_error():
    """adx_noise_normal against the restatement in fp64 ON THE SAME WORDS, over 2^20 + 5 elements starting at element 3.
    Bound: four times the distance of the restatement evaluated in fp32 (numpy) from those fp64 values -- two accurate fp32
    evaluations may disagree by the sum of their errors; the factor leaves room for libm differences and still fails a
    fast-intrinsic build.  Measured on an MI355X: device 6.7e-7, fp32 restatement 2.8e-5 (its u = (k + 0.5) * 2^-24 rounds once
    k >= 2^23, which the kernel's evaluation avoids: csrc/noise.h), bound 1.1e-4; profiles/README.md ("In-kernel sampler noise")."""
    seed, tick, slot, first, n = 20261016, 3, 57, 3, (1 << 20) + 5
    z = DeviceNoise(seed, DEV)
    z.seek(tick)
    got = z.normal(slot, (n,), row_offset=first).cpu().numpy()
    want = NR.normals(seed, tick, slot, first, n)
    own = np.abs(NR.normals(seed, tick, slot, first, n, dtype=np.float32).astype(np.float64) - want).max()
    dist = np.abs(got.astype(np.float64) - want).max()
    print(f"normals over {n} elements: device max |z - fp64| = {dist:.3e}; fp32 restatement {own:.3e}; bound {4 * own:.3e}")
    assert got.dtype == np.float32 and np.isfinite(got).all()
    assert dist <= 4 * own, (dist, own)


def test_moments_of_the_device_normals():
    """2^22 normals: |mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N) (five standard errors of each estimate)."""
    n = 1 << 22
    z = DeviceNoise(11, DEV)
    z.begin_tick()
    g = z.normal(INIT, (n,)).double()
    mean, var = g.mean().item(), g.var(unbiased=False).item()
    print(f"moments over 2^22 device normals: mean {mean:+.3e} (bound {5 / math.sqrt(n):.3e}), var - 1 {var - 1:+.3e} "
          f"(bound {5 * math.sqrt(2 / n):.3e})")
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(var - 1) <= 5 * math.sqrt(2 / n)


def _cfg():
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    return create_cfg()


def _inputs(shape, seed=21):
    u = lambda name, lo=-1.5, hi=1.5, sh=shape: P._uniform(name, seed, sh, lo, hi).to(DEV)  # noqa: E731
    mask = (P._uniform("noise.tm", seed, shape, 0, 1) > 0.5).float().to(DEV)
    return u("noise.mo"), u("noise.x"), u("noise.tt", -1, 1), mask, u("noise.mo2", sh=(2 * shape[0],) + tuple(shape[1:]))


def _step_cases(cfg, shape):
    """(name, scheduler, timestep, kwargs, whether the step uses noise)"""
    mo, x, tt, tm, mo2 = _inputs(shape)
    inp = dict(target_traj=tt, target_mask=tm)
    gddpm, gddim = S.GuidanceDDPMScheduler(cfg=cfg, **SCHED_KW), S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
    ddpm, iddim, iddpm = S.DDPMScheduler(**SCHED_KW), S.InpaintingDDIMScheduler(**SCHED_KW), S.InpaintingDDPMScheduler(**SCHED_KW)
    for q in (gddpm, gddim, ddpm, iddim, iddpm):
        q.set_timesteps(10, device=DEV)
    return mo, x, [
        ("guidance ddpm t=50", gddpm, 50, dict(model_output=mo), True),
        ("guidance ddpm t=0", gddpm, 0, dict(model_output=mo), False),
        ("stock ddpm t=90", ddpm, 90, dict(model_output=mo), True),
        ("guidance ddim eta=0.5", gddim, 50, dict(model_output=mo, eta=0.5), True),
        ("guidance ddim eta=0.5 clipped output", gddim, 10, dict(model_output=mo, eta=0.5, use_clipped_model_output=True), True),
        ("inpainting ddim eta=0 mask", iddim, 50, dict(model_output=mo, **inp), True),
        ("inpainting ddim eta=0.5 mask", iddim, 50, dict(model_output=mo, eta=0.5, **inp), True),
        ("inpainting ddim eta=0.5 no mask", iddim, 50, dict(model_output=mo, eta=0.5), True),
        ("inpainting ddim t=0 mask", iddim, 0, dict(model_output=mo, **inp), False),
        ("inpainting ddpm mask", iddpm, 50, dict(model_output=mo, **inp), True),
        ("inpainting ddpm t=0 mask", iddpm, 0, dict(model_output=mo, **inp), False),
        ("guidance ddpm cfg combine + zero_first", gddpm, 30, dict(model_output=mo2, cfg_scale=7.5, zero_first=True), True),
        ("guidance ddim eta=0.5 cfg combine + zero_first", gddim, 30, dict(model_output=mo2, eta=0.5, cfg_scale=7.5, zero_first=True), True),
    ]


@pytest.mark.parametrize("shape", [(3, 16, 7), (5, 16, 2), (3, 5, 7), (37, 16, 7)])
def test_step_with_the_stream_equals_the_step_on_the_streams_tensor_bit_for_bit(shape):
    """step(generator=noise) == step(variance_noise=noise.normal(t, shape)): DDPM at t > 0 and t = 0, DDIM with eta = 0.5, both
    inpainting schedulers with a mask (the RePaint known-noise term shares the step's draw), the classifier-free combine
    with zero_first, D = 2 and 7, and B*H*D = 105 (a multiple of neither 4 nor 256) up to 4144 (several workgroups)."""
    z = DeviceNoise(5, DEV)
    z.begin_tick()
    mo, x, cases = _step_cases(_cfg(), shape)
    for name, sch, t, kw, uses_noise in cases:
        kw = dict(kw)
        m = kw.pop("model_output")
        T = torch.tensor(t)
        a = sch.step(m, T, x, generator=z, **kw)
        tensor = z.normal(t, shape)
        b = sch.step(m, T, x, variance_noise=tensor, **kw)
        assert torch.equal(a.prev_sample, b.prev_sample), (name, (a.prev_sample - b.prev_sample).abs().max().item())
        assert torch.equal(a.pred_original_sample, b.pred_original_sample), name
        assert torch.isfinite(a.prev_sample).all(), name
        c = sch.step(m, T, x, variance_noise=torch.zeros_like(tensor), **kw)
        assert torch.equal(a.prev_sample, c.prev_sample) == (not uses_noise), name      # the draw is really in the result
        if uses_noise:
            with pytest.raises(ValueError, match="Cannot pass both generator and variance_noise"):
                sch.step(m, T, x, generator=z, variance_noise=tensor, **kw)
    # generator=None and a torch.Generator are untouched: the same torch.randn tensor as before
    g1, g2 = torch.Generator(device=DEV).manual_seed(3), torch.Generator(device=DEV).manual_seed(3)
    sch = cases[0][1]
    want = sch.step(mo, torch.tensor(50), x, variance_noise=torch.randn(shape, generator=g2, device=DEV)).prev_sample
    assert torch.equal(sch.step(mo, torch.tensor(50), x, generator=g1).prev_sample, want)


def test_a_shard_of_rows_draws_what_the_full_batch_draws_there():
    shape, a, b = (6, 16, 7), 2, 5
    z = DeviceNoise(9, DEV)
    z.begin_tick()
    assert torch.equal(z.normal(50, (b - a, 16, 7), row_offset=a), z.normal(50, shape)[a:b])
    assert torch.equal(z.shard(a).normal(50, (b - a, 16, 7)), z.normal(50, shape)[a:b])
    _, x, cases = _step_cases(_cfg(), shape)
    for name, sch, t, kw, uses_noise in cases:
        kw = dict(kw)
        m = kw.pop("model_output")
        full = sch.step(m, torch.tensor(t), x, generator=z, **kw).prev_sample
        part = {k: (v[a:b] if torch.is_tensor(v) else v) for k, v in kw.items()}
        mp = torch.cat([m[a:b], m[6 + a:6 + b]]) if "cfg_scale" in kw else m[a:b]
        got = sch.step(mp, torch.tensor(t), x[a:b], generator=z.shard(a), **part).prev_sample
        assert torch.equal(got, full[a:b]), name
        if uses_noise:      # and an unsharded draw on the same rows does NOT (the offset is what makes it so)
            assert not torch.equal(sch.step(mp, torch.tensor(t), x[a:b], generator=z, **part).prev_sample, full[a:b]), name


def _model(use_cond):
    from autonomous_driving_with_diffusion_model_amd.modeling import build_model
    cfg = _cfg()
    cfg.MODEL.HORIZON = 16
    cfg.TRAIN.USE_COND = cfg.GUIDANCE.USE_COND = use_cond
    m = build_model(cfg)
    P.load_procedural(m, 0)
    m = m.to(DEV).eval()
    cfg.EVAL.SAMPLE_STEPS = 10
    cfg.GUIDANCE.FREE_SCALE, cfg.GUIDANCE.CLASSIFIER_SCALE = 7.5, 15.0
    if use_cond == "CLASSIFIER_GUIDANCE":
        cfg.GUIDANCE.LOSS_LIST = [["TargetGuidance", []]]
    return m, cfg, S.GuidanceDDPMScheduler(cfg=cfg, **SCHED_KW)


@pytest.mark.parametrize("use_cond", ["NO_GUIDANCE", "FREE_GUIDANCE", "CLASSIFIER_GUIDANCE"])
@pytest.mark.parametrize("fuse", [True, False])
def test_loop_with_the_stream_equals_the_loop_on_injected_tensors(use_cond, fuse):
    """generate_traj(noise=n) == generate_traj(init_trajs=n.normal(INIT_SLOT, ...), step_noise=n.normal(t_i, ...)) at the same
    tick, for the 10-step DDPM loop on the small image.  The right-hand path is the one the golden tests hold to the reference
    for arbitrary injected noise."""
    from autonomous_driving_with_diffusion_model_amd.sampling import generate_traj
    m, cfg, sch = _model(use_cond)
    B = 2
    d = {k: v.to(DEV) for k, v in P.synthetic_batch(B, 16, image_hw=IMG_SMALL, seed=31).items()}
    tgt = None if use_cond == "NO_GUIDANCE" else d["target"]
    z = DeviceNoise(1234, DEV)
    seen = []
    for tick in (1, 2):
        got = generate_traj(m, sch, cfg, d["imgs"], tgt, fuse=fuse, noise=z)
        assert z.tick() == tick
        ts = sch.timesteps.tolist()
        want = generate_traj(m, sch, cfg, d["imgs"], tgt, z.normal(INIT, (B, 16, 7)), fuse=fuse,
                             step_noise=lambda i, s: z.normal(ts[i], s))
        assert torch.equal(got, want), (tick, (got - want).abs().max().item())
        assert torch.isfinite(got).all()
        seen.append(got)
    assert not torch.equal(seen[0], seen[1])          # a new tick is new noise
    with pytest.raises(ValueError):
        generate_traj(m, sch, cfg, d["imgs"], tgt, noise=z, step_noise=lambda i, s: z.normal(0, s))
    assert z.tick() == 2


def test_evaluate_sample_with_the_stream_equals_injected_tensors():
    from autonomous_driving_with_diffusion_model_amd.sampling import evaluate_sample
    m, _, _ = _model("NO_GUIDANCE")
    d = P.synthetic_batch(8, 16, image_hw=IMG_SMALL, seed=34)
    img = d["imgs"][:1].repeat(8, 1, 1, 1).to(DEV)
    sch = S.DDPMScheduler(**SCHED_KW)
    z = DeviceNoise(77, DEV)
    got = evaluate_sample(m, sch, img, None, 10, noise=z)
    ts = sch.timesteps.tolist()
    want = evaluate_sample(m, sch, img, z.normal(INIT, (8, 16, 7)), 10, step_noise=lambda i, s: z.normal(ts[i], s))
    assert torch.equal(got, want) and torch.isfinite(got).all()
    init = d["init_trajs"].to(DEV)                    # a caller's own initial trajectory, steps from the stream
    got = evaluate_sample(m, sch, img, init, 10, noise=z)
    want = evaluate_sample(m, sch, img, init, 10, step_noise=lambda i, s: z.normal(ts[i], s))
    assert z.tick() == 2 and torch.equal(got, want)
    with pytest.raises(ValueError):
        evaluate_sample(m, sch, img, init, 10, noise=z, step_noise=lambda i, s: z.normal(0, s))


@pytest.mark.parametrize("use_cond,B", [("NO_GUIDANCE", 1), ("NO_GUIDANCE", 4), ("FREE_GUIDANCE", 1), ("CLASSIFIER_GUIDANCE", 4)])
def test_graphed_ddpm_tick_draws_fresh_noise_on_every_replay(use_cond, B):
    """GraphedSampler(m, ddpm, cfg, noise=n): replay k with a new camera frame == the eager generate_traj(noise=...) at tick k;
    identical inputs give different samples; reseed + seek(0) reproduces replay 1; without `noise` the DDPM scheduler is
    still refused.  One scene (the pipeline-launch path of the UNet) and B = 4."""
    from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler, generate_traj
    m, cfg, sch = _model(use_cond)
    with pytest.raises(ValueError):
        GraphedSampler(m, sch, cfg)
    seed = (9 << 32) | 5
    z = DeviceNoise(seed, DEV)
    gs = GraphedSampler(m, sch, cfg, noise=z)
    frames = [{k: v.to(DEV) for k, v in P.synthetic_batch(B, 16, image_hw=IMG_SMALL, seed=20 + k).items()} for k in (1, 2, 3)]
    tgt = lambda d: None if use_cond == "NO_GUIDANCE" else d["target"]  # noqa: E731
    got = [gs(d["imgs"], tgt(d)) for d in frames]                       # capture + replay 1, replays 2 and 3
    assert z.tick() == 3
    again = gs(frames[2]["imgs"], tgt(frames[2]))                        # tick 4, same inputs as tick 3
    assert not torch.equal(again, got[2])
    z2 = DeviceNoise(seed, DEV)
    for k, d in enumerate(frames):
        want = generate_traj(m, sch, cfg, d["imgs"], tgt(d), noise=z2)
        assert z2.tick() == k + 1
        assert torch.equal(got[k], want), (k + 1, (got[k] - want).abs().max().item())
    z.reseed(seed)
    z.seek(0)
    assert torch.equal(gs(frames[0]["imgs"], tgt(frames[0])), got[0])
    # a caller's own initial trajectory: only the steps draw from the stream (tick 2 again)
    init = frames[1]["init_trajs"]
    a = gs(frames[1]["imgs"], tgt(frames[1]), init)
    z2.seek(1)
    assert torch.equal(a, generate_traj(m, sch, cfg, frames[1]["imgs"], tgt(frames[1]), init, noise=z2))
    assert z.tick() == 2


def test_tick_kernel_is_capturable_and_host_writes_are_refused_while_a_capture_is_open():
    """begin_tick() is a launch: captured, it runs on every replay and not at capture time.  seek() / reseed() copy host words
    into the state, which a capture cannot record as intended: they raise instead."""
    z = DeviceNoise(3, DEV)
    z.begin_tick()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        z.begin_tick()
        with pytest.raises(RuntimeError, match="capture"):
            z.seek(0)
        with pytest.raises(RuntimeError, match="capture"):
            z.reseed(1)
    assert z.tick() == 1
    g.replay()
    g.replay()
    assert z.tick() == 3
    assert np.array_equal(_u32(z.words(0, (8,))), NR.words(3, 3, 0, 0, 8))
