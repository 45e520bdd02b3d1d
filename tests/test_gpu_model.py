"""GPU parity, model level: ResNet-34, whole TemporalMapUnet forwards and the callers' sampling loops
through the drop-in Python surface, against (a) the golden vectors produced by the real reference and
(b) the CPU oracle on the same seeded inputs.  north_star tolerance: fp32 trajectories within 1e-4."""
import os

import pytest
import torch

from oracle import resnet as R
from oracle import sampling as OS
from oracle import unet as U
from autonomous_driving_with_diffusion_model_amd.utils import procedural as P
from helpers import IMG_SMALL, SCHED_KW, close, close_traj, oracle_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAJ_TOL = 1e-4


def make_model(use_cond, H, seed=0):
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    from autonomous_driving_with_diffusion_model_amd.modeling import build_model
    cfg = create_cfg()
    cfg.MODEL.HORIZON = H
    cfg.TRAIN.USE_COND = use_cond
    cfg.GUIDANCE.USE_COND = use_cond
    m = build_model(cfg)
    P.load_procedural(m, seed)
    if os.environ.get("ADX_TEST_STATE"):          # e.g. "imagenet_like": the perception state at real-weight scale (helpers.py)
        from helpers import oracle_sd
        m.load_state_dict(oracle_sd(use_cond, seed))
    return m.to(DEV).eval(), cfg


def test_library_loaded_and_no_fallback():
    from autonomous_driving_with_diffusion_model_amd import _lib
    assert _lib.lib().adx_version() >= 1
    m, _ = make_model("NO_GUIDANCE", 16)
    with pytest.raises(_lib.AdxError):   # CPU tensors are refused, there is no CPU path
        m.cpu()(torch.zeros(1, 16, 7), torch.zeros(1, 3, 64, 96), torch.zeros(1, dtype=torch.int64))


def test_resnet_small_vs_golden_and_oracle(golden):
    m, _ = make_model("CLASSIFIER_GUIDANCE", 16)
    img = P.synthetic_batch(2, 16, image_hw=IMG_SMALL, seed=3)["imgs"]
    with torch.no_grad():
        f = m.perception(img.to(DEV)).cpu()
    close(f, golden("ops")["ops.resnet34_small"], 1e-4)
    close(f, R.resnet34_forward(oracle_sd("CLASSIFIER_GUIDANCE"), "perception.", img), 1e-4)


def test_resnet_full_size_vs_golden(golden):
    m, _ = make_model("CLASSIFIER_GUIDANCE", 16)
    img = P.synthetic_batch(1, 16, image_hw=(256, 900), seed=4)["imgs"]
    with torch.no_grad():
        f = m.perception(img.to(DEV)).cpu()
    close(f, golden("ops")["ops.resnet34_full"], 2e-4, rtol=1e-5)   # |feature| ~ 30 here


def test_resnet_ragged_sizes_and_batch():
    sd = oracle_sd("NO_GUIDANCE")
    m, _ = make_model("NO_GUIDANCE", 16)
    # the larger cases change layout decisions layer by layer (cell tensors and batch-wide column tiles where a layer's convs are
    # plain launches, fp32 NCHW where they split their reduction; maps narrower than 16 columns tile per image)
    for hw, b in (((70, 101), 3), ((33, 47), 1), ((128, 131), 2), ((200, 333), 3), ((129, 515), 9), ((97, 131), 33), ((64, 2048), 2),
                  # the smallest image, on each side of every format change there (tests/test_resnet_plan_cpu.py: PINNED) and on an
                  # uneven and an even pair of sub-batches
                  ((32, 32), 9), ((32, 32), 17), ((32, 32), 33), ((32, 32), 40)):
        img = P.synthetic_batch(b, 16, image_hw=hw, seed=5)["imgs"]
        with torch.no_grad():
            f = m.perception(img.to(DEV)).cpu()
        close(f, R.resnet34_forward(sd, "perception.", img), 1e-4)


def test_perception_cell_layout_vs_fp32_layout_and_oracle(tmp_path):
    """csrc/conv2d_hs.hip: between plain launches of the pipelined 3x3 kernel the activations travel as 16-byte cells of
    eight channels already split into fp16 hi / lo (the stride-2 kernel and the average pool read them too); launches that
    split their reduction (few tiles) keep fp32 NCHW, so the batch decides layer by layer: B = 2 at 256x900 has cells in
    layer1 only, B = 6 in layers 1-3, B = 12 everywhere.  Products are bit-identical in both layouts and a residual read
    from cells is the tensor to 2^-23, so the features must agree far inside the oracle tolerance -- and with
    ADX_CONV_CELLS=0 (a process of its own) the old path is still there to compare against."""
    import os
    import subprocess
    import sys
    import perception_worker as W
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "fp32_layout.pt")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "perception_worker.py"), out],
                       env=dict(os.environ, ADX_CONV_CELLS="0"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    plain = torch.load(out)
    cells = W.features()
    sd = oracle_sd("NO_GUIDANCE")
    for (hw, b) in W.CASES:
        key = f"{hw[0]}x{hw[1]}b{b}"
        scale = plain[key].abs().max().item()
        err = (cells[key] - plain[key]).abs().max().item()
        assert err <= 2e-6 * max(1.0, scale), (key, err, scale)
        if b <= 6:
            img = P.synthetic_batch(b, 16, image_hw=hw, seed=5 + b)["imgs"]
            close(cells[key], R.resnet34_forward(sd, "perception.", img), 2e-4, rtol=1e-5)


def test_perception_sub_batch_streams_match_the_single_stream_pass(tmp_path):
    """csrc/conv2d.hip (round 5): at B >= 32 the inference perception pass runs as two sub-batches on streams of their own (one
    sub-batch's launches fill the CUs the other's last round of workgroups leaves idle).  Same kernels and per-image arithmetic,
    so the features equal the single-stream pass (ADX_RESNET_STREAMS=1, a process of its own) up to the tile-mode decisions that
    depend on the launch's batch -- including uneven halves whose layers make DIFFERENT layout decisions (33 = 17 + 16 at 97x131:
    one half in cells, the other splitting its reductions) and are at different layers at the same time (each sub-batch owns a
    fixed region of every rotating buffer)."""
    import os
    import subprocess
    import sys
    import streams_worker as W
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "one_stream.pt")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "streams_worker.py"), out],
                       env=dict(os.environ, ADX_RESNET_STREAMS="1"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    one = torch.load(out)
    # ... and with the stem and layer1 per sub-batch as well (ADX_RESNET_SPLIT_FROM=0; by default they stay one chain on the whole batch)
    out0 = str(tmp_path / "split_everything.pt")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "streams_worker.py"), out0],
                       env=dict(os.environ, ADX_RESNET_SPLIT_FROM="0"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    for name, two in (("default", W.features()), ("split from the stem", torch.load(out0))):
        for key, runs in two.items():
            ref = one[key][0]
            scale = max(1.0, ref.abs().max().item())
            for f in runs:
                assert torch.equal(f, runs[0]), (name, key)              # run to run: bit-equal
                err = (f - ref).abs().max().item()
                assert err <= 2e-6 * scale, (name, key, err, scale)


def test_perception_pass_stream_runs_ahead_only_of_work_it_does_not_depend_on():
    """modeling/perception.py: eval passes of >= 16 images run on a stream of their own; a pass on the SAME, unwritten image tensor
    does not wait for what the caller queued since the previous pass (the reference-faithful loop's previous step).  It must still
    see (a) an in-place write to the image (version counter), (b) a new image object at the same address, (c) changed weights;
    and its result must be ordered in front of the caller's next use."""
    m, _ = make_model("NO_GUIDANCE", 16)
    p = m.perception
    img = P.synthetic_batch(20, 16, image_hw=(64, 96), seed=3)["imgs"].to(DEV)
    with torch.no_grad():
        p.run_ahead = False
        ref1 = p(img).clone()
        ref2 = p(img * 0.5 + 0.1).clone()
        p.run_ahead = "version"             # identity + version counter (the default only runs ahead inside frozen_image)
        busy = torch.randn(4096, 4096, device=DEV)
        a = p(img)
        for _ in range(6):                      # the caller's stream is busy when the second pass is issued
            busy = busy @ busy.t() * 1e-4
        b = p(img)                              # same object, same version: runs ahead of the matmuls
        assert torch.equal(a, ref1) and torch.equal(b, ref1)
        for _ in range(6):
            busy = busy @ busy.t() * 1e-4
        img.mul_(0.5).add_(0.1)                 # queued BEHIND the matmuls on the caller's stream: the pass must wait for it
        c = p(img)
        assert torch.equal(c, ref2)
        img2 = img.clone()
        d = p(img2)                             # another object
        assert torch.equal(d, ref2)
        w0 = p.conv1.weight.detach().clone()
        p.conv1.weight.mul_(1.5)                # weights re-laid on the caller's stream
        e = p(img2)
        assert not torch.equal(e, ref2)
        p.conv1.weight.copy_(w0)
        assert torch.equal(p(img2), ref2)
        torch.cuda.synchronize()
        assert torch.isfinite(busy).all()


@pytest.mark.parametrize("H", [16, 32])
def test_unet_forward_vs_golden(golden, H):
    g = golden("unet")
    d = {k: v.to(DEV) for k, v in P.synthetic_batch(2, H, image_hw=IMG_SMALL, seed=11).items()}
    t = torch.tensor([90, 3], dtype=torch.int64, device=DEV)
    with torch.no_grad():
        m, _ = make_model("NO_GUIDANCE", H)
        close(m(d["trajs"], d["imgs"], t).cpu(), g[f"unet.no.h{H}"], TRAJ_TOL)
        close(m(d["trajs"], d["imgs"], t[:1].repeat(2)).cpu(), g[f"unet.no.h{H}.t1"], TRAJ_TOL)
        m, _ = make_model("FREE_GUIDANCE", H)
        close(m(d["trajs"], d["imgs"], t, cond=d["target"]).cpu(), g[f"unet.free.h{H}.cond"], TRAJ_TOL)
        close(m(d["trajs"], d["imgs"], t).cpu(), g[f"unet.free.h{H}.nocond"], TRAJ_TOL)
        x2 = torch.cat([d["trajs"], d["trajs"]], 0)
        c2 = torch.cat([d["target"], torch.zeros_like(d["target"])], 0)
        close(m(x2, d["imgs"], t[:1], cond=c2).cpu(), g[f"unet.free.h{H}.cfg"], TRAJ_TOL)
        m, _ = make_model("CLASSIFIER_GUIDANCE", H)
        a, te = m(d["trajs"], d["imgs"], t, return_action_and_time_only=True)
        close(a.cpu(), g[f"unet.cls.h{H}.action"], TRAJ_TOL)
        close(te.cpu(), g[f"unet.cls.h{H}.time_embed"], TRAJ_TOL)


def test_perception_pass_sees_undeclared_image_writes():
    """modeling/perception.py, default `run_ahead = "frozen"`: a pass only runs ahead of the caller's queued work inside a
    `frozen_image(img)` context, i.e. where the caller SAID nothing writes the image.  Outside one, writes that move no version
    counter -- through `img.data`, through a raw data_ptr() handed to a native call -- are queued on the caller's stream like any
    other work and the pass must see them (round 5 keyed the decision on identity + `._version` alone: such a write was neither
    waited for nor seen).  Inside a context the same image object runs ahead, bit-identically; a context on another tensor, or a
    closed one, does not carry over; the weight images' re-lay with an EQUAL key (native running-statistics writes move no
    counter) is joined too."""
    from autonomous_driving_with_diffusion_model_amd import _lib as L
    import ctypes as C
    m, _ = make_model("NO_GUIDANCE", 16)
    p = m.perception
    assert p.run_ahead == "frozen"
    src = P.synthetic_batch(20, 16, image_hw=(64, 96), seed=3)["imgs"].to(DEV)
    img = src.clone()
    new1 = (src * 0.5 + 0.1).contiguous()
    frames = torch.randint(0, 256, (20, 64, 96, 3), dtype=torch.uint8, device=DEV)
    mean, std = (C.c_float * 3)(0.485, 0.456, 0.406), (C.c_float * 3)(0.229, 0.224, 0.225)
    with torch.no_grad():
        ref0 = p(src.clone()).clone()
        ref1 = p(new1.clone()).clone()
        new2 = torch.empty_like(src)
        L.check(L.lib().adx_image_normalize(frames.data_ptr(), new2.data_ptr(), 20, 64, 96, mean, std, L.stream_ptr(src.device)))
        ref2 = p(new2.clone()).clone()
        busy = torch.randn(4096, 4096, device=DEV)

        def load():
            nonlocal busy
            for _ in range(6):
                busy = busy @ busy.t() * 1e-4

        a = p(img)
        v0 = img._version
        load()
        img.data.copy_(new1)                    # queued behind the matmuls; moves no counter of `img`
        assert img._version == v0
        b = p(img)
        load()
        # a raw-pointer producer: the uint8 front-end writes the normalised frames INTO the image's storage
        L.check(L.lib().adx_image_normalize(frames.data_ptr(), img.data_ptr(), 20, 64, 96, mean, std, L.stream_ptr(img.device)))
        assert img._version == v0
        c = p(img)
        assert torch.equal(a, ref0) and torch.equal(b, ref1) and torch.equal(c, ref2)
        # inside a context: the first pass joins the caller's stream (the write above), the others run ahead of the matmuls
        with p.frozen_image(img):
            load()
            d0 = p(img)
            seen0 = p._pass_seen
            load()
            d1 = p(img)
            assert p._pass_seen[4] is seen0[4] and seen0[4] is not None
            other = new1.clone()
            e = p(other)                        # not the frozen tensor: joins
            assert p._pass_seen[4] is None
        assert torch.equal(d0, ref2) and torch.equal(d1, ref2) and torch.equal(e, ref1)
        load()
        img.data.copy_(src)                     # the context is closed: an undeclared write again
        f = p(img)
        assert torch.equal(f, ref0)
        # a pass that bypasses the pass stream (run_ahead off) in between resets what the next one may assume
        with p.frozen_image(img):
            p(img)
            p.run_ahead = False
            p(img)
            assert p._pass_seen is None
            p.run_ahead = "frozen"
            g = p(img)
        assert torch.equal(g, ref0)
        # re-laid weight images under an unchanged key: train-mode forward (native running-statistics update), back to eval
        with p.frozen_image(img):
            p(img)
            gen = p._pack_gen
            p.train()
            p(img[:4])
            p.eval()
            h1 = p(img)
            assert p._pack_gen > gen
            p.invalidate()
            h2 = p(img)                         # repacked again from the same statistics: same key as h1's, another generation
        assert torch.equal(h1, h2) and not torch.equal(h1, ref0)



def test_unet_batch64_h32_vs_oracle():
    """BASELINE sizes (B=64, H=32) for the temporal stack; the perception feature is shared input."""
    m, _ = make_model("NO_GUIDANCE", 32)
    sd = oracle_sd("NO_GUIDANCE")
    d = P.synthetic_batch(64, 32, image_hw=(32, 32), seed=12)
    feat = P._uniform("feat64", 12, (64, 64), -3.0, 3.0)
    m.perception.forward = lambda img: feat.to(DEV)   # test-only stub of the encoder output
    with torch.no_grad():
        y = m(d["trajs"].to(DEV), d["imgs"].to(DEV), d["t"].to(DEV)).cpu()
    close(y, U.unet_forward(sd, d["trajs"], None, d["t"], img_feature=feat), TRAJ_TOL)


def test_unet_batch_independence_at_b128():
    """Size-independent property at the CFG batch (2 x 64): row i of a batched call equals a B=1 call."""
    m, _ = make_model("FREE_GUIDANCE", 32)
    d = P.synthetic_batch(128, 32, image_hw=(32, 32), seed=13)
    feat = P._uniform("feat128", 13, (128, 64), -3.0, 3.0).to(DEV)
    x, t, c = d["trajs"].to(DEV), d["t"].to(DEV), d["target"].to(DEV)
    with torch.no_grad():
        m.perception.forward = lambda img: feat
        y = m(x, d["imgs"].to(DEV), t, cond=c)
        for i in (0, 63, 127):
            m.perception.forward = lambda img, i=i: feat[i:i + 1]
            yi = m(x[i:i + 1], d["imgs"][:1].to(DEV), t[i:i + 1], cond=c[i:i + 1])
            close(yi.cpu(), y[i:i + 1].cpu(), 2e-5)


def _sched(cfg, kind="ddim", thresholding=True):
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    cls = S.GuidanceDDIMScheduler if kind == "ddim" else S.GuidanceDDPMScheduler
    return cls(cfg=cfg, thresholding=thresholding, **SCHED_KW)


@pytest.mark.parametrize("fuse", [True, False])
def test_generate_traj_vs_golden(golden, fuse):
    from autonomous_driving_with_diffusion_model_amd.sampling import generate_traj
    g = golden("loop")
    d = {k: v.to(DEV) for k, v in P.synthetic_batch(1, 16, image_hw=IMG_SMALL, seed=31).items()}
    for name, n, scale in (("NO_GUIDANCE", 10, None), ("FREE_GUIDANCE", 10, 7.5)):
        m, cfg = make_model(name, 16)
        cfg.EVAL.SAMPLE_STEPS = n
        if scale:
            cfg.GUIDANCE.FREE_SCALE = scale
        tgt = None if name == "NO_GUIDANCE" else d["target"][0]
        r = generate_traj(m, _sched(cfg), cfg, d["imgs"], tgt, d["init_trajs"], fuse=fuse)
        close_traj(r.cpu(), g[f"loop.ddim.{name}"], TRAJ_TOL)
        # reference-faithful mode (perception re-run every step) gives the same trajectory
        m.cache_perception = False
        r2 = generate_traj(m, _sched(cfg), cfg, d["imgs"], tgt, d["init_trajs"], fuse=fuse)
        assert torch.equal(r, r2)
    m, cfg = make_model("NO_GUIDANCE", 16)
    cfg.EVAL.SAMPLE_STEPS = 10
    r = generate_traj(m, _sched(cfg, "ddpm", False), cfg, d["imgs"], None, d["init_trajs"], fuse=fuse,
                      step_noise=lambda i, s: P.step_noise(i, s, seed=33))
    close_traj(r.cpu(), g["loop.ddpm.NO_GUIDANCE"], TRAJ_TOL)


def test_cfg3_ddim50_free_h32_vs_golden(golden):
    """BASELINE cfg-3 shape: 50-step DDIM, FREE guidance (scale 7.5), H = 32, per-scene targets."""
    from autonomous_driving_with_diffusion_model_amd.sampling import generate_traj
    d = {k: v.to(DEV) for k, v in P.synthetic_batch(2, 32, image_hw=IMG_SMALL, seed=32).items()}
    m, cfg = make_model("FREE_GUIDANCE", 32)
    cfg.EVAL.SAMPLE_STEPS, cfg.GUIDANCE.FREE_SCALE = 50, 7.5
    r = generate_traj(m, _sched(cfg), cfg, d["imgs"], d["target"], d["init_trajs"])
    close_traj(r.cpu(), golden("loop")["loop.ddim50.FREE_GUIDANCE.h32"], TRAJ_TOL)


def test_cfg1_evaluate_vs_golden(golden):
    """BASELINE cfg-1: B = 8, H = 16, 10 stock-DDPM steps (train.evaluate), injected noise."""
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    from autonomous_driving_with_diffusion_model_amd.sampling import evaluate_sample
    d = P.synthetic_batch(8, 16, image_hw=IMG_SMALL, seed=34)
    img = d["imgs"][:1].repeat(8, 1, 1, 1).to(DEV)
    m, _ = make_model("NO_GUIDANCE", 16)
    r = evaluate_sample(m, S.DDPMScheduler(**SCHED_KW), img, d["init_trajs"].to(DEV), 10,
                        step_noise=lambda i, s: P.step_noise(i, s, seed=35))
    close(r.cpu(), golden("loop")["loop.evaluate.cfg1"], TRAJ_TOL)


def test_weight_updates_are_seen():
    """load_state_dict / in-place optimizer-style updates / EMA-style copies re-pack the HIP weights."""
    from autonomous_driving_with_diffusion_model_amd.misc.load_param import copy_parameters
    m, _ = make_model("NO_GUIDANCE", 16, seed=0)
    d = {k: v.to(DEV) for k, v in P.synthetic_batch(2, 16, image_hw=IMG_SMALL, seed=11).items()}
    t = torch.tensor([90, 3], device=DEV)
    with torch.no_grad():
        y0 = m(d["trajs"], d["imgs"], t)
        m2, _ = make_model("NO_GUIDANCE", 16, seed=1)
        y1 = m2(d["trajs"], d["imgs"], t)
        assert not torch.allclose(y0, y1)
        copy_parameters([p.detach().clone() for p in m2.parameters()], m.parameters())
        for b, b2 in zip(m.buffers(), m2.buffers()):
            b.copy_(b2)
        assert torch.equal(m(d["trajs"], d["imgs"], t), y1)
        m.load_state_dict(P.procedural_state_dict(((k, tuple(v.shape)) for k, v in m.state_dict().items()), 0))
        assert torch.equal(m(d["trajs"], d["imgs"], t), y0)


# ---------------------------------------------------------------------------------------------
# classifier guidance: TrajPredict forward / input gradient, GuidanceLoss, fused guided output
def test_trajpredict_forward_and_input_grad_vs_golden(golden):
    from helpers import uni
    g = golden("ops")
    m, _ = make_model("CLASSIFIER_GUIDANCE", 16)
    a = uni("ops.action", (2, 15, 3)).to(DEV).requires_grad_()
    te = uni("ops.te", (2, 64)).to(DEV)
    s = m.state_pred(a, te)
    close(s.detach().cpu(), g["ops.traj_predict"], 2e-5)
    (ga,) = torch.autograd.grad((s * uni("ops.traj_w", (2, 15, 4)).to(DEV)).sum(), [a])
    close(ga.cpu(), g["ops.traj_predict_dact"], 2e-5)
    # strided input (action[:, :-1] is a view) and the oracle at T = 31
    sd = oracle_sd("CLASSIFIER_GUIDANCE")
    m32, _ = make_model("CLASSIFIER_GUIDANCE", 32)
    a32 = uni("tp.a32", (5, 32, 3))
    te32 = uni("tp.te32", (5, 64))
    ref_in = a32.clone().requires_grad_()
    ref = U.traj_predict(sd, "state_pred.", ref_in[:, :-1], te32)
    w = uni("tp.w32", (5, 31, 4))
    (gref,) = torch.autograd.grad((ref * w).sum(), [ref_in])
    ad = a32.to(DEV).requires_grad_()
    out = m32.state_pred(ad[:, :-1], te32.to(DEV))
    close(out.detach().cpu(), ref.detach(), 2e-5)
    (gd,) = torch.autograd.grad((out * w.to(DEV)).sum(), [ad])
    close(gd.cpu(), gref, 2e-5)


def test_guidance_loss_generic_and_fused_vs_golden(golden):
    """G1/G2 through the reference-shaped API (autograd through the HIP TrajPredict node) and through
    the single fused launch; both against the reference's own outputs (both branches of the rule)."""
    from helpers import uni
    from autonomous_driving_with_diffusion_model_amd.control import GuidanceLoss
    g = golden("ops")
    m, cfg = make_model("CLASSIFIER_GUIDANCE", 16)
    cfg.GUIDANCE.LOSS_LIST = [["TargetGuidance", []]]
    cfg.GUIDANCE.CLASSIFIER_SCALE = 15.0
    gl = GuidanceLoss(cfg)
    te = uni("ops.g_te", (1, 64)).to(DEV)
    for tag, tgt in (("near", torch.tensor([0.05, -0.02])), ("far", torch.tensor([0.9, 0.7]))):
        a1 = uni("ops.g_action." + tag, (1, 16, 3)).to(DEV).requires_grad_()
        st = m.state_pred(a1[:, :-1], te)
        st = torch.cat([torch.zeros_like(st[:, :1]), st], dim=1)
        xg = torch.cat([st, a1], dim=-1)
        out = gl(xg, a1, tgt.to(DEV), torch.tensor(1.5582221))
        close(out.cpu(), g[f"ops.guidance_loss.{tag}"], 5e-5)
        fused = m.state_pred.guided_output(a1.detach(), te, tgt.to(DEV), 1.5582221, 15.0)
        close(fused.cpu(), g[f"ops.guidance_loss.{tag}"], 5e-5)


def test_classifier_guidance_loop_vs_golden_and_batched_vmap(golden):
    from autonomous_driving_with_diffusion_model_amd.sampling import generate_traj
    d = {k: v.to(DEV) for k, v in P.synthetic_batch(1, 16, image_hw=IMG_SMALL, seed=31).items()}
    m, cfg = make_model("CLASSIFIER_GUIDANCE", 16)
    cfg.GUIDANCE.LOSS_LIST = [["TargetGuidance", []]]
    cfg.GUIDANCE.CLASSIFIER_SCALE, cfg.EVAL.SAMPLE_STEPS = 15.0, 5
    for fuse in (True, False):
        r = generate_traj(m, _sched(cfg), cfg, d["imgs"], d["target"][0], d["init_trajs"], fuse=fuse)
        close_traj(r.cpu(), golden("loop")["loop.ddim.CLASSIFIER_GUIDANCE"], TRAJ_TOL)
    # BASELINE cfg-4 rule: a batch is B independent B = 1 problems (vmap of the reference)
    Bn = 6
    d = P.synthetic_batch(Bn, 32, image_hw=IMG_SMALL, seed=36)
    m, cfg = make_model("CLASSIFIER_GUIDANCE", 32)
    cfg.GUIDANCE.LOSS_LIST = [["TargetGuidance", []]]
    cfg.GUIDANCE.CLASSIFIER_SCALE, cfg.EVAL.SAMPLE_STEPS = 15.0, 4
    got = generate_traj(m, _sched(cfg), cfg, d["imgs"].to(DEV), d["target"].to(DEV), d["init_trajs"].to(DEV))
    want = OS.generate_traj(oracle_sd("CLASSIFIER_GUIDANCE"), d["imgs"], d["init_trajs"], d["target"],
                            use_cond="CLASSIFIER_GUIDANCE", n_steps=4, classifier_scale=15.0, hoist_perception=True)
    close_traj(got.cpu(), want, TRAJ_TOL)


@pytest.mark.parametrize("H", [40, 64])
def test_classifier_guidance_loop_long_horizons_vs_oracle(H):
    """Classifier guidance above horizon 32 (modeling/temporal.py:119 builds state_pred for any horizon; T = H - 1 = 39 / 63
    rows run TrajPredict's 64-row kernels): the eager loop and the graph replay against the oracle's loop."""
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler, generate_traj
    from helpers import SCHED_KW
    Bn = 3
    d = P.synthetic_batch(Bn, H, image_hw=IMG_SMALL, seed=40 + H)
    m, cfg = make_model("CLASSIFIER_GUIDANCE", H)
    cfg.GUIDANCE.LOSS_LIST = [["TargetGuidance", []]]
    cfg.GUIDANCE.CLASSIFIER_SCALE, cfg.EVAL.SAMPLE_STEPS = 15.0, 4
    got = generate_traj(m, _sched(cfg), cfg, d["imgs"].to(DEV), d["target"].to(DEV), d["init_trajs"].to(DEV))
    want = OS.generate_traj(oracle_sd("CLASSIFIER_GUIDANCE"), d["imgs"], d["init_trajs"], d["target"],
                            use_cond="CLASSIFIER_GUIDANCE", n_steps=4, classifier_scale=15.0, hoist_perception=True)
    close_traj(got.cpu(), want, TRAJ_TOL)
    sch = S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
    gs = GraphedSampler(m, sch, cfg)
    for _ in range(2):        # capture, then replay
        assert torch.equal(gs(d["imgs"].to(DEV), d["target"].to(DEV), d["init_trajs"].to(DEV)), got)


@pytest.mark.parametrize("use_cond,B", [("FREE_GUIDANCE", 1), ("NO_GUIDANCE", 2), ("CLASSIFIER_GUIDANCE", 2)])
def test_graphed_sampler_replays_the_eager_loop_bit_for_bit(use_cond, B):
    """sampling.GraphedSampler: the DDIM loop captured as one HIP graph; replays with new inputs (camera frame
    included: the perception pass is inside the graph) equal the eager loop exactly."""
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler, generate_traj
    from helpers import SCHED_KW
    m, cfg = make_model(use_cond, 16)
    cfg.EVAL.SAMPLE_STEPS = 10
    cfg.GUIDANCE.FREE_SCALE, cfg.GUIDANCE.CLASSIFIER_SCALE = 7.5, 15.0
    if use_cond == "CLASSIFIER_GUIDANCE":
        cfg.GUIDANCE.LOSS_LIST = [["TargetGuidance", []]]
    sch = S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
    gs = GraphedSampler(m, sch, cfg)
    for seed in (21, 22, 23):            # the first call captures, the others replay with new inputs
        d = {k: v.to(DEV) for k, v in P.synthetic_batch(B, 16, image_hw=IMG_SMALL, seed=seed).items()}
        tgt = None if use_cond == "NO_GUIDANCE" else d["target"]
        got = gs(d["imgs"], tgt, d["init_trajs"])
        want = generate_traj(m, sch, cfg, d["imgs"], tgt, d["init_trajs"])
        assert torch.equal(got, want), (seed, (got - want).abs().max().item())


@pytest.mark.parametrize("use_cond,B", [("FREE_GUIDANCE", 1), ("FREE_GUIDANCE", 3), ("NO_GUIDANCE", 2), ("CLASSIFIER_GUIDANCE", 2)])
def test_time_conditioning_table_equals_the_per_step_recomputation(use_cond, B):
    """TemporalMapUnet.time_conditioning (adx_unet_time_conditioning): the time MLP, condition MLP and 16 block Linears
    for all timesteps of a loop in one pass; a forward that starts from the table -- and, at one scene, reads the single
    trajectory for both rows of the classifier-free pair -- must equal the reference-shaped forward bit for bit."""
    m, _ = make_model(use_cond, 16)
    d = {k: v.to(DEV) for k, v in P.synthetic_batch(B, 16, image_hw=IMG_SMALL, seed=31).items()}
    free = use_cond == "FREE_GUIDANCE"
    cond = torch.cat([d["target"], torch.zeros_like(d["target"])], 0) if free else None
    rows = 2 * B if free else B
    ts = torch.tensor([97, 50, 3, 0], dtype=torch.int64, device=DEV)
    x = d["init_trajs"]
    xin = torch.cat([x, x], 0) if free else x
    with torch.no_grad():
        tc = m.time_conditioning(d["imgs"], ts, cond=cond, rows=rows)
        assert tc.time_bias.shape[:2] == (4, rows) and tc.time_embed.shape == (4, rows, m.dim)
        for i in range(4):
            t = ts[i].reshape(-1) if free else ts[i].reshape(-1).repeat(B)
            kw = dict(return_action_and_time_only=True) if use_cond == "CLASSIFIER_GUIDANCE" else {}
            want = m(xin, d["imgs"], t, cond=cond, **kw)
            got = m(xin, None, None, time_cond=(tc, i), **kw)
            if free and B == 1:
                got1 = m(x, None, None, time_cond=(tc, i))          # one trajectory row feeds both rows of the pair
                assert torch.equal(got1, want)
            for g, w in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
                assert torch.equal(g, w), (i, (g - w).abs().max().item())
    with pytest.raises(ValueError):
        m(torch.zeros(rows + 1, 16, 7, device=DEV), None, None, time_cond=(tc, 0))


@pytest.mark.parametrize("H", [24, 40, 48, 56])
def test_unet_horizons_that_are_not_powers_of_two_vs_oracle(H):
    """The reference accepts any horizon divisible by 8 (modeling/temporal.py:59-75: 24 -> 24, 12, 6, 3).  Such lengths
    run on the next power of two with the real lengths as masks (adx_tconv_desc::lin_valid / lout_valid): zero padding,
    GroupNorm statistics and the strided / transposed convs must all see the real length."""
    from autonomous_driving_with_diffusion_model_amd.sampling import generate_traj
    d = P.synthetic_batch(3, H, image_hw=(32, 32), seed=40 + H)
    feat = P._uniform(f"feat.h{H}", 12, (3, 64), -3.0, 3.0)
    for name in ("NO_GUIDANCE", "FREE_GUIDANCE"):
        m, cfg = make_model(name, H)
        m.perception.forward = lambda img: feat.to(DEV)   # test-only stub of the encoder output
        cond = d["target"] if name == "FREE_GUIDANCE" else None
        with torch.no_grad():
            y = m(d["trajs"].to(DEV), d["imgs"].to(DEV), d["t"].to(DEV), cond=None if cond is None else cond.to(DEV)).cpu()
        want = U.unet_forward(oracle_sd(name), d["trajs"], None, d["t"], cond, use_cond=name, img_feature=feat)
        close(y, want, TRAJ_TOL)
    # ... and through the whole sampling loop (scheduler steps at the ragged length)
    cfg.EVAL.SAMPLE_STEPS, cfg.GUIDANCE.FREE_SCALE = 5, 7.5
    got = generate_traj(m, _sched(cfg), cfg, d["imgs"].to(DEV), d["target"].to(DEV), d["init_trajs"].to(DEV)).cpu()
    want = OS.generate_traj(oracle_sd("FREE_GUIDANCE"), d["imgs"], d["init_trajs"], d["target"], use_cond="FREE_GUIDANCE",
                            n_steps=5, free_scale=7.5, img_feature=feat)
    close_traj(got, want, 1e-4)


def test_training_step_at_a_ragged_horizon_vs_oracle_loss():
    """Whole-model train-mode forward + backward at H = 24 (perception included): the loss equals the oracle's and every
    parameter receives a finite gradient (per-tensor gradient parity of the temporal stack: test_gpu_train.py)."""
    import torch.nn.functional as F
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    m, _ = make_model("NO_GUIDANCE", 24)
    m.train()
    d = P.synthetic_batch(2, 24, image_hw=IMG_SMALL, seed=5)
    dd = {k: v.to(DEV) for k, v in d.items()}
    noisy = S.DDPMScheduler(**SCHED_KW).add_noise(dd["trajs"], dd["noise"], dd["t"], zero_first=True)
    loss = F.mse_loss(m(noisy, dd["imgs"], dd["t"]), dd["trajs"])
    loss.backward()
    want = OS.training_loss(oracle_sd("NO_GUIDANCE"), d["imgs"], d["trajs"], d["target"], d["t"], d["noise"], use_cond="NO_GUIDANCE")
    assert abs(loss.item() - want.item()) <= 2e-5 * max(1.0, abs(want.item())), (loss.item(), want.item())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


@pytest.mark.parametrize("dim,mults,H", [(64, (1, 2, 4), 16), (128, (1, 2, 4, 8), 32), (64, (1, 2), 16),
                                         (48, (1, 2, 4, 8), 32), (96, (1, 2, 4), 16), (64, (1, 2, 4, 8), 8), (48, (1, 2, 4, 8), 24)])
def test_unet_other_widths_and_depths_vs_oracle(dim, mults, H):
    """MODEL.DIM / MODEL.DIM_MULTS / MODEL.HORIZON other than the default (64, (1, 2, 4, 8), 16): the executor builds its
    launch list from the config (csrc/unet.hip: build), nothing is specialised for one width.  The reference takes any
    DIM divisible by 8 (GroupNorm(8, C), modeling/helpers.py:105-107) and any horizon divisible by 2^(levels - 1): layers
    whose GroupNorm groups are not a power of two wide (DIM = 48: 6, 12, 24, 48 channels; 96: 12, 24, 48) or hold fewer than
    64 elements (H = 8: 32 at the bottom of the up path) run on the general-shape kernel (csrc/tconv_generic.hip)."""
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    from autonomous_driving_with_diffusion_model_amd.modeling import build_model
    g = torch.Generator().manual_seed(dim + H)
    d = P.synthetic_batch(3, H, image_hw=(32, 32), seed=9)
    feat = torch.randn(3, dim, generator=g)
    for name in ("NO_GUIDANCE", "FREE_GUIDANCE"):
        cfg = create_cfg()
        cfg.MODEL.HORIZON, cfg.MODEL.DIM, cfg.MODEL.DIM_MULTS = H, dim, list(mults)
        cfg.TRAIN.USE_COND = cfg.GUIDANCE.USE_COND = name
        m = build_model(cfg)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 / p[0].numel() ** 0.5 if p.dim() > 1 else 0.1))
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        m = m.to(DEV).eval()
        m.perception.forward = lambda img: feat.to(DEV)   # test-only stub of the encoder output
        cond = d["target"] if name == "FREE_GUIDANCE" else None
        with torch.no_grad():
            y = m(d["trajs"].to(DEV), d["imgs"].to(DEV), d["t"].to(DEV), cond=None if cond is None else cond.to(DEV)).cpu()
        want = U.unet_forward(sd, d["trajs"], None, d["t"], cond, use_cond=name, dim=dim, dim_mults=mults, img_feature=feat)
        close(y, want, 2e-5)
    if dim % 32 != 0 or H < 16:
        # such a model samples but does not train (the backward kernels tile like the MFMA forward kernels): said, not crashed
        m.train()
        m.perception.forward = lambda img: feat.to(DEV).requires_grad_()
        with pytest.raises(ValueError, match="sampling only"):
            m(d["trajs"].to(DEV), d["imgs"].to(DEV), d["t"].to(DEV), cond=None if cond is None else cond.to(DEV))


def test_levels_layer_by_layer_vs_oracle():
    """csrc/tconv_chain.hip runs the 64/128-channel levels (two residual blocks + down / up conv, + final_conv) as one launch
    each, and every other test in this file goes through it.  ADX_UNET_CHAIN=0 (read once per process, hence a process of its
    own) sends those levels through the per-layer kernels again -- the path ragged horizons, exact-fp32 mode and wider models
    still take -- and it must compute the same forward (modeling/temporal.py:197-245)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # ADX_UNET_PIPE=0: the deepest level's seven same-shaped convs as launches instead of the one pipeline launch the small
    # batches at H = 16 take by default (csrc/tconv_pipe.hip); the worker's (2, 16) and (5, 16) cases cross that switch
    for switch in ("ADX_UNET_CHAIN", "ADX_UNET_PIPE"):
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "chain_worker.py")], env=dict(os.environ, **{switch: "0"}),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        cases = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("CASE")]
        assert len(cases) == 4, r.stdout
        for _, name, rows, H, err in cases:
            assert float(err) <= 2e-5, (switch, name, rows, H, err)


@pytest.mark.parametrize("use_cond,rows", [("NO_GUIDANCE", 1), ("FREE_GUIDANCE", 2), ("NO_GUIDANCE", 3), ("FREE_GUIDANCE", 8),
                                           ("CLASSIFIER_GUIDANCE", 4), ("NO_GUIDANCE", 5), ("NO_GUIDANCE", 9)])
def test_pipeline_launch_of_the_deepest_level_vs_oracle(use_cond, rows):
    """csrc/tconv_pipe.hip: at MODEL.HORIZON = 16 (two positions at the deepest level) and up to 5 rows, block 0's second conv,
    block 1 and both mid blocks -- seven Conv1d(512, 512, 5) + GroupNorm + Mish -- run as ONE launch: 7 x 32 workgroups that
    hand raw conv sums on through memory, the consumer applying GroupNorm / Mish / time bias / residual.  Whole forwards against
    the oracle for every row count the launch takes (6 rows and more do not fit its LDS: back on the launch chain, which the
    layout export must say), twice each (a second call must not depend on the first one's counters), modeling/temporal.py:197-245."""
    from helpers import pipe_layout
    m, _ = make_model(use_cond, 16)
    d = P.synthetic_batch(rows, 16, image_hw=(32, 32), seed=90 + rows)
    feat = P._uniform("pipe.feat", 90 + rows, (rows, 64), -3.0, 3.0)
    m.perception.forward = lambda img, f=feat: f.to(DEV)
    cond = d["target"] if use_cond == "FREE_GUIDANCE" else None
    kw = dict(cond=cond.to(DEV)) if cond is not None else {}
    if use_cond == "CLASSIFIER_GUIDANCE":
        kw["return_action_and_time_only"] = True
    want = U.unet_forward(oracle_sd(use_cond), d["trajs"], None, d["t"], cond, use_cond=use_cond, img_feature=feat)
    outs = []
    with torch.no_grad():
        for _ in range(2):
            y = m(d["trajs"].to(DEV), d["imgs"].to(DEV), d["t"].to(DEV), **kw)
            outs.append((y[0] if isinstance(y, tuple) else y).cpu())
    assert torch.equal(outs[0], outs[1])
    assert pipe_layout(m._native(), rows)["runs"] == (1 if rows <= 5 else 0), rows     # the path this test is named after ran
    w = want if want.shape[-1] == outs[0].shape[-1] else want[..., -outs[0].shape[-1]:]
    close(outs[0], w, 2e-5)


@pytest.mark.parametrize("use_cond,B,H,dims", [("FREE_GUIDANCE", 1, 16, None), ("NO_GUIDANCE", 64, 32, None),
                                                ("NO_GUIDANCE", 2, 16, (64, (1, 2)))])
def test_forward_does_not_depend_on_what_the_workspace_held(use_cond, B, H, dims):
    """adx_unet_forward clears the ticket words of its split reductions itself (the first 256 words of the caller's
    workspace): a workspace full of garbage -- uninitialised memory of a C-ABI caller, the debris of a launch that never
    finished -- gives the same bits as a zero-filled one, on the path that opens with a chained level (precomputed
    conditioning), on the path that opens with the embedding kernel, and on a model without chained first level."""
    from autonomous_driving_with_diffusion_model_amd import _lib as L
    if dims is None:
        m, _ = make_model(use_cond, H)
    else:
        from autonomous_driving_with_diffusion_model_amd.config import create_cfg
        from autonomous_driving_with_diffusion_model_amd.modeling import build_model
        cfg = create_cfg()
        cfg.MODEL.HORIZON, cfg.MODEL.DIM, cfg.MODEL.DIM_MULTS = H, dims[0], dims[1]
        m = build_model(cfg)
        P.load_procedural(m, 0)
        m = m.to(DEV).eval()
    d = {k: v.to(DEV) for k, v in P.synthetic_batch(B, H, image_hw=IMG_SMALL, seed=77).items()}
    free = use_cond == "FREE_GUIDANCE"
    cond = torch.cat([d["target"], torch.zeros_like(d["target"])], 0) if free else None
    rows = 2 * B if free else B
    x = torch.cat([d["init_trajs"]] * 2, 0) if free else d["init_trajs"]
    ts = torch.tensor([40], dtype=torch.int64, device=DEV)
    t = ts if free else ts.repeat(B)
    with torch.no_grad():
        tc = m.time_conditioning(d["imgs"], ts, cond=cond, rows=rows)
        want_tc, want = m(x, None, None, time_cond=(tc, 0)), m(x, d["imgs"], t, cond=cond)
        nbytes = L.lib().adx_unet_workspace_bytes(m._native(), rows)
        for fill in (0xFF, 0x01, 0x5A):
            m._ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
            assert torch.equal(m(x, None, None, time_cond=(tc, 0)), want_tc), hex(fill)
            m._ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
            assert torch.equal(m(x, d["imgs"], t, cond=cond), want), hex(fill)


def test_check_range_mode_names_the_first_layer_that_leaves_the_fp16_range():
    """ADX_CHECK_RANGE=1 (read once per process, so a process of its own): the split-fp16 perception kernels turn a forward
    activation of |x| >= 65504 into inf and carry it on; in this mode the pass fails with the first tensor that left the range
    instead.  Procedural weights pass; the same model with one BatchNorm scale multiplied by 1e6 fails and names the block."""
    import subprocess
    import sys
    code = r'''
import sys, torch
sys.path.insert(0, "tests")
from test_gpu_model import make_model, P, IMG_SMALL, DEV
from autonomous_driving_with_diffusion_model_amd._lib import AdxError
m, _ = make_model("NO_GUIDANCE", 16)
img = P.synthetic_batch(2, 16, image_hw=IMG_SMALL, seed=3)["imgs"].to(DEV)
with torch.no_grad():
    f = m.perception(img)
    assert bool(torch.isfinite(f).all())
    dict(m.named_parameters())["perception.layer2.1.bn1.weight"].mul_(1e6)
    m.refresh_weights()
    try:
        m.perception(img)
    except AdxError as e:
        assert "BasicBlock 4" in str(e) and "65504" in str(e), str(e)
        print("RANGE_OK")
    else:
        raise SystemExit("no range error")
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, ADX_CHECK_RANGE="1"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "RANGE_OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
