"""GPU: MODEL.USE_ATTN (the LayerNorm + LinearAttention block, csrc/attn.hip) -- the kernels in isolation against fp64
torch autograd, the model against the real reference (tests/golden/attn.npz) and the fp64 restatement
(tests/attn_ref.py), sampling loops eager and as a graph, training against fp64 autograd, checkpoint, refusals."""
import pytest
import torch
import torch.nn.functional as F

from oracle import sampling as OS
from autonomous_driving_with_diffusion_model_amd import _lib as L
from autonomous_driving_with_diffusion_model_amd.modeling.spec import unet_entries
from autonomous_driving_with_diffusion_model_amd.utils import procedural as P
import attn_ref as AR
from helpers import IMG_SMALL, SCHED_KW, close, close_traj

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAJ_TOL = 1e-4
CASES = {
    "a": ("NO_GUIDANCE", 7, (2, 2, 2), 16),
    "b": ("FREE_GUIDANCE", 7, (1, 1, 1), 32),
    "c": ("CLASSIFIER_GUIDANCE", 7, (1, 1), 16),
    "d": ("NO_GUIDANCE", 7, (1, 1, 1, 1), 24),
}


def _rand(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale + shift)


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / (b.double().cpu().norm() + 1e-300)).item()


# ---- kernels in isolation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 128, 512])
@pytest.mark.parametrize("Lp,Lv", [(1, 1), (2, 2), (8, 8), (16, 16), (64, 64), (32, 24)])
def test_chan_layernorm_kernels(C, Lp, Lv):
    B = 3
    lib, s = L.lib(), L.stream_ptr(torch.device(DEV))
    # x as a strided view: a wider buffer's first Lp positions (the executor hands in such views)
    xb = _rand((B, C, Lp + 3), 1, 1.5, 0.3)
    x64 = xb[:, :, :Lp].clone()
    g64, b64 = _rand((C,), 2, 0.1, 1.0), _rand((C,), 3, 0.1)
    dy64 = _rand((B, C, Lp), 4)
    xd = xb.float().to(DEV)
    g, b = g64.float().to(DEV), b64.float().to(DEV)
    xn = torch.full((B, C, Lp), float("nan"), device=DEV)
    mean = torch.empty((B, Lp), device=DEV)
    rstd = torch.empty((B, Lp), device=DEV)
    sb, sc, sl = xd.stride()
    L.check(lib.adx_chan_layernorm_forward(xd.data_ptr(), sb, sc, sl, g.data_ptr(), b.data_ptr(), xn.data_ptr(), mean.data_ptr(),
                                           rstd.data_ptr(), B, C, Lp, Lv, s), "ln fwd")
    xv = x64[:, :, :Lv].clone().requires_grad_()
    gv, bv = g64.clone().requires_grad_(), b64.clone().requires_grad_()
    want = AR.chan_layernorm(xv, gv, bv)
    torch.cuda.synchronize()
    close(xn[:, :, :Lv].cpu(), want.detach(), 2e-5)
    assert torch.all(xn[:, :, Lv:] == 0)
    want.backward(dy64[:, :, :Lv])
    dy = dy64.float().to(DEV)
    pre = _rand((B, C, Lp), 5).float().to(DEV)
    for acc in (0, 1):
        dx = pre.clone() if acc else torch.full((B, C, Lp), float("nan"), device=DEV)
        dg = torch.full((C,), float("nan"), device=DEV)
        db = torch.full((C,), float("nan"), device=DEV)
        L.check(lib.adx_chan_layernorm_backward(dy.data_ptr(), xd.data_ptr(), sb, sc, sl, mean.data_ptr(), rstd.data_ptr(),
                                                g.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), B, C, Lp, Lv, acc, s),
                "ln bwd")
        torch.cuda.synchronize()
        got = dx.cpu() - (pre.cpu() if acc else 0)
        assert _rel(got[:, :, :Lv], xv.grad) <= 1e-5
        if not acc:
            assert torch.all(dx[:, :, Lv:] == 0)
        else:
            assert torch.equal(dx[:, :, Lv:], pre[:, :, Lv:])
        assert _rel(dg, gv.grad) <= 1e-5 and _rel(db, bv.grad) <= 1e-5


@pytest.mark.parametrize("Lp,Lv", [(1, 1), (2, 2), (8, 8), (16, 16), (64, 64), (32, 24), (8, 3)])
def test_linattn_core_kernels(Lp, Lv):
    B = 3
    lib, s = L.lib(), L.stream_ptr(torch.device(DEV))
    qkv64 = _rand((B, 384, Lp), 6, 1.2)
    do64 = _rand((B, 128, Lp), 7)
    qkv = qkv64.float().to(DEV)
    o = torch.full((B, 128, Lp), float("nan"), device=DEV)
    L.check(lib.adx_linattn_forward(qkv.data_ptr(), o.data_ptr(), B, Lp, Lv, s), "core fwd")
    qv = qkv64[:, :, :Lv].clone().requires_grad_()
    want = AR.linattn_core(qv)
    torch.cuda.synchronize()
    close(o[:, :, :Lv].cpu(), want.detach(), 2e-5 * max(1.0, want.abs().max().item()))
    assert torch.all(o[:, :, Lv:] == 0)
    want.backward(do64[:, :, :Lv])
    do = do64.float().to(DEV)
    dqkv = torch.full((B, 384, Lp), float("nan"), device=DEV)
    L.check(lib.adx_linattn_backward(qkv.data_ptr(), do.data_ptr(), dqkv.data_ptr(), B, Lp, Lv, s), "core bwd")
    torch.cuda.synchronize()
    for part in range(3):           # q, k (through the softmax), v
        sl = slice(128 * part, 128 * (part + 1))
        assert _rel(dqkv[:, sl, :Lv], qv.grad[:, sl]) <= 1e-5, part
    assert torch.all(dqkv[:, :, Lv:] == 0)


# ---- the model ------------------------------------------------------------------------------------------------------------
def make_model(case, seed=0, dim=64):
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    from autonomous_driving_with_diffusion_model_amd.modeling import build_model
    use_cond, D, mults, H = CASES[case]
    cfg = create_cfg()
    cfg.MODEL.HORIZON, cfg.MODEL.TRANSITION_DIM, cfg.MODEL.DIM_MULTS, cfg.MODEL.USE_ATTN = H, D, mults, True
    cfg.MODEL.DIM = dim
    cfg.TRAIN.USE_COND = cfg.GUIDANCE.USE_COND = use_cond
    cfg.GUIDANCE.FREE_SCALE, cfg.GUIDANCE.CLASSIFIER_SCALE = 7.5, 15.0
    if use_cond == "CLASSIFIER_GUIDANCE":
        cfg.GUIDANCE.LOSS_LIST = [["TargetGuidance", []]]
    m = build_model(cfg)
    P.load_procedural(m, seed)
    return m.to(DEV).eval(), cfg


def entries(case):
    use_cond, D, mults, _ = CASES[case]
    return unet_entries(use_cond, D, 64, mults, attention=True)


def sd_of(case, seed=0):
    return P.procedural_state_dict(((e.key, e.shape) for e in entries(case)), seed)


def _sched(cfg):
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    return S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)


def _gpu(d):
    return {k: v.to(DEV) for k, v in d.items()}


def _sd64(case):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd_of(case).items()}


@pytest.mark.parametrize("case", list(CASES))
def test_unet_forward(golden, case):
    """Forwards against the reference (the UNet bar, 2e-5) and against the fp64 restatement."""
    g = golden("attn")
    use_cond, D, mults, H = CASES[case]
    d = P.synthetic_batch(2, H, D, image_hw=IMG_SMALL, seed=11)
    dg = _gpu(d)
    t = torch.tensor([90, 3], dtype=torch.int64)
    m, _ = make_model(case)
    sd64, c64 = _sd64(case), (lambda v: v.double())
    kw = dict(use_cond=use_cond, dim_mults=mults)
    with torch.no_grad():
        if use_cond == "FREE_GUIDANCE":
            got = m(dg["trajs"], dg["imgs"], t.to(DEV), cond=dg["target"]).cpu()
            close(got, g[f"{case}.unet.cond"], 2e-5)
            close(got, AR.unet_forward(sd64, c64(d["trajs"]), c64(d["imgs"]), t, c64(d["target"]), **kw), 2e-5)
            x2 = torch.cat([dg["trajs"], dg["trajs"]], 0)
            c2 = torch.cat([dg["target"], torch.zeros_like(dg["target"])], 0)
            close(m(x2, dg["imgs"], t[:1].to(DEV), cond=c2).cpu(), g[f"{case}.unet.cfg"], 2e-5)
        else:
            got = m(dg["trajs"], dg["imgs"], t.to(DEV)).cpu()
            close(got, g[f"{case}.unet"], 2e-5)
            close(got, AR.unet_forward(sd64, c64(d["trajs"]), c64(d["imgs"]), t, **kw), 2e-5)


@pytest.mark.parametrize("case", list(CASES))
def test_loops_eager_and_graph(golden, case):
    """10-step DDIM loops ((c): 2-step classifier-guided) against the reference; GraphedSampler replays the eager loop
    bit for bit."""
    from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler, generate_traj
    want = golden("attn")[f"{case}.loop"]
    use_cond, D, mults, H = CASES[case]
    d = _gpu(P.synthetic_batch(1, H, D, image_hw=IMG_SMALL, seed=31))
    m, cfg = make_model(case)
    cfg.EVAL.SAMPLE_STEPS = 2 if use_cond == "CLASSIFIER_GUIDANCE" else 10
    tgt = None if use_cond == "NO_GUIDANCE" else d["target"][0]
    eager = generate_traj(m, _sched(cfg), cfg, d["imgs"], tgt, d["init_trajs"])
    close_traj(eager.cpu(), want, TRAJ_TOL)
    gs = GraphedSampler(m, _sched(cfg), cfg)
    for _ in range(2):       # capture, then replay
        assert torch.equal(gs(d["imgs"], tgt, d["init_trajs"]), eager)


def _train_step(case, seed=41):
    """One training step (B = 2): loss and every parameter gradient against fp64 autograd of the restatement."""
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    use_cond, D, mults, H = CASES[case]
    m, _ = make_model(case)
    m.train()
    d = _gpu(P.synthetic_batch(2, H, D, image_hw=IMG_SMALL, seed=seed))
    noisy = S.DDPMScheduler(**SCHED_KW).add_noise(d["trajs"], d["noise"], d["t"], zero_first=True)
    cond = d["target"] if use_cond == "FREE_GUIDANCE" else None
    loss = F.mse_loss(m(noisy, d["imgs"], d["t"], cond=cond), d["trajs"])
    loss.backward()
    named = dict(m.named_parameters())
    pkeys = [e.key for e in entries(case) if not e.is_buffer]
    dc = {k: v.cpu() for k, v in d.items()}
    sd64 = {k: (v.requires_grad_(k in pkeys) if v.is_floating_point() else v) for k, v in _sd64(case).items()}
    c64 = lambda t: t.double() if t.is_floating_point() else t  # noqa: E731
    with AR.with_attention():
        loss64 = OS.training_loss(sd64, c64(dc["imgs"]), c64(dc["trajs"]), c64(dc["target"]), dc["t"], c64(dc["noise"]),
                                  use_cond=use_cond, dim_mults=mults)
    loss64.backward()
    assert abs(loss.item() - loss64.item()) <= 2e-5 * max(1.0, abs(loss64.item()))
    n_attn = 0
    for k in pkeys:
        e = _rel(named[k].grad.detach(), sd64[k].grad)
        assert e <= (3e-2 if k.startswith("perception.") else 1e-3), (k, e)
        n_attn += ".2.fn." in k or k.startswith("mid_attn.")
    assert n_attn == 5 * 2 * len(mults)
    return m, d, loss


@pytest.mark.parametrize("case", ["a", "b"])
def test_training_step(golden, case):
    g = golden("attn")
    m, _, loss = _train_step(case)
    assert abs(loss.item() - float(g[f"{case}.train.loss"])) < 2e-5
    named = dict(m.named_parameters())
    for k in g.files:
        if k.startswith(f"{case}.train.gradnorm."):
            ref, got = float(g[k]), named[k[len(f"{case}.train.gradnorm."):]].grad.norm().item()
            assert abs(got - ref) <= 2e-3 * max(1.0, abs(ref)), (k, got, ref)
        if k.startswith(f"{case}.train.gradfull."):
            ref = torch.from_numpy(g[k])
            got = named[k[len(f"{case}.train.gradfull."):]].grad.cpu()
            assert ((got - ref).norm() / (ref.norm() + 1e-30)).item() <= 1e-3, k


def test_ragged_horizon_training_step():
    """H = 24 runs on 32 (and 16) positions: the softmax, the context and the gradients cover the 24 (12) real ones.  Two
    levels: at four, the deepest level's GroupNorm groups (8 channels x 3 positions) are sampling-only."""
    CASES["e"] = ("NO_GUIDANCE", 7, (1, 1), 24)
    try:
        _train_step("e", seed=43)
    finally:
        del CASES["e"]


def test_checkpoint_and_optimizer_step(golden, tmp_path):
    """A state dict in the reference's key order loads; one optimizer step; a checkpoint round trip."""
    from autonomous_driving_with_diffusion_model_amd.checkpoint import load_checkpoint, save_checkpoint
    from autonomous_driving_with_diffusion_model_amd.optim import FusedAdamWEMA
    g = golden("attn")
    m, d, _ = _train_step("a")
    ref_sd = {k: v for k, v in sd_of("a", seed=9).items()}
    assert list(ref_sd.keys()) == list(g["a.keys"])
    m2, _ = make_model("a", seed=5)
    m2.load_state_dict(ref_sd)
    assert all(torch.equal(v.cpu(), ref_sd[k]) for k, v in m2.state_dict().items())
    opt = FusedAdamWEMA(m.parameters())
    before = m.state_dict()["mid_attn.fn.fn.to_qkv.weight"].clone()
    opt.step()
    assert not torch.equal(m.state_dict()["mid_attn.fn.fn.to_qkv.weight"], before)
    path = str(tmp_path / "checkpoint_attn.pth")
    save_checkpoint(path, m, opt, iteration=1)
    load_checkpoint(path, m2, use_ema=False)
    sd1, sd2 = m.state_dict(), m2.state_dict()
    assert sd1.keys() == sd2.keys() and all(torch.equal(sd1[k].cpu(), sd2[k].cpu()) for k in sd1)
    m.eval()
    m2.eval()
    with torch.no_grad():      # the re-packed weights of both models compute the same forward
        assert torch.equal(m(d["trajs"], d["imgs"], d["t"]), m2(d["trajs"], d["imgs"], d["t"]))


def test_refusals():
    from autonomous_driving_with_diffusion_model_amd.misc.constant import GuidanceType
    from autonomous_driving_with_diffusion_model_amd.modeling.temporal import TemporalMapUnet
    with pytest.raises(NotImplementedError, match="DIM_MULTS"):
        TemporalMapUnet(16, 7, attention=True, dim=64, dim_mults=(1, 2, 4, 8), use_cond=GuidanceType.NO_GUIDANCE)
    # GroupNorm groups of 6 channels (DIM = 48): samples, does not train
    m, _ = make_model("a", dim=48)
    d = _gpu(P.synthetic_batch(1, 16, 7, image_hw=IMG_SMALL, seed=3))
    with torch.no_grad():
        y = m(d["trajs"], d["imgs"], d["t"])
    assert y.shape == (1, 16, 7) and torch.isfinite(y).all()
    m.train()
    with pytest.raises(ValueError, match="sampling only"):
        m(d["trajs"], d["imgs"], d["t"])
