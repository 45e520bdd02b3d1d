#!/usr/bin/env python3
"""Generate tests/golden/dims.npz: the REAL reference at trajectory widths (MODEL.TRANSITION_DIM) other than 7.

Same setup as make_golden.py (imported from it: fake `diffusers`, resnet34(pretrained=False), procedural weights and
inputs); only cfg.MODEL.TRANSITION_DIM differs.  Usage:  python tests/golden/make_golden_dims.py

  * D in {2, 3}, NO and FREE guidance: UNet forwards at H = 16 / 32 (the CFG call shape included) and a 10-step DDIM loop;
    for D = 2 one NO_GUIDANCE training step (loss, gradient norms, whole final_conv.1 / first-conv gradients).
  * D in {4, 5, 8}, CLASSIFIER guidance (state width D - 3): state_pred forward and d/d(action), the TargetGuidance +
    GuidanceLoss output on both branches of its rule (near / far, and `mid`: a target
    beside a row of x inside the horizon), and a 5-step classifier-guided DDIM loop.  At D = 4 the
    state is one column wide, so x[..., 1] is action column 0; two more cases pin the chosen row h* to 0 and to T there.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402  (installs the fake diffusers, patches resnet34, puts the reference on sys.path)

P, MT, RS = MG.P, MG.MT, MG.RS
GuidanceType, GuidanceLoss, TargetGuidance = MG.GuidanceType, MG.GuidanceLoss, MG.TargetGuidance
IMG_SMALL, SCHED_KW = MG.IMG_SMALL, MG.SCHED_KW

out = {}


def put(name, t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    out[name] = np.asarray(t)


def make_cfg(use_cond, horizon, D):
    cfg = MG.make_cfg(use_cond, horizon)
    cfg.MODEL.TRANSITION_DIM = D
    return cfg


def ref_model(use_cond, horizon, D, seed=0):
    m = MT.build_model(make_cfg(use_cond, horizon, D))
    P.load_procedural(m, seed)
    return m.eval()


def choose_row(xg, tgt):
    """TargetGuidance's h* for one sample (control/guidance_loss.py:14-20)."""
    x = xg[0, :, :2]
    if torch.norm(x[-1] - x[0]) < torch.norm(tgt - x[0]):
        return 0
    return int(torch.sum((x - tgt) ** 2, dim=-1).argmin())


def gen_unet_loops():
    for D in (2, 3):
        for H in (16, 32):
            data = P.synthetic_batch(2, H, D, image_hw=IMG_SMALL, seed=11)
            t = torch.tensor([90, 3], dtype=torch.int64)
            with torch.no_grad():
                m = ref_model("NO_GUIDANCE", H, D)
                put(f"d{D}.unet.no.h{H}", m(data["trajs"], data["imgs"], t))
                m = ref_model("FREE_GUIDANCE", H, D)
                put(f"d{D}.unet.free.h{H}.cond", m(data["trajs"], data["imgs"], t, cond=data["target"]))
                x2 = torch.cat([data["trajs"], data["trajs"]], 0)
                c2 = torch.cat([data["target"], torch.zeros_like(data["target"])], 0)
                put(f"d{D}.unet.free.h{H}.cfg", m(x2, data["imgs"], t[:1], cond=c2))
        data = P.synthetic_batch(1, 16, D, image_hw=IMG_SMALL, seed=31)
        for name in ("NO_GUIDANCE", "FREE_GUIDANCE"):
            cfg = make_cfg(name, 16, D)
            m = ref_model(name, 16, D)
            sch = RS.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
            tg = None if name == "NO_GUIDANCE" else data["target"][0]
            with torch.no_grad():
                r = MG.drive_generate_traj(m, sch, cfg, data["imgs"], tg, data["init_trajs"], 10, GuidanceType[name])
            put(f"d{D}.loop.ddim.{name}", r)


def gen_train():
    D = 2
    data = P.synthetic_batch(2, 16, D, image_hw=IMG_SMALL, seed=41)
    sch = MG.DB.DDPMScheduler(**SCHED_KW)
    m = ref_model("NO_GUIDANCE", 16, D).train()
    noisy = sch.add_noise(data["trajs"], data["noise"], data["t"])
    noisy[..., 0, :3] = 0
    pred = m(noisy, data["imgs"], data["t"])
    loss = torch.nn.functional.mse_loss(pred.float(), data["trajs"].float())
    loss.backward()
    put("d2.train.loss", loss)
    named = dict(m.named_parameters())
    for k in ("perception.conv1.weight", "perception.fc.weight", "time_mlp.1.weight", "downs.0.0.blocks.0.block.0.weight",
              "downs.0.0.residual_conv.weight", "mid_block1.time_mlp.1.weight", "ups.2.3.conv.weight",
              "final_conv.0.block.0.weight", "final_conv.1.weight"):
        put(f"d2.train.gradnorm.{k}", named[k].grad.norm())
    for k in ("final_conv.1.weight", "final_conv.1.bias", "downs.0.0.blocks.0.block.0.weight", "downs.0.0.residual_conv.weight"):
        put(f"d2.train.gradfull.{k}", named[k].grad)


def gen_classifier():
    g = lambda n, s: P._uniform(n, 7, s, -1.0, 1.0)  # noqa: E731
    std = torch.tensor(1.5582221)
    for D in (4, 5, 8):
        od = D - 3
        m = ref_model("CLASSIFIER_GUIDANCE", 16, D)
        a = g("dims.action", (2, 15, 3)).requires_grad_()
        te = g("dims.te", (2, 64))
        s = m.state_pred(a, te)
        put(f"d{D}.traj_predict", s)
        (ga,) = torch.autograd.grad((s * g(f"dims.traj_w{od}", (2, 15, od))).sum(), [a])
        put(f"d{D}.traj_predict_dact", ga)
        gl = GuidanceLoss(make_cfg("CLASSIFIER_GUIDANCE", 16, D))
        te1 = g("dims.g_te", (1, 64))
        cases = [("near", g("dims.g_action.near", (1, 16, 3)), torch.tensor([0.05, -0.02])),
                 ("far", g("dims.g_action.far", (1, 16, 3)), torch.tensor([0.9, 0.7]))]
        if D == 4:
            # x[..., 1] = action[..., 0]: a ramp in it, the target beyond its far end (h* = T) / behind the start (h* = 0)
            ramp = torch.linspace(-0.9, 0.9, 16)
            a_ramp = g("dims.g_action.ramp", (1, 16, 3)) * 0.1
            a_ramp[0, :, 0] = ramp
            cases += [("hT", a_ramp, None), ("h0", a_ramp, None)]
        cases.append(("mid", g("dims.g_action.mid", (1, 16, 3)), None))
        for tag, a1, tgt in cases:
            a1 = a1.clone().requires_grad_()
            st = m.state_pred(a1[:, :-1], te1)
            st = torch.cat([torch.zeros_like(st[:, :1]), st], dim=1)
            xg = torch.cat([st, a1], dim=-1)
            if tag in ("hT", "h0"):
                want = 15 if tag == "hT" else 0
                # hT: a little inside x[T] = (state[T, 0], 0.9), so x[T] stays the nearest row, the target is no farther
                # from x[0] than x[T] is (the argmin branch) and the loss is not zero; h0: beyond x[0] = (0, -0.9)
                cands = [torch.tensor([x0, y0]) for y0 in ((0.87, 0.85, 0.8) if want else (-0.95, -1.0))
                         for x0 in (float(xg.detach()[0, -1 if want else 0, 0]), 0.0, 0.3, -0.3)]
                tgt = next(c for c in cands if choose_row(xg.detach(), c) == want)
                assert float(TargetGuidance()(xg.detach(), tgt)) > 1e-4, tag      # a zero loss would leave g_x = 0
                put(f"d{D}.g_target.{tag}", tgt)
            if tag == "mid":      # beside a row of x inside the horizon: the argmin branch, gradient through state_pred
                x = xg.detach()[0, :, :2]
                r = torch.norm(x[-1] - x[0])       # a target no farther from x[0] than x[T] is: the argmin branch
                grid = [x[0] + f * r * torch.tensor([np.cos(th), np.sin(th)], dtype=torch.float32)
                        for f in (0.5, 0.7, 0.3, 0.9) for th in np.linspace(0, 2 * np.pi, 24, endpoint=False)]
                tgt = next(c for c in grid if choose_row(xg.detach(), c) not in (0, 15))
                put(f"d{D}.g_target.{tag}", tgt)
            put(f"d{D}.g_hstar.{tag}", np.array(choose_row(xg.detach(), tgt)))
            put(f"d{D}.target_loss.{tag}", TargetGuidance()(xg, tgt))
            put(f"d{D}.guidance_loss.{tag}", gl(xg, a1, tgt, std))
        data = P.synthetic_batch(1, 16, D, image_hw=IMG_SMALL, seed=31)
        cfg = make_cfg("CLASSIFIER_GUIDANCE", 16, D)
        sch = RS.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
        with torch.enable_grad():
            r = MG.drive_generate_traj(m, sch, cfg, data["imgs"], data["target"][0], data["init_trajs"], 5,
                                       GuidanceType.CLASSIFIER_GUIDANCE)
        put(f"d{D}.loop.ddim.CLASSIFIER_GUIDANCE", r)


if __name__ == "__main__":
    gen_unet_loops()
    gen_train()
    gen_classifier()
    path = os.path.join(MG.HERE, "dims.npz")
    np.savez_compressed(path, **out)
    print(f"dims: {len(out)} arrays -> {path} ({os.path.getsize(path) / 1024:.1f} KiB)")
