#!/usr/bin/env python3
"""Generate tests/golden/attn.npz: the REAL reference with MODEL.USE_ATTN = True.

Same setup as make_golden.py (imported from it: fake `diffusers`, resnet34(pretrained=False), procedural weights and
inputs); only USE_ATTN, DIM_MULTS, HORIZON (and for (c) the guidance) differ.  The reference's forward runs with
attention only where every DIM_MULTS entry is equal (each up level applies LinearAttention(dim_out) to dim_in channels).
Usage:  python tests/golden/make_golden_attn.py

  (a) NO_GUIDANCE, (2, 2, 2), H = 16      (b) FREE_GUIDANCE, (1, 1, 1), H = 32 (the CFG call shape included)
  (c) CLASSIFIER_GUIDANCE, D = 7, (1, 1), H = 16      (d) NO_GUIDANCE, (1, 1, 1, 1), H = 24 (a ragged horizon)

For each: the state-dict keys and shapes, a UNet forward and a 10-step DDIM loop ((c): a 2-step classifier-guided loop).
For (a) and (b) one training step: the loss, the norm of every temporal-stack gradient and the whole gradient of every
tensor of at most 1024 elements (biases, norm affines, final_conv.1).  Also whether the reference's forward raises at
(1, 2, 4, 8).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402  (installs the fake diffusers, patches resnet34, puts the reference on sys.path)

P, MT, RS = MG.P, MG.MT, MG.RS
GuidanceType = MG.GuidanceType
IMG_SMALL, SCHED_KW = MG.IMG_SMALL, MG.SCHED_KW

CASES = {
    "a": ("NO_GUIDANCE", 7, (2, 2, 2), 16),
    "b": ("FREE_GUIDANCE", 7, (1, 1, 1), 32),
    "c": ("CLASSIFIER_GUIDANCE", 7, (1, 1), 16),
    "d": ("NO_GUIDANCE", 7, (1, 1, 1, 1), 24),
}
FULL_GRAD_MAX = 1024

out = {}


def put(name, t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    out[name] = np.asarray(t)


def make_cfg(use_cond, horizon, mults):
    cfg = MG.make_cfg(use_cond, horizon)
    cfg.MODEL.USE_ATTN = True
    cfg.MODEL.DIM_MULTS = tuple(mults)
    return cfg


def ref_model(case, seed=0):
    use_cond, _, mults, H = CASES[case]
    m = MT.build_model(make_cfg(use_cond, H, mults))
    P.load_procedural(m, seed)
    return m.eval()


def gen_case(case):
    use_cond, D, mults, H = CASES[case]
    m = ref_model(case)
    sd = m.state_dict()
    put(f"{case}.keys", np.array(list(sd.keys())))
    put(f"{case}.shapes", np.array([",".join(map(str, v.shape)) for v in sd.values()]))
    data = P.synthetic_batch(2, H, D, image_hw=IMG_SMALL, seed=11)
    t = torch.tensor([90, 3], dtype=torch.int64)
    with torch.no_grad():
        if use_cond == "FREE_GUIDANCE":
            put(f"{case}.unet.cond", m(data["trajs"], data["imgs"], t, cond=data["target"]))
            x2 = torch.cat([data["trajs"], data["trajs"]], 0)
            c2 = torch.cat([data["target"], torch.zeros_like(data["target"])], 0)
            put(f"{case}.unet.cfg", m(x2, data["imgs"], t[:1], cond=c2))
        else:
            put(f"{case}.unet", m(data["trajs"], data["imgs"], t))
    loop = P.synthetic_batch(1, H, D, image_hw=IMG_SMALL, seed=31)
    cfg = make_cfg(use_cond, H, mults)
    sch = RS.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
    if use_cond == "CLASSIFIER_GUIDANCE":
        with torch.enable_grad():
            r = MG.drive_generate_traj(m, sch, cfg, loop["imgs"], loop["target"][0], loop["init_trajs"], 2,
                                       GuidanceType.CLASSIFIER_GUIDANCE)
    else:
        tg = None if use_cond == "NO_GUIDANCE" else loop["target"][0]
        with torch.no_grad():
            r = MG.drive_generate_traj(m, sch, cfg, loop["imgs"], tg, loop["init_trajs"], 10, GuidanceType[use_cond])
    put(f"{case}.loop", r)


def gen_train(case):
    use_cond, D, mults, H = CASES[case]
    data = P.synthetic_batch(2, H, D, image_hw=IMG_SMALL, seed=41)
    sch = MG.DB.DDPMScheduler(**SCHED_KW)
    m = ref_model(case).train()
    noisy = sch.add_noise(data["trajs"], data["noise"], data["t"])
    noisy[..., 0, :3] = 0
    cond = data["target"] if use_cond == "FREE_GUIDANCE" else None
    pred = m(noisy, data["imgs"], data["t"], cond=cond)
    loss = torch.nn.functional.mse_loss(pred.float(), data["trajs"].float())
    loss.backward()
    put(f"{case}.train.loss", loss)
    for k, p in m.named_parameters():
        if k.startswith("perception."):
            continue
        put(f"{case}.train.gradnorm.{k}", p.grad.norm())
        if p.numel() <= FULL_GRAD_MAX:
            put(f"{case}.train.gradfull.{k}", p.grad)


def gen_refusal():
    """The reference's own forward with attention at the default (1, 2, 4, 8): it raises (up level 0 applies
    LinearAttention(512) to 256 channels)."""
    cfg = make_cfg("NO_GUIDANCE", 16, (1, 2, 4, 8))
    m = MT.build_model(cfg).eval()
    data = P.synthetic_batch(1, 16, 7, image_hw=IMG_SMALL, seed=11)
    try:
        with torch.no_grad():
            m(data["trajs"], data["imgs"], torch.tensor([5]))
        put("raises.1248", np.array(0))
    except RuntimeError as e:
        put("raises.1248", np.array(1))
        put("raises.1248.message", np.array(str(e).splitlines()[0]))


if __name__ == "__main__":
    for c in CASES:
        gen_case(c)
    for c in ("a", "b"):
        gen_train(c)
    gen_refusal()
    path = os.path.join(MG.HERE, "attn.npz")
    np.savez_compressed(path, **out)
    print(f"attn: {len(out)} arrays -> {path} ({os.path.getsize(path) / 1024:.1f} KiB)")
