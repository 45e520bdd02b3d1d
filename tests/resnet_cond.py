"""Test infrastructure: a ResNet-34 training forward in fp64 CONDITIONED on given discrete decisions, and the decoders of what
the native training forward keeps on its tape (csrc/resnet_train.hip, adx_resnet_tape_describe).

With batch-statistics BatchNorm the training gradients are not a smooth function of the arithmetic: fp32 rounding flips ReLU
units that lie near zero, and which ones flip depends on the summation order.  Once the forward's discrete decisions -- every
ReLU mask and the max-pool's arg-max -- are fixed, the backward IS smooth in the arithmetic.  `forward64` evaluates the
network of oracle/resnet.py (same parameter names) with every ReLU as `x * mask` and the max-pool as a gather through a tap
code (ty * 3 + tx of the window's first maximum, as the native forward stores it); BatchNorm stays the ordinary
batch-statistics F.batch_norm, so the gradient through the batch mean and variance is kept.  Plain torch-CPU ops."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

LAYERS = (3, 4, 6, 3)


def records():
    """The conv records in the native forward's launch order: (conv key, bn prefix, stride, pad, relu mode); relu 0 none,
    1 after the residual add (a block's conv2), 2 straight after BatchNorm (the stem, a block's conv1)."""
    out = [("conv1.weight", "bn1.", 2, 3, 2)]
    for li, n in enumerate(LAYERS, start=1):
        for bi in range(n):
            p = f"layer{li}.{bi}."
            s = 2 if (li > 1 and bi == 0) else 1
            out.append((p + "conv1.weight", p + "bn1.", s, 1, 2))
            if s == 2:
                out.append((p + "downsample.0.weight", p + "downsample.1.", s, 0, 0))
            out.append((p + "conv2.weight", p + "bn2.", 1, 1, 1))
    return out


def fma32(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """fp32 fused multiply-add, correctly rounded (what __builtin_fmaf computes): a * b is exact in fp64, the fp64 sum's rounding
    error e is recovered exactly (TwoSum), and where e != 0 the fp64 sum is moved one fp64 ulp towards it -- which changes the
    fp32 rounding only when the sum sat exactly on an fp32 midpoint, where e decides."""
    p = a.double() * b.double()
    c = c.double()
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    s = torch.where(e != 0, torch.nextafter(s, torch.where(e > 0, float("inf"), float("-inf")).to(s.dtype)), s)
    return s.float()


def bn_constants(gamma, beta, mean, rstd):
    """bn_affine of csrc/resnet_train.hip: scale = gamma * rstd, shift = fma(-mean, scale, beta), all fp32."""
    scale = gamma.float() * rstd.float()
    return scale, fma32(-mean.float(), scale, beta.float())


def bn_eval32(raw, gamma, beta, mean, rstd):
    """The kernels' BatchNorm value of `raw` [N, C, H, W]: fma(raw, scale, shift) in fp32."""
    scale, shift = bn_constants(gamma, beta, mean, rstd)
    return fma32(raw, scale.view(1, -1, 1, 1).expand_as(raw), shift.view(1, -1, 1, 1).expand_as(raw))


def pack_bits(mask: torch.Tensor) -> torch.Tensor:
    """bool [N, C, H, W] (C % 8 == 0) -> the tape's mask bits: byte [n][c / 8][pixel], bit c % 8 (uint8 [N, C / 8, H * W])."""
    n, c, h, w = mask.shape
    m = mask.reshape(n, c // 8, 8, h * w).to(torch.int32)
    sh = torch.arange(8, dtype=torch.int32).view(1, 1, 8, 1)
    return (m << sh).sum(dim=2).to(torch.uint8)


def unpack_bits(bits: torch.Tensor, shape) -> torch.Tensor:
    """Inverse of pack_bits: uint8 [N, C / 8, H * W] (or its flat bytes) -> bool [N, C, H, W]."""
    n, c, h, w = shape
    b = bits.reshape(n, c // 8, 1, h * w).to(torch.int32)
    sh = torch.arange(8, dtype=torch.int32, device=b.device).view(1, 1, 8, 1)
    return ((b >> sh) & 1).bool().reshape(n, c, h, w)


def pool_windows(a: torch.Tensor):
    """The 3x3 stride-2 pad-1 windows of `a` [N, C, H, W] as [N, C, 9, OH, OW], taps ty * 3 + tx, padding -inf."""
    n, c, h, w = a.shape
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    ap = F.pad(a, (1, 1, 1, 1), value=float("-inf"))
    win = F.unfold(ap.reshape(n * c, 1, h + 2, w + 2), 3, stride=2)          # [N C, 9, OH OW]
    return win.reshape(n, c, 9, oh, ow)


def pool_gather(a: torch.Tensor, code: torch.Tensor) -> torch.Tensor:
    """The max-pool as a gather: out[n, c, oy, ox] = a[n, c, 2 oy - 1 + ty, 2 ox - 1 + tx], code = ty * 3 + tx (uint8 [N, C, OH, OW])."""
    n, c, h, w = a.shape
    oh, ow = code.shape[-2:]
    code = code.long()
    ty, tx = code // 3, code % 3
    oy = torch.arange(oh).view(1, 1, oh, 1)
    ox = torch.arange(ow).view(1, 1, 1, ow)
    idx = (2 * oy + ty) * (w + 2) + (2 * ox + tx)                           # into the map padded by one on every side
    ap = F.pad(a, (1, 1, 1, 1))
    return torch.gather(ap.reshape(n, c, -1), 2, idx.reshape(n, c, -1)).reshape(n, c, oh, ow)


def forward64(sd: Dict[str, torch.Tensor], img: torch.Tensor, masks: Optional[List[Optional[torch.Tensor]]] = None,
              pool_code: Optional[torch.Tensor] = None, defect: Optional[dict] = None):
    """ResNet-34 training forward (oracle/resnet.py:resnet34_forward(training=True)) on the dtype of `sd` / `img`.

    masks: per record of records() the ReLU decision (bool, the shape of the record's output; None for records without ReLU);
    masks = None: the decisions of this very evaluation (pre-activation > 0), pool_code likewise (its own first maximum).
    Returns (feature, recs, code): recs[i] = {"raw": conv output, "y": BatchNorm output (retains its gradient: dz after a
    backward), "pre": the value the ReLU decides on, "out": the record's output}; code = the pool codes used.
    defect (power checks only): {"zero_last_col": i} zeroes the last column of record i's incoming gradient; {"dz_scale": (i, c, f)}
    multiplies record i's dz of channel c by f."""
    defect = defect or {}
    recs = []
    spec = records()

    def run(i, x, identity=None):
        key, bn, stride, pad, relu = spec[i]
        raw = F.conv2d(x, sd[key], None, stride=stride, padding=pad)
        y = F.batch_norm(raw, None, None, sd[bn + "weight"], sd[bn + "bias"], True, 0.1, 1e-5)
        if y.requires_grad:
            y.retain_grad()
            if "dz_scale" in defect and defect["dz_scale"][0] == i:
                _, c, f = defect["dz_scale"]
                sc = torch.ones(y.shape[1], dtype=y.dtype)
                sc[c] = f
                y.register_hook(lambda g: g * sc.view(1, -1, 1, 1))
        pre = y if identity is None else y + identity
        if relu:
            m = (pre > 0) if masks is None else masks[i]
            out = pre * m.to(pre.dtype)
        else:
            out = pre
        if out.requires_grad and defect.get("zero_last_col") == i:
            def cut(g):
                g = g.clone()
                g[..., -1] = 0
                return g
            out.register_hook(cut)
        recs.append({"raw": raw, "y": y, "pre": pre, "out": out})
        return out

    ri = 0
    a0 = run(ri, img)
    ri += 1
    if pool_code is None:
        pool_code = pool_windows(a0.detach()).argmax(dim=2).to(torch.uint8)       # first maximum
    x = pool_gather(a0, pool_code)
    for li, n in enumerate(LAYERS, start=1):
        for bi in range(n):
            o1 = run(ri, x)
            ri += 1
            if li > 1 and bi == 0:
                idt = run(ri, x)
                ri += 1
            else:
                idt = x
            x = run(ri, o1, idt)
            ri += 1
    feat = F.linear(x.mean(dim=(2, 3)), sd["fc.weight"], sd["fc.bias"])
    return feat, recs, pool_code


def param_keys():
    """The perception parameters (named_parameters order of oracle/resnet.py's state dict without buffers)."""
    keys = ["conv1.weight", "bn1.weight", "bn1.bias"]
    for key, bn, *_ in records()[1:]:
        keys += [key, bn + "weight", bn + "bias"]
    return keys + ["fc.weight", "fc.bias"]


def grads64(sd: Dict[str, torch.Tensor], img: torch.Tensor, d_feature: torch.Tensor, masks=None, pool_code=None, defect=None):
    """fp64 parameter gradients of sum(feature * d_feature) under the given decisions; also dz and xhat of every BatchNorm."""
    keys = param_keys()
    s = {k: (v.detach().double().requires_grad_(k in keys) if v.is_floating_point() else v) for k, v in sd.items()}
    feat, recs, code = forward64(s, img.double(), masks, pool_code, defect)
    (feat * d_feature.double()).sum().backward()
    bn = []
    for r in recs:
        raw = r["raw"].detach()
        mu = raw.mean(dim=(0, 2, 3), keepdim=True)
        var = raw.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
        bn.append({"dz": r["y"].grad, "xhat": (raw - mu) / torch.sqrt(var + 1e-5)})
    return feat.detach(), {k: s[k].grad for k in keys}, bn, recs, code
