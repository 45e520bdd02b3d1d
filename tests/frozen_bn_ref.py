"""Test infrastructure for fine-tuning with frozen BatchNorm statistics: the fp64 ResNet-34 training forward of
tests/resnet_cond.py with a per-layer BatchNorm mode -- a frozen layer is F.batch_norm(training=False) on its running
statistics, the others batch statistics -- conditioned on the native forward's ReLU masks and max-pool codes, and the parameter
gradients of that evaluation.  Plain torch-CPU ops."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

import resnet_cond as RC


def forward64(sd: Dict[str, torch.Tensor], img: torch.Tensor, frozen: List[bool], masks=None, pool_code=None):
    """(feature, per-record {"raw", "out"}, pool codes); frozen[i]: record i's BatchNorm uses running_mean / running_var."""
    spec = RC.records()
    recs = []

    def run(i, x, identity=None):
        key, bn, stride, pad, relu = spec[i]
        raw = F.conv2d(x, sd[key], None, stride=stride, padding=pad)
        if frozen[i]:
            y = F.batch_norm(raw, sd[bn + "running_mean"], sd[bn + "running_var"], sd[bn + "weight"], sd[bn + "bias"], False, 0.1, 1e-5)
        else:
            y = F.batch_norm(raw, None, None, sd[bn + "weight"], sd[bn + "bias"], True, 0.1, 1e-5)
        pre = y if identity is None else y + identity
        if relu:
            m = (pre > 0) if masks is None else masks[i]
            out = pre * m.to(pre.dtype)
        else:
            out = pre
        recs.append({"raw": raw, "out": out})
        return out

    ri = 0
    a0 = run(ri, img)
    ri += 1
    if pool_code is None:
        pool_code = RC.pool_windows(a0.detach()).argmax(dim=2).to(torch.uint8)
    x = RC.pool_gather(a0, pool_code)
    for li, n in enumerate(RC.LAYERS, start=1):
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


def grads64(sd, img, d_feature, frozen, masks=None, pool_code=None):
    """fp64 feature and parameter gradients of sum(feature * d_feature) under the given decisions."""
    keys = RC.param_keys()
    s = {k: (v.detach().double().requires_grad_(k in keys) if v.is_floating_point() else v) for k, v in sd.items()}
    feat, _, _ = forward64(s, img.double(), frozen, masks, pool_code)
    (feat * d_feature.double()).sum().backward()
    return feat.detach(), {k: s[k].grad for k in keys}


def set_running_stats_from(perc, img_other: torch.Tensor) -> None:
    """Running statistics of every BatchNorm := the fp64 batch statistics of ANOTHER image batch (unbiased variance), so that
    frozen and batch statistics differ while the activations stay at the scale batch statistics give them."""
    sd = {k: v.detach().cpu().double() for k, v in perc.state_dict().items() if v.is_floating_point()}
    with torch.no_grad():
        _, recs, _ = forward64(sd, img_other.cpu().double(), [False] * len(RC.records()))
        for (key, bn, *_), r in zip(RC.records(), recs):
            holder = dict(perc.named_modules())[bn[:-1]]
            raw = r["raw"]
            holder.running_mean.copy_(raw.mean(dim=(0, 2, 3)).float())
            holder.running_var.copy_(raw.var(dim=(0, 2, 3), unbiased=True).float())


def rel_errors(got: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor]) -> Dict[str, float]:
    return {k: ((got[k].double().cpu() - r).norm() / (r.norm() + 1e-300)).item() for k, r in ref.items()}


def holder_order(perc) -> List[str]:
    """The BatchNorm prefixes of tests/resnet_cond.records() (the native layer order), without the trailing dot."""
    return [bn[:-1] for _, bn, *_ in RC.records()]


def masks_of(res) -> Optional[list]:
    from test_gpu_resnet_conditioned import decode
    return decode(res)[0]
