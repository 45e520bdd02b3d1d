"""Test infrastructure: the reference's attention block (modeling/helpers.py:120-175) restated in plain torch, and a
TemporalMapUnet forward with MODEL.USE_ATTN composed from oracle/unet.py's block functions.  Works in any float dtype
(the GPU tests run it in fp64).

  LayerNorm over channels (biased variance, eps 1e-5, g / b [1, C, 1]) -> to_qkv (1x1, no bias) -> q, k, v of 4 heads x
  32 channels (channel = head * 32 + c) -> q *= 32^-0.5, k = softmax over positions -> context = k v^T per head ->
  out = context^T q -> to_out (1x1 + bias) -> + x
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F

from oracle import unet as U
from oracle.resnet import resnet34_forward

HEADS, DIM_HEAD = 4, 32


def chan_layernorm(x, g, b, eps=1e-5):
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * g.reshape(1, -1, 1) + b.reshape(1, -1, 1)


def linattn_core(qkv):
    """qkv [B, 384, L] -> [B, 128, L]."""
    B, _, L = qkv.shape
    q, k, v = qkv.reshape(B, 3, HEADS, DIM_HEAD, L).unbind(1)
    q = q * DIM_HEAD ** -0.5
    k = k.softmax(dim=-1)
    ctx = torch.einsum("bhdn,bhen->bhde", k, v)
    return torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(B, HEADS * DIM_HEAD, L)


def attention_block(sd, p, x):
    """Residual(PreNorm(C, LinearAttention(C))) with its parameters under prefix p (e.g. "downs.0.2.")."""
    xn = chan_layernorm(x, sd[p + "fn.norm.g"], sd[p + "fn.norm.b"])
    qkv = F.conv1d(xn, sd[p + "fn.fn.to_qkv.weight"])
    return F.conv1d(linattn_core(qkv), sd[p + "fn.fn.to_out.weight"], sd[p + "fn.fn.to_out.bias"]) + x


def unet_forward(sd, x, img, time, cond=None, *, use_cond=U.NO_GUIDANCE, dim=64, dim_mults=(1, 1),
                 return_action_and_time_only=False, img_feature=None):
    """oracle.unet.unet_forward with the attention blocks of USE_ATTN (modeling/temporal.py:215-231)."""
    if img_feature is None:
        img_feature = resnet34_forward(sd, "perception.", img)
    x = x.transpose(1, 2)
    te = U.time_mlp(sd, time, dim)
    if use_cond == U.FREE_GUIDANCE:
        if cond is None:
            cond = torch.zeros((x.shape[0], 2), device=x.device, dtype=x.dtype)
        if te.shape[0] != cond.shape[0]:
            te = te.repeat(cond.shape[0] // te.shape[0], 1)
        if img_feature.shape[0] != cond.shape[0]:
            img_feature = img_feature.repeat(cond.shape[0] // img_feature.shape[0], 1)
        te = te + U.cond_mlp(sd, cond)
    ci = torch.cat([te, img_feature], dim=-1)
    n = len(dim_mults)
    skips = []
    for i in range(n):
        x = U.residual_block(sd, f"downs.{i}.0.", x, ci)
        x = U.residual_block(sd, f"downs.{i}.1.", x, ci)
        x = attention_block(sd, f"downs.{i}.2.", x)
        skips.append(x)
        if i < n - 1:
            x = U.downsample(sd, f"downs.{i}.3.", x)
    x = U.residual_block(sd, "mid_block1.", x, ci)
    x = attention_block(sd, "mid_attn.", x)
    x = U.residual_block(sd, "mid_block2.", x, ci)
    for i in range(n - 1):
        x = torch.cat((x, skips.pop()), dim=1)
        x = U.residual_block(sd, f"ups.{i}.0.", x, ci)
        x = U.residual_block(sd, f"ups.{i}.1.", x, ci)
        x = attention_block(sd, f"ups.{i}.2.", x)
        x = U.upsample(sd, f"ups.{i}.3.", x)
    if use_cond == U.CLASSIFIER_GUIDANCE:
        a = U.conv1d_block(sd, "act_conv.0.", x)
        a = F.conv1d(a, sd["act_conv.1.weight"], sd["act_conv.1.bias"]).transpose(1, 2)
        if return_action_and_time_only:
            return a, te
        return U.state_from_action(sd, a, te, detach=True)
    y = U.conv1d_block(sd, "final_conv.0.", x)
    y = F.conv1d(y, sd["final_conv.1.weight"], sd["final_conv.1.bias"])
    return y.transpose(1, 2)


@contextlib.contextmanager
def with_attention():
    """oracle.sampling's loops and training loss call oracle.unet.unet_forward: route them through the forward above."""
    orig = U.unet_forward
    U.unet_forward = unet_forward
    try:
        yield
    finally:
        U.unet_forward = orig
