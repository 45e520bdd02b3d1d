"""The launches of tests/test_gpu_conv2d_pair.py in a process of its own, so that a switch that is read once per process (ADX_HS_PAIR)
can be set for it.  usage: python tests/conv_pair_worker.py OUT.pt; saves {case: {"plain": fp32, "post": fp32, "cells": cells}}."""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
# (cin, cout, n, h, w) -- what each exercises: tests/test_gpu_conv2d_pair.py
CASES = ((32, 64, 1, 8, 31), (64, 64, 3, 9, 33), (96, 64, 2, 16, 16), (64, 192, 1, 5, 3), (128, 64, 40, 3, 5), (64, 64, 2, 64, 225))


def inputs(case):
    """x, weight, BatchNorm scale / shift, residual of a case (CPU, seeded)."""
    cin, cout, n, h, w = case
    g = torch.Generator().manual_seed(1000 * cin + 10 * cout + n + h + w)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    res = torch.randn(n, cout, h, w, generator=g)
    return x, wt, sc, sh, res


def cells_supported(case):
    """Whether the cell-layout launch of this shape exists (a shape whose fp32 launch may split its reduction has none)."""
    from autonomous_driving_with_diffusion_model_amd import _lib as L
    cin, cout, n, h, w = case
    d = L.Conv2dDesc(cin, cout, 3, 1, 1)
    return bool(L.lib().adx_conv2d_cells_supported(C.byref(d), n, h, w))


def outputs():
    from autonomous_driving_with_diffusion_model_amd import ops
    out = {}
    for case in CASES:
        cin, cout, n, h, w = case
        x, wt, sc, sh, res = (t.to(DEV) for t in inputs(case))
        plain, packed = ops.conv2d(x, wt, stride=1, pad=1)
        post, _ = ops.conv2d(x, wt, stride=1, pad=1, scale=sc, shift=sh, res=res, relu=True, packed=packed)
        o = {"plain": plain.cpu(), "post": post.cpu()}
        if cells_supported(case):
            o["cells"] = ops.conv2d_cells(ops.to_cells(x), packed, cin, cout, n, h, w, x_cells=True, scale=sc, shift=sh,
                                          res=ops.to_cells(res), res_cells=True, relu=True).cpu()
        out[case] = o
    return out


if __name__ == "__main__":
    torch.save(outputs(), sys.argv[1])
