"""The PAIR form of conv2d_hs3x3_kernel (csrc/conv2d_hs.hip): the 4-wave 3x3 stride-1 tile on v_mfma_f32_16x16x32_f16, K = two
taps x 16 channels.  Every plain launch of that tile takes it, whatever its operand formats, so each case is checked in all of them:
against an fp64 evaluation with the bar of tests/test_gpu_conv2d.py, for bit equality between the fp32 and the cell launches, for
determinism, and against the 32x32x16 code (ADX_HS_PAIR=0, a process of its own).

Cases (cin, cout, n, h, w):
  (32, 64, 1, 8, 31)     one chunk pair, one tile, columns that do not fill it
  (64, 64, 3, 9, 33)     a second tile row with one valid row; image boundaries inside a tile of the virtual row
  (96, 64, 2, 16, 16)    three pairs: the weight buffers' parity comes round an odd number of times
  (64, 192, 1, 5, 3)     three slabs; a map smaller than 16 columns
  (128, 64, 40, 3, 5)    more images than a tile has columns (40 workgroups of 8 chunks: the shape has no cell launch -- the
                         plan keeps such shapes for the split reduction -- so only its fp32 launches are checked)
  (64, 64, 2, 64, 225)   the layer itself, two images"""
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conv_pair_worker as W  # noqa: E402

DEV = W.DEV
EXACT = os.environ.get("ADX_CONV_EXACT") == "1"
BAR = 4.0 if EXACT else 1.5          # as tests/test_gpu_conv2d.py
# the form is on: not pinned to the 32x32x16 code by a switch of the process that runs the suite
PAIR_ON = not EXACT and os.environ.get("ADX_HS_MODE") is None and os.environ.get("ADX_HS_PAIR") != "0"


def _ops():
    from autonomous_driving_with_diffusion_model_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _ref(case):
    """fp64 references of a case (plain; affine + residual + ReLU), their maxima, and the error of torch's own fp32 convs (CPU
    and GPU, whichever is worse) against them: computed once per case."""
    x, wt, sc, sh, res = W.inputs(case)
    post = lambda c: torch.relu(c * sc.to(c.dtype)[None, :, None, None] + sh.to(c.dtype)[None, :, None, None] + res.to(c.dtype))  # noqa: E731
    ref = F.conv2d(x.double(), wt.double(), padding=1)
    f32 = F.conv2d(x, wt, padding=1)
    g32 = F.conv2d(x.to(DEV), wt.to(DEV), padding=1).cpu()
    out = {}
    for name, fn in (("plain", lambda c: c), ("post", post)):
        r = fn(ref)
        den = r.abs().max().item() + 1e-300
        e32 = max((fn(t).double() - r).abs().max().item() / den for t in (f32, g32))
        out[name] = (r, den, e32)
    return out


def _err(y, case, name):
    r, den, e32 = _ref(case)[name]
    return (y.double().cpu() - r).abs().max().item() / den, e32


@pytest.mark.parametrize("case", W.CASES)
def test_pair_form_is_fp32_grade_in_every_format(case):
    cin, cout, n, h, w = case
    ops = _ops()
    x, wt, sc, sh, res = (t.to(DEV) for t in W.inputs(case))
    # fp64 bar: plain, and with affine + residual + ReLU
    y1, packed = ops.conv2d(x, wt, stride=1, pad=1)
    e_hip, e_f32 = _err(y1, case, "plain")
    print(case, "plain", e_hip, e_f32)
    assert e_f32 > 0
    assert e_hip <= BAR * e_f32 + 1e-7, (e_hip, e_f32)
    y0, _ = ops.conv2d(x, wt, stride=1, pad=1, scale=sc, shift=sh, res=res, relu=True, packed=packed)
    e_hip, e_f32 = _err(y0, case, "post")
    print(case, "post", e_hip, e_f32)
    assert e_f32 > 0
    assert e_hip <= BAR * e_f32 + 1e-7, (e_hip, e_f32)
    for rep in range(3):         # determinism
        assert torch.equal(ops.conv2d(x, wt, stride=1, pad=1, scale=sc, shift=sh, res=res, relu=True, packed=packed)[0], y0), rep
    if not W.cells_supported(case):
        assert case == (128, 64, 40, 3, 5)
        return
    # format equality: a cell output is the split of the fp32-layout launch's output, fed fp32 or cells
    want = ops.to_cells(y0)
    xc, rc = ops.to_cells(x), ops.to_cells(res)
    mag = max(1.0, y0.abs().max().item(), res.abs().max().item())
    first = None
    for rep in range(3):
        for x_cells in (False, True):
            got = ops.conv2d_cells(xc if x_cells else x, packed, cin, cout, n, h, w, x_cells=x_cells, scale=sc, shift=sh, res=res, relu=True)
            assert torch.equal(got, want), (x_cells, rep, (ops.from_cells(got, y0.shape) - y0).abs().max().item())
            got = ops.conv2d_cells(xc if x_cells else x, packed, cin, cout, n, h, w, x_cells=x_cells, scale=sc, shift=sh, res=rc,
                                   res_cells=True, relu=True)
            err = (ops.from_cells(got, y0.shape) - y0).abs().max().item()
            assert err <= 2.0 ** -21 * mag, (x_cells, rep, err)
            if x_cells:
                first = got if first is None else first
                assert torch.equal(got, first), rep
    e_hip, e_f32 = _err(ops.from_cells(first, y0.shape), case, "post")
    print(case, "post, cell residual", e_hip, e_f32)
    assert e_hip <= BAR * e_f32 + 4e-7, (e_hip, e_f32)     # + the 2^-22 of a residual held as hi + lo / 2^11 and of the split output
    assert torch.equal(ops.conv2d_cells(xc, packed, cin, cout, n, h, w, x_cells=True), ops.to_cells(y1))     # no epilogue operands


def test_pair_switch_selects_the_32x32x16_code(tmp_path):
    """ADX_HS_PAIR=0: the same launches on the 32x32x16 code meet the same fp64 bars, and they ARE other launches: on the largest
    case the two forms differ in at least one bit (another summation order)."""
    out = str(tmp_path / "pair_off.pt")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "conv_pair_worker.py"), out],
                       env=dict(os.environ, ADX_HS_PAIR="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    off = torch.load(out)
    assert set(off) == set(W.CASES)
    for case in W.CASES:
        for name, slack in (("plain", 1e-7), ("post", 1e-7)):
            e_hip, e_f32 = _err(off[case][name], case, name)
            assert e_hip <= BAR * e_f32 + slack, (case, name, e_hip, e_f32)
        if "cells" in off[case]:
            cin, cout, n, h, w = case
            e_hip, e_f32 = _err(_ops().from_cells(off[case]["cells"].to(DEV), (n, cout, h, w)), case, "post")
            assert e_hip <= BAR * e_f32 + 4e-7, (case, e_hip, e_f32)
    if PAIR_ON:
        big = max(W.CASES, key=lambda c: c[2] * c[3] * c[4] * c[0] * c[1])
        x, wt, sc, sh, res = (t.to(DEV) for t in W.inputs(big))
        y, _ = _ops().conv2d(x, wt, stride=1, pad=1)
        assert not torch.equal(y.cpu(), off[big]["plain"])
