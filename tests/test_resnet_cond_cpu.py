"""Host-side checks of the decision-conditioned fp64 oracle (tests/resnet_cond.py) and of the tape description export
(adx_resnet_tape_describe): no GPU needed."""
import ctypes

import pytest
import torch

import resnet_cond as RC
from autonomous_driving_with_diffusion_model_amd import ops
from autonomous_driving_with_diffusion_model_amd.modeling.spec import resnet34_entries
from autonomous_driving_with_diffusion_model_amd.utils import procedural as P


def _sd(seed=5):
    return P.procedural_state_dict(((e.key, e.shape) for e in resnet34_entries("", 64)), seed)


@pytest.mark.parametrize("b,hw", [(2, (32, 32)), (2, (70, 102))])
def test_conditioned_oracle_on_its_own_decisions_equals_oracle_autograd(b, hw):
    """With the decisions of its own fp64 forward, the conditioned evaluation IS oracle.resnet's training forward + autograd."""
    from oracle import resnet as R
    sd = _sd()
    img = P.synthetic_batch(b, 16, image_hw=hw, seed=3)["imgs"].double()
    w = P._uniform("perc.cond.w", 3, (b, 64), -1.0, 1.0).double()
    keys = RC.param_keys()
    s = {k: (v.double().requires_grad_(k in keys) if v.is_floating_point() else v) for k, v in sd.items()}
    f_ref = R.resnet34_forward(s, "", img, training=True)
    (f_ref * w).sum().backward()
    with torch.no_grad():
        _, recs, code = RC.forward64({k: v.double() for k, v in sd.items() if v.is_floating_point()}, img)
    masks = [r["pre"] > 0 if relu else None for r, (*_, relu) in zip(recs, RC.records())]
    f, g, bn, _, _ = RC.grads64(sd, img, w, masks, code)
    assert (f - f_ref.detach()).abs().max().item() <= 1e-12 * f_ref.abs().max().item()
    assert len(g) == 110 and len(bn) == 36
    for k in keys:
        ref = s[k].grad
        assert (g[k] - ref).abs().max().item() <= 1e-12 * ref.abs().max().item() + 1e-300, k
    # dz hooks: d beta = sum dz, d gamma = sum dz xhat per channel
    for (key, p, *_), q in zip(RC.records(), bn):
        assert torch.allclose(q["dz"].sum(dim=(0, 2, 3)), g[p + "bias"], rtol=1e-10, atol=1e-14)
        assert torch.allclose((q["dz"] * q["xhat"]).sum(dim=(0, 2, 3)), g[p + "weight"], rtol=1e-9, atol=1e-12)


def test_pool_gather_is_maxpool_with_first_maximum():
    g = torch.Generator().manual_seed(0)
    a = torch.rand(2, 3, 9, 13, generator=g, dtype=torch.float64).clamp_min(0.4) - 0.4     # ties at zero, as after a ReLU
    code = RC.pool_windows(a).argmax(dim=2).to(torch.uint8)
    assert torch.equal(RC.pool_gather(a, code), torch.nn.functional.max_pool2d(a, 3, 2, 1))
    assert int(code.max()) <= 8


def test_mask_bits_and_cells_decoders_round_trip():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 24, 5, 7, generator=g)
    m = x > 0.3
    bits = RC.pack_bits(m)
    assert bits.shape == (2, 3, 35) and bits.dtype == torch.uint8
    assert torch.equal(RC.unpack_bits(bits, m.shape), m)
    assert torch.equal(RC.unpack_bits(bits.reshape(-1), m.shape), m)
    # bit c % 8 of byte [n][c / 8][pixel]
    assert int(bits[1, 2, 3 * 7 + 4]) >> 5 & 1 == int(m[1, 2 * 8 + 5, 3, 4])
    cells = ops.to_cells(x)
    y = ops.from_cells(cells, x.shape)
    assert ((y - x).abs() <= 2.0 ** -22 * x.abs()).all()
    hi = x.half().float()
    assert torch.equal(y, hi + (((x - hi) * 2048.0).half().float() / 2048.0))


def test_fma32_is_correctly_rounded():
    """a * b + c rounded once to fp32: here the fp64 sum lands on an fp32 midpoint (a naive fp64 evaluation rounds the wrong
    way), and an ordinary random set agrees with the naive evaluation wherever that one is not a midpoint."""
    a = torch.tensor([2.0 ** -24 * (1 + 2.0 ** -23)], dtype=torch.float32)
    b = torch.tensor([1 - 2.0 ** -23], dtype=torch.float32)
    c = torch.tensor([1 + 2.0 ** -23], dtype=torch.float32)
    assert (a.double() * b.double() + c.double()).float().item() == 1 + 2.0 ** -22       # naive: double rounding
    assert RC.fma32(a, b, c).item() == 1 + 2.0 ** -23
    g = torch.Generator().manual_seed(2)
    a, b, c = (torch.randn(10000, generator=g) for _ in range(3))
    assert torch.equal(RC.fma32(a, b, c), (a.double() * b.double() + c.double()).float())


def test_tape_describe_refusals_without_gpu():
    """adx_resnet_tape_describe refuses a null tape / workspace / output and a tape that holds no forward (an index out of range
    on a filled tape: test_gpu_resnet_conditioned.py's worker)."""
    from autonomous_driving_with_diffusion_model_amd import _lib as L
    lib = L.lib()
    n, ints, offs = ctypes.c_int32(), (ctypes.c_int32 * 12)(), (ctypes.c_int64 * 7)()
    ws = ctypes.create_string_buffer(64)
    assert lib.adx_resnet_tape_describe(None, ws, 0, ctypes.byref(n), ints, offs) == -1
    assert b"null argument" in lib.adx_last_error()
    t = L.vp()
    assert lib.adx_resnet_tape_create(ctypes.byref(t)) == 0
    try:
        assert lib.adx_resnet_tape_describe(t, None, 0, ctypes.byref(n), ints, offs) == -1
        assert lib.adx_resnet_tape_describe(t, ws, 0, None, ints, offs) == -1
        assert lib.adx_resnet_tape_describe(t, ws, 0, ctypes.byref(n), None, offs) == -1
        assert lib.adx_resnet_tape_describe(t, ws, 0, ctypes.byref(n), ints, None) == -1
        for idx in (-1, 0, 5):
            assert lib.adx_resnet_tape_describe(t, ws, idx, ctypes.byref(n), ints, offs) == -1
            assert b"no forward" in lib.adx_last_error()
    finally:
        lib.adx_resnet_tape_destroy(t)
