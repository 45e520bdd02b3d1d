"""Fine-tuning with frozen BatchNorm statistics and frozen parameters, host side: the C ABI's layer table and refusals, and the
Python routing around the native calls (stubbed out, as in test_grad_modes_cpu.py).  No GPU."""
import ctypes

import pytest
import torch

from autonomous_driving_with_diffusion_model_amd import _lib as L
from autonomous_driving_with_diffusion_model_amd.modeling import perception as PM
from autonomous_driving_with_diffusion_model_amd.modeling.perception import PerceptionResNet34
from autonomous_driving_with_diffusion_model_amd.modeling.spec import resnet34_entries

import resnet_cond as RC

ALL = (1 << 36) - 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return L.lib()


def test_bn_layer_table_follows_the_records(lib):
    """adx_resnet_bn_layers = 36; adx_resnet_bn_tensor(l) = the gamma slot of the l-th record's BatchNorm (stem, then per block
    conv1, [downsample], conv2); -1 outside."""
    h = L.vp()
    assert lib.adx_resnet_create(64, ctypes.byref(h)) == 0
    try:
        assert lib.adx_resnet_bn_layers(h) == 36
        keys = [e.key for e in resnet34_entries("", 64) if e.dtype == "f32"]
        got = [keys[lib.adx_resnet_bn_tensor(h, i)] for i in range(36)]
        assert got == [bn + "weight" for _, bn, *_ in RC.records()]
        assert lib.adx_resnet_bn_tensor(h, -1) == -1 and lib.adx_resnet_bn_tensor(h, 36) == -1
    finally:
        lib.adx_resnet_destroy(h)


def test_mask_out_of_range_and_tape_mismatch_refused(lib):
    """A frozen bit >= 36 is refused by both _ex entry points; a backward given another mask than its tape's forward is refused.
    Host-side validation: nothing is launched (the pointers are never dereferenced)."""
    h = L.vp()
    assert lib.adx_resnet_create(64, ctypes.byref(h)) == 0
    tape = L.vp()
    assert lib.adx_resnet_tape_create(ctypes.byref(tape)) == 0
    try:
        n = lib.adx_resnet_num_tensors(h)
        fake = (L.vp * n)(*([16] * n))
        p = 16
        for bit in (36, 63):
            rc = lib.adx_resnet_forward_train_ex(h, fake, n, p, p, 1 << 20, p, 2, 64, 64, p, tape, 1, 1 << bit, None)
            assert rc != 0 and b"frozen mask" in lib.adx_last_error(), lib.adx_last_error()
            rc = lib.adx_resnet_backward_ex(h, fake, fake, n, p, 1 << 20, tape, p, 1 << bit, None, 0, None)
            assert rc != 0 and b"frozen mask" in lib.adx_last_error(), lib.adx_last_error()
        rc = lib.adx_resnet_backward_ex(h, fake, fake, n, p, 1 << 20, tape, p, 1, None, 0, None)     # the (empty) tape has mask 0
        assert rc != 0 and b"the backward was given" in lib.adx_last_error(), lib.adx_last_error()
    finally:
        lib.adx_resnet_tape_destroy(tape)
        lib.adx_resnet_destroy(h)


class _Recorder:
    """Stands in for _PerceptionTrainFn / the eval pass: records which route a call took and with which mask."""

    def __init__(self, monkeypatch):
        self.calls = []
        rec = self

        class Fn:
            @staticmethod
            def apply(img, module, frozen, *params):
                rec.calls.append(("train", frozen))
                return torch.zeros(img.shape[0], module.out_dim)
        monkeypatch.setattr(PM, "_PerceptionTrainFn", Fn)
        monkeypatch.setattr(PerceptionResNet34, "_forward_eval", lambda self, img: rec.calls.append(("eval", None)) or img)
        monkeypatch.setattr(L, "require_gpu_f32", lambda t, name, dtype=torch.float32: t)


@pytest.fixture
def perc(lib):
    return PerceptionResNet34(64)


def test_mask_from_holders(perc):
    holders = perc._bn_holders()
    names = {id(m): n for n, m in perc.named_modules()}
    assert [names[id(m)] for m in holders] == [bn[:-1] for _, bn, *_ in RC.records()]
    perc.train()
    assert perc.frozen_mask() == 0
    perc.eval()
    assert perc.frozen_mask() == ALL
    perc.train()
    perc.bn1.eval()
    perc.layer2._modules["0"].eval()
    want = 1 | (0b111 << 7)          # the stem; layer2.0's conv1, downsample, conv2 are records 7, 8, 9
    assert perc.frozen_mask() == want


def test_batch_counters_per_layer_mode(perc):
    perc.train()
    assert len(perc._batch_counters(0)) == 36
    assert [id(b) for b in perc._batch_counters(0)] == [id(b) for b in perc.buffers() if b.dtype == torch.int64]
    mask = 1 | (1 << 5)
    holders = perc._bn_holders()
    got = [id(b) for b in perc._batch_counters(mask)]
    assert got == [id(m.num_batches_tracked) for i, m in enumerate(holders) if i not in (0, 5)]
    assert perc._batch_counters(ALL) == []


def test_routing(perc, monkeypatch):
    r = _Recorder(monkeypatch)
    img = torch.zeros(2, 3, 64, 64)
    # 1. encoder in train mode: the taped forward, mask from the holders (0: today's call)
    perc.train()
    perc(img)
    perc.forward_in_training(img)
    perc.layer4.eval()
    perc(img)
    assert r.calls == [("train", 0), ("train", 0), ("train", sum(1 << i for i in range(36 - 7, 36)))]
    r.calls.clear()
    # 2. encoder in eval mode inside a training forward, grad enabled, a trainable parameter: the taped forward, all frozen
    perc.eval()
    perc.forward_in_training(img)
    assert r.calls == [("train", ALL)]
    r.calls.clear()
    # ... but a plain eval-mode call stays the eval pass, and so does a training forward under no_grad
    perc(img)
    with torch.no_grad():
        perc.forward_in_training(img)
    assert r.calls == [("eval", None), ("eval", None)]
    r.calls.clear()
    # 3. encoder in eval mode, no trainable parameter: the eval pass
    for p in perc.parameters():
        p.requires_grad_(False)
    perc.forward_in_training(img)
    assert r.calls == [("eval", None)]


def test_temporal_training_forward_routes_through_forward_in_training(monkeypatch):
    """TemporalMapUnet's training forward hands the image to perception.forward_in_training (case 2 of the routing); its
    eval-mode forward does not."""
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    from autonomous_driving_with_diffusion_model_amd.modeling import build_model
    m = build_model(create_cfg())
    seen = []
    monkeypatch.setattr(m.perception, "forward_in_training", lambda img: seen.append(img) or torch.zeros(img.shape[0], m.dim))
    monkeypatch.setattr(m, "unet_forward_train", lambda x, feat, time, cond=None: feat)
    m.train()
    m.perception.eval()
    img = torch.zeros(1, 3, 64, 64)
    m(torch.zeros(1, m.horizon, m.transition_dim), img, torch.zeros(1, dtype=torch.int64))
    assert len(seen) == 1 and seen[0] is img


def test_null_slots_for_frozen_parameters(perc, monkeypatch):
    """The backward hands NULL for every slot whose parameter does not require grad (and for the running statistics); the
    returned gradients are None exactly there."""
    got = {}

    def fake_backward(h, T, garr, n, ws, nbytes, tape, g, *rest):
        got["slots"] = [garr[i] for i in range(n)]
        return 0
    fake_lib = type("Lib", (), {"adx_resnet_backward_events": staticmethod(fake_backward),
                                "adx_resnet_backward_ex": staticmethod(lambda h, T, garr, n, ws, nb, tape, g, frozen, *rest:
                                                                       fake_backward(h, T, garr, n, ws, nb, tape, g))})()
    monkeypatch.setattr(L, "lib", lambda: fake_lib)
    monkeypatch.setattr(L, "require_gpu_f32", lambda t, name, dtype=torch.float32: t)
    monkeypatch.setattr(PerceptionResNet34, "_backward_events", lambda self, dev: None)
    monkeypatch.setattr(PerceptionResNet34, "_native", lambda self: None)
    monkeypatch.setattr(L, "stream_ptr", lambda device=None: 0)
    for k, p in perc.named_parameters():
        p.requires_grad_(not k.startswith(("conv1.", "bn1.", "layer1.")))
    entries = [e for e in perc._entries if e.dtype == "f32"]
    params = [p for _, p in perc.named_parameters()]

    class Tape:
        alive, handle = True, None

        def release(self):
            pass

    class Ctx:
        module, tape, ws, nbytes, frozen = perc, Tape(), torch.zeros(1), 0, ALL
        ts = perc._tensors()
        needs_input_grad = (False, False, False, *[p.requires_grad for p in params])
    out = PM._PerceptionTrainFn.backward(Ctx, torch.zeros(1, 64))
    slots = got["slots"]
    named = dict(perc.named_parameters())
    for e, s in zip(entries, slots):
        want_null = e.is_buffer or not named[e.key].requires_grad
        assert (s is None) == want_null, e.key
    grads = out[3:]
    assert [g is None for g in grads] == [not p.requires_grad for p in params]
