"""Fine-tuning bit-for-bit checks in a process of their own (run under ADX_WGRAD_DETERMINISTIC=1: the weight gradients reduced in
index order).  Writes to OUT:
  "recipe": the detectron-style recipe (every BatchNorm frozen, the stem and layer1 with requires_grad=False) -- the trainable
            gradients of that truncated backward, and of the same forward differentiated with every slot requested;
  "ex0":    one training step through adx_resnet_forward_train + adx_resnet_backward, and through the _ex entry points with
            frozen mask 0 (features and gradients).
usage: python tests/frozen_bn_worker.py OUT"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RECIPE_FROZEN = ("conv1.", "bn1.", "layer1.")


def native_step(perc, img, dfeat, ex):
    """One forward (running buffers not updated) + backward through the C ABI, every gradient slot requested."""
    from autonomous_driving_with_diffusion_model_amd import _lib as L
    lib, h = L.lib(), perc._native()
    B, _, H, W = img.shape
    ts = [t.detach() for t in perc._tensors()]
    nbytes = lib.adx_resnet_train_workspace_bytes(h, B, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
    packed = torch.empty(lib.adx_resnet_packed_bytes(h), dtype=torch.uint8, device=img.device)
    tape = L.NativeTape(lib.adx_resnet_tape_create, lib.adx_resnet_tape_destroy, "adx_resnet_tape_create")
    out = torch.empty((B, perc.out_dim), dtype=torch.float32, device=img.device)
    st = L.stream_ptr(img.device)
    args = (h, L.ptr_array(ts), len(ts), packed.data_ptr(), ws.data_ptr(), nbytes, img.data_ptr(), B, H, W, out.data_ptr(), tape.handle, 0)
    if ex:
        L.check(lib.adx_resnet_forward_train_ex(*args, 0, st), "adx_resnet_forward_train_ex")
    else:
        L.check(lib.adx_resnet_forward_train(*args, st), "adx_resnet_forward_train")
    entries = [e for e in perc._entries if e.dtype == "f32"]
    grads = [None if e.is_buffer else torch.empty_like(t) for e, t in zip(entries, ts)]
    garr = (L.vp * len(grads))(*[None if g is None else g.data_ptr() for g in grads])
    bargs = (h, L.ptr_array(ts), garr, len(ts), ws.data_ptr(), nbytes, tape.handle, dfeat.data_ptr())
    if ex:
        L.check(lib.adx_resnet_backward_ex(*bargs, 0, None, 0, st), "adx_resnet_backward_ex")
    else:
        L.check(lib.adx_resnet_backward(*bargs, st), "adx_resnet_backward")
    torch.cuda.synchronize()
    tape.release()
    return out.cpu(), {e.key: g.cpu() for e, g in zip(entries, grads) if g is not None}


def recipe_grads(perc, img, w, all_slots):
    for k, p in perc.named_parameters():
        p.grad = None
        p.requires_grad_(all_slots or not k.startswith(RECIPE_FROZEN))
    feat = perc.forward_in_training(img)
    (feat * w).sum().backward()
    torch.cuda.synchronize()
    return {k: p.grad.detach().cpu().clone() for k, p in perc.named_parameters() if p.grad is not None}


def main(out):
    from test_gpu_model import make_model
    from autonomous_driving_with_diffusion_model_amd.utils import procedural as P
    import frozen_bn_ref as FR
    m, _ = make_model("NO_GUIDANCE", 16)
    perc = m.perception
    img = P.synthetic_batch(3, 16, image_hw=(64, 96), seed=73)["imgs"].to("cuda:0")
    other = P.synthetic_batch(3, 16, image_hw=(64, 96), seed=74)["imgs"]
    w = P._uniform("perc.frozen.w", 73, (3, perc.out_dim), -1.0, 1.0).to("cuda:0")
    FR.set_running_stats_from(perc, other)
    res = {}
    m.train()
    ex0 = {name: native_step(perc, img, w, ex) for name, ex in (("plain", False), ("ex", True))}
    res["ex0"] = ex0
    perc.eval()
    res["recipe"] = {"truncated": recipe_grads(perc, img, w, False), "all": recipe_grads(perc, img, w, True)}
    torch.save(res, out)


if __name__ == "__main__":
    main(sys.argv[1])
