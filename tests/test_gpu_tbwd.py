"""GPU parity, one launch at a time: the temporal stack's backward kernels (csrc/tbwd.hip) and the data-gradient launches the
training executor makes (adx_tconv_forward on csrc/unet_train.hip's dgrad_desc, exact = 1) against torch autograd in float64 on the
host, at the batch sizes and lengths where their launch geometry changes.  The cases are tests/tbwd_plan.py's;
tests/test_tbwd_plan_cpu.py vouches that they take both sides of every flip.

Error of a tensor: max |got - fp64| per output channel over that channel's max |fp64|, worst channel (dc and dx: over the tensor's
max).  The bar is BAR x the same error of torch's own fp32 evaluation of the operation on the same inputs (the worse of CPU and
GPU) + 2e-7: the bar of the other sequential fp32 MFMA chains (tests/test_gpu_conv2d.py: test_exact_fp32_mfma_conv_shapes).  Sums
that cancel (d gamma, d beta, the bias gradients, d time-bias) get K x 2^-22 x sum |terms| of slack per channel, the terms in fp64.

MEASURED on an MI355X (every figure of a run also joins the parity records of tests/test_gpu_fullsize.py: _record), worst case
per check:
  tconv_wgrad_kernel       e_hip / e_f32 = 1.22 (w64-32.L16.b3: 1.8e-7 against 1.5e-7; every other case below 0.94, the 512-channel
                           ragged ones 0.35 .. 0.49); nsplit = 1 cases bit-equal run to run
  data gradient (exact)    1.03 (g512.L4.b37; the two-chunk cases 0.54 .. 0.79, the time Linear's 0.18 and 0.43)
  gn_mish_bwd_kernel  dc   1.09 (gn.cg64.L8.b37: 2.5e-7 against 2.3e-7)
     the cancelling sums, |got - fp64| in units of 2^-22 sum |terms| (torch's fp32 in brackets):
     d gamma 0.30 (0.38), d beta 0.32 (0.26), d conv-bias 0.27 (0.20), d time-bias 0.64 (0.65)
  bias_grad_kernel         0.085 (0.16) of the same unit
No check needs more than the 4 x of the other sequential fp32 chains.  SUM_K = 2: three times the worst measured figure of
either implementation, and half of what a tree sum of 4096 terms whose terms carry a few roundings of their own may lose
((log2 n + 4) 2^-24 = 4 x 2^-22); a dropped term weighs sum |terms| / n >= 1.2e-4 of the mass, 250 times the slack.
The planted defects of the power check miss their bars by 0.14 .. 1.3 (bars: ~3e-6).
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import tbwd_plan as T
from helpers import uni

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = 3.0e4            # what the positions past a real length hold: a kernel that reads one is off by orders of magnitude
BAR = 4.0              # x torch's fp32 error (+ FLOOR)
FLOOR = 2e-7
SUM_K = 2.0            # slack of the cancelling sums in units of 2^-22 sum |terms| (module docstring)


def _record(payload):
    """Every measured figure joins the parity records tests/test_gpu_fullsize.py keeps, as test "tbwd/<case>"."""
    from test_gpu_fullsize import _record as record
    payload = dict(payload)
    record("tbwd/" + payload.pop("case"), payload)


def chan_err(got, ref, per_channel=True, slack=None):
    """max |got - ref| per channel (dim 0) over the channel's max |ref|, worst channel; per_channel=False: over the tensor's max.
    `slack` [channels]: absolute error forgiven per channel (a cancelling sum's K 2^-22 sum |terms|)."""
    ref = ref.double()
    diff = (got.detach().double().cpu() - ref).abs()
    if not per_channel:
        return (diff.max() / (ref.abs().max() + 1e-300)).item()
    diff, mag = diff.reshape(ref.shape[0], -1).amax(1), ref.abs().reshape(ref.shape[0], -1).amax(1)
    if slack is not None:
        diff = (diff - slack).clamp_min(0.0)
    return (diff / (mag + 1e-300)).max().item()


def sum_k(got, ref, terms):
    """A cancelling sum's error in units of 2^-22 sum |terms|, worst channel."""
    return ((got.detach().double().cpu() - ref.double()).abs() / (2.0 ** -22 * terms + 1e-300)).max().item()


def _lib():
    from autonomous_driving_with_diffusion_model_amd import _lib as L
    return L


def _stream():
    return _lib().stream_ptr(torch.device(DEV))


def _mask_tail(t, valid, value):
    if 0 < valid < t.shape[-1]:
        t[..., valid:] = value
    return t


# --------------------------------------------------------------------------------------------------------- weight gradient
def wgrad_inputs(name, d, batch, big=BIG):
    """x [B][cin][lin] and the gradient of the conv's output [B][cout][lout], padded lengths; past the real lengths: `big`
    (None: ordinary values, for the planted defect that reads them)."""
    cin = d.c0 + d.c1
    x = uni(name + ".x", (batch, cin, d.lin))
    dy = uni(name + ".dy", (batch, d.cout, d.lout))
    if big is not None:
        _mask_tail(x, d.lin_valid, big)
        _mask_tail(dy, d.lout_valid, big)
    return x, dy


def wgrad_ref(d, x, dy, dtype, device="cpu", lout_valid=None):
    """dW of the conv `d` by autograd: [cout][cin][taps] (kind 1: the ConvTranspose1d layout [cin][cout][taps])."""
    cin = d.c0 + d.c1
    liv = d.lin_valid or d.lin
    lov = lout_valid or d.lout_valid or d.lout
    xm = x.to(device=device, dtype=dtype).clone()
    xm[..., liv:] = 0
    g = dy.to(device=device, dtype=dtype)
    if d.kind == 0:
        w = torch.zeros((d.cout, cin, d.taps), dtype=dtype, device=device, requires_grad=True)
        y = F.conv1d(xm, w, stride=d.stride, padding=d.pad)
    else:
        w = torch.zeros((cin, d.cout, d.taps), dtype=dtype, device=device, requires_grad=True)
        y = F.conv_transpose1d(xm, w, stride=d.stride, padding=d.pad)
    assert y.shape[-1] == d.lout
    (y[..., :lov] * g[..., :lov]).sum().backward()
    return w.grad.detach().cpu()


def wgrad_hip(d, x, dy, xmode, runs=2):
    """adx_tconv_wgrad as the training executor calls it for the conv `d`: `runs` results."""
    L = _lib()
    B, cin = x.shape[0], d.c0 + d.c1
    io = L.TConvIO()
    io.batch = B
    keep = []
    if d.kind == 1:            # the ConvTranspose weight: the mirrored strided conv reads dy as its input and x as its output gradient
        m = T.mirror_desc(d)
        xin, dc = dy.to(DEV).contiguous(), x.to(DEV).contiguous()
        io.x0, io.x0_sb, io.x0_sc, io.x0_sl = xin.data_ptr(), d.cout * d.lout, d.lout, 1
        keep += [xin]
        shape = (cin, d.cout, d.taps)
    else:
        m = d
        dc = dy.to(DEV).contiguous()
        shape = (d.cout, cin, d.taps)
        if xmode == "bhd":          # the trajectory in place: [B][H][D]
            xd = x.permute(0, 2, 1).contiguous().to(DEV)
            io.x0, io.x0_sb, io.x0_sc, io.x0_sl = xd.data_ptr(), d.lin * cin, 1, cin
            keep += [xd]
        elif xmode == "tlin":       # one position, position stride 0
            assert d.lin == 1 and d.c1 == 0
            xd = x.reshape(B, cin).contiguous().to(DEV)
            io.x0, io.x0_sb, io.x0_sc, io.x0_sl = xd.data_ptr(), cin, 1, 0
            keep += [xd]
        else:
            x0 = x[:, :d.c0].contiguous().to(DEV)
            io.x0, io.x0_sb, io.x0_sc, io.x0_sl = x0.data_ptr(), d.c0 * d.lin, d.lin, 1
            keep += [x0]
            if d.c1:
                x1 = x[:, d.c0:].contiguous().to(DEV)
                io.x1, io.x1_sb, io.x1_sc, io.x1_sl = x1.data_ptr(), d.c1 * d.lin, d.lin, 1
                keep += [x1]
    cd = T.c_desc(m)
    out = []
    for _ in range(runs):
        dw = torch.full(shape, 9.0, device=DEV)           # adx_tconv_wgrad zeroes dW itself
        L.check(L.lib().adx_tconv_wgrad(C.byref(cd), C.byref(io), dc.data_ptr(), dw.data_ptr(), _stream()), "adx_tconv_wgrad")
        out.append(dw.cpu())
    return out


# ----------------------------------------------------------------------------------------------------------- data gradient
def dgrad_inputs(name, d, batch):
    cin = d.c0 + d.c1
    bound = (3.0 / (d.taps * cin)) ** 0.5
    w = uni(name + ".w", (d.cout, cin, d.taps) if d.kind == 0 else (cin, d.cout, d.taps), lo=-bound, hi=bound)
    dc = _mask_tail(uni(name + ".dc", (batch, d.cout, d.lout)), d.lout_valid, BIG)
    r0 = uni(name + ".r0", (batch, cin, d.lin))           # what the output buffer holds before an accumulating launch
    return w, dc, r0


def dgrad_ref(d, w, dc, r0, acc, dtype, device="cpu", drop_channels=None):
    """dx [B][cin][lin_valid] of the conv `d` by autograd (+ the buffer's contents when the launch accumulates)."""
    cin, liv, lov = d.c0 + d.c1, d.lin_valid or d.lin, d.lout_valid or d.lout
    x = torch.zeros((dc.shape[0], cin, d.lin), dtype=dtype, device=device, requires_grad=True)
    wt, g = w.to(device=device, dtype=dtype), dc.to(device=device, dtype=dtype).clone()
    if drop_channels is not None:
        g[:, drop_channels[0]:drop_channels[1]] = 0
    y = F.conv1d(x, wt, stride=d.stride, padding=d.pad) if d.kind == 0 else F.conv_transpose1d(x, wt, stride=d.stride, padding=d.pad)
    assert y.shape[-1] == d.lout
    (y[..., :lov] * g[..., :lov]).sum().backward()
    dx = x.grad.detach()[..., :liv]
    if acc:
        dx = dx + r0.to(device=device, dtype=dtype)[..., :liv]
    return dx.cpu()


def dgrad_hip(g, w, dc, r0, acc, x_strides=None, y_strides=None):
    """adx_tconv_forward on the data-gradient descriptor `g` with the forward layer's own weight tensor, as adx_unet_backward
    launches it.  Returns the whole output buffer (padded length)."""
    L = _lib()
    cg = T.c_desc(g)
    nbytes = L.lib().adx_tconv_packed_bytes(C.byref(cg))
    assert nbytes > 0, L.lib().adx_last_error()
    packed = torch.empty(nbytes // 4, device=DEV)
    wd, dcd = w.to(DEV).contiguous(), dc.to(DEV).contiguous()
    L.check(L.lib().adx_tconv_pack(C.byref(cg), wd.data_ptr(), packed.data_ptr(), _stream()), "adx_tconv_pack")
    B = dc.shape[0]
    y = r0.to(DEV).contiguous().clone()
    io = L.TConvIO()
    io.x0 = dcd.data_ptr()
    io.x0_sb, io.x0_sc, io.x0_sl = x_strides or (g.c0 * g.lin, g.lin, 1)
    io.packed_w = packed.data_ptr()
    io.y = y.data_ptr()
    io.y_sb, io.y_sc, io.y_sl = y_strides or (g.cout * g.lout, g.lout, 1)
    if acc:
        io.res, io.res_sb, io.res_sc, io.res_sl = io.y, io.y_sb, io.y_sc, io.y_sl
    io.batch = B
    L.check(L.lib().adx_tconv_forward(C.byref(cg), C.byref(io), _stream()), "adx_tconv_forward")
    return y.cpu()


# ---------------------------------------------------------------------------------------------- GroupNorm / Mish backward
def gn_inputs(name, B, Cc, Ln, Lv):
    lv = Lv or Ln
    pre = uni(name + ".pre", (B, Cc, Ln), lo=-2.0, hi=2.0)
    dy = uni(name + ".dy", (B, Cc, Ln))
    gamma = uni(name + ".g", (Cc,), lo=0.5, hi=1.5)
    beta = uni(name + ".be", (Cc,), lo=-0.3, hi=0.3)
    p = pre[..., :lv].double().reshape(B, 8, -1)
    mean, var = p.mean(-1), p.var(-1, unbiased=False)
    stats = torch.stack([mean, (var + 1e-5).rsqrt()], -1).float()          # what the forward launch leaves: [B][G][2] in fp32
    _mask_tail(pre, Lv, BIG)
    _mask_tail(dy, Lv, BIG)
    return pre, dy, gamma, beta, stats


def gn_ref(pre, dy, gamma, beta, Lv, dtype, device="cpu"):
    """dc, d gamma, d beta, d conv-bias, d time-bias of y = Mish(GroupNorm8(pre)) + tb[:, :, None] by autograd, and -- in the given
    precision -- the sums of |terms| behind the four reductions."""
    lv = Lv or pre.shape[-1]
    to = lambda t: t.detach().to(device=device, dtype=dtype, copy=True)  # noqa: E731
    p = to(pre)[..., :lv].clone().requires_grad_()
    ga, be = to(gamma).requires_grad_(), to(beta).requires_grad_()
    tb = torch.zeros(pre.shape[:2], dtype=dtype, device=device, requires_grad=True)
    g = to(dy)[..., :lv]
    u = F.group_norm(p, 8, ga, be, 1e-5)
    u.retain_grad()
    (F.mish(u) + tb[:, :, None]).backward(g)
    dz = u.grad
    xh = (u.detach() - be.detach()[None, :, None]) / ga.detach()[None, :, None]
    out = {"dc": p.grad, "dgamma": ga.grad, "dbeta": be.grad, "dbias": p.grad.sum((0, 2)), "dtb": tb.grad}
    terms = {"dgamma": (dz * xh).abs().sum((0, 2)), "dbeta": dz.abs().sum((0, 2)), "dbias": p.grad.abs().sum((0, 2)),
             "dtb": g.abs().sum(2)}
    return {k: v.detach().cpu() for k, v in out.items()}, {k: v.detach().cpu() for k, v in terms.items()}


def gn_hip(pre, dy, gamma, beta, stats, Lv, with_dtb, with_dbias):
    L = _lib()
    B, Cc, Ln = pre.shape
    pd, dyd, gd, bd, sd = (t.to(DEV).contiguous() for t in (pre, dy, gamma, beta, stats))
    dc = torch.full((B, Cc, Ln), 9.0, device=DEV)
    dg, dbe, dbi = (torch.zeros(Cc, device=DEV) for _ in range(3))
    dtb = torch.full((B, Cc + 3), 5.0, device=DEV)          # L <= 64: stored, not added to
    L.check(L.lib().adx_gn_mish_backward_ex(dyd.data_ptr(), Cc * Ln, Ln, 1, pd.data_ptr(), sd.data_ptr(), gd.data_ptr(), bd.data_ptr(),
                                            dc.data_ptr(), dg.data_ptr(), dbe.data_ptr(), dbi.data_ptr() if with_dbias else None,
                                            dtb.data_ptr() if with_dtb else None, Cc + 3, B, Cc, Ln, 8, Lv, _stream()),
            "adx_gn_mish_backward_ex")
    return {"dc": dc.cpu(), "dgamma": dg.cpu(), "dbeta": dbe.cpu(), "dbias": dbi.cpu(), "dtb": dtb.cpu()}


# ------------------------------------------------------------------------------------------------------------ the results
def _baseline(fn):
    """torch's own fp32 evaluation: on the host and on the GPU."""
    return [fn(torch.float32, "cpu"), fn(torch.float32, DEV)]


@pytest.fixture(scope="module")
def results():
    """Every case run once (the weight gradients twice), every figure recorded; the tests below only judge."""
    res = {}
    for name, d, batch, xmode in T.WGRAD_CASES:
        x, dy = wgrad_inputs(name, d, batch)
        truth = wgrad_ref(d, x, dy, torch.float64)
        base = max(chan_err(b, truth) for b in _baseline(lambda dt, dev: wgrad_ref(d, x, dy, dt, dev)))
        got = wgrad_hip(d, x, dy, xmode)
        p = T.wgrad_plan(T.mirror_desc(d) if d.kind == 1 else d, batch)
        res[name] = {"check": "wgrad", "e_hip": max(chan_err(g_, truth) for g_ in got), "e_f32": base, "nsplit": p["nsplit"],
                     "bit_equal": bool(torch.equal(got[0], got[1])), "_got": got[0], "_truth": truth, "_in": (x, dy)}
    for name, d, batch, acc in T.DGRAD_CASES:
        w, dc, r0 = dgrad_inputs(name, d, batch)
        liv = d.lin_valid or d.lin
        truth = dgrad_ref(d, w, dc, r0, acc, torch.float64)
        base = max(chan_err(b, truth, False) for b in _baseline(lambda dt, dev: dgrad_ref(d, w, dc, r0, acc, dt, dev)))
        buf = dgrad_hip(T.dgrad_desc(d), w, dc, r0, acc)
        res[name] = {"check": "dgrad", "e_hip": chan_err(buf[..., :liv], truth, False), "e_f32": base,
                     "tail_untouched": bool(torch.equal(buf[..., liv:], r0[..., liv:])), "_got": buf[..., :liv], "_truth": truth,
                     "_in": (w, dc, r0)}
    for name, sum_c, two_dim, batch in T.TLIN_DGRAD_CASES:
        bound = (3.0 / two_dim) ** 0.5
        w = uni(name + ".w", (sum_c, two_dim, 1), lo=-bound, hi=bound)
        dtb = uni(name + ".dtb", (batch, sum_c, 1))
        r0 = uni(name + ".r0", (batch, two_dim, 1))
        mm = lambda dt, dev: (dtb[..., 0].to(device=dev, dtype=dt) @ w[..., 0].to(device=dev, dtype=dt)).cpu()  # noqa: E731
        truth = mm(torch.float64, "cpu")
        base = max(chan_err(b, truth, False) for b in _baseline(mm))
        buf = dgrad_hip(T.tlin_dgrad_desc(sum_c, two_dim), w, dtb, r0, False, x_strides=(sum_c, 1, 0), y_strides=(two_dim, 1, 0))
        res[name] = {"check": "dgrad", "e_hip": chan_err(buf[..., 0], truth, False), "e_f32": base, "tail_untouched": True}
    for name, B, Cc, Ln, Lv, with_dtb, with_dbias in T.GN_CASES:
        pre, dy, gamma, beta, stats = gn_inputs(name, B, Cc, Ln, Lv)
        truth, terms = gn_ref(pre, dy, gamma, beta, Lv, torch.float64)
        base = _baseline(lambda dt, dev: gn_ref(pre, dy, gamma, beta, Lv, dt, dev)[0])
        got = gn_hip(pre, dy, gamma, beta, stats, Lv, with_dtb, with_dbias)
        lv = Lv or Ln
        r = {"check": "gn", "dc_tail_zero": bool((got["dc"][..., lv:] == 0).all()),
             "dtb_pad_untouched": bool((got["dtb"][:, Cc:] == 5.0).all()), "with_dtb": with_dtb, "with_dbias": with_dbias,
             "skipped_untouched": bool((with_dtb or (got["dtb"] == 5.0).all()) and (with_dbias or (got["dbias"] == 0).all()))}
        r["dc"] = {"e_hip": chan_err(got["dc"][..., :lv], truth["dc"], False),
                   "e_f32": max(chan_err(b["dc"], truth["dc"], False) for b in base)}
        for k in ("dgamma", "dbeta", "dbias", "dtb"):
            if (k == "dbias" and not with_dbias) or (k == "dtb" and not with_dtb):
                continue
            g_ = got[k][:, :Cc] if k == "dtb" else got[k]
            r[k] = {"k_hip": sum_k(g_, truth[k], terms[k]), "k_f32": max(sum_k(b[k], truth[k], terms[k]) for b in base),
                    "_got": g_, "_truth": truth[k], "_terms": terms[k], "_base": [b[k] for b in base]}
        res[name] = r
    for name, B, Cc, Ln, Lv, layout in T.BIAS_CASES:
        L = _lib()
        dc = _mask_tail(uni(name + ".dc", (B, Cc, Ln)), Lv, BIG)
        lv = Lv or Ln
        truth, terms = dc[..., :lv].double().sum((0, 2)), dc[..., :lv].double().abs().sum((0, 2))
        base = _baseline(lambda dt, dev: dc[..., :lv].to(device=dev, dtype=dt).sum((0, 2)).cpu())
        dcd = dc.to(DEV).contiguous()
        db = torch.full((Cc,), 9.0, device=DEV)
        strides = (Cc, 1, 0) if layout == "tlin" else (Cc * Ln, Ln, 1)
        L.check(L.lib().adx_bias_grad_ex(dcd.data_ptr(), *strides, db.data_ptr(), B, Cc, Ln, Lv, _stream()), "adx_bias_grad_ex")
        res[name] = {"check": "bias", "db": {"k_hip": sum_k(db, truth, terms), "k_f32": max(sum_k(b, truth, terms) for b in base),
                                             "_got": db.cpu(), "_truth": truth, "_terms": terms, "_base": base}}

    def public(v):
        return {k: (public(x) if isinstance(x, dict) else x) for k, x in v.items() if not k.startswith("_")}
    for name, r in res.items():
        _record({"case": name, **public(r)})
    return res


def _sum_ok(e):
    """A cancelling sum per channel: |got - fp64| <= (BAR e_f32 + FLOOR) |fp64| + SUM_K 2^-22 sum |terms|, e_f32 torch's own
    fp32 error under the same slack."""
    slack = SUM_K * 2.0 ** -22 * e["_terms"].reshape(-1)
    shape = (-1, 1)
    e_hip = chan_err(e["_got"].reshape(shape), e["_truth"].reshape(shape), slack=slack)
    e_f32 = max(chan_err(b.reshape(shape), e["_truth"].reshape(shape), slack=slack) for b in e["_base"])
    return e_hip, e_f32


# --------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("case", [c[0] for c in T.WGRAD_CASES])
def test_wgrad_launch_vs_fp64(results, case):
    r = results[case]
    print(case, {k: v for k, v in r.items() if not k.startswith("_")})
    assert r["e_hip"] <= BAR * r["e_f32"] + FLOOR, (case, r["e_hip"], r["e_f32"])          # both runs
    if r["nsplit"] == 1:
        assert r["bit_equal"], case          # plain stores: nothing depends on the arrival order


@pytest.mark.parametrize("case", [c[0] for c in T.DGRAD_CASES + T.TLIN_DGRAD_CASES])
def test_dgrad_launch_as_training_runs_it_vs_fp64(results, case):
    r = results[case]
    print(case, {k: v for k, v in r.items() if not k.startswith("_")})
    assert r["e_hip"] <= BAR * r["e_f32"] + FLOOR, (case, r["e_hip"], r["e_f32"])
    assert r["tail_untouched"], case         # positions past the real length are not stored


@pytest.mark.parametrize("case", [c[0] for c in T.GN_CASES])
def test_gn_mish_backward_ex_vs_fp64(results, case):
    r = results[case]
    print(case, {k: ({a: b for a, b in v.items() if not a.startswith("_")} if isinstance(v, dict) else v) for k, v in r.items()})
    assert r["dc_tail_zero"] and r["dtb_pad_untouched"] and r["skipped_untouched"], case
    assert r["dc"]["e_hip"] <= BAR * r["dc"]["e_f32"] + FLOOR, (case, r["dc"])
    for k in ("dgamma", "dbeta", "dbias", "dtb"):
        if k in r:
            e_hip, e_f32 = _sum_ok(r[k])
            assert e_hip <= BAR * e_f32 + FLOOR, (case, k, e_hip, e_f32, r[k]["k_hip"], r[k]["k_f32"])


@pytest.mark.parametrize("case", [c[0] for c in T.BIAS_CASES])
def test_bias_grad_ex_vs_fp64(results, case):
    r = results[case]["db"]
    print(case, {a: b for a, b in r.items() if not a.startswith("_")})
    e_hip, e_f32 = _sum_ok(r)
    assert e_hip <= BAR * e_f32 + FLOOR, (case, e_hip, e_f32, r["k_hip"], r["k_f32"])


def test_power_check_planted_defects_fail_the_bars(results):
    """The bars would notice the bugs this module exists for: each defect below is planted in the fp64 side of one case and the GPU
    result already computed is judged against it with the case's own bar -- every one must fail."""
    def fails(r, planted, per_channel):
        e = chan_err(r["_got"], planted, per_channel)
        return e > BAR * r["e_f32"] + FLOOR, e

    out = {}
    # 1. the last sample of a ragged super-tile dropped (512 -> 512, L 4, batch 37: super-tiles of 32 and 5 samples)
    name, d, batch, _ = T.WGRAD_CASES[0]
    p = T.wgrad_plan(d, batch)
    assert p["nsplit"] == 1 and p["sbt"] < batch and batch % p["sbt"] != 0
    x, dy = results[name]["_in"]
    out["ragged_last_sample"] = fails(results[name], wgrad_ref(d, x[:-1], dy[:-1], torch.float64), True)
    # 2. position lout_valid counted in a masked case (ordinary values there, so that nothing but the bar can notice)
    name, d, batch, _ = next(c for c in T.WGRAD_CASES if c[0] == "w256.L6of8.b37")
    x, dy = wgrad_inputs(name, d, batch, big=None)
    x0, dy0 = results[name]["_in"]
    assert torch.equal(x[..., :6], x0[..., :6]) and torch.equal(dy[..., :6], dy0[..., :6])
    out["position_lout_valid"] = fails(results[name], wgrad_ref(d, x, dy, torch.float64, lout_valid=d.lout_valid + 1), True)
    # 3. one 16-channel block at the chunk boundary of a two-chunk data gradient dropped
    name, d, batch, acc = next(c for c in T.DGRAD_CASES if c[0] == "g512.L4.b67")
    pl = T.dgrad_plan(T.dgrad_desc(d), batch)
    assert pl["chunks"] == 2
    w, dc, r0 = results[name]["_in"]
    planted = dgrad_ref(d, w, dc, r0, acc, torch.float64, drop_channels=(pl["ck"], pl["ck"] + 16))
    out["chunk_boundary_block"] = fails(results[name], planted, False)
    # 4. the first channel of x1 and the last of x0 swapped in a concat weight gradient
    name, d, batch, _ = next(c for c in T.WGRAD_CASES if c[1].c1 > 0)
    planted = results[name]["_truth"].clone()
    planted[:, [d.c0 - 1, d.c0]] = planted[:, [d.c0, d.c0 - 1]]
    out["concat_seam"] = fails(results[name], planted, True)
    _record({"case": "power_check", **{k: {"fails": bool(v[0]), "e": v[1]} for k, v in out.items()}})
    print(out)
    assert all(v[0] for v in out.values()), out
