"""GPU: whole UNet eval forwards at every row count where a launch plan changes, against the oracle in fp64.

How a forward runs depends on its rows (pipeline launch, chain samples per workgroup, the K-split kernel's staging budget and
reduction split, pair / mixed launches, every kernel's partial last row tile).  The row counts come from the code: the plan
export (include/adx.h: adx_unet_plan_describe) for rows 1..640 reduced by tests/unet_plan.py: plan_cases -- first and last row
count of every run of one per-launch signature of every layer, plus a partial and a full last tile where the run has them
(tests/test_unet_plan_cpu.py asserts the coverage; its docstring has the counts: 112 forwards over ten configurations).

Truth: oracle.unet.unet_forward on the state dict and the inputs in fp64.  Bar: 2e-5 max-abs PER SAMPLE ROW, the bar of this
operator everywhere in the suite (test_gpu_ops.py, chain_worker.py), here against fp64.  The fp32 CPU oracle itself is
2.1e-6 .. 2.8e-6 from fp64 on these inputs (|y| up to 3.5), so the bar is about 8x the reference's own error.  Each forward runs
three times -- on a fresh workspace, on one refilled with 0xFF and on one refilled with 0x5A -- and the three results are bit
equal; the range status reports nothing; a value of 1e5 planted in the last real sample is reported in the group that splits it.
No bit equality between different row counts is asserted: summation order differs between plans.

Measured on an MI355X, per horizon: the worst per-sample max-abs error against fp64 over the module's cases, and the fp32 CPU
oracle's error on that same case (measured against the reference, not tuned to the kernels):
    H = 16  rows 513  (1, 2, 4, 8) NO_GUIDANCE    HIP 1.906e-06   fp32 oracle 2.258e-06
    H = 24  rows 640  (1, 2, 4, 8) FREE_GUIDANCE  HIP 2.054e-06   fp32 oracle 2.395e-06
    H = 32  rows 128  (1, 2, 4, 8) FREE_GUIDANCE  HIP 1.849e-06   fp32 oracle 2.258e-06
    H = 64  rows 255  (1, 2, 4) FREE_GUIDANCE     HIP 1.888e-06   fp32 oracle 2.026e-06
    ADX_UNET_CHAIN=0: 1.677e-06 (H = 16), 2.115e-06 (H = 32); ADX_UNET_PIPE=0: 1.714e-06, 1.781e-06; op level: 2.1e-06 at most.
No case failed, before or after: no kernel or planner bug was found.  Wall time of the module on the MI355X box: 57 s (29 tests;
the suite before it: 589 s).

Op level: the 1024-channel concat conv (512 + 512 -> 256) of the deepest up level at the first batch where the export reports two
staged chunks for the K-split kernel (513 at L = 2, 257 at L = 4, 129 at L = 8 -- what hs_tile's 70 KB budget gives once the grid
leaves one workgroup per CU) and at a ragged batch above it, 512 -> 512 and 256 + 256 -> 128 at the same batches, with and
without scratch + ticket words, time bias and residual included, against conv1d / group_norm / mish in fp64."""
import os
import subprocess
import sys
import time

import pytest
import torch
import torch.nn.functional as F

import unet_plan as UP
from unet_plan import GPU_CONFIGS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 2e-5
SEED = 12


def build(H, dim, mults, use_cond, seed=0):
    """(model on the GPU, its state dict in fp32 on the host)"""
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    from autonomous_driving_with_diffusion_model_amd.modeling import build_model
    from autonomous_driving_with_diffusion_model_amd.utils import procedural as P
    cfg = create_cfg()
    cfg.MODEL.HORIZON, cfg.MODEL.DIM, cfg.MODEL.DIM_MULTS = H, dim, list(mults)
    cfg.TRAIN.USE_COND = cfg.GUIDANCE.USE_COND = use_cond
    m = build_model(cfg)
    P.load_procedural(m, seed)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.to(DEV).eval(), sd


def inputs(rows, H, dim, use_cond):
    from autonomous_driving_with_diffusion_model_amd.utils import procedural as P
    d = P.synthetic_batch(rows, H, image_hw=(32, 32), seed=SEED)
    feat = P._uniform("feat", SEED, (rows, dim), -3.0, 3.0)           # a feature row per sample, as chain_worker.py
    cond = d["target"] if use_cond == "FREE_GUIDANCE" else None
    return d["trajs"], d["imgs"], d["t"], feat, cond


def truth64(sd, x, t, feat, cond, use_cond, dim, mults):
    from oracle import unet as U
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        y = U.unet_forward(sd64, x.double(), None, t, None if cond is None else cond.double(), use_cond=use_cond, dim=dim,
                           dim_mults=tuple(mults), img_feature=feat.double())
    assert y.dtype == torch.float64
    return y


def hip_forward(m, x, imgs, t, feat, cond):
    """One eval forward with the perception pass stubbed out (the feature rows are the input)."""
    f = feat.to(DEV)
    m.perception.forward = lambda img: f
    m._feat_cache = None
    with torch.no_grad():
        return m(x.to(DEV), imgs.to(DEV), t.to(DEV), cond=None if cond is None else cond.to(DEV))


def per_sample_err(y, truth):
    return (y.double().cpu() - truth).abs().amax(dim=(1, 2))


def judge(err, recs, rows, bar=BAR):
    """None, or the failure text: per-sample errors above the bar, split into the samples that sit in the partial last row tile of
    some launch and the rest, with the plan of that forward."""
    tail = set(UP.tail_samples(recs, rows))
    bad = [(i, e) for i, e in enumerate(err.tolist()) if not e <= bar]
    if not bad:
        return None
    t = [(i, f"{e:.3e}") for i, e in bad if i in tail]
    o = [(i, f"{e:.3e}") for i, e in bad if i not in tail]
    worst_tail = max([err[i].item() for i in tail], default=0.0)
    worst_rest = max([err[i].item() for i in range(rows) if i not in tail], default=0.0)
    return (f"rows={rows}: {len(bad)} sample(s) above {bar:g}; in a partial last row tile of some launch: {t[:8]} (worst of the "
            f"{len(tail)} such samples {worst_tail:.3e}); the rest: {o[:8]} (worst {worst_rest:.3e})\n  plan:\n    " +
            "\n    ".join(UP.describe(r) for r in recs))


def run_cases(m, sd, H, dim, mults, use_cond, cases, out=sys.stdout):
    """Every row count of `cases` on model m: [failure texts], {rows: (worst HIP error, worst tail error, worst rest error)}"""
    from autonomous_driving_with_diffusion_model_amd import _lib as L
    failures, stats = [], {}
    for rows in cases:
        recs = UP.plan(m._native(), rows, flags=0)        # this process has packed: the plan is the one the forward takes
        print(f"FORWARD H={H} dim={dim} mults={mults} {use_cond} rows={rows}: " + " | ".join(UP.describe(r) for r in recs), file=out,
              flush=True)                                 # before the forward: a fault names its launch
        x, imgs, t, feat, cond = inputs(rows, H, dim, use_cond)
        m.clear_range_status()
        y = hip_forward(m, x, imgs, t, feat, cond)
        status = m.range_status()
        nbytes = L.lib().adx_unet_workspace_bytes(m._native(), rows)
        for fill in (0xFF, 0x5A):
            m._ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
            if not torch.equal(hip_forward(m, x, imgs, t, feat, cond), y):
                failures.append(f"rows={rows}: the forward on a workspace full of {hex(fill)} differs from the first")
        if status or m.range_status():
            failures.append(f"rows={rows}: range status {status or m.range_status()} on clean inputs (padding rows must not raise it)")
        err = per_sample_err(y, truth64(sd, x, t, feat, cond, use_cond, dim, mults))
        tail = UP.tail_samples(recs, rows)
        rest = [i for i in range(rows) if i not in set(tail)]
        stats[rows] = (err.max().item(), err[tail].max().item() if tail else 0.0, err[rest].max().item() if rest else 0.0)
        print(f"ERR rows={rows} worst={stats[rows][0]:.3e} tail({len(tail)})={stats[rows][1]:.3e} rest={stats[rows][2]:.3e}", file=out,
              flush=True)
        msg = judge(err, recs, rows)
        if msg:
            failures.append(msg)
    return failures, stats


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from autonomous_driving_with_diffusion_model_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def wall():
    t0 = time.time()
    yield
    print(f"\ntest_gpu_unet_rows.py: {time.time() - t0:.0f} s")


@pytest.mark.parametrize("H,dim,mults,use_cond", GPU_CONFIGS)
def test_unet_forward_at_every_plan_boundary_vs_fp64(lib, wall, H, dim, mults, use_cond):
    m, sd = build(H, dim, mults, use_cond)
    hip_forward(m, *inputs(1, H, dim, use_cond))          # packs: from here on the export is this process's own plan
    cases = UP.plan_cases(UP.plans(m._native(), UP.R_MAX, flags=0))
    assert len(cases) >= 4 and cases[0] == 1 and cases[-1] == UP.R_MAX, cases
    failures, stats = run_cases(m, sd, H, dim, mults, use_cond, cases)
    worst = max(stats.values())
    print(f"SUMMARY H={H} dim={dim} mults={mults} {use_cond}: {len(cases)} forwards, worst per-sample error {worst[0]:.3e}")
    assert not failures, f"H={H} dim={dim} mults={mults} {use_cond}: {len(failures)} failure(s)\n" + "\n".join(failures)


def test_fp32_oracle_error_on_the_same_cases_is_far_below_the_bar(lib):
    """Where the bar comes from: the fp32 CPU oracle against the fp64 one on this module's inputs (first, middle and last case of
    H = 16 and 32).  The bar is not tuned to the kernels: it must sit well above this and it does (about 8x)."""
    from oracle import unet as U
    for H in (16, 32):
        m, sd = build(H, 64, (1, 2, 4, 8), "FREE_GUIDANCE")
        for rows in (9, 257, 640):
            x, imgs, t, feat, cond = inputs(rows, H, 64, "FREE_GUIDANCE")
            with torch.no_grad():
                y32 = U.unet_forward(sd, x, None, t, cond, use_cond="FREE_GUIDANCE", img_feature=feat)
            e = per_sample_err(y32, truth64(sd, x, t, feat, cond, "FREE_GUIDANCE", 64, (1, 2, 4, 8)))
            print(f"FP32_ORACLE H={H} rows={rows} worst={e.max().item():.3e} median={e.median().item():.3e}")
            assert e.max().item() < BAR / 4


def test_the_comparison_notices_one_wrong_sample_and_a_swapped_tail():
    """Power check on the host: a truth perturbed by 5e-5 in one channel of one sample, or two samples of the last tile swapped,
    fails the per-sample comparison; the unperturbed one passes."""
    H, rows = 32, 33
    m_sd = None
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    from autonomous_driving_with_diffusion_model_amd.modeling import build_model
    from autonomous_driving_with_diffusion_model_amd.utils import procedural as P
    cfg = create_cfg()
    cfg.MODEL.HORIZON = H
    mm = build_model(cfg)
    P.load_procedural(mm, 0)
    m_sd = {k: v.detach().clone() for k, v in mm.state_dict().items()}
    x, imgs, t, feat, cond = inputs(rows, H, 64, "NO_GUIDANCE")
    truth = truth64(m_sd, x, t, feat, cond, "NO_GUIDANCE", 64, (1, 2, 4, 8))
    recs = [dict(family="ksplit", bt=8, row_tiles=5, rows_mod_bt=1, group=3, block=0, conv=1, conv_b=-1, ctiles=8, ctiles_b=0, grid=40,
                 ksplit=1, reduce=0, chunks=1, ck=512, vec_stage=1, fast_epi=1, ntap=5),
            dict(family="shortk", bt=4, row_tiles=9, rows_mod_bt=1, group=2, block=0, conv=1, conv_b=-1, ctiles=8, ctiles_b=0, grid=72,
                 ksplit=1, reduce=0, chunks=1, ck=256, vec_stage=1, fast_epi=1, ntap=5)]
    assert UP.tail_samples(recs, rows) == [32]
    y = truth.float()
    assert judge(per_sample_err(y, truth), recs, rows) is None
    bad = y.clone()
    bad[17, 5, 3] += 5e-5
    msg = judge(per_sample_err(bad, truth), recs, rows)
    assert msg and "(17," in msg and "the rest: [(17" in msg, msg
    recs[0]["rows_mod_bt"], recs[1]["rows_mod_bt"] = 3, 3          # a 35-row forward: samples 32..34 share the last tiles
    x, imgs, t, feat, cond = inputs(35, H, 64, "NO_GUIDANCE")
    truth = truth64(m_sd, x, t, feat, cond, "NO_GUIDANCE", 64, (1, 2, 4, 8))
    swapped = truth.float().clone()
    swapped[[33, 34]] = swapped[[34, 33]]
    msg = judge(per_sample_err(swapped, truth), recs, 35)
    assert msg and "partial last row tile of some launch: [(33," in msg and "the rest: []" in msg, msg


# ---- a planted overflow in the last real sample is reported in the group that splits it ------------------------------------

def _plant_time_bias(m, block_prefix, rows, H, dim, use_cond):
    """The mechanism of test_gpu_range_status.py (a scaled parameter), confined to ONE sample: the block's time_mlp Linear is
    scaled by 1e3 and the last sample's feature row holds 3e3, so that block's time bias -- added to the first conv's output --
    is ~1e5 for the last sample alone (a few hundred for the others), and the block's second conv splits it."""
    x, imgs, t, feat, cond = inputs(rows, H, dim, use_cond)
    feat = feat.clone()
    feat[rows - 1, :] = 3e3
    with torch.no_grad():
        dict(m.named_parameters())[block_prefix + "time_mlp.1.weight"].mul_(1e3)
    m.refresh_weights()
    return x, imgs, t, feat, cond


# One case per kernel family that a single sample can reach.  The short-K pair launch reads the trajectory only with ADX_UNET_CHAIN=0:
# its case is in test_plan_boundaries_of_the_switched_off_paths_vs_fp64.  The mixed launch and the general-shape kernel read only
# conv outputs of normalised activations in these models -- no input or per-sample bias reaches them at 1e5 without passing a launch
# that reports first --, so they have no case.
PLANTS = [
    # (family of the launch that splits the value, H, rows, what is planted, group reported first)
    ("chain", 32, 257, "x", "unet.down0"),                                  # the trajectory is split by the first level's chain
    ("shortk", 32, 257, "downs.2.0.", "unet.down2"),                         # block b of down level 2
    ("ksplit", 32, 257, "downs.3.0.", "unet.down3"),                         # block b of down level 3, one chunk
    ("shortk", 32, 257, "ups.0.0.", "unet.up0"),                             # added by the epilogue of the two-chunk concat conv
    ("pipeline", 16, 3, "downs.3.1.", "unet.down3"),                         # conv 2 of the pipeline run forms its input with it
    ("exact", 24, 81, "downs.2.0.", "unet.down2"),                           # ragged horizon: the exact-fp32 kernel splits nothing
]


@pytest.mark.parametrize("family,H,rows,what,group", PLANTS)
def test_overflow_planted_in_the_last_real_sample_is_reported_in_its_group(lib, family, H, rows, what, group):
    m, _ = build(H, 64, (1, 2, 4, 8), "NO_GUIDANCE")
    hip_forward(m, *inputs(1, H, 64, "NO_GUIDANCE"))
    names = [n for n in m.range_group_names() if n.startswith("unet.")]
    recs = UP.plan(m._native(), rows, flags=0)
    g = names.index(group)
    if what == "x":
        reader = [r for r in recs if r["group"] == g and r["family"] != "aux" and r["conv"] != 7][0]
        x, imgs, t, feat, cond = inputs(rows, H, 64, "NO_GUIDANCE")
        x = x.clone()
        x[rows - 1, 5, 1] = 1e5
    else:
        blk = int(what.split(".")[2])
        reader = [r for r in recs if r["group"] == g and (r["conv"] in (10, 11) or (r["block"], r["conv"]) == (blk, 1))][0]
        x, imgs, t, feat, cond = _plant_time_bias(m, what, rows, H, 64, "NO_GUIDANCE")
    assert reader["family"] == family, UP.describe(reader)
    m.clear_range_status()
    hip_forward(m, x, imgs, t, feat, cond)
    st = [s for s in m.range_status() if s.startswith("unet.")]
    if family == "exact":       # nothing is split on that path: nothing to report, and the sample is simply large
        assert st == [], st
        return
    assert group in st, (st, UP.describe(reader))
    assert not [s for s in st if names.index(s) < g], (st, "a group that runs before the planted one reported")
    # the overflow stays in its sample: every other sample is finite and where the oracle puts it.  (Not the 2e-5 bar: the planted
    # block's activations are ~1e3 for every sample here, and an fp32 sum of such terms carries ~1e3 x 2^-24 x sqrt(K) of rounding
    # into a GroupNorm that divides by their spread -- 1e-3 separates "rounded differently" from "read the neighbour's inf".)
    y = hip_forward(m, x, imgs, t, feat, cond)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    truth = truth64(sd, x, t, feat, cond, "NO_GUIDANCE", 64, (1, 2, 4, 8))
    err = per_sample_err(y, truth)[:rows - 1]
    assert bool(torch.isfinite(y[:rows - 1]).all()) and err.max().item() <= 1e-3, err.max().item()


# ---- the switch variants the default hides -----------------------------------------------------------------------------------

@pytest.mark.parametrize("switch", ["ADX_UNET_CHAIN", "ADX_UNET_PIPE"])
def test_plan_boundaries_of_the_switched_off_paths_vs_fp64(lib, switch):
    """ADX_UNET_CHAIN=0 / ADX_UNET_PIPE=0 are read once per process: a child runs H = 16 and 32 at the plan boundaries the export
    gives IN THAT CHILD (tests/unet_rows_worker.py) under the same checks."""
    env = dict(os.environ)
    env[switch] = "0"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "unet_rows_worker.py"), "16", "32"], env=env, capture_output=True,
                       text=True, timeout=900)
    tail = r.stdout[-6000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    done = [ln for ln in r.stdout.splitlines() if ln.startswith("DONE")]
    assert len(done) == 2, tail
    for ln in done:
        print(switch + "=0", ln)
        assert ln.split()[-1] == "failures=0", "\n".join(ln2 for ln2 in r.stdout.splitlines() if not ln2.startswith("FORWARD"))[-6000:]
    fams = {ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("FAMILIES")}
    assert fams, tail
    if switch == "ADX_UNET_CHAIN":
        assert all("chain" not in f.split(",") for f in fams), fams
        # ... and there the trajectory is split by the first level's pair launch: 1e5 planted in the last real sample of a ragged batch
        plants = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("PLANT")]
        assert len(plants) == 2, tail
        for _, fam, first, status in plants:
            assert fam == "shortk_pair" and first == "unet.down0" and "unet.down0" in status.split(","), plants
    else:
        assert all("pipeline" not in f.split(",") for f in fams), fams


# ---- op level: the two-chunk staging of the concat conv ----------------------------------------------------------------------

def _op_batches(lib, c0, c1, cout, L):
    """(first batch where the export reports two staged chunks for 512 + 512 -> 256 at this length, a ragged batch above it)"""
    d = lib.TConvDesc(0, 5, 1, 2, 512, 512, 256, L, L, 8, 1e-5)
    first = next(b for b in range(1, 2049) if UP.tconv_plan(d, b)[0]["chunks"] == 2)
    bt = UP.tconv_plan(d, first)[0]["bt"]
    return first, next(b for b in range(first + 43, first + 143) if b % bt != 0)


@pytest.mark.parametrize("L", [2, 4, 8])
@pytest.mark.parametrize("c0,c1,cout", [(512, 512, 256), (512, 0, 512), (256, 256, 128)])
def test_conv1d_block_past_one_workgroup_per_cu_vs_fp64(lib, c0, c1, cout, L):
    from autonomous_driving_with_diffusion_model_amd import ops
    from helpers import uni
    first, ragged = _op_batches(lib, c0, c1, cout, L)
    assert first == {2: 513, 4: 257, 8: 129}[L], first          # what reading hs_tile gives: 256 workgroups = 32 row tiles x 8 slabs
    d = lib.TConvDesc(0, 5, 1, 2, c0, c1, cout, L, L, 8, 1e-5)
    for B in (first, ragged):
        for with_scratch in (False, True):
            recs = UP.tconv_plan(d, B, scratch_floats=(2 << 20) if with_scratch else 0, tickets=with_scratch)
            # (256 + 256 -> 128 at L = 2 has GroupNorm groups of 32 elements: the general-shape kernel, one sample per workgroup)
            assert len(recs) == 1 and recs[0]["family"] in ("ksplit", "shortk", "generic"), recs
            assert recs[0]["chunks"] == (2 if c0 + c1 == 1024 else 1) and recs[0]["ksplit"] == 1, UP.describe(recs[0])
            if B == ragged and recs[0]["bt"] > 1:
                assert recs[0]["rows_mod_bt"] != 0, UP.describe(recs[0])
        name = f"rows.{c0}.{c1}.{cout}.{L}.{B}"
        cin = c0 + c1
        x0 = uni(name + ".x0", (B, c0, L))
        x1 = uni(name + ".x1", (B, c1, L)) if c1 else None
        w = uni(name + ".w", (cout, cin, 5), lo=-(3.0 / (5 * cin)) ** 0.5, hi=(3.0 / (5 * cin)) ** 0.5)
        b, g, be = uni(name + ".b", (cout,), lo=-.1, hi=.1), uni(name + ".g", (cout,), lo=.9, hi=1.1), uni(name + ".be", (cout,), lo=-.1, hi=.1)
        tb, res = uni(name + ".tb", (B, cout)), uni(name + ".res", (B, cout, L))
        xin = (x0 if x1 is None else torch.cat([x0, x1], 1)).double()
        ref = F.mish(F.group_norm(F.conv1d(xin, w.double(), b.double(), padding=2), 8, g.double(), be.double(), 1e-5)) + \
            tb.double()[:, :, None] + res.double()
        kw = dict(x1=None if x1 is None else x1.to(DEV), pad=2, gn_weight=g.to(DEV), gn_bias=be.to(DEV), groups=8, tbias=tb.to(DEV),
                  res=res.to(DEV))
        y = ops.tconv(x0.to(DEV), w.to(DEV), b.to(DEV), **kw)
        scratch = torch.full((2 << 20,), float("nan"), device=DEV)
        tickets = torch.zeros(256, dtype=torch.int32, device=DEV)
        ys = ops.tconv(x0.to(DEV), w.to(DEV), b.to(DEV), scratch=scratch, tickets=tickets, **kw)
        for what, got in (("plain", y), ("scratch + tickets", ys)):
            err = (got.double().cpu() - ref).abs().amax(dim=(1, 2))
            worst = int(err.argmax())
            print(f"OP {c0}+{c1}->{cout} L={L} B={B} {what}: worst per-sample error {err.max().item():.3e} (sample {worst})")
            assert err.max().item() <= BAR, (c0, c1, cout, L, B, what, worst, err.max().item(), UP.describe(recs[0]))
        assert int(tickets.abs().sum()) == 0
