"""GPU: no UNet forward may read what an earlier forward left in the deepest level's hand-off state (csrc/tconv_pipe.hip).

The pipeline launch hands raw conv sums on as 16-byte units {d0, d1, d2, tag} that sit at the same workspace address on every
forward of a (model, rows); a consumer takes a unit once its tag is THIS forward's, and the tag hashes a forward number that the
launch opening the forward draws from one device-wide counter.  The block outputs ya / yb / yc carry no tag, and the K-split
launches' partial tiles sit in the same scratch on every forward.  A forward that reused a number, or read a residual before its
writer had stored it, would return the previous forward's bits -- which a test repeating ONE input cannot tell from the right
ones.  So here:
  (a) every forward draws a new number, on every path that opens a forward;
  (b) forwards of several inputs, interleaved, give each input's bits every time (per-step and precomputed conditioning);
  (c) the same with the hand-off state poisoned between forwards: payloads NaN, tags kept -- exactly what an earlier forward
      left, made loud (a torn 16-byte unit would also show as NaN here);
  (d) each input's forward against the fp64 oracle and against the launch chain (ADX_UNET_PIPE=0, a process of its own).
Where the layout lives: adx_unet_pipe_describe (tests/helpers.py: pipe_layout)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from oracle import unet as U
from autonomous_driving_with_diffusion_model_amd.utils import procedural as P
from helpers import pipe_layout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_INPUTS = 3
# a fixed interleaving of the inputs, 24 forwards: every input follows every other one and itself
ORDER = [0, 1, 0, 2, 1, 2, 0, 2, 1, 1, 0, 0, 2, 2, 1, 0, 1, 2, 0, 1, 2, 2, 0, 1]
# which conditioning path each forward of ORDER takes.  "mixed": two per-step, two precomputed, ... -- a precomputed forward
# follows a precomputed one AND a per-step one
FORMS = {"per_step": lambda i: False, "precomputed": lambda i: True, "mixed": lambda i: (i // 2) % 2 == 1}

# (case id, guidance, H, rows, MODEL.DIM, one trajectory row for the classifier-free pair, takes the pipeline launch)
CASES = [
    ("no_h16_r1", "NO_GUIDANCE", 16, 1, 64, False, True),
    ("no_h16_r3", "NO_GUIDANCE", 16, 3, 64, False, True),
    ("free_h16_pair", "FREE_GUIDANCE", 16, 2, 64, True, True),
    ("free_h16_r4", "FREE_GUIDANCE", 16, 4, 64, False, True),          # two scenes' classifier-free pairs
    ("cls_h16_r4", "CLASSIFIER_GUIDANCE", 16, 4, 64, False, True),
    ("no_dim32_h16_r8", "NO_GUIDANCE", 16, 8, 32, False, True),        # deepest width 256: P = 16, the 16-row tile full
    # outside pipe_shape_ok (tests/test_pipe_layout_cpu.py): the launch chain, whose K-split scratch is poisoned the same way
    ("free_h16_r8", "FREE_GUIDANCE", 16, 8, 64, False, False),
    ("no_h32_r4", "NO_GUIDANCE", 32, 4, 64, False, False),
]
CASE_IDS = [c[0] for c in CASES]
# Bars against fp64: about 10x the largest error measured on an MI355X over the K inputs of each case, pipeline or launch chain
# (never looser than the 2e-5 the fp32-oracle tests use).  Measured (pipeline / launch chain): no_h16_r1 9.6e-7 / 8.2e-7,
# no_h16_r3 1.10e-6 / 9.9e-7, free_h16_pair 1.11e-6 / 9.7e-7, free_h16_r4 1.16e-6 / 1.12e-6, cls_h16_r4 9.4e-7 / 9.4e-7,
# no_dim32_h16_r8 1.54e-6 / 1.17e-6, free_h16_r8 and no_h32_r4 (launch chain in both) 1.39e-6 and 1.33e-6.  The kernels are
# bit-reproducible, so these are the same on every run of the same inputs.
FP64_BAR = {"no_h16_r1": 1e-5, "no_h16_r3": 1.1e-5, "free_h16_pair": 1.1e-5, "free_h16_r4": 1.2e-5, "cls_h16_r4": 1e-5,
            "no_dim32_h16_r8": 1.5e-5, "free_h16_r8": 1.4e-5, "no_h32_r4": 1.3e-5}
# The pipeline's error against fp64 stays within 2x the launch chain's plus SLACK: the two round differently (measured between
# them: up to 9.5e-7, about one fp32 ulp of the outputs' largest entries), so a pipeline error slightly above the launch chain's
# on one input is rounding, not a defect.
SLACK = 1e-6


_MODELS = {}


def build(guidance, H, dim=64, seed=0):
    """A model as test_gpu_model.make_model builds it (procedural weights), with the encoder stubbed; one per configuration."""
    key = (guidance, H, dim, seed)
    if key not in _MODELS:
        _MODELS[key] = _build(guidance, H, dim, seed)
    return _MODELS[key]


def _build(guidance, H, dim, seed):
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    from autonomous_driving_with_diffusion_model_amd.modeling import build_model
    cfg = create_cfg()
    cfg.MODEL.HORIZON, cfg.MODEL.DIM = H, dim
    cfg.TRAIN.USE_COND = cfg.GUIDANCE.USE_COND = guidance
    m = build_model(cfg)
    P.load_procedural(m, seed)
    m = m.to(DEV).eval()
    m.cache_perception = False
    feats = {}
    m.perception.forward = lambda img: feats[id(img)]       # test-only stub of the encoder: one seeded feature per image object
    m._test_feats = feats
    return m


def make_inputs(m, case, k, seed_base=0):
    """Input k of a case: trajectory, timestep, condition and image feature, seeded by (case, k)."""
    name, guidance, H, rows, dim, pair, _ = case
    s = 1000 * sum(name.encode()) + 17 * k + seed_base
    g = torch.Generator().manual_seed(s)
    free = guidance == "FREE_GUIDANCE"
    x = torch.randn(1 if pair else rows, H, m.transition_dim, generator=g)
    t = int(torch.randint(0, 100, (1,), generator=g))
    feat = (torch.rand(1 if pair else rows, dim, generator=g) * 6 - 3)
    cond = None
    if free:
        tgt = torch.randn(rows // 2, 2, generator=g)
        cond = torch.cat([tgt, torch.zeros_like(tgt)], 0)         # the classifier-free pair: target rows, then null rows
    img = torch.zeros(1, 3, 8, 8, device=DEV)                     # a distinct object per input; its content is never read
    m._test_feats[id(img)] = feat.to(DEV)
    return dict(x=x, t=t, feat=feat, cond=cond, img=img, rows=rows, guidance=guidance, pair=pair)


def run(m, inp, precomputed):
    """One forward; returns the outputs as a tuple of fresh tensors (CLASSIFIER: action and time_embed)."""
    rows, guidance = inp["rows"], inp["guidance"]
    free = guidance == "FREE_GUIDANCE"
    kw = dict(return_action_and_time_only=True) if guidance == "CLASSIFIER_GUIDANCE" else {}
    cond = None if inp["cond"] is None else inp["cond"].to(DEV)
    x = inp["x"].to(DEV)
    if precomputed:
        if "tc" not in inp:
            ts = torch.tensor([inp["t"]], dtype=torch.int64, device=DEV)
            inp["tc"] = m.time_conditioning(inp["img"], ts, cond=cond, rows=rows)
        y = m(x, None, None, time_cond=(inp["tc"], 0), **kw)
    else:
        xin = x.expand(rows, -1, -1).contiguous() if inp["pair"] else x
        t = torch.full((1 if free else rows,), inp["t"], dtype=torch.int64, device=DEV)
        y = m(xin, inp["img"], t, cond=cond, **kw)
    return tuple(v.clone() for v in (y if isinstance(y, tuple) else (y,)))


def epoch(m):
    """This model's last forward number (the ticket word the forward leaves it in)."""
    o = pipe_layout(m._native(), 1)["epoch"]
    return int(m._ws[o:o + 4].view(torch.int32).item()) & 0xFFFFFFFF


def poison(m, rows):
    """What an earlier forward leaves in this forward's hand-off state, made loud: words 0-2 of every record unit NaN with the tag
    (word 3) kept, the block outputs ya / yb / yc NaN, the K-split launches' part of the scratch NaN.  In stream order."""
    d = pipe_layout(m._native(), rows)
    ws = m._ws
    f32 = lambda o, n: ws[o:o + n].view(torch.float32)      # noqa: E731
    nan = float("nan")
    f32(d["scratch"], d["ksplit_bytes"]).fill_(nan)
    if d["shape_ok"]:
        f32(d["records"], d["record_bytes"]).view(-1, 4)[:, :3].fill_(nan)
        for k in ("ya", "yb", "yc"):
            f32(d[k], d["y_bytes"]).fill_(nan)


def oracle64(m, inp):
    """The same forward by the oracle in float64 (model's own procedural state dict)."""
    rows, guidance, dim = inp["rows"], inp["guidance"], m.dim
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.cpu()) for k, v in m.state_dict().items()}
    x = inp["x"].double().expand(rows, -1, -1)
    feat = inp["feat"].double().expand(rows, -1)
    t = torch.full((rows,), inp["t"], dtype=torch.int64)
    cond = None if inp["cond"] is None else inp["cond"].double()
    want = U.unet_forward(sd, x, None, t, cond, use_cond=guidance, dim=dim, dim_mults=tuple(m.dim_mults), img_feature=feat)
    return want[..., -3:] if guidance == "CLASSIFIER_GUIDANCE" else want


def case_model(case, check_runs=True):
    name, guidance, H, rows, dim, pair, pipes = case
    m = build(guidance, H, dim)
    inputs = [make_inputs(m, case, k) for k in range(K_INPUTS)]
    with torch.no_grad():
        run(m, inputs[0], False)                  # packs the weights (the device's forward-number counter exists from here on)
    lay = pipe_layout(m._native(), rows)
    if check_runs:
        assert lay["runs"] == (1 if pipes else 0), (name, lay)
    return m, inputs


def first_outputs(case, check_runs=True):
    """The per-step forward of every input of a case (what the launch-chain worker computes too)."""
    m, inputs = case_model(case, check_runs)
    with torch.no_grad():
        outs = [run(m, inp, False)[0].cpu() for inp in inputs]
    return m, inputs, outs, pipe_layout(m._native(), case[3])["runs"]


# ---- (a) forward numbers ------------------------------------------------------------------------------------------------------
def _deltas(m, inp, precomputed, n=6):
    seen = [epoch(m)]
    with torch.no_grad():
        for _ in range(n):
            run(m, inp, precomputed)
            seen.append(epoch(m))
    return [b - a for a, b in zip(seen, seen[1:])]


@pytest.mark.parametrize("path", ["per_step", "precomputed"])
def test_every_forward_draws_a_new_number(path):
    """Per-step conditioning: the reset kernel draws the number; precomputed: the chained first level's workgroup 0 does."""
    case = CASES[CASE_IDS.index("free_h16_pair")]
    m, inputs = case_model(case)
    d = _deltas(m, inputs[0], path == "precomputed")
    assert d == [1] * len(d), (path, d)


def test_a_graph_replay_draws_one_number_per_unet_forward():
    from autonomous_driving_with_diffusion_model_amd import _lib as L
    from autonomous_driving_with_diffusion_model_amd import scheduler as S
    from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler, generate_traj
    from helpers import SCHED_KW
    from test_gpu_model import make_model
    m, cfg = make_model("FREE_GUIDANCE", 16)
    cfg.EVAL.SAMPLE_STEPS, cfg.GUIDANCE.FREE_SCALE = 10, 7.5
    sch = S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
    ds = [{k: v.to(DEV) for k, v in P.synthetic_batch(1, 16, image_hw=(64, 96), seed=s).items()} for s in (41, 42)]
    lib = L.lib()
    fwd, calls = lib.adx_unet_forward, [0]

    def counting(*a):
        calls[0] += 1
        return fwd(*a)
    with torch.no_grad():
        generate_traj(m, sch, cfg, ds[0]["imgs"], ds[0]["target"], ds[0]["init_trajs"])    # packs, sizes the workspace
        e0 = epoch(m)
        lib.adx_unet_forward = counting
        try:
            generate_traj(m, sch, cfg, ds[1]["imgs"], ds[1]["target"], ds[1]["init_trajs"])
        finally:
            lib.adx_unet_forward = fwd
        n_fwd, e1 = calls[0], epoch(m)
        assert n_fwd == cfg.EVAL.SAMPLE_STEPS and e1 - e0 == n_fwd, ("eager", n_fwd, e1 - e0)
        assert pipe_layout(m._native(), 2)["runs"] == 1
        gs = GraphedSampler(m, sch, cfg)
        gs(ds[0]["imgs"], ds[0]["target"], ds[0]["init_trajs"])                          # captures (and replays once)
        for d in (ds[1], ds[0], ds[1]):
            a = epoch(m)
            gs(d["imgs"], d["target"], d["init_trajs"])
            assert epoch(m) - a == n_fwd, ("graph replay", epoch(m) - a, n_fwd)


def test_two_models_share_one_sequence_of_numbers():
    ca, cb = CASES[CASE_IDS.index("free_h16_pair")], CASES[CASE_IDS.index("no_h16_r3")]
    ma, ia = case_model(ca)
    mb, ib = case_model(cb)
    seen = []
    with torch.no_grad():
        for i in range(12):
            m, inp, tag = (ma, ia[i % 3], ca[0]) if i % 2 == 0 else (mb, ib[i % 3], cb[0])
            run(m, inp, i % 4 >= 2)
            seen.append((tag, "precomputed" if i % 4 >= 2 else "per_step", epoch(m)))
    assert [b[2] - a[2] for a, b in zip(seen, seen[1:])] == [1] * 11, seen


def test_forward_numbers_without_chained_levels_and_on_the_launch_chain(tmp_path):
    """ADX_UNET_CHAIN=0 (read once per process): no chained level opens the precomputed forward, the reset kernel draws its
    number, and the pipeline still runs.  ADX_UNET_PIPE=0: the launch chain, which the export must report as not taking the
    pipeline (no pipeline image is packed, so the device's counter is never made and nothing reads a tag)."""
    for switch, runs in (("ADX_UNET_CHAIN", 1), ("ADX_UNET_PIPE", 0)):
        out = tmp_path / f"{switch}.json"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pipe_handoff_worker.py"), "epochs", str(out)],
                           env=dict(os.environ, **{switch: "0"}), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        res = json.loads(out.read_text())
        assert res["runs"] == runs, (switch, res)
        if runs:
            for path in ("per_step", "precomputed"):
                assert res[path] == [1] * len(res[path]), (switch, path, res[path])


# ---- (b) + (c) interleaved inputs, clean and poisoned -------------------------------------------------------------------------
def _interleave(models_inputs, form, poisoned, refs=None):
    """Run ORDER over (model, input) pairs; every forward of a pair must give the pair's bits.  Returns the references."""
    refs = {} if refs is None else refs
    use_pre = FORMS[form]
    with torch.no_grad():
        for pos, k in enumerate(ORDER):
            m, inp, tag = models_inputs[k]
            if poisoned:
                poison(m, inp["rows"])
            y = run(m, inp, use_pre(pos))
            path = "precomputed" if use_pre(pos) else "per_step"
            if poisoned:
                assert all(bool(torch.isfinite(v).all()) for v in y), (tag, form, path, pos, "non-finite after poisoning")
            if k not in refs:
                refs[k] = (y, f"{path} forward {pos} of the clean run")
            else:
                for a, b in zip(y, refs[k][0]):
                    assert torch.equal(a, b), (tag, form, f"{path} forward {pos}", "poisoned" if poisoned else "clean", f"input {k}",
                                               "differs from its " + refs[k][1], (a - b).abs().max().item())
    return refs


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_interleaved_inputs_give_their_own_bits(case, form):
    m, inputs = case_model(case)
    mi = [(m, inputs[k], case[0]) for k in range(K_INPUTS)]
    refs = _interleave(mi, form, poisoned=False)
    assert not torch.equal(refs[0][0][0], refs[1][0][0]) and not torch.equal(refs[1][0][0], refs[2][0][0]), case[0]
    _interleave(mi, form, poisoned=True, refs=refs)


@pytest.mark.parametrize("form", ["per_step", "mixed"])
def test_rows_switching_on_one_model(form):
    """2 <-> 5 rows on one model: the records and block outputs move with the rows (both take the pipeline launch)."""
    c2 = ("no_h16_r2", "NO_GUIDANCE", 16, 2, 64, False, True)
    c5 = ("no_h16_r5", "NO_GUIDANCE", 16, 5, 64, False, True)
    m = build("NO_GUIDANCE", 16)
    i2, i5, i2b = make_inputs(m, c2, 0), make_inputs(m, c5, 0), make_inputs(m, c2, 1)
    with torch.no_grad():
        run(m, i5, False)
    for c in (c2, c5):
        assert pipe_layout(m._native(), c[3])["runs"] == 1, c
    assert pipe_layout(m._native(), 2)["records"] != pipe_layout(m._native(), 5)["records"]
    mi = [(m, i2, "rows2"), (m, i5, "rows5"), (m, i2b, "rows2b")]
    refs = _interleave(mi, form, poisoned=False)
    _interleave(mi, form, poisoned=True, refs=refs)


@pytest.mark.parametrize("form", ["per_step", "mixed"])
def test_two_models_with_different_weights_alternate_on_one_stream(form):
    case = CASES[CASE_IDS.index("free_h16_pair")]
    ma = build("FREE_GUIDANCE", 16, seed=0)
    mb = build("FREE_GUIDANCE", 16, seed=1)
    ia = make_inputs(ma, case, 0)
    ib = make_inputs(mb, case, 0)            # the same input: only the weights differ
    ib2 = make_inputs(mb, case, 1)
    mi = [(ma, ia, "model_a"), (mb, ib, "model_b"), (mb, ib2, "model_b_input1")]
    refs = _interleave(mi, form, poisoned=False)
    assert not torch.equal(refs[0][0][0], refs[1][0][0])
    _interleave(mi, form, poisoned=True, refs=refs)


# ---- (d) fp64 and the launch chain -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def launch_chain(tmp_path_factory):
    """Every case's first forwards in a process of its own under ADX_UNET_PIPE=0 (the launch chain)."""
    out = tmp_path_factory.mktemp("launch") / "outs.pt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pipe_handoff_worker.py"), "outputs", str(out)],
                       env=dict(os.environ, ADX_UNET_PIPE="0"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(out)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_each_forward_against_fp64_and_the_launch_chain(case, launch_chain):
    name = case[0]
    m, inputs, outs, runs = first_outputs(case)
    lc = launch_chain[name]
    assert lc["runs"] == 0, (name, "the ADX_UNET_PIPE=0 process took the pipeline")
    errs = []
    for k, inp in enumerate(inputs):
        truth = oracle64(m, inp)
        e_pipe = (outs[k].double() - truth).abs().max().item()
        e_launch = (lc["outs"][k].double() - truth).abs().max().item()
        e_between = (outs[k] - lc["outs"][k]).abs().max().item()
        errs.append((k, e_pipe, e_launch, e_between))
        print(f"PIPE_ERR {name} input={k} runs={runs} pipe_vs_fp64={e_pipe:.3e} launch_vs_fp64={e_launch:.3e} "
              f"pipe_vs_launch={e_between:.3e}", flush=True)
    for k, e_pipe, e_launch, e_between in errs:
        if not runs:                      # both processes ran the launch chain: the same kernels, the same bits
            assert torch.equal(outs[k], lc["outs"][k]), (name, k, e_between)
        assert e_pipe <= FP64_BAR[name], (name, k, "pipeline vs fp64", e_pipe)
        assert e_launch <= FP64_BAR[name], (name, k, "launch chain vs fp64", e_launch)
        assert e_pipe <= 2 * e_launch + SLACK, (name, k, "pipeline vs 2x launch chain", e_pipe, e_launch)
