"""GPU: the cell convs compute, bit for bit, what they computed at the commit named in tests/golden/conv_handover_parent.json.

Work that removes instructions from these kernels without touching the arithmetic must not change a bit of their outputs:
conv2d_hs3x3q_kernel (csrc/conv2d_hs16.hip) takes the gather offsets of a workgroup's second and later tiles from the words the
previous visit parked in LDS, and a launch without a residual runs an epilogue without the residual path; the PAIR form of
conv2d_hs3x3_kernel (csrc/conv2d_hs.hip) has such an epilogue too and pitches the k-halves of its patch image 688 cells apart
(profiles/README.md, "Cell convs").  The check is a SHA-256 per output against the file, recorded with that commit's library
(the inputs come from CPU generators, so the digests do not depend on the machine):

  * the launches of tests/hs3x3q_walk_worker.py -- stride 1 with and without a cell residual, both outputs of the block entries
    -- on the default grid, under ADX_HS_GRID_CAP=8 (one workgroup per XCD, two to six units deep with the cout tile changing:
    every visit but the first takes its offsets from LDS) and under ADX_HS_PERSIST=0 (every tile a first tile: offsets computed);
  * the PAIR form on 64 -> 64 at B = 3, 17 x 33 and B = 2, 9 x 29 (an image boundary inside a 32-column tile, a partial row tile):
    fp32 and cell input, cell output, with and without a cell residual, ReLU on and off -- and each of these against an fp64
    evaluation under the bar of tests/test_gpu_conv2d_pair.py.

To record the file again (on the commit to compare against): python tests/test_gpu_conv2d_handover.py OUT.json COMMIT."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_handover_parent.json")
SWITCHES = ("ADX_HS_PERSIST", "ADX_HS_RESERVE_CUS", "ADX_HS_GRID_CAP", "ADX_RESNET_STREAMS")
WALKS = {"default": {}, "cap8": {"ADX_HS_GRID_CAP": "8"}, "persist0": {"ADX_HS_PERSIST": "0"}}
PAIR_CASES = ((64, 64, 3, 17, 33), (64, 64, 2, 9, 29))         # (cin, cout, n, h, w)
DEV = "cuda:0"


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def walk_keys():
    import hs3x3q_walk_worker as W
    keys = [f"conv {cin}x{cout}b{b}@{h}x{w} res={r}" for cin, cout, b, h, w in W.CONVS for r in (0, 1)]
    keys += [f"entry {cin}x{cout}b{b}@{h}x{w} {o}" for cin, cout, b, h, w in W.ENTRIES for o in ("conv1", "downsample")]
    return keys


def walk_digests(name, tmp_dir):
    """Digests of the worker's conv and entry outputs under the switches of WALKS[name]: the default grid in this process when no
    switch of the walk is set for it, anything else in a child (the switches are read once per process)."""
    import hs3x3q_walk_worker as W
    env = WALKS[name]
    if not env and not any(k in os.environ for k in SWITCHES):
        out = W.outputs()
    else:
        path = os.path.join(str(tmp_dir), f"{name}.pt")
        base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hs3x3q_walk_worker.py"), path], env=dict(base, **env),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out = torch.load(path)
    return {k: digest(out[k]) for k in walk_keys()}


@functools.lru_cache(maxsize=None)
def pair_inputs(case):
    import conv_pair_worker as P
    return P.inputs(case)


@functools.lru_cache(maxsize=None)
def pair_refs(case):
    """fp64 references of a case per (residual, relu), their maxima, and the error of torch's own fp32 convs (CPU and GPU,
    whichever is worse) against them, as tests/test_gpu_conv2d_pair.py computes its bar: once per case."""
    x, wt, sc, sh, res = pair_inputs(case)
    ref = F.conv2d(x.double(), wt.double(), padding=1)
    f32 = F.conv2d(x, wt, padding=1)
    g32 = F.conv2d(x.to(DEV), wt.to(DEV), padding=1).cpu()
    out = {}
    for with_res in (False, True):
        for relu in (False, True):
            def post(c):
                y = c * sc.to(c.dtype)[None, :, None, None] + sh.to(c.dtype)[None, :, None, None]
                y = y + res.to(c.dtype) if with_res else y
                return torch.relu(y) if relu else y
            r = post(ref)
            den = r.abs().max().item() + 1e-300
            out[(with_res, relu)] = (r, den, max((post(t).double() - r).abs().max().item() / den for t in (f32, g32)))
    return out


def pair_outputs(case):
    """{key: cell output} of a PAIR case in every form the test covers."""
    import conv_pair_worker as P
    from autonomous_driving_with_diffusion_model_amd import ops
    assert P.cells_supported(case), case
    cin, cout, n, h, w = case
    x, wt, sc, sh, res = (t.to(DEV) for t in pair_inputs(case))
    _, packed = ops.conv2d(x[:1], wt, stride=1, pad=1)
    xc, rc = ops.to_cells(x), ops.to_cells(res)
    out = {}
    for x_cells in (False, True):
        for with_res in (False, True):
            for relu in (False, True):
                y = ops.conv2d_cells(xc if x_cells else x, packed, cin, cout, n, h, w, x_cells=x_cells, scale=sc, shift=sh,
                                     res=rc if with_res else None, res_cells=with_res, relu=relu)
                out[f"pair {cin}x{cout}b{n}@{h}x{w} xcells={int(x_cells)} res={int(with_res)} relu={int(relu)}"] = y
    torch.cuda.synchronize()
    return out


def pair_digests():
    return {k: digest(v) for case in PAIR_CASES for k, v in pair_outputs(case).items()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(WALKS))
def test_walk_launches_match_the_parent_bit_for_bit(name, golden, tmp_path):
    got = walk_digests(name, tmp_path)
    want = golden["walk"][name]
    assert set(got) == set(want) and len(got) == len(walk_keys())
    diff = [k for k in got if got[k] != want[k]]
    assert diff == [], diff
    # the walk never changes a bit either: all three recordings of the parent agree, so do these
    assert want == golden["walk"]["persist0"]


pair_on = pytest.mark.skipif(os.environ.get("ADX_CONV_EXACT") == "1" or os.environ.get("ADX_HS_MODE") is not None or
                             os.environ.get("ADX_HS_PAIR") == "0", reason="the PAIR form is switched off for this process")


@pair_on
@pytest.mark.parametrize("case", PAIR_CASES)
def test_pair_form_matches_the_parent_bit_for_bit(case, golden):
    got = {k: digest(v) for k, v in pair_outputs(case).items()}
    assert len(got) == 8
    diff = [k for k in got if got[k] != golden["pair"][k]]
    assert diff == [], diff


@pytest.mark.parametrize("case", PAIR_CASES)
def test_pair_cases_are_fp32_grade(case):
    from test_gpu_conv2d_pair import BAR
    from autonomous_driving_with_diffusion_model_amd import ops
    cin, cout, n, h, w = case
    refs = pair_refs(case)
    for key, y in pair_outputs(case).items():
        with_res, relu = "res=1" in key, "relu=1" in key
        r, den, e_f32 = refs[(with_res, relu)]
        e_hip = (ops.from_cells(y, (n, cout, h, w)).double().cpu() - r).abs().max().item() / den
        print(key, e_hip, e_f32)
        assert e_f32 > 0
        # (+ the 2^-22 of a residual held as hi + lo / 2^11 and of the split output, as tests/test_gpu_conv2d_pair.py allows)
        assert e_hip <= BAR * e_f32 + 4e-7, (key, e_hip, e_f32)


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        rec = {"commit": sys.argv[2], "what": "sha256 of each output's bytes; see tests/test_gpu_conv2d_handover.py",
               "walk": {name: walk_digests(name, tmp) for name in WALKS}, "pair": pair_digests()}
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
