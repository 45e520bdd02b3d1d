"""GPU: the flat unit walk of conv2d_hs3x3q_kernel (csrc/conv2d_hs16.hip) changes which workgroup computes a tile and in which
order, never a bit of the result.  The cell-layout launches of tests/hs3x3q_walk_worker.py -- stride 1 with and without a cell
residual, two block entries, one perception pass at B = 32 -- in this process (the default grid) and in child processes that leave
16 CUs free on one chain (ADX_HS_RESERVE_CUS=16 ADX_RESNET_STREAMS=1) or cap the grid at 8 workgroups (ADX_HS_GRID_CAP=8: one
workgroup per XCD, walks several units deep with the cout tile changing on the way), against the same launches with
ADX_HS_PERSIST=0 (one unit per workgroup, no walk).  The shapes: tests/hs3x3q_walk_worker.py.  The training forward and
data-gradient instantiations walk the same way: one small training step under the cap against ADX_HS_PERSIST=0."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
SWITCHES = ("ADX_HS_PERSIST", "ADX_HS_RESERVE_CUS", "ADX_HS_GRID_CAP", "ADX_RESNET_STREAMS")


def child(tmp_path_factory, name, **env):
    out = str(tmp_path_factory.mktemp("walk") / f"{name}.pt")
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hs3x3q_walk_worker.py"), out], env=dict(base, **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(out)


@pytest.fixture(scope="module")
def one_unit_per_workgroup(tmp_path_factory):
    return child(tmp_path_factory, "persist0", ADX_HS_PERSIST="0")


def same(got, ref):
    import hs3x3q_walk_worker as W
    assert set(got) == set(ref) and len(got) == 2 * len(W.CONVS) + 2 * len(W.ENTRIES) + 1
    for k, v in got.items():
        assert torch.equal(v, ref[k]), k


@pytest.fixture(scope="module")
def in_process():
    import hs3x3q_walk_worker as W
    return W.outputs()


def test_default_grid_matches_one_unit_per_workgroup(in_process, one_unit_per_workgroup):
    same(in_process, one_unit_per_workgroup)


def test_reserve_16_matches(in_process, one_unit_per_workgroup, tmp_path_factory):
    """Reserve 16 under the default plan's streams: every launch and the perception features are bit for bit the default's."""
    got = child(tmp_path_factory, "reserve16", ADX_HS_RESERVE_CUS="16")
    same(got, one_unit_per_workgroup)
    assert torch.equal(got["perception"], in_process["perception"])


def test_reserve_16_on_one_chain_matches(in_process, one_unit_per_workgroup, tmp_path_factory):
    """Reserve 16 on one chain (ADX_RESNET_STREAMS=1).  The launches are bit-identical; the perception features are bit for bit
    those of one chain with one unit per workgroup.  Against the DEFAULT plan (two sub-batches of 16 at B = 32) one chain is not
    bit-equal and was not before the walk: a sub-batch of 16 and a batch of 32 take different tile modes on some layers
    (tests/test_gpu_model.py::test_perception_sub_batch_streams_match_the_single_stream_pass), measured 3.3e-6 at |f| <= 7.7
    with the parent library and with this one alike -- so there the bound is that test's 2e-6 x scale."""
    got = child(tmp_path_factory, "reserve16_one_chain", ADX_HS_RESERVE_CUS="16", ADX_RESNET_STREAMS="1")
    one = child(tmp_path_factory, "persist0_one_chain", ADX_HS_PERSIST="0", ADX_RESNET_STREAMS="1")
    same(got, one)
    for k in got:
        if k != "perception":
            assert torch.equal(got[k], one_unit_per_workgroup[k]), k
    ref = in_process["perception"]
    err, scale = (got["perception"] - ref).abs().max().item(), max(1.0, ref.abs().max().item())
    print(f"one chain, reserve 16, against the default plan: max |diff| = {err:.3e} at scale {scale:.3f}")
    assert err <= 2e-6 * scale, (err, scale)


def test_grid_capped_to_8_workgroups_matches(one_unit_per_workgroup, tmp_path_factory):
    same(child(tmp_path_factory, "cap8", ADX_HS_GRID_CAP="8"), one_unit_per_workgroup)


def test_training_launches_under_a_capped_grid_match(tmp_path):
    """`conv2d_hs3x3q_kernel<DMA, 1>` (training forward: fp32 output + BatchNorm partial sums per tile) and `<DMA, 2>` (data gradient
    + the consumer BatchNorm's backward sums, whose constants are per cout tile) on a deep walk: one NO_GUIDANCE training step at
    B = 8, 128 x 450 -- 30 x 1, 8 x 2 and 4 x 4 (spatial tiles x cout tiles) units on the 128 / 256 / 512-channel layers, so one
    workgroup per XCD (ADX_HS_GRID_CAP=8) visits two to four units and changes cout tile on the way -- against ADX_HS_PERSIST=0, both
    with ADX_WGRAD_DETERMINISTIC=1: same loss bits, and every gradient tensor that two ADX_HS_PERSIST=0 runs reproduce bit for bit
    (the encoder's 3x3 conv weights among them, as in tests/test_gpu_train.py's full-size comparison) has the same checksums."""
    import json
    runs = {}
    for tag, env in (("a", {"ADX_HS_PERSIST": "0"}), ("b", {"ADX_HS_PERSIST": "0"}), ("cap8", {"ADX_HS_GRID_CAP": "8"})):
        out = str(tmp_path / f"{tag}.json")
        base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "train_checksum_worker.py"), out, "8", "32", "128", "450", "7"],
                           env=dict(base, ADX_WGRAD_DETERMINISTIC="1", **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        runs[tag] = json.load(open(out))
    stable = [k for k, v in runs["a"]["sums"].items() if runs["b"]["sums"][k] == v]
    enc = [k for k in stable if k.startswith("perception.layer") and (k.endswith("conv1.weight") or k.endswith("conv2.weight"))]
    print(f"{len(stable)} of {len(runs['a']['sums'])} gradient tensors reproduce, {len(enc)} encoder 3x3 weights among them")
    assert len(enc) >= 28, (len(stable), len(enc))
    assert runs["a"]["loss"] == runs["cap8"]["loss"]
    diff = [k for k in stable if runs["cap8"]["sums"][k] != runs["a"]["sums"][k]]
    assert diff == [], diff[:8]
