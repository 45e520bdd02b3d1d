"""CPU: the plan of a ResNet-34 eval forward (adx_resnet_plan_describe, include/adx.h) for every batch 1..96 at five image sizes,
outside and inside a stream capture.  The export runs resnet_eval_plan (csrc/conv2d_internal.h), the pure function the
executor carries out, and needs no device.

Checked per case: every read finds the tensor it expects, in the format its producer wrote, in a buffer nothing has overwritten;
the sub-batches tile the batch and keep to regions and scratch slices of their own inside the workspace; the formats equal a
restatement of the format rule driven by adx_conv2d_cells_supported at each segment's batch; and, for one chain on the whole
batch, the cell layers are the ones read off the predicate before the plan existed (PINNED)."""
import ctypes as C
import os

import pytest

if any(k.startswith("ADX_") for k in os.environ):      # the switches are read once per process and change the plan
    pytest.skip("an ADX_* switch is set", allow_module_level=True)

SIZES = ((32, 32), (64, 96), (97, 131), (129, 515), (256, 900))
BATCHES = range(1, 97)
FIELDS = ("segment", "stream", "n0", "n", "nf", "kind", "block", "conv", "H", "W", "OH", "OW", "cin", "cout", "fmt", "x", "res", "y", "y2",
          "scratch_off", "scratch_floats", "status", "nsub", "first_split")
KINDS = ("stem_pool", "stem", "maxpool", "conv", "entry", "avgpool_fc")
X, Y, RES = 1, 2, 4
STEM_BUF = 3
# ResNet-34: (planes, blocks) per layer; the first block of layers 2..4 has stride 2 and a downsample conv
LAYERS = ((64, 3), (128, 4), (256, 6), (512, 3))
BLOCKS = [(li, bi, LAYERS[li - 1][0] if bi == 0 and li > 0 else pl, pl, li > 0 and bi == 0)       # layer, index in it, cin, cout, has_ds
          for li, (pl, nb) in enumerate(LAYERS) for bi in range(nb)]
# single chain, nf = batch: {image sizes: [(first batch, last batch, layers whose tensors are cells)]}
PINNED = {
    ((32, 32), (64, 96)): [(1, 8, {1}), (9, 16, {1, 4}), (17, 32, {1, 3, 4}), (33, 96, {1, 2, 3, 4})],
    ((97, 131),): [(1, 8, {1}), (9, 16, {1, 4}), (17, 96, {1, 2, 3, 4})],
    ((129, 515),): [(1, 3, {1}), (4, 4, {1, 2}), (5, 8, {1, 2, 3}), (9, 96, {1, 2, 3, 4})],
    ((256, 900),): [(1, 2, {1}), (3, 4, {1, 2}), (5, 8, {1, 2, 3}), (9, 96, {1, 2, 3, 4})],
}


def out_dim(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def align64(v):
    return (v + 63) // 64 * 64


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from autonomous_driving_with_diffusion_model_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def handle(lib):
    h = lib.vp()
    lib.check(lib.lib().adx_resnet_create(64, C.byref(h)), "adx_resnet_create")
    yield h
    lib.lib().adx_resnet_destroy(h)


_PLANS = {}


def plan(lib, handle, hw, batch, flags):
    key = (hw, batch, flags)
    if key not in _PLANS:
        cap = 256
        ints, n = (lib.i32 * (cap * len(FIELDS)))(), lib.i32(0)
        lib.check(lib.lib().adx_resnet_plan_describe(handle, batch, hw[0], hw[1], flags, C.byref(n), ints, cap), "adx_resnet_plan_describe")
        recs = [dict(zip(FIELDS, ints[i * len(FIELDS):(i + 1) * len(FIELDS)])) for i in range(n.value)]
        for r in recs:
            r["kind"] = KINDS[r["kind"]]
        _PLANS[key] = recs
    return _PLANS[key]


def segments(recs):
    """{segment: its records in issue order}"""
    out = {}
    for r in recs:
        out.setdefault(r["segment"], []).append(r)
    return out


CASES = [(hw, flags) for hw in SIZES for flags in (0, 1)]


@pytest.mark.parametrize("hw,flags", CASES)
def test_every_read_finds_its_tensor_in_the_format_it_was_written_in(lib, handle, hw, flags):
    for batch in BATCHES:
        segs = segments(plan(lib, handle, hw, batch, flags))
        left = {}                                    # what the prefix leaves in the buffers: {buffer: (tensor, cells)}
        for sid in sorted(segs):
            content = dict(left)
            for r in segs[sid]:
                ctx = (hw, batch, flags, sid, r)
                b, k = r["block"], r["kind"]
                before = ("out", b - 1) if b > 0 else ("pooled",)
                has_ds = b >= 0 and BLOCKS[b][4]
                if k in ("stem_pool", "stem"):
                    reads, writes = [], [(r["y"], ("pooled",) if k == "stem_pool" else ("stem",))]
                elif k == "maxpool":
                    reads, writes = [(r["x"], ("stem",), False)], [(r["y"], ("pooled",))]
                elif k == "entry":
                    reads, writes = [(r["x"], before, r["fmt"] & X)], [(r["y"], ("mid", b)), (r["y2"], ("ds", b))]
                elif k == "conv" and r["conv"] == 0:
                    reads, writes = [(r["x"], before, r["fmt"] & X)], [(r["y"], ("mid", b))]
                elif k == "conv" and r["conv"] == 2:
                    reads, writes = [(r["x"], before, r["fmt"] & X)], [(r["y"], ("ds", b))]
                elif k == "conv":
                    reads = [(r["x"], ("mid", b), r["fmt"] & X), (r["res"], ("ds", b) if has_ds else before, r["fmt"] & RES)]
                    writes = [(r["y"], ("out", b))]
                else:
                    assert k == "avgpool_fc" and r["y"] == -1, ctx
                    reads, writes = [(r["x"], ("out", len(BLOCKS) - 1), r["fmt"] & X)], []
                for buf, tensor, cells in reads:     # the expected tensor, not overwritten since, in the format the reader takes
                    assert content.get(buf) == (tensor, bool(cells)), (ctx, buf, content.get(buf))
                outs = [buf for buf, _ in writes]
                assert len(set(outs)) == len(outs) and not set(outs) & {buf for buf, _, _ in reads}, ctx
                if k == "conv" and r["conv"] == 2:   # the downsample conv runs between conv1 and conv2: conv1's output is live
                    assert content[r["y"]][0] != ("mid", b), ctx
                for buf, tensor in writes:
                    assert 0 <= buf <= (STEM_BUF if tensor == ("stem",) else 2), ctx
                    content[buf] = (tensor, bool(r["fmt"] & Y))
            if sid == 0:
                left = content


@pytest.mark.parametrize("hw,flags", CASES)
def test_segments_tile_the_batch_inside_the_workspace(lib, handle, hw, flags):
    h1, w1 = out_dim(hw[0], 7, 2, 3), out_dim(hw[1], 7, 2, 3)
    h2, w2 = out_dim(h1, 3, 2, 1), out_dim(w1, 3, 2, 1)
    for batch in BATCHES:
        recs = plan(lib, handle, hw, batch, flags)
        segs = segments(recs)
        nsub, first_split = recs[0]["nsub"], recs[0]["first_split"]
        assert all((r["nsub"], r["first_split"]) == (nsub, first_split) for r in recs)
        # one chain when captured or below 32 images (a half would be under 16); two sub-batches otherwise, behind layer1
        assert nsub == (1 if flags & 1 or batch < 32 else 2), (hw, batch, flags, nsub)
        assert first_split == (3 if nsub > 1 else 0), (hw, batch, flags)
        subs = sorted(s for s in segs if s > 0)
        assert subs == list(range(1, nsub + 1)) and (0 in segs) == (first_split > 0), (hw, batch, flags, sorted(segs))
        stem_floats, act_floats = align64(batch * 64 * h1 * w1), align64(batch * 64 * h2 * w2)
        assert lib.lib().adx_resnet_workspace_bytes(handle, batch, hw[0], hw[1]) == 4 * (stem_floats + 3 * act_floats)
        at, regions, slices = 0, [], []
        for sid in sorted(segs):
            first = segs[sid][0]
            for r in segs[sid]:                      # one (stream, images, nf, scratch slice) per segment
                assert all(r[f] == first[f] for f in ("stream", "n0", "n", "nf", "scratch_off", "scratch_floats")), (hw, batch, flags, r)
            n0, n = first["n0"], first["n"]
            if sid == 0:
                assert (n0, n, first["nf"], first["stream"]) == (0, batch, batch, 0), (hw, batch, flags, first)
            else:
                assert (n0, first["nf"], first["stream"]) == (at, n, sid - 1) and n >= 1, (hw, batch, flags, first)
                at += n
            # the floats the segment's launches write, per buffer, from its first image's slot of the buffer's largest map
            ext = {}
            for r in segs[sid]:
                for buf in (r["y"], r["y2"]):
                    if buf >= 0:
                        ext[buf] = max(ext.get(buf, 0), n * r["cout"] * r["OH"] * r["OW"])
            for buf, floats in ext.items():
                start = n0 * 64 * (h1 * w1 if buf == STEM_BUF else h2 * w2)
                assert start + floats <= (stem_floats if buf == STEM_BUF else act_floats), (hw, batch, flags, sid, buf)
                if sid > 0:
                    regions.append((buf, start, start + floats))
            lo, hi = 64 * first["scratch_off"], 64 * (first["scratch_off"] + first["scratch_floats"])
            assert hi <= stem_floats, (hw, batch, flags, sid)
            assert (hi > lo) == (STEM_BUF not in ext), (hw, batch, flags, sid)       # scratch only where the stem map is never written
            if sid > 0 and hi > lo:
                slices.append((STEM_BUF, lo, hi))
        assert at == batch, (hw, batch, flags)
        for spans in (regions, slices):              # pairwise disjoint between the sub-batches
            for i, (ba, a0, a1) in enumerate(spans):
                for bb, b0, b1 in spans[i + 1:]:
                    assert ba != bb or a1 <= b0 or b1 <= a0, (hw, batch, flags, spans)


def rule(lib, nf, hw2, b0, b1, in_cells):
    """The format rule (csrc/conv2d_internal.h) for blocks [b0, b1) of one chain at batch nf, restated on adx_conv2d_cells_supported:
    [(in_cells, mid_cells, id_cells, out_cells)] per block and the pooled map's format (None unless b0 == 0)."""
    def plain(cin, cout, H, W):
        return bool(lib.lib().adx_conv2d_cells_supported(C.byref(lib.Conv2dDesc(cin, cout, 3, 1, 1)), nf, H, W))

    def reads(b, H, W):           # a fused block entry reads what it finds; a plain block reads its input twice (conv1, conv2's residual)
        _, _, cin, cout, has_ds = BLOCKS[b]
        return has_ds or (plain(cin, cout, H, W) and plain(cout, cout, H, W))

    H, W = hw2
    for b in range(b0):           # the map size block b0 starts from
        if BLOCKS[b][4]:
            H, W = out_dim(H, 3, 2, 1), out_dim(W, 3, 2, 1)
    pooled = reads(0, H, W) if b0 == 0 else None
    cells, out = pooled if b0 == 0 else in_cells, []
    for b in range(b0, b1):
        _, _, cin, cout, has_ds = BLOCKS[b]
        r = reads(b, H, W)
        if has_ds:
            H, W = out_dim(H, 3, 2, 1), out_dim(W, 3, 2, 1)
        mid = plain(cout, cout, H, W) if has_ds else r
        o = plain(cout, cout, H, W) and (b + 1 == len(BLOCKS) or reads(b + 1, H, W))
        out.append((cells, mid, mid if has_ds else cells, o))
        cells = o
    return out, pooled


def formats(seg):
    """[(in_cells, mid_cells, id_cells, out_cells)] per block of a segment's records, and the pooled map's format."""
    out, pooled = {}, None
    for r in seg:
        if r["kind"] == "stem_pool":
            pooled = bool(r["fmt"] & Y)
        elif r["kind"] in ("entry", "conv") and r["conv"] == 0:
            out[r["block"]] = [bool(r["fmt"] & X), bool(r["fmt"] & Y), None, None]
        elif r["kind"] == "conv" and r["conv"] == 1:
            assert bool(r["fmt"] & X) == out[r["block"]][1], r
            out[r["block"]][2:] = [bool(r["fmt"] & RES), bool(r["fmt"] & Y)]
    return [tuple(out[b]) for b in sorted(out)], pooled


@pytest.mark.parametrize("hw,flags", CASES)
def test_formats_follow_the_rule_at_each_segments_batch(lib, handle, hw, flags):
    h2, w2 = out_dim(out_dim(hw[0], 7, 2, 3), 3, 2, 1), out_dim(out_dim(hw[1], 7, 2, 3), 3, 2, 1)
    for batch in BATCHES:
        recs = plan(lib, handle, hw, batch, flags)
        segs = segments(recs)
        first_split = recs[0]["first_split"]
        assert all(r["kind"] == "entry" for r in recs if r["conv"] == 0 and BLOCKS[r["block"]][4]), (hw, batch, flags)   # every entry fuses
        assert not any(r["kind"] in ("stem", "maxpool") or r["conv"] == 2 for r in recs), (hw, batch, flags)
        handed = None
        for sid in sorted(segs):
            got, pooled = formats(segs[sid])
            b0, b1 = (0, first_split) if sid == 0 else (first_split, len(BLOCKS))
            want, want_pooled = rule(lib, segs[sid][0]["nf"], (h2, w2), b0, b1, handed)
            assert got == want and pooled == want_pooled, (hw, batch, flags, sid, got, want)
            if sid == 0:
                handed = got[-1][3]          # the producer's decision stands at the hand-off


def test_one_chain_has_the_pinned_cell_layers(lib, handle):
    for sizes, rows in PINNED.items():
        assert [r[0] for r in rows] == [1] + [r[1] + 1 for r in rows[:-1]] and rows[-1][1] == BATCHES[-1]
        for hw in sizes:
            for lo, hi, layers in rows:
                for batch in range(lo, hi + 1):
                    recs = plan(lib, handle, hw, batch, 1)
                    got, pooled = formats(recs)
                    assert pooled is True and len(got) == len(BLOCKS), (hw, batch)
                    for (li, *_), (_, mid, _, out) in zip(BLOCKS, got):
                        assert mid == out == (li + 1 in layers), (hw, batch, li + 1, mid, out)


def test_batch_33_at_32x32_hands_cells_to_two_sub_batches_that_differ_in_layer3(lib, handle):
    segs = segments(plan(lib, handle, (32, 32), 33, 0))
    assert [(s, segs[s][0]["n0"], segs[s][0]["n"], segs[s][0]["nf"]) for s in sorted(segs)] == [(0, 0, 33, 33), (1, 0, 17, 17), (2, 17, 16, 16)]
    pre, _ = formats(segs[0])
    assert pre == [(True, True, True, True)] * 3               # layer1 at nf = 33
    for sid, layer3 in ((1, True), (2, False)):
        got, _ = formats(segs[sid])
        by_layer = {li + 1: {f for (l, *_), f in zip(BLOCKS[3:], got) if l == li} for li in (1, 2, 3)}
        assert got[0] == (True, False, False, False)            # layer2's block entry reads cells and writes fp32
        assert {f[1:] for f in by_layer[2]} == {(False, False, False)}
        assert {f[3] for f in by_layer[3]} == {layer3} and {f[3] for f in by_layer[4]} == {True}, (sid, by_layer)
        assert got[4][0] is False and got[4][1] is layer3       # layer3's entry reads fp32


def test_issue_order_prefix_first_then_the_sub_batches_block_by_block(lib, handle):
    recs = plan(lib, handle, (64, 96), 40, 0)
    order = [(r["segment"], r["block"]) for r in recs if r["conv"] in (-1, 1)]       # one entry per stem / block / pool
    want = [(0, -1)] + [(0, b) for b in range(3)] + [(s, b) for b in range(3, 16) for s in (1, 2)] + [(1, -1), (2, -1)]
    assert order == want
    assert [r["status"] for r in recs if r["conv"] in (-1, 1)] == [0, 1, 2, 3] + [1 + b for b in range(3, 16) for _ in (1, 2)] + [17, 17]


def test_plan_export_refuses_bad_arguments(lib, handle):
    f = lib.lib().adx_resnet_plan_describe
    ints, n = (lib.i32 * (256 * len(FIELDS)))(), lib.i32(0)
    assert f(None, 1, 32, 32, 0, C.byref(n), ints, 256) == -1
    assert f(handle, 0, 32, 32, 0, C.byref(n), ints, 256) == -1
    assert f(handle, 1, 31, 32, 0, C.byref(n), ints, 256) == -1 and b"too small" in lib.lib().adx_last_error()
    assert f(handle, 1, 32, 32, 2, C.byref(n), ints, 256) == -1
    assert f(handle, 1, 32, 32, 0, None, ints, 256) == -1
    assert f(handle, 1, 32, 32, 0, C.byref(n), None, 256) == -1
    assert f(handle, 1, 32, 32, 0, C.byref(n), ints, 3) == -1 and b"room for 3" in lib.lib().adx_last_error()
    assert f(handle, 1, 32, 32, 0, C.byref(n), ints, 256) == 0 and n.value == 1 + 16 * 2 + 1
