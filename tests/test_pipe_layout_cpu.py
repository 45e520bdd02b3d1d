"""CPU: adx_unet_pipe_describe (include/adx.h) -- where a UNet forward keeps the hand-off state of the deepest level's pipeline
launch (csrc/tconv_pipe.hip) in the caller's workspace.  The GPU tests poison those regions between forwards
(tests/test_gpu_pipe_handoff.py), so the layout itself must be right: inside the workspace, 16-byte aligned, disjoint, the
K-split launches' part of the scratch ahead of the pipeline's records.  adx_unet_create needs no GPU."""
import ctypes
import itertools

import pytest

from helpers import pipe_layout


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from autonomous_driving_with_diffusion_model_amd import _lib
    return _lib


def _create(L, H, dim=64, mults=(1, 2, 4, 8), guidance=0):
    cfg = L.UnetConfig()
    cfg.horizon, cfg.transition_dim, cfg.dim, cfg.n_mults, cfg.guidance = H, 7, dim, len(mults), guidance
    for i, m in enumerate(mults):
        cfg.dim_mults[i] = m
    h = L.vp()
    assert L.lib().adx_unet_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, L.lib().adx_last_error()
    return h


# Where pipe_shape_ok admits the deepest level's seven convs (csrc/tconv_pipe.hip).  One workgroup holds its weight share for the
# live taps in LDS plus the stage's whole input tile (M = rows x L rows of C channels, as fp32 and as fp16 hi / lo cells) within
# 150 KB.  Default model, H = 16: C = 512, L = 2, three live taps = 96 KB of weights, and 4128 bytes per row on top of them
# leave M <= 11, so rows <= 5.  H = 32: five live taps = 160 KB of weights alone: never.  DIM = 32, H = 16: C = 256, 48 KB of
# weights; the 16-row tile (rows x L <= 16) and 8 GroupNorm groups x rows <= 64 stop it at rows = 8.
CASES = [
    # (H, dim, guidance, rows tried, rows that fit)
    (16, 64, 0, range(1, 10), range(1, 6)),
    (16, 64, 1, range(1, 10), range(1, 6)),
    (16, 64, 2, range(1, 10), range(1, 6)),
    (32, 64, 0, range(1, 6), range(0)),
    (32, 64, 1, range(1, 6), range(0)),
    (16, 32, 0, range(1, 10), range(1, 9)),
    (16, 32, 1, range(1, 10), range(1, 9)),
]


@pytest.mark.parametrize("H,dim,guidance,tried,fits", CASES)
def test_pipe_layout_is_inside_the_workspace_aligned_and_disjoint(lib, H, dim, guidance, tried, fits):
    h = _create(lib, H, dim, guidance=guidance)
    try:
        for rows in tried:
            d = pipe_layout(h, rows)
            ctx = (H, dim, guidance, rows, d)
            assert d["shape_ok"] == (1 if rows in fits else 0), ctx
            assert d["runs"] <= d["shape_ok"], ctx
            assert (d["C"], d["L"], d["P"]) == (8 * dim, H // 8, 8 * dim // 16), ctx
            assert (d["n_tickets"], d["epoch_slot"]) == (256, 240), ctx
            ws = d["workspace_bytes"]
            assert ws == lib.lib().adx_unet_workspace_bytes(h, rows), ctx
            regions = {"tickets": (d["tickets"], 4 * d["n_tickets"]), "ksplit": (d["scratch"], d["ksplit_bytes"])}
            assert 0 < d["ksplit_bytes"] < d["scratch_bytes"], ctx
            assert d["scratch"] + d["scratch_bytes"] <= ws, ctx
            if d["shape_ok"]:
                # seven stages x P workgroups x 16 rows x 6 units of 16 bytes; block outputs [rows x L][C] fp32
                assert d["record_bytes"] == 7 * d["P"] * 16 * 6 * 16, ctx
                assert d["y_bytes"] == 4 * rows * d["L"] * d["C"], ctx
                regions["records"] = (d["records"], d["record_bytes"])
                for k in ("ya", "yb", "yc"):
                    regions[k] = (d[k], d["y_bytes"])
                # the K-split launches' part of the scratch ends before the records begin, and the pipeline's tail is in the scratch
                assert d["scratch"] + d["ksplit_bytes"] <= d["records"], ctx
                for k in ("records", "ya", "yb", "yc"):
                    o, n = regions[k]
                    assert d["scratch"] + d["ksplit_bytes"] <= o and o + n <= d["scratch"] + d["scratch_bytes"], (k, ctx)
            else:
                assert all(d[k] == -1 for k in ("records", "record_bytes", "ya", "yb", "yc", "y_bytes")), ctx
            for k, (o, n) in regions.items():
                assert o % 16 == 0 and n > 0 and 0 <= o and o + n <= ws, (k, ctx)
            for (ka, (oa, na)), (kb, (ob, nb)) in itertools.combinations(regions.items(), 2):
                assert oa + na <= ob or ob + nb <= oa, (ka, kb, ctx)
    finally:
        lib.lib().adx_unet_destroy(h)


def test_pipe_describe_refuses_bad_arguments(lib):
    L = lib
    h = _create(L, 16)
    try:
        ints, offs = (L.i32 * 8)(), (L.i64 * 12)()
        assert L.lib().adx_unet_pipe_describe(None, 2, ints, offs) == -1
        assert L.lib().adx_unet_pipe_describe(h, 2, None, offs) == -1
        assert L.lib().adx_unet_pipe_describe(h, 2, ints, None) == -1
        for rows in (0, -1, -(2 ** 31)):
            assert L.lib().adx_unet_pipe_describe(h, rows, ints, offs) == -1, rows
            assert b"rows" in L.lib().adx_last_error()
        assert L.lib().adx_unet_pipe_describe(h, 2, ints, offs) == 0
    finally:
        L.lib().adx_unet_destroy(h)
