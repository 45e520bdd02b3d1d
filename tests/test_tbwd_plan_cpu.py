"""No GPU: the launch geometry of the temporal stack's backward (tests/tbwd_plan.py).  The weight gradient's plan
(adx_tconv_wgrad_plan_describe, the function tconv_wgrad itself calls) keeps its invariants on every layer of eight configurations at
batches 1..160, and the op-level case list tests/test_gpu_tbwd.py runs takes both sides of every geometry flip."""
import pytest

import tbwd_plan as T


@pytest.fixture(scope="module")
def tables():
    return {cfg: T.layer_table(cfg[0], cfg[1], cfg[2]) for cfg in T.SWEEP_CONFIGS}


def test_layer_table_matches_the_native_model(tables):
    """The table is written from csrc/unet.hip's structure; the native object agrees with it where it can be asked without a GPU:
    the last conv of every launch of an eval forward (its cout and lout, from adx_unet_plan_describe) is a row of the table, and
    the fused time Linear is as wide as the blocks' outputs together (adx_unet_time_bias_width)."""
    import unet_plan as UP
    for (H, dim, mults), table in tables.items():
        assert table[-1].name == "tlin" and table[-1].d.cout == sum(l.d.cout for l in table if l.name.endswith(".a"))
        n = len(mults)
        # 2 blocks per down level, 2 mid, 2 per up level, each with convs a and b; the blocks whose width changes add conv r
        assert sum(l.name.endswith((".a", ".b")) for l in table) == 2 * (2 * n + 2 + 2 * (n - 1))
        assert sum(l.name.endswith(".down") for l in table) == n - 1 == sum(l.name.endswith(".up") for l in table)
        assert sum(l.dgrad is None for l in table) == 2           # the noisy trajectory: conv a and conv r of the first block
        h = UP.make_handle(H, dim, mults)
        have = {(l.d.cout, l.d.lout) for l in table}
        for r in UP.plan(h, 3):
            if r["family"] not in ("aux", "reduce"):
                assert (r["cout"], r["lout"]) in have, (H, dim, r)
        from autonomous_driving_with_diffusion_model_amd import _lib as L
        assert L.lib().adx_unet_time_bias_width(h) == table[-1].d.cout
        L.lib().adx_unet_destroy(h)


def test_dgrad_desc_forms(tables):
    """Every form dgrad_desc produces occurs in the default model: stride-1 (flipped taps, swapped roles), a strided conv's
    (kind 1), an upsample's (kind 0, stride 2), the time Linear's."""
    forms = {T.dgrad_form(l.dgrad) for l in tables[(32, 64, (1, 2, 4, 8))] if l.dgrad is not None}
    assert forms == {"of_stride1", "of_strided", "of_upsample", "tlin"}
    assert all(l.dgrad.exact == 1 for t in tables.values() for l in t if l.dgrad is not None)


def test_wgrad_plan_invariants_on_every_layer_and_batch(tables):
    seen = 0
    for cfg, table in tables.items():
        for d in T.distinct_launches(table)[0]:
            cin = d.c0 + d.c1
            for batch in range(1, T.B_MAX + 1):
                p = T.wgrad_plan(d, batch)
                ctx = (cfg, d, batch, p)
                assert p["per4"] == (1 if d.lout >= 4 else 4 // d.lout), ctx
                assert p["n_ci_tiles"] * 16 >= cin > (p["n_ci_tiles"] - 1) * 16, ctx
                assert p["n_co_tiles"] * 16 * p["nfo"] >= d.cout > (p["n_co_tiles"] - 1) * 16 * p["nfo"], ctx
                assert p["tiles"] == p["n_ci_tiles"] * p["n_co_tiles"] and p["grid"] == p["tiles"] * p["nsplit"], ctx
                # the splits [i nb, min((i + 1) nb, batch)) cover [0, batch) exactly once, none of them empty
                assert p["nsplit"] >= 1 and p["nb"] >= 1, ctx
                assert (p["nsplit"] - 1) * p["nb"] < batch <= p["nsplit"] * p["nb"], ctx
                assert p["nb"] % p["per4"] == 0 and p["sbt"] % p["per4"] == 0 and 1 <= p["sbt"] <= p["nb"], ctx
                assert (p["sbt"] * d.lout) % 4 == 0, ctx
                # 8 K-steps per wave x 4 waves x 4 rows: the kernel's KSW loop drops the rows of a super-tile beyond 128
                assert p["sbt"] * d.lout <= 128, ctx
                # staged tile: every tap of every output position reads inside its sample's [0, lp) columns
                lo = min(l * d.stride + t - d.pad for l in range(d.lout) for t in range(d.taps)) + p["pl"]
                hi = max(l * d.stride + t - d.pad for l in range(d.lout) for t in range(d.taps)) + p["pl"]
                assert lo >= 0 and hi < p["lp"] and p["pl"] + d.lin <= p["lp"], ctx
                assert p["rs"] >= p["sbt"] * p["lp"], ctx
                assert p["lds_stage"] == 4 * 16 * p["rs"] and p["lds_red"] == 4 * 16 * p["nfo"] * 16 * d.taps, ctx
                assert max(p["lds_stage"], p["lds_red"]) <= p["lds_bytes"] <= 65536, ctx
                seen += 1
    assert seen > 10000


def test_op_cases_cover_both_sides_of_every_flip(tables):
    """The case list of tests/test_gpu_tbwd.py reaches every geometry of the weight gradient and of the data gradient that a kernel
    bug could hide behind; a list without one of them fails here."""
    assert T.n_cases() <= 40
    names = [c[0] for c in T.WGRAD_CASES + T.DGRAD_CASES + T.TLIN_DGRAD_CASES + T.GN_CASES + T.BIAS_CASES]
    assert len(set(names)) == len(names)
    missing = T.WGRAD_REQUIRED - T.wgrad_case_flips()
    assert not missing, missing
    need = T.dgrad_required()
    assert {v for k, v in need if k == "nf"} == {1, 2, 4} and {v for k, v in need if k == "nw"} == {4, 8, 16}
    missing = need - T.dgrad_case_flips()
    assert not missing, missing
    # the weight gradient's other paths: every tap count, stride 2, the mirrored descriptor, every way x is read, and real lengths
    # below the padded ones on stride-1, stride-2 and mirrored launches
    assert {d.taps for _, d, _, _ in T.WGRAD_CASES} == {1, 3, 4, 5}
    assert {x for _, _, _, x in T.WGRAD_CASES} == {"dense", "bhd", "tlin"}
    assert any(d.c1 > 0 for _, d, _, _ in T.WGRAD_CASES)
    kinds = {(d.kind, d.stride) for _, d, _, _ in T.WGRAD_CASES}
    masked = {(d.kind, d.stride) for _, d, _, _ in T.WGRAD_CASES if d.lin_valid > 0}
    assert kinds == masked == {(0, 1), (0, 2), (1, 2)}
    assert {(d.lin_valid, d.lin) for _, d, _, _ in T.WGRAD_CASES if d.lin_valid} >= {(6, 8), (3, 4), (5, 8)}
    # the data gradient: every form, each with and without accumulation into the output (res == y) somewhere, masked lengths
    forms = {T.dgrad_form(T.dgrad_desc(d)) for _, d, _, _ in T.DGRAD_CASES}
    assert forms == {"of_stride1", "of_strided", "of_upsample"} and len(T.TLIN_DGRAD_CASES) >= 1
    assert {acc for _, _, _, acc in T.DGRAD_CASES} == {False, True}
    assert {T.dgrad_form(T.dgrad_desc(d)) for _, d, _, _ in T.DGRAD_CASES if d.lin_valid > 0} == forms
    # every op-level case is a launch some configuration the reference accepts makes, or a narrower one of the same kernel: the
    # plans exist (the descriptors pass the library's own checks)
    for _, d, batch, _x in T.WGRAD_CASES:
        T.wgrad_plan(T.mirror_desc(d) if d.kind == 1 else d, batch)
    # GroupNorm backward: every group size the kernel's chunk loop distinguishes, L = 64, a masked length, both pointers absent once
    assert {C // 8 * L for _, _, C, L, _, _, _ in T.GN_CASES} == {64, 128, 256, 512}
    assert any(L == 64 for _, _, _, L, _, _, _ in T.GN_CASES) and any(0 < lv < L for _, _, _, L, lv, _, _ in T.GN_CASES)
    assert {dtb for *_, dtb, _ in T.GN_CASES} == {False, True} == {dbi for *_, dbi in T.GN_CASES}
    assert {B for _, B, *_ in T.GN_CASES} == {37, 128}
    assert any(B * L > 256 for _, B, _, L, _, _ in T.BIAS_CASES) and any(lay == "tlin" for *_, lay in T.BIAS_CASES)
    assert any(0 < lv < L for _, _, _, L, lv, _ in T.BIAS_CASES)


def test_coverage_check_notices_a_missing_case():
    """Without the only nfo = 2 case, the only cout < 16 case or the two-chunk data gradients the coverage sets come out short."""
    without = tuple(c for c in T.WGRAD_CASES if c[0] != "w64-32.L16.b3")
    assert T.WGRAD_REQUIRED - T.wgrad_case_flips(without) == {("nfo", 2)}
    without = tuple(c for c in T.WGRAD_CASES if c[0] != "w64-7.L32.b9")
    assert T.WGRAD_REQUIRED - T.wgrad_case_flips(without) == {("nfo", 1), ("cout<16", True)}
    one_chunk = tuple(c for c in T.DGRAD_CASES if T.dgrad_plan(T.dgrad_desc(c[1]), c[2])["chunks"] < 2)
    assert len(one_chunk) < len(T.DGRAD_CASES)
    assert T.dgrad_required() - T.dgrad_case_flips(one_chunk) == {("chunks>=2", True)}


def test_wgrad_plan_describe_refuses_bad_arguments():
    import ctypes as C
    from autonomous_driving_with_diffusion_model_amd import _lib as L
    ints = (L.i32 * len(T.WG_FIELDS))()
    d = T.c_desc(T.conv_desc(0, 5, 1, 2, 64, 0, 64, 16, 16, 8))
    assert L.lib().adx_tconv_wgrad_plan_describe(C.byref(d), 0, ints) != 0
    assert L.lib().adx_tconv_wgrad_plan_describe(C.byref(d), 4, None) != 0
    up = T.c_desc(T.conv_desc(1, 4, 2, 1, 64, 0, 64, 8, 16))
    assert L.lib().adx_tconv_wgrad_plan_describe(C.byref(up), 4, ints) != 0
    assert b"mirrored" in L.lib().adx_last_error()
