"""CPU: the launch plan of an eval UNet forward (adx_unet_plan_describe, include/adx.h) for every row count 1..R_MAX, and the rule
that reduces those plans to the row counts tests/test_gpu_unet_rows.py runs on the GPU (tests/unet_plan.py: plan_cases).

How a forward runs is a function of its rows: the pipeline launch of the deepest level, the chains' samples per workgroup, the
K-split kernel's staging budget (one chunk or two), its reduction split (16, 8, 4, 2, 1; ticket words or a reduce launch), the
short-K pair and the mixed launch all flip at some row count, and every kernel has a partial last row tile when rows % bt != 0.
The export is the forward's own host code with a recorder in place of the launches, so these tests read the thresholds off
the code instead of restating them, and a threshold that moves changes the GPU case list by itself.

GPU forwards per configuration (plan_cases, R_MAX = 640; printed by test_plan_cases_cover_every_signature_and_both_sides_of_
every_change, run with -s to see them).  The plan does not depend on the guidance mode (asserted below), so NO_GUIDANCE and
FREE_GUIDANCE share a count:

    H   DIM  DIM_MULTS      cases  distinct (layer, signature)   reached by rows {1,2,3,4,5,7,8,9,64,128} (the suite before)
    16   64  (1, 2, 4, 8)     17        58                          45
    24   64  (1, 2, 4, 8)     21        85                          56
    32   64  (1, 2, 4, 8)     10        52                          40
    64   64  (1, 2, 4, 8)     10        50                          46
    16   64  (1, 2, 4)         6        22                          20
    24   64  (1, 2, 4)        13        57                          42
    32   64  (1, 2, 4)         4        21                          20
    64   64  (1, 2, 4)         4        33                          31

All eight configurations under both guidance modes would be 170 forwards, above the cap of 150: the GPU module runs H = 16 and
H = 32 at the default width under both modes (54 forwards) and each of the other six under one mode (58), 112 in all
(GPU_CONFIGS below; the coverage rule is the same everywhere).

The two-chunk staging of the K-split kernel (the 1024-channel concat layers of the up path, ck < cin_pad) starts at 513 rows
at horizon 16, 257 at horizon 32 and 129 at horizon 64 -- nowhere in the row counts the suite ran before."""
import pytest

import unet_plan as UP

WIDTHS = ((64, (1, 2, 4, 8)), (64, (1, 2, 4)))
HORIZONS = (16, 24, 32, 64)
BEFORE = (1, 2, 3, 4, 5, 7, 8, 9, 64, 128)      # rows of whole UNet forwards in the suite before this module
CAP = 150
GPU_CONFIGS = UP.GPU_CONFIGS


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from autonomous_driving_with_diffusion_model_amd import _lib
    return _lib


_PLANS = {}


def all_plans(lib, H, dim, mults, use_cond="NO_GUIDANCE", flags=UP.ASSUME_PACKED):
    key = (H, dim, mults, use_cond, flags)
    if key not in _PLANS:
        h = UP.make_handle(H, dim, mults, use_cond)
        try:
            _PLANS[key] = UP.plans(h, UP.R_MAX, flags)      # the export succeeds for every rows in 1..R_MAX (L.check raises otherwise)
        finally:
            lib.lib().adx_unet_destroy(h)
    return _PLANS[key]


CONFIGS = [(H, dim, mults) for dim, mults in WIDTHS for H in HORIZONS]


@pytest.mark.parametrize("H,dim,mults", CONFIGS)
def test_every_record_is_consistent_with_its_row_count_and_the_scratch(lib, H, dim, mults):
    from helpers import pipe_layout
    h = UP.make_handle(H, dim, mults)
    try:
        for rows, recs in all_plans(lib, H, dim, mults).items():
            lay = pipe_layout(h, rows)
            ksplit_floats = lay["ksplit_bytes"] // 4
            assert recs, rows
            for i, r in enumerate(recs):
                ctx = (H, dim, mults, rows, i, UP.describe(r))
                if r["family"] == "aux" and r["aux"] == 2:      # the ticket reset: one workgroup, no rows
                    assert r["grid"] == 1, ctx
                    continue
                assert r["bt"] >= 1 and r["row_tiles"] * r["bt"] >= rows > (r["row_tiles"] - 1) * r["bt"], ctx
                assert r["rows_mod_bt"] == rows % r["bt"], ctx
                if r["family"] == "reduce":       # one workgroup per (row tile, channel tile) of the split launch before it
                    prev = recs[i - 1]
                    assert prev["reduce"] == 2 and UP.layer_key(prev)[:3] == UP.layer_key(r)[:3], ctx
                    assert r["grid"] == r["row_tiles"] * r["ctiles"], ctx
                elif r["family"] == "pipeline":   # every row in one tile; ctiles = 7 stages x P + the finisher
                    assert r["row_tiles"] == 1 and r["grid"] == r["ctiles"] == 7 * lay["P"] + 1, ctx
                elif r["family"] != "aux":
                    assert r["grid"] == r["row_tiles"] * (r["ctiles"] * r["ksplit"] + r["ctiles_b"]), ctx
                assert (r["conv_b"] >= 0) == (r["family"] in ("shortk_pair", "mixed")) == (r["ctiles_b"] > 0), ctx
                if r["family"] in ("ksplit", "mixed", "shortk", "shortk_pair", "exact") and r["ksplit"] == 1:
                    assert r["chunks"] == -(-r["cin_pad"] // r["ck"]) >= 1, ctx
                if r["ksplit"] > 1:
                    # a split has ticket words or a reduce launch behind it, and its partial tiles sit inside the part of the forward's
                    # scratch that is ahead of the pipeline's records (pipe_layout: ksplit_bytes)
                    assert r["family"] in ("ksplit", "mixed", "reduce"), ctx
                    assert r["reduce"] in (1, 2), ctx
                    if r["reduce"] == 2 and r["family"] != "reduce":
                        assert i + 1 < len(recs) and recs[i + 1]["family"] == "reduce", ctx
                    assert r["part_off"] == 0 and 0 < r["part_floats"] <= ksplit_floats, ctx
                    assert r["part_floats"] % (r["row_tiles"] * r["ctiles"] * r["ksplit"]) == 0, ctx
                else:
                    assert r["reduce"] == 0 and r["part_off"] == -1 and r["part_floats"] == 0, ctx
            # the pipeline family appears exactly where adx_unet_pipe_describe says the shape fits (the plans above are those of a
            # process that has packed; without ADX_PLAN_ASSUME_PACKED it appears exactly where `runs`)
            n_pipe = sum(r["family"] == "pipeline" for r in recs)
            assert n_pipe == lay["shape_ok"], (H, dim, mults, rows)
            if rows <= 12 or rows % 97 == 0:
                here = UP.plan(h, rows, flags=0)
                assert sum(r["family"] == "pipeline" for r in here) == lay["runs"], (H, dim, mults, rows)
    finally:
        lib.lib().adx_unet_destroy(h)


@pytest.mark.parametrize("H,dim,mults", CONFIGS)
def test_the_plan_does_not_depend_on_the_guidance_mode(lib, H, dim, mults):
    a, b = all_plans(lib, H, dim, mults, "NO_GUIDANCE"), all_plans(lib, H, dim, mults, "FREE_GUIDANCE")
    assert a == b


def test_plan_cases_cover_every_signature_and_both_sides_of_every_change(lib):
    total_all, total_gpu = 0, 0
    print()
    for H, dim, mults in CONFIGS:
        ap = all_plans(lib, H, dim, mults)
        cases = UP.plan_cases(ap)
        cs = set(cases)
        every, reached = UP.coverage(ap, cs)
        assert reached == every, sorted(every - reached)[:5]
        # both sides of every change of every layer, and a partial and a full last tile in every run that has them
        table = UP.signature_table(ap)
        rows_all = sorted(ap)
        for k, by_rows in table.items():
            for sig, rr in UP.runs_of(by_rows, rows_all):
                assert rr[0] in cs and rr[-1] in cs, (H, dim, mults, k, rr[0], rr[-1])
                if sig is None:
                    continue
                for ragged in (True, False):
                    have = [r for r in rr if (by_rows[r][1] != 0) == ragged]
                    assert not have or cs & set(have), (H, dim, mults, k, sig, ragged)
        # nothing changes between the last boundary and R_MAX ... and nothing new appears up to 2048 rows: R_MAX is past every threshold
        h = UP.make_handle(H, dim, mults)
        try:
            for rows in list(range(UP.R_MAX + 1, 2049, 37)) + [1024, 1025, 2048]:
                for r in UP.plan(h, rows):
                    assert (UP.layer_key(r), UP.signature(r)) in every, (H, dim, mults, rows, UP.describe(r))
        finally:
            lib.lib().adx_unet_destroy(h)
        assert max(c for c in cases if c != UP.R_MAX) < UP.R_MAX - 64, cases
        _, before = UP.coverage(ap, set(BEFORE))
        two = [rows for rows in rows_all if any(r["family"] in ("ksplit", "mixed") and r["chunks"] > 1 for r in ap[rows])]
        print(f"H={H:2d} dim={dim} mults={mults}: {len(cases):2d} GPU cases {cases}; {len(every)} distinct (layer, signature), "
              f"{len(before)} reached by rows {BEFORE}; two-chunk K-split staging from rows "
              f"{two[0] if two else 'never'}")
        total_all += 2 * len(cases)
    for H, dim, mults, _ in GPU_CONFIGS:
        total_gpu += len(UP.plan_cases(all_plans(lib, H, dim, mults)))
    print(f"all configurations x both guidance modes: {total_all} forwards; the GPU module runs {total_gpu} (cap {CAP})")
    assert total_gpu <= CAP
    # the GPU module keeps H = 16 and 32 at the default width under both modes and every other configuration under one
    assert {(H, dim, mults) for H, dim, mults, _ in GPU_CONFIGS} == set(CONFIGS)
    for H in (16, 32):
        assert sum(c[:3] == (H, 64, (1, 2, 4, 8)) for c in GPU_CONFIGS) == 2


def test_the_two_chunk_staging_of_the_concat_layers_starts_above_the_old_row_counts(lib):
    """What the export shows for the K-split kernel's second staged chunk (tconv_hs.hip: hs_tile leaves the 140 KB budget once the
    grid no longer fits one workgroup per CU): the 1024-channel concat conv and its 1x1 residual conv of the deepest up level, from
    513 rows at horizon 16, 257 at horizon 32 and 129 at horizon 64 -- above every row count a whole forward ran at before."""
    for H, first in ((16, 513), (32, 257), (64, 129)):
        ap = all_plans(lib, H, 64, (1, 2, 4, 8))
        two = {rows: [r for r in recs if r["family"] in ("ksplit", "mixed") and r["chunks"] > 1] for rows, recs in ap.items()}
        rows2 = sorted(rows for rows, rr in two.items() if rr)
        assert rows2 == list(range(first, UP.R_MAX + 1)), (H, rows2[:3])
        assert first > max(BEFORE)
        for r in two[first]:
            assert (r["cin_pad"], r["ck"], r["chunks"], r["group"], r["block"]) == (1024, 512, 2, 5, 0), UP.describe(r)
        assert sorted(r["conv"] for r in two[first]) == [0, 2]


def test_op_level_plan_matches_the_layer_inside_the_model(lib):
    """adx_tconv_plan_describe for the concat layer alone gives the record the UNet export gives for it (same functions, and the
    scratch a forward hands its convs)."""
    from helpers import pipe_layout
    H = 32
    h = UP.make_handle(H)
    try:
        for rows in (2, 33, 129, 256, 257, 300):
            lay = pipe_layout(h, rows)
            want = [r for r in UP.plan(h, rows) if (r["group"], r["block"], r["conv"]) == (5, 0, 0)]
            d = lib.TConvDesc(0, 5, 1, 2, 512, 512, 256, 4, 4, 8, 1e-5)
            got = UP.tconv_plan(d, rows, scratch_floats=lay["ksplit_bytes"] // 4, tickets=True)
            assert len(got) == len(want) == 1
            for k in UP.SIGNATURE + ("row_tiles", "grid", "part_floats"):
                assert got[0][k] == want[0][k], (rows, k, got[0][k], want[0][k])
    finally:
        lib.lib().adx_unet_destroy(h)


def test_plan_export_refuses_bad_arguments(lib):
    import ctypes as C
    L = lib
    h = UP.make_handle(16)
    try:
        ints, n = (L.i32 * (256 * len(UP.FIELDS)))(), L.i32(0)
        f = L.lib().adx_unet_plan_describe
        assert f(None, 1, 0, C.byref(n), ints, 256) == -1
        assert f(h, 0, 0, C.byref(n), ints, 256) == -1
        assert f(h, 1, 4, C.byref(n), ints, 256) == -1
        assert f(h, 1, 0, None, ints, 256) == -1
        assert f(h, 1, 0, C.byref(n), None, 256) == -1
        assert f(h, 1, 0, C.byref(n), ints, 3) == -1 and b"room for 3" in L.lib().adx_last_error()
        assert f(h, 1, 0, C.byref(n), ints, 256) == 0 and n.value > 3
    finally:
        L.lib().adx_unet_destroy(h)


def test_a_precomputed_time_bias_drops_the_conditioning_launches_and_nothing_else(lib):
    """ADX_PLAN_TIME_BIAS: the forward of a sampling loop (adx_unet_io::time_bias) has no embedding and no fused block Linear, and
    where its first level is chained that launch clears the ticket words, so the reset launch goes too; every conv launch is the
    one of the forward that computes its own conditioning."""
    for H, dim, mults in ((16, 64, (1, 2, 4, 8)), (32, 64, (1, 2, 4, 8)), (24, 64, (1, 2, 4, 8))):
        h = UP.make_handle(H, dim, mults)
        try:
            for rows in (1, 2, 5, 6, 33, 129, 257, 640):
                own = UP.plan(h, rows)
                pre = UP.plan(h, rows, flags=UP.ASSUME_PACKED | UP.TIME_BIAS)
                convs = [r for r in own if r["family"] != "aux" and r["conv"] != 7]
                assert [r for r in pre if r["family"] != "aux"] == convs, (H, rows)
                assert [r["aux"] for r in own if r["family"] == "aux"] == [2, 1], (H, rows)          # ticket reset, embedding
                chained_first = convs[0]["family"] == "chain"
                assert [r["aux"] for r in pre if r["family"] == "aux"] == ([] if chained_first else [2]), (H, rows)
        finally:
            lib.lib().adx_unet_destroy(h)


SWITCH_CHILD = r'''
import sys
sys.path.insert(0, "tests")
import unet_plan as UP
for H in (16, 32):
    h = UP.make_handle(H)
    fams = sorted({r["family"] for rows in (1, 2, 5, 33, 129, 257, 640) for r in UP.plan(h, rows)})
    print("FAMILIES", H, ",".join(fams))
'''


@pytest.mark.parametrize("switch,value,gone,stays", [
    ("ADX_UNET_CHAIN", "0", {"chain"}, {"pipeline", "ksplit", "shortk", "shortk_pair", "mixed"}),
    ("ADX_UNET_PIPE", "0", {"pipeline"}, {"chain", "ksplit", "shortk", "shortk_pair", "mixed"}),
    ("ADX_TCONV_EXACT", "1", {"chain", "pipeline", "ksplit", "shortk", "shortk_pair", "mixed"}, {"exact"}),
    ("ADX_UNET_CHAIN", "1", set(), {"chain", "pipeline", "ksplit", "shortk", "shortk_pair", "mixed"}),
])
def test_the_export_honours_the_process_wide_switches(lib, switch, value, gone, stays):
    """The switches are read once per process, by the forward and by the export alike: a child per setting."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("ADX_UNET_CHAIN", "ADX_UNET_PIPE", "ADX_TCONV_EXACT", "ADX_CHAIN_MASK")}
    env[switch] = value
    r = subprocess.run([sys.executable, "-c", SWITCH_CHILD], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("FAMILIES")]
    assert len(lines) == 2, r.stdout
    seen = set()
    for _, H, fams in lines:
        seen |= set(fams.split(","))
    assert not seen & gone and stays <= seen, (switch, value, sorted(seen))
