"""CPU: the unit walk of the persistent 16x16x32 conv launches (csrc/conv2d_internal.h: hs3x3q_walk, exported as
adx_conv2d_hs3x3q_walk from the range and unit functions conv2d_hs3x3q_kernel itself uses; the kernel's own loop is covered by
tests/test_gpu_hs3x3q_walk.py).  A launch is `units` = spatial tiles x
cout tiles pieces, unit u = spatial tile * cout_tiles + cout tile; XCD x owns [x units / 8, (x + 1) units / 8) and workgroup
(x, slot) of a grid of 8 Q visits slot, slot + Q, ... of that range.  Any grid must cover every unit exactly once, and a grid that
leaves two CUs per XCD free must cost no round on the B = 64 shapes of the perception pass (adx_resnet_plan_grids)."""
import ctypes as C

import pytest

import __graft_entry__ as g

g.build()
from autonomous_driving_with_diffusion_model_amd import _lib as L  # noqa: E402

GRIDS = (256, 240, 224, 8)
# spatial tiles x cout tiles: the three B = 64 shapes (128 / 256 / 512 channels), then small and odd ranges
SHAPES = [(912, 1), (232, 2), (60, 4)] + [(sp, ct) for sp in (1, 7, 9, 61) for ct in (1, 2, 4)]


def walk(units, cout_tiles, grid):
    """[(spatial tile, cout tile), ...] per workgroup, in visiting order."""
    counts, visits = (L.i32 * grid)(), (L.i32 * (2 * units))()
    L.check(L.lazy("adx_conv2d_hs3x3q_walk")(units, cout_tiles, grid, counts, visits), "adx_conv2d_hs3x3q_walk")
    out, at = [], 0
    for b in range(grid):
        out.append([(visits[2 * i], visits[2 * i + 1]) for i in range(at, at + counts[b])])
        at += counts[b]
    assert at == units
    return out


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("sp,ct", SHAPES)
def test_walk_covers_every_unit_once(sp, ct, grid):
    units, q = sp * ct, grid // 8
    w = walk(units, ct, grid)
    flat = [s * ct + c for wg in w for s, c in wg]
    assert all(0 <= c < ct and 0 <= s < sp for wg in w for s, c in wg)
    assert sorted(flat) == list(range(units))                      # every unit exactly once
    lengths = []
    for x in range(8):
        mine = sorted(s * ct + c for b in range(x, grid, 8) for s, c in w[b])
        lo, hi = x * units // 8, (x + 1) * units // 8
        assert mine == list(range(lo, hi))                         # a contiguous range per XCD
        lengths.append(hi - lo)
        for slot in range(q):                                      # slot, slot + Q, ... in order
            assert [s * ct + c for s, c in w[8 * slot + x]] == list(range(lo + slot, hi, q))
    assert max(lengths) - min(lengths) <= 1
    assert max(len(wg) for wg in w) == max(-(-n // q) for n in lengths)        # the deepest workgroup: ceil(range / Q)


@pytest.mark.parametrize("sp,ct,rounds", [(912, 1, 4), (232, 2, 2), (60, 4, 1)])
@pytest.mark.parametrize("grid", (256, 240))
def test_b64_shapes_keep_their_rounds_with_two_cus_per_xcd_free(sp, ct, rounds, grid):
    """128 / 256 / 512 channels at B = 64 (and the block entries that produce those maps): 114 / 58 / 30 units per XCD run in
    4 / 2 / 1 rounds on 32 workgroups per XCD and on 30."""
    w = walk(sp * ct, ct, grid)
    assert sp * ct // 8 == {1: 114, 2: 58, 4: 30}[ct] and sp * ct % 8 == 0
    assert max(len(wg) for wg in w) == rounds


def _resnet():
    h = L.vp()
    L.check(L.lib().adx_resnet_create(512, C.byref(h)), "adx_resnet_create")
    return h


@pytest.mark.parametrize("reserve,per_xcd", [(0, 32), (16, 30)])
def test_plan_grids_follow_the_reserve(reserve, per_xcd):
    """adx_resnet_plan_grids at B = 64, 256 x 900, one chain (a capture's plan) on 256 CUs with the plan's reserve pinned to 0 and
    to 16 (as ADX_HS_RESERVE_CUS pins it per process): the reserve reaches every persistent launch's grid through the plan field,
    min(longest range, (256 - reserve) / 8) workgroups per XCD; with -1 the plan's own reserve (0: no default changed) answers."""
    h = _resnet()
    try:
        cap = 64
        n, ints = L.i32(0), (L.i32 * (cap * 6))()
        L.check(L.lazy("adx_resnet_plan_grids")(h, 64, 256, 900, 1, 256, reserve, C.byref(n), ints, cap), "adx_resnet_plan_grids")
        recs = [ints[6 * i:6 * i + 6] for i in range(n.value)]
        persistent = [r for r in recs if r[0] == 1]
        assert len(persistent) == 26                               # 23 stride-1 convs + 3 block entries on the 16x16x32 kernel
        for _, units, slots, grid, plan_reserve, usable in persistent:
            assert plan_reserve == reserve and usable == 256 - reserve
            assert slots == min(-(-units // 8), per_xcd) and grid == 8 * slots
        assert sorted({r[1] for r in persistent}) == [240, 464, 912]
        L.check(L.lazy("adx_resnet_plan_grids")(h, 64, 256, 900, 1, 256, -1, C.byref(n), ints, cap), "adx_resnet_plan_grids")
        assert all(ints[6 * i + 4] == 0 and ints[6 * i + 5] == 256 for i in range(n.value))
    finally:
        L.lib().adx_resnet_destroy(h)
