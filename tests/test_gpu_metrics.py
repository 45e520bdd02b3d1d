"""GPU: open-loop metrics -- the metrics kernel (adx_traj_metrics) against the fp64 restatement of "open-loop metrics v1"
(tests/metrics_ref.py) within the bound derived there, the decisions exactly (tests/test_metrics_cpu.py vets the margins of the
shared construction; every check here asserts them again first); the accumulation (adx_metrics_accumulate) bit for bit against
the host's fp64 sums over the kernel's own records, eagerly and replayed from a captured graph; evaluate_open_loop over a dataset
written in the reference's format.  No timing is asserted anywhere (tools/open_loop_eval.py and profiles/README.md measure)."""
import os

import numpy as np
import pytest
import torch

import metrics_ref as R
from autonomous_driving_with_diffusion_model_amd import DeviceNoise, OpenLoopMetrics, TrajectorySelector, evaluate_open_loop
from autonomous_driving_with_diffusion_model_amd import scheduler as S
from autonomous_driving_with_diffusion_model_amd.utils import procedural as P
from helpers import IMG_SMALL, SCHED_KW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _host(batch):
    torch.cuda.synchronize()
    return type(batch)(*(t.cpu().numpy() for t in batch))


def _launch(trajs, gt, valid=None, index=None, h0=1, metrics=None, blocked=None):
    m = OpenLoopMetrics(h0=h0, xy_scale=R.XY_SCALE) if metrics is None else metrics
    return m.update(_dev(trajs), _dev(gt), _dev(valid, torch.int32), index=_dev(index, torch.int32), blocked=_dev(blocked, torch.int32))


def _verify(got, trajs, gt, valid, index, h0, what):
    """The precondition first (every decision of the restatement clears twice the bound: it fails loudly, nothing is skipped),
    then floats within the bound and best, both miss fields and the flags exactly.  Returns (restatement, largest error / bound)."""
    ref = R.metrics(trajs, gt, valid, index, h0)
    b = R.bound(ref, h0)
    for s, m in R.margins(ref, b):
        for name, (margin, allowed) in m.items():
            assert margin > 2 * allowed, (what, "precondition", s, name, margin, allowed)
    worst = 0.0
    for name, g, r, e in (("ade", got.ade, ref.ade, b.ade), ("fde", got.fde, ref.fde, b.fde), ("disp_sel", got.disp_sel, ref.disp_sel, b.disp_sel),
                          ("rec", got.rec[:, :6], ref.rec[:, :6], b.rec[:, :6])):
        g = g.astype(np.float64)
        assert g.shape == r.shape, (what, name)
        finite = np.isfinite(r)
        assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(g[~finite & ~np.isnan(r)], r[~finite & ~np.isnan(r)]), (what, name)
        err = np.abs(g[finite] - r[finite])
        print(f"{what} {name}: max |kernel - fp64| = {err.max() if err.size else 0.0:.3e}, bound up to {e[finite].max() if err.size else 0.0:.3e}")
        assert (err <= e[finite]).all(), (what, name, float((err - e[finite]).max()))
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nan_to_num(err / e[finite], nan=0.0).max()) if err.size else 0.0)
    assert np.array_equal(got.best, ref.best), (what, got.best.tolist(), ref.best.tolist())
    assert np.array_equal(got.rec[:, 6:], ref.rec[:, 6:]), what
    assert np.array_equal(got.flags, ref.flags), (what, got.flags.tolist(), ref.flags.tolist())
    return ref, worst


def _bits_equal(a, b):
    return all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))


@pytest.mark.parametrize("Sn,K,H,D", R.SHAPES)
@pytest.mark.parametrize("h0", [0, 1])
def test_kernel_against_the_fp64_restatement(Sn, K, H, D, h0):
    """tests/metrics_ref.py: case() builds the inputs, bound() is the tolerance (gamma_{m+7} ade, gamma_7 fde, gamma_12 of the
    products of along / cross -- at most 5.1e-5 m at the 12 m errors of the largest shape), margins() the precondition.  Full
    rows with index NULL and with a given index; ragged `valid` holding 0, h0, h0 + 1 and values beyond both ends; an index outside
    [0, K): the scene is zeros; two launches: the same bits; the [K, S, H, D] layout."""
    trajs, gt, p = R.case(Sn, K, H, D)
    what = (Sn, K, H, D, h0)
    a = _host(_launch(trajs, gt, h0=h0))
    again = _host(_launch(trajs, gt, h0=h0))
    assert _bits_equal(a, again), what
    ref, worst = _verify(a, trajs, gt, None, None, h0, what)
    assert np.array_equal(ref.best, np.argsort(p, axis=1)[:, 0]) and (a.flags & 1).all()
    zeros = _host(_launch(trajs, gt, index=np.zeros(Sn, dtype=np.int32), h0=h0))
    assert _bits_equal(a, zeros), what                                     # index NULL is candidate 0
    four_d = OpenLoopMetrics(h0=h0, xy_scale=R.XY_SCALE).update(_dev(trajs).reshape(K, Sn, H, D), _dev(gt))
    assert _bits_equal(a, _host(four_d)), what
    rng = np.random.default_rng(7)
    index = rng.integers(0, K, size=Sn).astype(np.int32)
    index[0] = K - 1
    b = _host(_launch(trajs, gt, index=index, h0=h0))
    _verify(b, trajs, gt, None, index, h0, what + ("index",))
    assert _bits_equal((a.ade, a.fde, a.best), (b.ade, b.fde, b.best))       # the chosen candidate moves the record alone
    # ragged valid, every special length in some scene of some launch; the indices ride along
    lengths = (0, h0, h0 + 1, H, H + 3, -2, max(h0 + 2, H // 2))
    for start in range(0, len(lengths), Sn):
        valid = np.array([lengths[(start + s) % len(lengths)] for s in range(Sn)], dtype=np.int32)
        c = _host(_launch(trajs, gt, valid=valid, index=index, h0=h0))
        r, w = _verify(c, trajs, gt, valid, index, h0, what + ("valid", valid.tolist()))
        worst = max(worst, w)
        for s in range(Sn):
            if np.clip(valid[s], 0, H) <= h0:
                assert c.flags[s] == 0 and not c.ade[s].any() and not c.rec[s].any() and not c.disp_sel[s].any() and c.best[s] == 0
    # an index outside [0, K) leaves its scene unscored, whatever it is: it is never an address
    for bad in (-1, K, 1 << 30, -(1 << 31)):
        index2 = index.copy()
        index2[Sn - 1] = bad
        d = _host(_launch(trajs, gt, index=index2, h0=h0))
        _verify(d, trajs, gt, None, index2, h0, what + ("bad index", bad))
        assert d.flags[Sn - 1] == 0 and not d.ade[Sn - 1].any() and not d.fde[Sn - 1].any() and not d.rec[Sn - 1].any()
        assert not d.disp_sel[Sn - 1].any() and _bits_equal([x[:Sn - 1] for x in d], [x[:Sn - 1] for x in b])
    print(f"{what}: largest |error| / bound = {worst:.3f}")
    assert worst <= 1.0


def test_nan_candidates_ties_and_a_zero_length_heading():
    """A candidate with a NaN waypoint loses the search and, chosen, clears bit 2; two bit-identical rows tie to the lower index;
    a zero-length last logged segment clears bit 1 and zeroes along / cross."""
    Sn, K, H, D, h0 = 5, 7, 24, 3, 1
    trajs, gt, p = R.case(Sn, K, H, D)
    t = trajs.reshape(K, Sn, H, D).copy()
    order = np.argsort(p, axis=1)                                           # order[s, 0]: the best candidate of scene s
    # scenes 0 and 1: the best candidate gets a NaN waypoint; scene 0 chooses it, scene 1 does not
    t[order[0, 0], 0, 9, 1] = np.nan
    t[order[1, 0], 1, 3, 0] = np.nan
    # scene 2: the best row copied bit for bit over the row of another index
    other = order[2, 3]
    t[other, 2] = t[order[2, 0], 2]
    # scene 3: the last logged segment has no length; the candidates move with the waypoint, so every error stays what it was
    g = gt.copy()
    t[:, 3, H - 1, :2] += g[3, H - 2] - g[3, H - 1]
    g[3, H - 1] = g[3, H - 2]
    index = np.array([order[0, 0], order[1, 2], order[2, 1], order[3, 0], order[4, 5]], dtype=np.int32)
    got = _host(_launch(t, g, index=index, h0=h0))
    ref, _ = _verify(got, t, g, None, index, h0, "special")
    assert got.best[0] == order[0, 1] and got.best[1] == order[1, 1]                          # the NaN rows lost
    assert np.isnan(got.ade[0, order[0, 0]]) and np.isnan(got.rec[0, 2]) and got.flags[0] & 7 == 1 | 2
    assert got.flags[1] & 7 == 7 and np.isfinite(got.rec[1]).all()
    assert got.best[2] == min(other, order[2, 0])
    assert got.ade[2, other].view(np.uint32) == got.ade[2, order[2, 0]].view(np.uint32)
    assert got.flags[3] & 7 == 1 | 4 and got.rec[3, 4] == 0 and got.rec[3, 5] == 0 and got.rec[3, 3] > 0
    assert got.flags[4] & 7 == 7 and (got.rec[4, 4] != 0 or got.rec[4, 5] != 0)
    # every candidate NaN: nothing finite to find, the search answers 0
    t2 = t.copy()
    t2[:, 4, 5, 0] = np.nan
    got2 = _host(_launch(t2, g, index=index, h0=h0))
    _verify(got2, t2, g, None, index, h0, "all NaN")
    assert got2.best[4] == 0 and np.isnan(got2.rec[4, 0]) and got2.flags[4] & 4 == 0 and got2.rec[4, 6] == 0


def _batches():
    """Three batches of different content (and scene count) at H = 16: ragged lengths, chosen indices, `blocked`, an unscored scene
    and one non-finite chosen plan."""
    out = []
    for seed, (Sn, K) in enumerate(((3, 2), (5, 4), (2, 2))):
        trajs, gt, _ = R.case(Sn, K, 16, 7, seed=seed + 10)
        rng = np.random.default_rng(seed)
        valid = rng.integers(2, 17, size=Sn).astype(np.int32)
        index = rng.integers(0, K, size=Sn).astype(np.int32)
        blocked = rng.integers(0, 2, size=Sn).astype(np.int32)
        if seed == 1:
            valid[2], index[4] = 1, K                                             # nothing to score; out of range
            trajs.reshape(K, Sn, 16, 7)[index[0], 0, 1, 0] = np.nan              # a non-finite chosen plan
        out.append((trajs, gt, valid, index, blocked))
    return out


def test_accumulation_equals_the_host_sums_bit_for_bit_eagerly_and_from_a_graph():
    batches = _batches()
    m = OpenLoopMetrics(h0=1, xy_scale=R.XY_SCALE)
    counts, sums = R.fresh_state()
    for trajs, gt, valid, index, blocked in batches:
        got = _host(_launch(trajs, gt, valid, index, 1, m, blocked))
        _verify(got, trajs, gt, valid, index, 1, "batch")
        R.accumulate(counts, sums, got.rec, got.flags, got.best, index, got.disp_sel, blocked, 16)      # the kernel's own fp32 records
    dev_counts, dev_sums = m.words()
    count_words = list(range(5)) + list(range(R.W_DISP_COUNT, R.WORDS))
    sum_words = [w for w in range(R.WORDS) if w not in count_words]
    assert np.array_equal(dev_counts[count_words], counts[count_words]), (dev_counts[:5], counts[:5])
    assert np.array_equal(dev_sums[sum_words].view(np.int64), sums[sum_words].view(np.int64))
    assert counts[R.W_SCORED] == 8 and counts[R.W_NONFINITE] == 1 and np.isfinite(dev_sums[sum_words]).all()
    assert (counts[R.W_DISP_COUNT:R.W_DISP_COUNT + 16] <= 7).all() and counts[R.W_DISP_COUNT] == 0 and counts[R.W_DISP_COUNT + 1] == 7
    out = m.compute()
    units = out.pop("units")
    np.testing.assert_equal(out, R.summary(counts, sums, 16))
    assert units["xy_scale"] == R.XY_SCALE and out["n"] == 7 and out["nonfinite"] == 1 and len(out["disp_at"]) == 16
    assert out["min_ade_k"] <= out["ade"] and out["selector_regret"] >= 0 and 0 <= out["blocked_rate"] <= 1
    eager = dev_counts.copy()

    # the same three updates as nodes of one captured graph, on a state of its own
    g_m = OpenLoopMetrics(h0=1, xy_scale=R.XY_SCALE)
    static = [tuple(_dev(a, torch.int32 if a.dtype == np.int32 else None) for a in b) for b in batches]
    run = lambda: [g_m.update(t, g, v, index=i, blocked=b) for t, g, v, i, b in static]      # noqa: E731
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        run()                                                                  # warm-up off the capture; it also allocates the state
    torch.cuda.current_stream(DEV).wait_stream(side)
    g_m.reset()
    assert not g_m.words()[0].any()                                            # the reset launch left an empty state
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        keep = run()
    assert not g_m.words()[0].any()                                            # a capture runs nothing
    graph.replay()
    assert np.array_equal(g_m.words()[0], eager)
    assert _bits_equal(_host(keep[1]), _host(_launch(*batches[1][:4], 1, None, batches[1][4])))
    # reset() empties the state and forgets the horizon
    m.reset()
    assert not m.words()[0].any() and m.compute()["n"] == 0
    m.update(_dev(R.case(1, 1, 2, 2)[0]), _dev(R.case(1, 1, 2, 2)[1]))
    assert m.compute()["n"] == 1 and len(m.compute()["disp_at"]) == 2
    with pytest.raises(ValueError, match="horizon 2"):
        m.update(static[0][0], static[0][1])
    with pytest.raises(TypeError, match="int32"):
        g_m.update(static[0][0], static[0][1], index=static[0][3].long())


def _write_dataset(root, n, horizon=16, seed=0):
    from PIL import Image
    os.makedirs(os.path.join(root, "front"))
    os.makedirs(os.path.join(root, "waypoints"))
    rng = np.random.default_rng(seed)
    for i in range(n):
        img = rng.integers(0, 256, size=IMG_SMALL + (3,), dtype=np.uint8)
        Image.fromarray(img).save(os.path.join(root, "front", f"{i:06d}.png"))
        wp = rng.uniform(-1.0, 1.0, size=(horizon, 7))
        wp[0, :3] = 0.0
        tgt = rng.uniform(-1, 1, size=2)
        with open(os.path.join(root, "waypoints", f"{i:06d}.txt"), "w") as f:   # misc/data_collect.py:200-208
            f.write(f"{tgt[0]} {tgt[1]}\n")
            for row in wp:
                f.write(" ".join(map(str, row)) + "\n")
            f.write("\n")


def _model_on_a_dataset(tmp_path):
    """6 samples in the reference's format (two batches of 3), a randomly initialised model, H = 16, 4 DDIM steps."""
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    from autonomous_driving_with_diffusion_model_amd.modeling import build_model
    root = str(tmp_path / "ds")
    _write_dataset(root, 6)
    cfg = create_cfg()
    cfg.MODEL.HORIZON = 16
    cfg.TRAIN.USE_COND = cfg.GUIDANCE.USE_COND = "FREE_GUIDANCE"
    cfg.EVAL.SAMPLE_STEPS, cfg.GUIDANCE.FREE_SCALE = 4, 7.5
    cfg.TRAIN.ROOT, cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.NUM_WORKERS = root, 3, 0
    model = build_model(cfg)
    P.load_procedural(model, 0)
    model = model.to(DEV).eval()
    return model, cfg, S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)


def test_evaluate_open_loop_over_a_dataset_in_the_reference_format(tmp_path):
    """6 samples in two batches, a randomly initialised model, H = 16, 4 DDIM steps, K = 4 under a DeviceNoise: evaluate_open_loop
    equals, bit for bit, the metrics fed by hand with what generate_traj returns under the same seed; those per-batch records
    lie within the bound of the restatement; graphed=True gives the same dict."""
    from autonomous_driving_with_diffusion_model_amd import ops
    from autonomous_driving_with_diffusion_model_amd.dataset import get_loader
    from autonomous_driving_with_diffusion_model_amd.sampling import generate_traj
    model, cfg, sch = _model_on_a_dataset(tmp_path)
    K, seed, sel = 4, (5 << 32) | 9, TrajectorySelector(1.0, 0.5, 0.25)
    got = evaluate_open_loop(model, sch, cfg, get_loader(cfg, train=False), candidates=K, selector=sel, noise=DeviceNoise(seed, DEV))

    by_hand, noise = OpenLoopMetrics(xy_scale=model.magic_num), DeviceNoise(seed, DEV)
    counts, sums = R.fresh_state()
    want_ade, allowed = [], []
    for img, wps, tgt in get_loader(cfg, train=False):
        _, s = generate_traj(model, sch, cfg, ops.image_transform(img.to(DEV)), tgt.to(DEV), noise=noise, candidates=K, selector=sel,
                             scale_xy=False, return_selection=True)
        batch = _host(by_hand.update(s.candidates, wps.to(DEV), selection=s))
        cands, index = s.candidates.cpu().numpy().reshape(K * 3, 16, 7), s.index.cpu().numpy()
        ref, _ = _verify(batch, cands, wps.numpy()[:, :, :2], None, index, 1, "tick")
        R.accumulate(counts, sums, batch.rec, batch.flags, batch.best, index, batch.disp_sel, None, 16)
        want_ade += ref.rec[:, 2].tolist()
        allowed += R.bound(ref, 1).rec[:, 2].tolist()
    np.testing.assert_equal(got, by_hand.compute())
    units = got.pop("units")
    np.testing.assert_equal(got, R.summary(counts, sums, 16))
    assert units == {"distance": "m", "xy_scale": 23.315, "miss_radius_m": 2.0, "h0": 1}
    assert got["n"] == 6 and got["nonfinite"] == 0 and got["blocked_rate"] == 0 and len(got["disp_at"]) == 16
    assert abs(got["ade"] - np.mean(want_ade)) <= np.mean(allowed) + 1e-12
    assert got["min_ade_k"] <= got["ade"] and got["min_fde_k"] <= got["fde"] and got["selector_regret"] >= 0
    assert np.isnan(got["disp_at"][0]) and all(v > 0 for v in got["disp_at"][1:])
    graphed = evaluate_open_loop(model, sch, cfg, get_loader(cfg, train=False), candidates=K, selector=sel,
                                 noise=DeviceNoise(seed, DEV), graphed=True)
    graphed.pop("units")
    np.testing.assert_equal(graphed, got)
    # one candidate per scene: no selector runs, the plan is its own best
    one = evaluate_open_loop(model, sch, cfg, get_loader(cfg, train=False), noise=DeviceNoise(seed, DEV), max_batches=1)
    assert one["n"] == 3 and one["selector_agreement"] == 1.0 and one["selector_regret"] == 0.0 and one["ade"] == one["min_ade_k"]


def test_evaluate_open_loop_counts_the_plans_a_guide_still_blocks(tmp_path):
    """`guide_fn`: a disc of radius 10 model units around the origin holds every waypoint a clamped plan can have, so every chosen
    plan is blocked -- at K = 1 through `Guide.cost`'s active count, at K = 4 through the `blocked` of a selector that reads the
    guide; a disc far away blocks nothing.  The guide's push is kept small: what is counted is the tick's own result."""
    from autonomous_driving_with_diffusion_model_amd import Guide
    from autonomous_driving_with_diffusion_model_amd.dataset import get_loader
    model, cfg, sch = _model_on_a_dataset(tmp_path)
    disc = lambda cx, r: torch.tensor([[[cx, 0.0, 0.0, 0.0, r]]] * 3, device=DEV)      # noqa: E731
    inside, far = Guide(disc(0.0, 10.0), scale=1e-3), Guide(disc(100.0, 1.0), scale=1e-3)
    seen = []
    run = lambda guide, **kw: evaluate_open_loop(model, sch, cfg, get_loader(cfg, train=False), noise=DeviceNoise(2, DEV),      # noqa: E731
                                                 guide_fn=lambda batch: seen.append(len(batch)) or guide, **kw)
    one = run(inside)
    assert one["n"] == 6 and one["blocked_rate"] == 1.0 and seen == [3, 3]
    assert run(far)["blocked_rate"] == 0.0
    hard = TrajectorySelector(1.0, 0.0, 0.0, w_guide=1.0, hard=True)
    assert run(inside, candidates=4, selector=hard)["blocked_rate"] == 1.0
    assert run(far, candidates=4, selector=hard, graphed=True)["blocked_rate"] == 0.0
    assert run(None)["blocked_rate"] == 0.0
    with pytest.raises(TypeError, match="guide_fn must return"):
        evaluate_open_loop(model, sch, cfg, get_loader(cfg, train=False), guide_fn=lambda batch: 3)
