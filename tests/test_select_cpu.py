"""CPU: best-of-K selection -- properties of the fp64 restatement of "selection cost v1" (tests/select_ref.py), the fixture
generator's promise that every scene it emits has a winner decided beyond fp32 rounding, the exported symbol and its ctypes
prototype, and adx_traj_select's argument checks, which answer before any GPU work (there is no GPU here)."""
import ctypes
import os
import re

import numpy as np
import pytest

import select_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _paths(K=5, S=2, H=16, D=7, seed=3):
    rng = np.random.default_rng(seed)
    return np.stack([R._scene(rng, K, H, D) for _ in range(S)], axis=1)          # [K, S, H, D]


def test_consensus_of_identical_candidates_is_zero():
    one = _paths(K=1)
    t = np.repeat(one, 6, axis=0)
    _, _, cons = R.terms(t, 2)
    assert np.array_equal(cons, np.zeros((2, 6)))
    cost, idx = R.select(t, 2, None, (0.0, 0.0, 1.0))
    assert np.array_equal(cost, np.zeros((2, 6))) and idx.tolist() == [0, 0]


def test_smoothness_of_a_straight_constant_speed_line_is_zero():
    H = 32
    tau = np.arange(H)[:, None] / 64.0                    # dyadic steps: the second difference cancels exactly
    line = np.array([-0.5, 0.25]) + tau * np.array([1.0, -0.5])
    t = np.zeros((3, 1, H, 4))
    t[0, 0, :, :2] = line
    t[1, 0, :, :2] = line + 0.01 * np.sin(np.arange(H))[:, None]
    t[2, 0, :, :2] = line[::-1]
    _, smooth, _ = R.terms(t, 1)
    assert smooth[0, 0] == 0.0 and smooth[0, 2] == 0.0 and smooth[0, 1] > 0.0
    assert R.select(t, 1, None, (0.0, 1.0, 0.0))[1].tolist() == [0]                  # the tie of 0 and 2 goes to 0
    assert np.array_equal(R.terms(t[:, :, :2], 1)[1], np.zeros((1, 3)))               # H = 2: no interior waypoint


def test_goal_is_zero_when_a_waypoint_sits_on_the_target_and_ignored_without_one():
    t = _paths(K=4, S=2)
    target = np.stack([t[2, 0, 5, :2], t[0, 1, 15, :2]])
    goal, _, _ = R.terms(t, 2, target)
    assert goal[0, 2] == 0.0 and goal[1, 0] == 0.0 and (goal >= 0).all() and goal[0, 0] > 0
    assert R.select(t, 2, target, (1.0, 0.0, 0.0))[1].tolist() == [2, 0]
    cost, idx = R.select(t, 2, None, (1.0, 0.0, 0.0))
    assert np.array_equal(cost, np.zeros((2, 4))) and idx.tolist() == [0, 0]
    one_d = t[..., :1]                                      # D = 1: y counts as 0
    g1, _, _ = R.terms(one_d, 2, target)
    want = ((one_d[..., 0].astype(np.float64) - target[None, :, None, 0]) ** 2 + target[None, :, None, 1].astype(np.float64) ** 2).min(-1).T
    assert np.allclose(g1, want, rtol=1e-15, atol=0)


def test_a_tie_goes_to_the_lowest_index():
    t = _paths(K=6, S=1)
    t[4] = t[1]
    target = t[1, :, 3, :2]
    cost, idx = R.select(t, 1, target, (1.0, 0.5, 0.0))
    assert cost[0, 1] == cost[0, 4] == cost.min() and idx.tolist() == [1]
    assert R.pick(np.array([[3.0, 1.0, 1.0], [2.0, 2.0, 2.0]])).tolist() == [1, 0]


def test_a_nan_candidate_is_never_chosen_unless_all_are_nan():
    t = _paths(K=5, S=2)
    target = np.zeros((2, 2))
    clean_cost, clean_idx = R.select(t, 2, target, (1.0, 1.0, 0.0))
    for k in range(5):
        bad = t.copy()
        bad[k, :, 7, 0] = np.nan
        cost, idx = R.select(bad, 2, target, (1.0, 1.0, 0.0))
        assert np.isnan(cost[:, k]).all() and np.isfinite(np.delete(cost, k, axis=1)).all()
        assert (idx != k).all()
        others = np.delete(np.arange(5), k)
        assert np.array_equal(idx, others[np.delete(clean_cost, k, axis=1).argmin(-1)])
    # a weight of 0 keeps a term out entirely: the NaN does not reach the others through a consensus nobody asked for ...
    bad = t.copy()
    bad[0, :, 0, 1] = np.nan
    assert (R.select(bad, 2, target, (1.0, 0.0, 0.0))[1] != 0).all()
    # ... and with the consensus term on, the scene's mean path is NaN, every cost is, and the index is 0 by rule
    cost, idx = R.select(bad, 2, target, (1.0, 0.0, 1.0))
    assert np.isnan(cost).all() and idx.tolist() == [0, 0]
    assert R.pick(np.array([[np.nan, np.inf, -np.inf], [np.inf, 5.0, np.nan]])).tolist() == [0, 1]


@pytest.fixture(scope="module")
def fixtures():
    return R.cases()


def test_fixtures_cover_the_grid_and_every_scene_has_a_decided_winner(fixtures):
    """Inputs in [-1, 1]; for EVERY scene the gap between the reference's best and second-best cost exceeds twice the fp32
    bound, so the GPU test compares the index of every scene and leaves none out."""
    seen = set()
    n_scenes = 0
    for c in fixtures:
        S, K, H, D = c["S"], c["K"], c["H"], c["D"]
        seen.add((S, K, H, D))
        assert c["trajs"].shape == (K * S, H, D) and c["trajs"].dtype == np.float32
        assert np.abs(c["trajs"]).max() <= 1.0 and (c["target"] is None or np.abs(c["target"]).max() <= 1.0)
        cost, idx = R.select(c["trajs"], S, c["target"], c["weights"])
        assert cost.shape == (S, K) and np.isfinite(cost).all()
        assert c["bound"] == R.cost_bound(K, H, c["weights"], c["target"] is not None) and 0 < c["bound"] < 1e-3
        g = R.gap(cost)
        assert (g > 2.0 * c["bound"]).all(), (S, K, H, D, c["weights"], g.min(), c["bound"])
        assert np.array_equal(idx, cost.argmin(-1))
        n_scenes += S
    assert seen == {(S, K, H, D) for S in R.SCENES for K in R.CANDIDATES for H in R.HORIZONS for D in R.DIMS}
    assert any(c["target"] is None for c in fixtures) and any(c["target"] is not None for c in fixtures)
    assert {c["weights"] for c in fixtures} == {w[:3] for w in R.WEIGHTS}
    again = R.cases()
    assert all(np.array_equal(a["trajs"], b["trajs"]) for a, b in zip(fixtures, again))       # seeded: the GPU test sees the same


def test_fp32_evaluation_on_the_host_stays_inside_the_bound(fixtures):
    """The bound is derived, not measured; this only guards the derivation against a slip: the same formula evaluated in
    fp32 NumPy (another summation order than the kernel's, which the bound does not depend on) must sit inside it."""
    for c in fixtures[::7]:
        S, K = c["S"], c["K"]
        wg, ws, wc = (np.float32(w) for w in c["weights"])
        p = np.zeros((K, S, c["H"], 2), dtype=np.float32)
        p[..., :min(c["D"], 2)] = c["trajs"].reshape(K, S, c["H"], c["D"])[..., :2]
        cost = np.zeros((S, K), dtype=np.float32)
        if c["target"] is not None and wg != 0:
            d = p - c["target"][None, :, None, :]
            cost = cost + wg * (d * d).sum(-1, dtype=np.float32).min(-1).T
        if ws != 0:
            a = (p[:, :, 2:] - np.float32(2) * p[:, :, 1:-1]) + p[:, :, :-2]
            cost = cost + ws * ((a * a).sum(-1, dtype=np.float32).sum(-1, dtype=np.float32) / np.float32(c["H"] - 2)).T
        if wc != 0:
            d = p - p.sum(0, dtype=np.float32, keepdims=True) / np.float32(K)
            cost = cost + wc * ((d * d).sum(-1, dtype=np.float32).sum(-1, dtype=np.float32) / np.float32(c["H"])).T
        assert cost.dtype == np.float32
        want, _ = R.select(c["trajs"], S, c["target"], c["weights"])
        assert np.abs(cost.astype(np.float64) - want).max() <= c["bound"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from autonomous_driving_with_diffusion_model_amd import _lib
    return _lib


def test_symbol_is_declared_exported_and_prototyped(built):
    header = open(os.path.join(ROOT, "include", "adx.h")).read()
    assert re.search(r"\bint\s+adx_traj_select\s*\(", header) and "adx_select_cfg" in header
    assert hasattr(ctypes.CDLL(built.LIB_PATH), "adx_traj_select")
    assert "adx_traj_select" in built.EXPORTED_SYMBOLS
    fn = built.lib().adx_traj_select
    assert fn.restype is built.i32 and len(fn.argtypes) == 7
    assert ctypes.sizeof(built.SelectCfg) == 28 and [f[0] for f in built.SelectCfg._fields_] == [
        "scenes", "candidates", "horizon", "dim", "w_goal", "w_smooth", "w_consensus"]
    import autonomous_driving_with_diffusion_model_amd as pkg
    from autonomous_driving_with_diffusion_model_amd.control.select import Selection, TrajectorySelector
    assert pkg.TrajectorySelector is TrajectorySelector and pkg.Selection is Selection
    s = TrajectorySelector()
    assert (s.w_goal, s.w_smooth, s.w_consensus) == (1.0, 0.0, 0.0)
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    cfg = create_cfg()
    assert cfg.EVAL.CANDIDATES == 1 and tuple(cfg.EVAL.SELECT) == (1.0, 0.0, 0.0)


def test_bad_arguments_come_back_as_error_codes_without_a_gpu(built):
    """The checks run on the host before any GPU work, so placeholder addresses (never dereferenced) are enough."""
    lib = built.lib()
    row = 16 * 7 * 4
    trajs, cost, index, best, target = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000

    def call(S=2, K=4, H=16, D=7, trajs=trajs, target=target, cost=cost, index=index, best=best):
        cfg = built.SelectCfg(S, K, H, D, 1.0, 0.5, 0.25)
        return lib.adx_traj_select(ctypes.byref(cfg), trajs, target, cost, index, best, None)

    for kw, word in ((dict(K=0), b"candidates"), (dict(K=65), b"candidates"), (dict(K=-1), b"candidates"),
                     (dict(H=0), b"horizon"), (dict(H=65), b"horizon"), (dict(D=0), b"dim"), (dict(D=17), b"dim"),
                     (dict(S=0), b"scenes"),
                     (dict(best=None), b"null"), (dict(trajs=None), b"null"), (dict(cost=None), b"null"), (dict(index=None), b"null"),
                     (dict(best=trajs), b"aliases trajs"), (dict(best=trajs + 7 * row), b"aliases trajs"),
                     (dict(best=trajs - row), b"aliases trajs"), (dict(cost=trajs + 4), b"aliases trajs"),
                     (dict(index=trajs + 8 * row - 4), b"aliases trajs"), (dict(cost=best + row), b"alias each other")):
        assert call(**kw) == -1, kw
        assert word in lib.adx_last_error(), (kw, lib.adx_last_error())
    assert lib.adx_traj_select(None, trajs, target, cost, index, best, None) == -1
    with pytest.raises(ValueError, match="candidates"):
        built.check(call(K=65), "adx_traj_select")


def test_python_surface_refuses_bad_shapes_before_any_launch(built):
    import torch
    from autonomous_driving_with_diffusion_model_amd import TrajectorySelector
    sel = TrajectorySelector(1.0, 0.5, 0.25)
    with pytest.raises(ValueError):
        sel(torch.zeros(7, 16, 7), 2)                       # 7 rows are not K * 2
    with pytest.raises(ValueError):
        sel(torch.zeros(3, 4, 16, 7), 2)                    # [K, S, H, D] with another S
    with pytest.raises(built.AdxError):
        sel(torch.zeros(8, 16, 7), 2)                       # a CPU tensor: there is no CPU path
