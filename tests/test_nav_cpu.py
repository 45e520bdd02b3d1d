"""CPU: "route planner v1" and "ego frame v1" without a device -- the NumPy restatement (tests/nav_ref.py) against every decision
the reference's RoutePlanner made on the recorded drives (tests/golden/nav_v1.npz); the condition that keeps those decisions clear
of rounding; the properties of the transform (motion consistency through warm start v1's re-base, the round trip, a plane's side);
every refusal of the C ABI (its checks run on the host before any GPU work, so placeholder addresses that are never dereferenced
are enough), of `Navigator`, `EgoFrame` and the `navigator=` / `pose=` arguments of the sampling entry points; and the symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import nav_ref as R
import test_tick_plan_cpu as TT
import warm_ref as W
from autonomous_driving_with_diffusion_model_amd import _lib as L
from autonomous_driving_with_diffusion_model_amd import EgoFrame, Navigator, Route
from autonomous_driving_with_diffusion_model_amd import navigation as NV
from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler, generate_traj

NAN, INF = float("nan"), float("inf")
K = 23.315
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def drives():
    return R.load_golden()


# ---- the reference's decisions ------------------------------------------------------------------------------------------------------
def test_the_fixture_holds_the_drives_it_should(drives):
    assert os.path.getsize(R.GOLDEN) < 100 * 1024
    assert {len(d["route"]) for d in drives} >= {1, 2, 3, 64, 65, 200}
    by = {d["name"]: d for d in drives}
    assert [d["name"] for d in drives if d["integer"]] == ["integer_ties"]
    assert all(d["min_distance"] == 7.0 and d["max_distance"] == 50.0 for d in drives)
    spacing = lambda d: float(np.median(np.hypot(*np.diff(d["route"], axis=0).T)))  # noqa: E731
    assert abs(spacing(by["dense_0.5m_G200"]) - 0.5) < 0.02 and abs(spacing(by["dense_0.9m_G200"]) - 0.9) < 1e-9
    assert abs(spacing(by["straight_3m_G64"]) - 3.0) < 1e-9 and abs(spacing(by["sparse_30m_G64"]) - 30.0) < 1e-9
    # the max_distance stop of the first tick: past the first 64 points on the 0.5 m route, within them on the 0.9 m one
    for name, lo, hi in (("dense_0.5m_G200", 65, 199), ("dense_0.9m_G200", 2, 63)):
        cum = np.concatenate([[0.0], np.cumsum(np.hypot(*np.diff(by[name]["route"], axis=0).T))])
        assert lo <= int(np.argmax(cum > 50.0)) + 1 <= hi, name
    jump = by["jump_past_len_minus_2"]          # the second tick: three points left, only the last in range -- 2 pops asked, 1 given
    far3, far4 = (float(np.hypot(*(jump["route"][i] - jump["pose"][1, :2]))) for i in (3, 4))
    assert jump["ret_len"].tolist() == [3, 2, 2] and far4 <= 7.0 < far3 and R.walk(jump["route"], 2, 5, jump["pose"][1, :2], 7.0, 50.0)[0] == 1
    assert by["route_ends"]["ret_len"][-1] == 2 and (by["route_ends"]["ret_idx"][-5:] == 11).all()
    assert len(set(map(tuple, by["stationary"]["pose"][:, :2]))) == 1 and len(set(by["stationary"]["ret_idx"])) == 1
    assert by["one_point_G1"]["ret_idx"].tolist() == [0, 0, 0] and by["one_point_G1"]["ret_len"].tolist() == [1, 1, 1]
    # the doubling-back route makes the planner skip ahead: more than ten points in one tick
    assert np.diff(by["hairpin_3m_G200"]["ret_idx"]).max() > 10


def test_the_restatement_reproduces_every_recorded_decision(drives):
    ticks = 0
    for d in drives:
        G = len(d["route"])
        state = R.fresh_state(1)
        for t, pose in enumerate(d["pose"]):
            got = R.nav_step(d["route"][None], d["cmd"][None], [G], pose[None], state, min_distance=d["min_distance"],
                             max_distance=d["max_distance"], xy_scale=K)
            where = (d["name"], t)
            assert int(got["next"][0]) == d["ret_idx"][t], where
            assert int(got["command"][0]) == d["ret_cmd"][t], where
            assert int(got["remaining"][0]) == d["ret_len"][t], where
            assert np.array_equal(d["route"][got["next"][0]], d["ret_pt"][t]), where
            state = got["state"]
            ticks += 1
    assert ticks == sum(len(d["pose"]) for d in drives) > 150


def test_every_recorded_comparison_stands_clear_of_equality(drives):
    """What tests/golden/make_golden_nav.py asserted when it recorded, on the stored data: for every drive that is not made of
    small integers, every d against min_distance, every cum against max_distance and every candidate d against the running far
    differ by more than 1e-9 relative -- so neither a contracted dot product nor a square root's last bit can flip a decision."""
    for d in drives:
        if d["integer"]:
            continue
        head, G = 0, len(d["route"])
        for t, pose in enumerate(d["pose"]):
            pops, clear = R.walk(d["route"], head, G, pose[:2], d["min_distance"], d["max_distance"])
            assert clear > 1e-9, (d["name"], t, clear)
            head += pops


def test_an_exact_tie_keeps_the_first(drives):
    d = next(d for d in drives if d["integer"])
    # from (0, 0): (7, 0) and (0, 7) are both exactly 7 away, the largest d <= 7; the first (index 7) is popped to, so next is 8
    assert d["ret_idx"][0] == 8 and R.walk(d["route"], 0, len(d["route"]), [0.0, 0.0], 7.0, 50.0) == (7, 0.0)


def test_head_and_len_are_clamped():
    route = np.arange(12, dtype=np.float64).reshape(1, 6, 2)
    cmd = np.arange(6, dtype=np.int32)[None]
    pose = np.zeros((1, 3))
    for length, head, want_next in ((0, 0, 0), (9, 0, 1), (3, 7, 2), (3, -4, 1)):
        st = R.fresh_state(1)
        st["head"][:] = head
        got = R.nav_step(route, cmd, [length], pose, st, min_distance=1e-3, xy_scale=K)
        assert got["next"][0] == want_next, (length, head)


# ---- the transform ------------------------------------------------------------------------------------------------------------------
def _poses(rng, S):
    return np.concatenate([rng.uniform(-300, 300, (S, 2)), rng.uniform(-7, 7, (S, 1))], axis=1)


def test_the_frame_is_the_reference_s_formula():
    """process_next_waypoint (interact.py:185-202) written out with NumPy's matrix product, against the restatement."""
    rng = np.random.default_rng(5)
    for compass in (0.3, -2.0, NAN, 4.0):
        cur, nxt = rng.uniform(-50, 50, 2), rng.uniform(-50, 50, (6, 2))
        yaw = 0.0 if np.isnan(compass) else compass
        yaw = yaw + np.pi / 2.0
        rot = np.array([[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]])
        local = rot.T.dot((nxt - cur).T).T
        want = np.stack([local[:, 1] / K, -local[:, 0] / K], axis=-1)
        got, bound = R.world_to_ego(R.POINTS, nxt[None], np.array([[cur[0], cur[1], compass]]), K)
        assert (np.abs(got[0] - want) <= bound[0]).all()
        # ... and agent_to_world (interact.py:249-260) on the metres
        agent = want * K
        back = np.array([[np.cos(yaw), np.sin(yaw)], [-np.sin(yaw), np.cos(yaw)]]).T.dot(np.stack([-agent[:, 1], agent[:, 0]], axis=-1).T).T + cur
        mine = R.ego_to_world(want.astype(np.float32)[None], np.array([[cur[0], cur[1], compass]]), K)[0]
        assert (np.abs(mine - back) <= R.roundtrip_bound(want, K, back)).all()


def test_motion_consistency_through_the_warm_start_s_re_base():
    """A world-fixed point seen from pose 0, re-based by warm start v1 with the motion the planner derives, is the point seen from
    pose 1 -- the (tx, ty, phi) convention, decided here and not by a sentence."""
    rng = np.random.default_rng(11)
    S, H = 5, 6
    route = np.cumsum(rng.uniform(1.0, 3.0, (S, 9, 2)), axis=1)
    cmd, length = np.zeros((S, 9), dtype=np.int32), np.full(S, 9)
    pose0 = _poses(rng, S)
    pose1 = pose0 + np.concatenate([rng.uniform(-3, 3, (S, 2)), rng.uniform(-3.5, 3.5, (S, 1))], axis=1)
    pose1[0, 2], pose0[1, 2] = pose0[0, 2] + 2 * np.pi + 0.4, NAN          # a wrap, and a NaN compass (counts as 0)
    world = pose0[:, None, :2] + rng.uniform(-12, 12, (S, H, 2))
    first = R.nav_step(route, cmd, length, pose0, R.fresh_state(S), xy_scale=K)
    assert first["fresh"].tolist() == [1] * S and not first["motion"].any()
    second = R.nav_step(route, cmd, length, pose1, first["state"], xy_scale=K)
    assert second["fresh"].tolist() == [0] * S
    mo = second["motion"]
    assert (np.abs(mo[:, 2]) <= np.float32(np.pi)).all() and abs(mo[0, 2] - 0.4) < 1e-6
    q0, _ = R.world_to_ego(R.POINTS, world, pose0, K)
    q1, _ = R.world_to_ego(R.POINTS, world, pose1, K)
    assert np.abs(q0).max() < 1 and np.abs(q1).max() < 1                      # inside the re-base's clamp
    bound = R.consistency_bound(q0, mo[:, :2])
    for dtype in (np.float32, np.float64):
        got = W.start(q0, 0, mo, dtype)
        assert np.abs(got.astype(np.float64) - q1).max() <= bound, dtype
    assert bound < 1e-5          # (25 Q + 2) u with Q < 2
    wrong = mo.copy()
    wrong[:, 2] = -wrong[:, 2]                                                # the other sign convention is not consistent
    assert np.abs(W.start(q0, 0, wrong, np.float64) - q1).max() > 1e-2


def test_to_world_undoes_points():
    rng = np.random.default_rng(3)
    for S, N in ((1, 1), (3, 5), (2, 32)):
        pose = _poses(rng, S)
        p = pose[:, None, :2] + rng.uniform(-80, 80, (S, N, 2))
        q, _ = R.world_to_ego(R.POINTS, p, pose, K)
        back = R.ego_to_world(q, pose, K)
        assert (np.abs(back - p) <= R.roundtrip_bound(q, K, p)).all()
        # candidate-major rows: row r of K * S uses pose r % S
        rows = np.concatenate([q, q], axis=0)
        assert np.array_equal(R.ego_to_world(rows, pose, K), np.concatenate([back, back], axis=0))


def test_a_plane_keeps_its_side_and_a_disc_its_shape():
    rng = np.random.default_rng(4)
    S, P, N = 3, 4, 20
    pose = _poses(rng, S)
    normal = rng.normal(size=(S, P, 2))
    planes = np.concatenate([normal, (normal * pose[:, None, :2]).sum(-1, keepdims=True) + rng.uniform(-20, 20, (S, P, 1))], axis=-1)
    pts = pose[:, None, :2] + rng.uniform(-40, 40, (S, N, 2))
    side = (planes[:, :, None, :2] * pts[:, None]).sum(-1) - planes[:, :, None, 2]            # [S, P, N] metres
    got, _ = R.world_to_ego(R.PLANES, planes, pose, K)
    q, _ = R.world_to_ego(R.POINTS, pts, pose, K)
    ego = (got[:, :, None, :2].astype(np.float64) * q[:, None].astype(np.float64)).sum(-1) - got[:, :, None, 2]
    clear = np.abs(side) > 1e-3 * np.linalg.norm(normal, axis=-1)[:, :, None]                  # a millimetre: far above fp32 rounding at 40 m
    assert clear.mean() > 0.99 and (np.sign(ego[clear]) == np.sign(side[clear])).all()
    assert np.allclose(ego * K, side, atol=1e-3)
    # discs: the radius scales, an empty slot stays empty, the velocity keeps its length (a rotation) and takes dt / xy_scale
    discs = np.concatenate([pts[:, :4], rng.uniform(-9, 9, (S, 4, 2)), np.array([1.5, 0.0, -1.0, NAN])[None, :, None].repeat(S, 0)], axis=-1)
    d, _ = R.world_to_ego(R.DISCS, discs, pose, K, dt=0.5)
    assert np.array_equal(d[..., 4][:, :3], np.float32(np.array([1.5, 0.0, -1.0]) / K)[None].repeat(S, 0)) and np.isnan(d[..., 4][:, 3]).all()
    assert np.allclose(np.hypot(d[..., 2], d[..., 3]), np.hypot(discs[..., 2], discs[..., 3]) * 0.5 / K, rtol=1e-6)
    assert np.array_equal(d[..., :2], q[:, :4])
    # boxes: a unit heading, rotated with the frame; sizes <= 0 and NaN pass through the division as they are
    boxes = np.concatenate([discs[..., :4], rng.uniform(-4, 4, (S, 4, 1)), np.array([[4.5, 2.0], [0.0, 2.0], [4.5, -1.0], [NAN, 2.0]])[None].repeat(S, 0)], axis=-1)
    b, _ = R.world_to_ego(R.BOXES, boxes, pose, K, dt=0.5)
    assert np.allclose(np.hypot(b[..., 4], b[..., 5]), 1.0, atol=1e-6) and np.array_equal(b[..., :4], d[..., :4])
    assert np.array_equal(b[:, 0, 6:], np.float32(np.array([4.5, 2.0]) / K)[None].repeat(S, 0))
    assert (b[:, 1, 6] == 0).all() and (b[:, 2, 7] < 0).all() and np.isnan(b[:, 3, 6]).all()
    # the frame turns the world by pi - compass: a world heading of angle a becomes the angle a + pi - compass
    own = np.array([[[0.0, 0.0, 0.0, 0.0, 1.1 - np.pi / 2, 4.0, 2.0]]])
    h, _ = R.world_to_ego(R.BOXES, own, np.array([[0.0, 0.0, 1.1]]), K, dt=0.5)
    assert np.allclose(h[0, 0, 4:6], [0.0, 1.0], atol=1e-6)


def test_the_bounds():
    # a point 100 m off: one fp32 ulp of 4.3 model units dominates, the fp64 part is 8 * 2^-52 * 200 / K
    out, bound = R.world_to_ego(R.POINTS, np.array([[[100.0, 100.0]]]), np.zeros((1, 3)), K)
    assert (bound >= np.spacing(np.abs(out))).all() and (bound <= np.spacing(np.abs(out)) * (1 + 1e-6)).all()
    # a cancelling coordinate: the result is ~0 and the fp64 part is what is left
    out, bound = R.world_to_ego(R.POINTS, np.array([[[0.0, 100.0]]]), np.zeros((1, 3)), K)
    assert abs(out[0, 0, 0]) < 1e-15 and 8 * 2.0 ** -52 * 100 / K <= bound[0, 0, 0] <= 9 * 2.0 ** -52 * 100 / K
    assert (R.C_POINT, R.C_HEADING) == (8.0, 26.0)


# ---- the symbols --------------------------------------------------------------------------------------------------------------------
NAMES = ("adx_nav_state_bytes", "adx_nav_reset", "adx_nav_step", "adx_world_to_ego", "adx_ego_to_world")


def test_the_symbols_are_declared_exported_and_prototyped():
    header = open(os.path.join(ROOT, "include", "adx.h")).read()
    api = open(os.path.join(ROOT, "autonomous_driving_with_diffusion_model_amd", "csrc", "api.cpp")).read()
    for name in NAMES:
        assert re.search(rf"^(int|size_t) {name}\(", header, re.M), name
        assert re.search(rf"^(int|size_t) {name}\(", api, re.M), name
        assert name in L.EXPORTED_SYMBOLS and name in L._LAZY_SIGS
        assert callable(L.lazy(name))                                        # the built library exports it
    assert "nav.hip" in open(os.path.join(ROOT, "autonomous_driving_with_diffusion_model_amd", "csrc", "build.sh")).read().split()
    assert C.sizeof(L.NavCfg) == 40
    size = L.lazy("adx_nav_state_bytes")
    assert [size(n) for n in (1, 3, 65535, 0, 65536, -1)] == [32, 96, 65535 * 32, 0, 0, 0]
    assert (NV.POINTS, NV.DISCS, NV.PLANES, NV.BOXES) == (R.POINTS, R.DISCS, R.PLANES, R.BOXES) == (0, 1, 2, 3)
    assert (NV.MAX_POINTS, NV.MIN_WINDOW, NV.MAX_WINDOW, NV.MAX_SCENES) == (65536, 2, 32, 65535)
    for n, v in (("ADX_EGO_POINTS", 0), ("ADX_EGO_DISCS", 1), ("ADX_EGO_PLANES", 2), ("ADX_EGO_BOXES", 3)):
        assert f"#define {n} {v}\n" in header


# ---- refusals of the C ABI, by their complete text ------------------------------------------------------------------------------------
S, G, RW = 3, 70, 16
ROUTE, CMD, LEN, POSE, STATE, TARGET, COMMAND, WINDOW, MOTION, FRESH, HEAD = (0x10000000 * (i + 1) for i in range(11))
GOOD = dict(scenes=S, max_points=G, window=RW, first=0, min_distance=7.0, max_distance=50.0, xy_scale=K, route=ROUTE, cmd=CMD, len=LEN,
            pose=POSE, state=STATE, target=TARGET, command=COMMAND, window_out=WINDOW, motion=MOTION, fresh=FRESH, head_out=HEAD)
STEP_REFUSALS = [
    (dict(cfg=None), "nav step: null configuration"),
    (dict(scenes=0), "nav step: 0 scenes, supported 1..65535"),
    (dict(scenes=65536), "nav step: 65536 scenes, supported 1..65535"),
    (dict(max_points=0), "nav step: 0 route points, supported 1..65536"),
    (dict(max_points=65537), "nav step: 65537 route points, supported 1..65536"),
    (dict(window=1), "nav step: a window of 1 points, supported 2..32"),
    (dict(window=33), "nav step: a window of 33 points, supported 2..32"),
    (dict(first=2), "nav step: first 2, supported 0 or 1"),
    (dict(first=-1), "nav step: first -1, supported 0 or 1"),
    (dict(min_distance=0.0), "nav step: min_distance 0 must be finite and > 0"),
    (dict(min_distance=INF), "nav step: min_distance inf must be finite and > 0"),
    (dict(min_distance=NAN), "nav step: min_distance nan must be finite and > 0"),
    (dict(max_distance=-1.0), "nav step: max_distance -1 must be finite and > 0"),
    (dict(max_distance=INF), "nav step: max_distance inf must be finite and > 0"),
    (dict(xy_scale=0.0), "nav step: xy_scale 0 must be finite and > 0"),
    (dict(xy_scale=NAN), "nav step: xy_scale nan must be finite and > 0"),
    (dict(route=None), "nav step: null route"),
    (dict(cmd=None), "nav step: null cmd"),
    (dict(len=None), "nav step: null len"),
    (dict(pose=None), "nav step: null pose"),
    (dict(state=None), "nav step: null state"),
    (dict(target=None), "nav step: null target"),
    (dict(command=None), "nav step: null command"),
    (dict(window_out=None), "nav step: null window"),
    (dict(motion=None), "nav step: null motion"),
    (dict(fresh=None), "nav step: null fresh"),
    (dict(head_out=None), "nav step: null head_out"),
    # an output against every input and the state ...
    (dict(target=ROUTE + S * G * 16 - 4), "nav step: target aliases route"),
    (dict(command=CMD), "nav step: command aliases cmd"),
    (dict(window_out=LEN - S * RW * 8 + 4), "nav step: window aliases len"),
    (dict(motion=POSE + S * 24 - 4), "nav step: motion aliases pose"),
    (dict(fresh=STATE + S * 32 - 4), "nav step: fresh aliases the state"),
    (dict(head_out=STATE), "nav step: head_out aliases the state"),
    # ... every output against the one before it, and the first against the last ...
    (dict(command=TARGET + S * 8 - 4), "nav step: target and command alias each other"),
    (dict(window_out=COMMAND), "nav step: command and window alias each other"),
    (dict(motion=WINDOW + S * RW * 8 - 4), "nav step: window and motion alias each other"),
    (dict(fresh=MOTION), "nav step: motion and fresh alias each other"),
    (dict(head_out=FRESH + 4), "nav step: fresh and head_out alias each other"),
    (dict(head_out=TARGET), "nav step: target and head_out alias each other"),
    # ... and the state, which the launch writes, against every input
    (dict(state=ROUTE + 16), "nav step: the state aliases route"),
    (dict(state=CMD - S * 32 + 4), "nav step: the state aliases cmd"),
    (dict(state=LEN), "nav step: the state aliases len"),
    (dict(state=POSE + 8), "nav step: the state aliases pose"),
]


@pytest.mark.parametrize("over,text", STEP_REFUSALS, ids=[r[1][10:] + " / " + ",".join(r[0]) for r in STEP_REFUSALS])
def test_adx_nav_step_refuses_before_any_gpu_work(over, text):
    a = dict(GOOD, **over)
    cfg = L.NavCfg(*(a[k] for k in ("scenes", "max_points", "window", "first", "min_distance", "max_distance", "xy_scale")))
    rc = L.lazy("adx_nav_step")(None if "cfg" in over else C.byref(cfg), a["route"], a["cmd"], a["len"], a["pose"], a["state"], a["target"],
                                a["command"], a["window_out"], a["motion"], a["fresh"], a["head_out"], None)
    assert (rc, L.lib().adx_last_error().decode()) == (-1, text)


RESET_REFUSALS = [
    (dict(scenes=0), "nav reset: 0 scenes, supported 1..65535"),
    (dict(scenes=65536), "nav reset: 65536 scenes, supported 1..65535"),
    (dict(state=None), "nav reset: null state"),
    (dict(mask=STATE + S * 32 - 1), "nav reset: the mask overlaps the state"),
    (dict(mask=STATE - S + 1), "nav reset: the mask overlaps the state"),
]


@pytest.mark.parametrize("over,text", RESET_REFUSALS, ids=[r[1][11:] + " / " + ",".join(r[0]) for r in RESET_REFUSALS])
def test_adx_nav_reset_refuses_before_any_gpu_work(over, text):
    a = dict(dict(state=STATE, scenes=S, mask=None), **over)
    rc = L.lazy("adx_nav_reset")(a["state"], a["scenes"], a["mask"], None)
    assert (rc, L.lib().adx_last_error().decode()) == (-1, text)


IN, OUT, N = 0x10000000, 0x20000000, 5
EGO_GOOD = dict(kind=0, inp=IN, pose=POSE, out=OUT, scenes=S, n=N, xy_scale=K, vel_scale=0.02)
EGO_REFUSALS = [
    (dict(kind=-1), "world to ego: kind -1, supported 0..3"),
    (dict(kind=4), "world to ego: kind 4, supported 0..3"),
    (dict(scenes=0), "world to ego: 0 scenes, supported 1..65535"),
    (dict(scenes=65536), "world to ego: 65536 scenes, supported 1..65535"),
    (dict(n=0), "world to ego: 0 records per scene, supported 1..65536"),
    (dict(n=65537), "world to ego: 65537 records per scene, supported 1..65536"),
    (dict(xy_scale=0.0), "world to ego: xy_scale 0 must be finite and > 0"),
    (dict(xy_scale=INF), "world to ego: xy_scale inf must be finite and > 0"),
    (dict(kind=1, vel_scale=NAN), "world to ego: vel_scale nan must be finite"),
    (dict(kind=3, vel_scale=INF), "world to ego: vel_scale inf must be finite"),
    (dict(inp=None), "world to ego: null in"),
    (dict(pose=None), "world to ego: null pose"),
    (dict(out=None), "world to ego: null out"),
    (dict(out=IN + S * N * 16 - 4), "world to ego: out aliases in"),
    (dict(kind=3, out=IN + S * N * 56 - 4), "world to ego: out aliases in"),
    (dict(kind=3, out=IN - S * N * 32 + 4), "world to ego: out aliases in"),
    (dict(out=POSE + S * 24 - 4), "world to ego: out aliases pose"),
]


@pytest.mark.parametrize("over,text", EGO_REFUSALS, ids=[r[1][14:] + " / " + ",".join(r[0]) for r in EGO_REFUSALS])
def test_adx_world_to_ego_refuses_before_any_gpu_work(over, text):
    a = dict(EGO_GOOD, **over)
    rc = L.lazy("adx_world_to_ego")(a["kind"], a["inp"], a["pose"], a["out"], a["scenes"], a["n"], a["xy_scale"], a["vel_scale"], None)
    assert (rc, L.lib().adx_last_error().decode()) == (-1, text)


def test_points_and_planes_do_not_read_vel_scale():
    """A NaN vel_scale passes the check of kinds 0 and 2, which do not read it: the next refusal is the one reported."""
    for kind in (0, 2):
        rc = L.lazy("adx_world_to_ego")(kind, None, POSE, OUT, S, N, K, NAN, None)
        assert (rc, L.lib().adx_last_error().decode()) == (-1, "world to ego: null in")


BACK_GOOD = dict(plans=IN, pose=POSE, out=OUT, rows=2 * S, scenes=S, horizon=8, dim=7, xy_scale=K)
BACK_REFUSALS = [
    (dict(scenes=0), "ego to world: 0 scenes, supported 1..65535"),
    (dict(rows=0), "ego to world: 0 rows, not a positive multiple of 3 scenes"),
    (dict(rows=7), "ego to world: 7 rows, not a positive multiple of 3 scenes"),
    (dict(horizon=0), "ego to world: horizon 0, supported 1..65536"),
    (dict(horizon=65537), "ego to world: horizon 65537, supported 1..65536"),
    (dict(dim=1), "ego to world: transition dim 1, supported 2..16"),
    (dict(dim=17), "ego to world: transition dim 17, supported 2..16"),
    (dict(rows=3 * 65536, horizon=65536), "ego to world: 196608 rows of 65536 waypoints, supported up to 2^30 waypoints"),
    (dict(xy_scale=-1.0), "ego to world: xy_scale -1 must be finite and > 0"),
    (dict(plans=None), "ego to world: null plans"),
    (dict(pose=None), "ego to world: null pose"),
    (dict(out=None), "ego to world: null out"),
    (dict(out=IN + 6 * 8 * 7 * 4 - 4), "ego to world: out aliases plans"),
    (dict(out=POSE - 6 * 8 * 16 + 4), "ego to world: out aliases pose"),
]


@pytest.mark.parametrize("over,text", BACK_REFUSALS, ids=[r[1][14:] + " / " + ",".join(r[0]) for r in BACK_REFUSALS])
def test_adx_ego_to_world_refuses_before_any_gpu_work(over, text):
    a = dict(BACK_GOOD, **over)
    rc = L.lazy("adx_ego_to_world")(a["plans"], a["pose"], a["out"], a["rows"], a["scenes"], a["horizon"], a["dim"], a["xy_scale"], None)
    assert (rc, L.lib().adx_last_error().decode()) == (-1, text)


# ---- refusals of Navigator and EgoFrame ---------------------------------------------------------------------------------------------
def _nav(**kw):
    route = torch.arange(2 * 5 * 2, dtype=torch.float64).reshape(2, 5, 2)
    a = dict(route_m=route, commands=torch.zeros(2, 5, dtype=torch.int32), lengths=torch.tensor([5, 3], dtype=torch.int32), xy_scale=K,
             device="cpu")
    a.update(kw)
    return Navigator(a.pop("route_m"), a.pop("commands"), a.pop("lengths"), **a)


def test_navigator_refuses_what_it_cannot_run():
    nv = _nav()
    assert (nv.scenes, nv.max_points, nv.points, nv.first, nv.min_distance, nv.max_distance, nv.xy_scale) == (2, 5, 16, 0, 7.0, 50.0, K)
    assert nv.state.shape == (2, 8) and nv.state.dtype == torch.int32 and not nv.state.any()
    for t, shape, dtype in ((nv.target, (2, 2), torch.float32), (nv.command, (2,), torch.int32), (nv.window, (2, 16, 2), torch.float32),
                            (nv.motion, (2, 3), torch.float32), (nv.fresh, (2,), torch.int32), (nv.head, (2,), torch.int32),
                            (nv.pose, (2, 3), torch.float64), (nv.previous_pose, (2, 3), torch.float64), (nv.valid, (2,), torch.int32)):
        assert tuple(t.shape) == shape and t.dtype == dtype
    nv.previous_pose[1, 2] = 0.5                                                  # views: they write through
    nv.state[1, 1] = 1
    assert nv.valid.tolist() == [0, 1] and nv.state[1, 6:].tolist() == [0, 0x3FE00000]
    route = nv.route(2.0 / K, weight=3.0)
    assert isinstance(route, Route) and route.points.data_ptr() == nv.window.data_ptr() and route.weight == 3.0 and route.R == 16
    snap = nv.state_snapshot()
    nv.state.zero_()
    nv.state_restore(snap)
    assert nv.valid.tolist() == [0, 1] and snap.data_ptr() != nv.state.data_ptr()
    with pytest.raises(ValueError, match="not a snapshot of this Navigator"):
        nv.state_restore(snap[:1])
    assert repr(nv) == f"Navigator(scenes=2, max_points=5, points=16, first=0, min_distance=7.0, max_distance=50.0, xy_scale={K}, device=cpu)"
    # the copies are the navigator's own
    src = torch.zeros(2, 5, 2, dtype=torch.float64)
    assert _nav(route_m=src).route_m.data_ptr() != src.data_ptr()
    with pytest.raises(TypeError, match="route_m must be a tensor, got list"):
        _nav(route_m=[[0.0, 0.0]])
    with pytest.raises(TypeError, match="route_m must be torch.float64, got torch.float32"):
        _nav(route_m=torch.zeros(2, 5, 2))
    with pytest.raises(TypeError, match="commands must be torch.int32, got torch.int64"):
        _nav(commands=torch.zeros(2, 5, dtype=torch.int64))
    with pytest.raises(TypeError, match="lengths must be torch.int32, got torch.int64"):
        _nav(lengths=torch.tensor([5, 3]))
    for bad in (torch.zeros(2, 5, 3, dtype=torch.float64), torch.zeros(5, 2, dtype=torch.float64), torch.zeros(0, 5, 2, dtype=torch.float64),
                torch.zeros(2, 0, 2, dtype=torch.float64)):
        with pytest.raises(ValueError, match=r"route_m must be \[S, G, 2\] world metres"):
            _nav(route_m=bad)
    with pytest.raises(ValueError, match=r"commands must be \[2, 5\], got \(2, 4\)"):
        _nav(commands=torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"lengths must be \[2\], got \(3,\)"):
        _nav(lengths=torch.tensor([5, 3, 1], dtype=torch.int32))
    for bad in ([0, 3], [5, 6]):
        with pytest.raises(ValueError, match=r"lengths must lie in 1..5 \(G\)"):
            _nav(lengths=torch.tensor(bad, dtype=torch.int32))
    for bad in (1, 33):
        with pytest.raises(ValueError, match=f"points must be 2..32, got {bad}"):
            _nav(points=bad)
    with pytest.raises(ValueError, match="first must be 0 or 1, got 2"):
        _nav(first=2)
    for name in ("xy_scale", "min_distance", "max_distance"):
        for bad in (0.0, -1.0, INF, NAN):
            with pytest.raises(ValueError, match=f"{name} must be finite and > 0"):
                _nav(**{name: bad})
    with pytest.raises(ValueError, match=r"pose must be \[2, 3\] = \(x, y, compass\) per scene, got \(3, 3\)"):
        nv.step(torch.zeros(3, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"pose must be \[2, 3\]"):
        nv.step([[0.0, 0.0, 0.0]])
    with pytest.raises(L.AdxError, match="the navigator lives on cpu; the adx kernels only run on an MI355X"):      # no CPU path
        nv.step(torch.zeros(2, 3, dtype=torch.float64))
    with pytest.raises(L.AdxError, match="the navigator lives on cpu"):
        nv.reset()
    for bad in (torch.zeros(3, dtype=torch.bool), torch.zeros(2), [True, False]):
        with pytest.raises(ValueError, match=r"mask must be \[2\] bool or uint8 on cpu"):
            nv.reset(bad)
    with pytest.raises(ValueError, match="scene must be 0..1, got 2"):
        nv.set_route(2, [[0.0, 0.0]])
    with pytest.raises(ValueError, match=r"route_m must be \[n, 2\] with 1 <= n <= 5, got \(6, 2\)"):
        nv.set_route(0, [[0.0, 0.0]] * 6)
    with pytest.raises(ValueError, match=r"commands must be \[2\], got \(3,\)"):
        nv.set_route(0, [[0.0, 0.0]] * 2, [1, 2, 3])
    with pytest.raises(L.AdxError, match="the navigator lives on cpu"):
        nv.set_route(0, [[0.0, 0.0]] * 2)


def test_from_physical_pads_with_the_last_point():
    nv = Navigator.from_physical([[(0.0, 1.0), (2.0, 3.0), (4.0, 5.5)], [(7.0, 8.0)]], [[1, 2, 3], [4]], xy_scale=K, device="cpu", points=4, first=1)
    assert nv.lengths.tolist() == [3, 1] and (nv.points, nv.first, nv.max_points) == (4, 1, 3)
    assert nv.route_m.tolist() == [[[0.0, 1.0], [2.0, 3.0], [4.0, 5.5]], [[7.0, 8.0]] * 3] and nv.route_m.dtype == torch.float64
    assert nv.commands.tolist() == [[1, 2, 3], [4, 4, 4]]
    assert not Navigator.from_physical([[(0.1, 0.2)]], xy_scale=K, device="cpu").commands.any()
    assert Navigator.from_physical([[(0.1, 0.2)]], xy_scale=K, device="cpu").route_m[0, 0, 0].item() == 0.1      # a double, not a float
    with pytest.raises(ValueError, match="every scene needs a route of at least one point"):
        Navigator.from_physical([[(0.0, 0.0)], []], xy_scale=K, device="cpu")
    with pytest.raises(ValueError, match="scene 0 has 2 points and 1 commands"):
        Navigator.from_physical([[(0.0, 0.0), (1.0, 1.0)]], [[1]], xy_scale=K, device="cpu")
    with pytest.raises(ValueError, match=r"scene 0's route must be \[n, 2\]"):
        Navigator.from_physical([[(0.0, 0.0, 0.0)]], xy_scale=K, device="cpu")


def test_ego_frame_refuses_what_it_cannot_run():
    pose = torch.zeros(3, 3, dtype=torch.float64)
    ef = EgoFrame(pose, K, dt=0.5)
    assert (ef.scenes, ef.xy_scale, ef.dt) == (3, K, 0.5) and ef.pose is pose and repr(ef) == f"EgoFrame(scenes=3, xy_scale={K}, dt=0.5, device=cpu)"
    with pytest.raises(TypeError, match="pose must be a tensor, got list"):
        EgoFrame([[0.0, 0.0, 0.0]], K)
    with pytest.raises(TypeError, match="pose must be float64, got torch.float32"):
        EgoFrame(torch.zeros(3, 3), K)
    for bad in (torch.zeros(3, 2, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), torch.zeros(0, 3, dtype=torch.float64),
                torch.zeros(3, 6, dtype=torch.float64)[:, ::2]):
        with pytest.raises(ValueError, match=r"pose must be contiguous \[S, 3\]"):
            EgoFrame(bad, K)
    for bad in (0.0, NAN, INF):
        with pytest.raises(ValueError, match="xy_scale must be finite and > 0"):
            EgoFrame(pose, bad)
    with pytest.raises(ValueError, match="dt must be finite"):
        EgoFrame(pose, K, dt=INF)
    for name, w in (("points", 2), ("discs", 5), ("planes", 3), ("boxes", 7)):
        call = getattr(ef, name)
        with pytest.raises(TypeError, match=f"EgoFrame.{name}: the input must be a tensor, got list"):
            call([[0.0]])
        with pytest.raises(TypeError, match=f"EgoFrame.{name}: the input must be float64, got torch.float32"):
            call(torch.zeros(3, 4, w))
        for shape in ((3, 4, w + 1), (2, 4, w), (3, w), (3, 0, w)):
            with pytest.raises(ValueError, match=rf"EgoFrame.{name}: the input must be \[3, N, {w}\]"):
                call(torch.zeros(shape, dtype=torch.float64))
        with pytest.raises(ValueError, match=f"EgoFrame.{name}: the pose lives on cpu, the input on meta"):
            call(torch.zeros(3, 4, w, dtype=torch.float64, device="meta"))
        wo = NV._WIDTH_OUT[NV._KIND_NAMES.index(name)]
        for out in (torch.zeros(3, 4, wo, dtype=torch.float64), torch.zeros(3, 5, wo), torch.zeros(3, 4, wo + 1)):
            with pytest.raises(ValueError, match=rf"EgoFrame.{name}: out must be contiguous float32 \(3, 4, {wo}\) on cpu"):
                call(torch.zeros(3, 4, w, dtype=torch.float64), out=out)
        with pytest.raises(L.AdxError, match=f"EgoFrame.{name}: the input lives on cpu; the adx kernels only run on an MI355X"):
            call(torch.zeros(3, 4, w, dtype=torch.float64))
    for name, w in (("discs", 5), ("boxes", 7)):
        with pytest.raises(ValueError, match=f"EgoFrame.{name}: velocities need dt"):
            getattr(EgoFrame(pose, K), name)(torch.zeros(3, 4, w, dtype=torch.float64))
    with pytest.raises(TypeError, match="traj must be a tensor, got list"):
        ef.to_world([[0.0]])
    with pytest.raises(TypeError, match="traj must be float32, got torch.float64"):
        ef.to_world(torch.zeros(3, 8, 7, dtype=torch.float64))
    for shape in ((4, 8, 7), (3, 8, 1), (3, 8, 17), (3, 0, 7), (0, 8, 7), (3, 8)):
        with pytest.raises(ValueError, match=r"traj must be \[K \* 3, H, D\] with 2 <= D <= 16"):
            ef.to_world(torch.zeros(shape))
    with pytest.raises(ValueError, match="the pose lives on cpu, traj on meta"):
        ef.to_world(torch.zeros(3, 8, 7, device="meta"))
    with pytest.raises(ValueError, match=r"out must be contiguous float64 \(6, 8, 2\) on cpu"):
        ef.to_world(torch.zeros(6, 8, 7), out=torch.zeros(6, 8, 2))
    with pytest.raises(L.AdxError, match="EgoFrame.to_world: traj lives on cpu"):
        ef.to_world(torch.zeros(6, 8, 7))


# ---- the sampling entry points ------------------------------------------------------------------------------------------------------
def test_the_ticks_refuse_a_navigator_they_cannot_run():
    """Every refusal comes before the navigator steps (its launch would raise on this CPU object) and before the model is touched
    (None here)."""
    nv = _nav()
    pose = torch.zeros(2, 3, dtype=torch.float64)
    tick = lambda **kw: generate_traj(None, None, None, TT.IMG, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="`pose` is what a navigator reads; pass navigator=Navigator\\(...\\) with it"):
        tick(pose=pose)
    with pytest.raises(TypeError, match="`navigator` must be a Navigator, got int"):
        tick(navigator=3, pose=pose)
    with pytest.raises(ValueError, match=r"a navigator needs `pose` \[S, 3\]"):
        tick(navigator=nv)
    with pytest.raises(ValueError, match="with a navigator `target` and `motion` are its outputs; pass neither"):
        tick(navigator=nv, pose=pose, target=torch.zeros(2))
    with pytest.raises(ValueError, match="with a navigator `target` and `motion` are its outputs; pass neither"):
        tick(navigator=nv, pose=pose, motion=torch.zeros(2, 3))
    with pytest.raises(ValueError, match="the Navigator holds the plans of 2 scenes on cpu, this tick is 3 scenes on cpu"):
        generate_traj(None, None, None, torch.zeros(3, 3, 16, 16), navigator=nv, pose=pose)
    with pytest.raises(ValueError, match="the Navigator holds the plans of 2 scenes on cpu, this tick is 2 scenes on meta"):
        generate_traj(None, None, None, torch.zeros(2, 3, 16, 16, device="meta"), navigator=nv, pose=pose)
    assert not nv.state.any()
    with pytest.raises(TypeError, match="GraphedSampler: `navigator` must be a Navigator, got str"):
        GraphedSampler(TT.MODEL, TT._Scheduler(), TT._cfg(), navigator="nav")
    gs = GraphedSampler(TT.MODEL, TT._Scheduler(), TT._cfg(), navigator=nv)
    assert gs.navigator is nv
    with pytest.raises(ValueError, match=r"a navigator needs `pose` \[S, 3\]"):
        gs(TT.IMG)
    with pytest.raises(ValueError, match="pass neither"):
        gs(TT.IMG, torch.zeros(2), pose=pose)
    with pytest.raises(ValueError, match="`pose` is what a navigator reads"):
        GraphedSampler(TT.MODEL, TT._Scheduler(), TT._cfg())(TT.IMG, pose=pose)


def test_the_probe_imports():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import nav_probe  # noqa: F401  (its module level needs no device)
