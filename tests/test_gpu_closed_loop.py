"""GPU: the closed loop (simulation.drive) at the tiny model -- S = 2 scenes, horizon 16, two DDIM steps, twelve ticks, a
`GraphedSampler(navigator=, controller=, noise=)` --: the runner against the same ticks written out by hand, the eager
`generate_traj` loop against the graphed one, a pinned drive that follows its route, and a scene that ends mid-drive.  The loop is
blind (one synthetic image at every tick) and the weights are procedural: these are plumbing checks, not driving results."""
import math

import numpy as np
import pytest
import torch

from autonomous_driving_with_diffusion_model_amd import (DeviceController, DeviceNoise, DriveMetrics, KinematicVehicle, Navigator, Pin,
                                                         drive, evaluate_closed_loop)
from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler
from autonomous_driving_with_diffusion_model_amd.simulation import EagerTick, World
from test_gpu_select import _frame, _setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 23.315
S, TICKS, DT = 2, 12, 0.25
SEED = (41 << 32) | 7


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _routes():
    """Two gently curving routes of 60 points 2 m apart, and start poses on their first point heading along them: the forward
    vector (sin c, -cos c) is the first segment's direction at c = atan2(dx, -dy)."""
    k = np.arange(60)
    heading = np.stack([0.3 + 0.004 * k, -1.0 - 0.006 * k])                     # [S, G] world angles of the segments
    step = 2.0 * np.stack([np.cos(heading), np.sin(heading)], axis=-1)
    route = np.array([[10.0, -5.0], [-40.0, 25.0]])[:, None] + np.cumsum(step, axis=1) - step[:, :1]
    d = route[:, 1] - route[:, 0]
    pose = np.concatenate([route[:, 0], np.arctan2(d[:, 0], -d[:, 1])[:, None]], axis=1)
    return route, pose


def _stack(m, cfg, sch, *, graphed=True, **metrics_kw):
    route, pose = _routes()
    nav = Navigator(torch.from_numpy(route), torch.zeros(S, 60, dtype=torch.int32), torch.full((S,), 60, dtype=torch.int32), xy_scale=K,
                    device=DEV)
    ctl = DeviceController(cfg, S, DEV)
    make = GraphedSampler if graphed else EagerTick
    sampler = make(m, sch, cfg, noise=DeviceNoise(SEED, DEV), controller=ctl, navigator=nav)
    veh = KinematicVehicle(S, DEV, dt=DT)
    veh.reset(pose)
    metrics = DriveMetrics(nav, dt=DT, **metrics_kw)
    return sampler, nav, ctl, veh, metrics


def _same(a, b, where):
    (sa, na, ca, va, ma), (sb, nb, cb, vb, mb) = a, b
    assert torch.equal(va.state, vb.state), (where, "vehicle")
    assert torch.equal(ma.words(), mb.words()) and torch.equal(ma.done, mb.done), (where, "metrics")
    assert torch.equal(na.state, nb.state) and torch.equal(_bits(na.window), _bits(nb.window)), (where, "navigator")
    assert torch.equal(ca.state, cb.state), (where, "controller")
    for x, y in zip(ca.windows(), cb.windows()):
        assert torch.equal(_bits(x), _bits(y)), (where, "controller windows")


@pytest.fixture(scope="module")
def model():
    m, cfg, sch = _setup("FREE_GUIDANCE", "ddim", steps=2)
    d, _ = _frame(S, 53, "FREE_GUIDANCE")
    return m, cfg, sch, d["imgs"]


def test_drive_is_the_twelve_ticks_written_out_by_hand(model):
    m, cfg, sch, img = model
    run, hand = _stack(m, cfg, sch), _stack(m, cfg, sch)
    assert drive(run[0], run[3], run[4], ticks=TICKS, image=img) == TICKS
    sampler, nav, ctl, veh, metrics = hand
    for t in range(TICKS):
        sampler(img, pose=veh.pose, velocity=veh.velocity)
        veh.step(sampler.last_control, hold=metrics.done)
        metrics.step(veh.pose, veh.velocity, veh.yaw_rate)
    _same(run, hand, "drive against the ticks by hand")
    f = DriveMetrics.fields(metrics.words())
    assert f["ticks"].tolist() == [TICKS] * S and nav.fresh.tolist() == [0] * S and veh.valid.tolist() == [1] * S
    # an image callable sees the tick and the pose the tick starts from
    seen = []
    again = _stack(m, cfg, sch)
    drive(again[0], again[3], again[4], ticks=TICKS, image=lambda t, pose: (seen.append((t, pose.data_ptr())), img)[1])
    _same(run, again, "an image callable")
    assert seen == [(t, again[3].pose.data_ptr()) for t in range(TICKS)]


def test_the_eager_loop_gives_what_the_graphed_one_gives(model):
    m, cfg, sch, img = model
    graphed, eager = _stack(m, cfg, sch), _stack(m, cfg, sch, graphed=False)
    out_g = evaluate_closed_loop(graphed[0], graphed[3], graphed[4], ticks=TICKS, image=img)
    out_e = evaluate_closed_loop(eager[0], eager[3], eager[4], ticks=TICKS, image=img)
    _same(graphed, eager, "graphed against eager")
    assert graphed[0].captured >= 1
    for k, v in out_g.items():
        assert np.array_equal(np.asarray(v), np.asarray(out_e[k]), equal_nan=True), k
    assert out_g["ticks"].tolist() == [TICKS] * S and out_g["time"].tolist() == [TICKS * DT] * S


def test_a_pinned_plan_is_driven_along_the_route(model):
    """The plan the controller reads is pinned onto the route ahead: waypoint 0 at the ego (where the sampler holds it anyway)
    and waypoints 1 .. 3 on the next three route points, from a scout navigator that walks the same plan one step ahead of the
    sampler's own.  So the controller sees the route, whatever the procedural weights make of the free waypoints: the ego's
    progress grows at every tick once it moves, and the cross-track error stays inside a 2 m corridor."""
    m, cfg, sch, img = model
    sampler, nav, ctl, veh, metrics = _stack(m, cfg, sch)
    route, _ = _routes()
    scout = Navigator(torch.from_numpy(route), torch.zeros(S, 60, dtype=torch.int32), torch.full((S,), 60, dtype=torch.int32), xy_scale=K,
                      first=1, device=DEV)
    H, D = 16, 7
    xy = torch.zeros(S, 4, 2, device=DEV)

    def pin_fn(t, pose):
        scout.step(pose)
        xy[:, 1:] = scout.window[:, :3]
        return Pin.points(H, D, [0, 1, 2, 3], xy, "clean")

    progress, xtrack = [], []
    for t in range(TICKS):
        drive(sampler, veh, metrics, ticks=1, image=img, pin_fn=pin_fn)
        f = DriveMetrics.fields(metrics.words())
        progress.append(f["progress_max"].copy())
        xtrack.append(f["xtrack"].copy())
    progress, xtrack = np.stack(progress), np.stack(xtrack)
    print("pinned drive: progress_max per tick", progress.T.round(3).tolist(), "xtrack max", xtrack.max(axis=0).tolist(),
          "speed", veh.velocity.tolist())
    assert (progress[-1] > 2.0).all(), progress[-1]                      # it left its first segment ...
    assert (np.diff(progress[2:], axis=0) > 0.0).all()                   # ... and moved on at every tick once under way
    assert (xtrack.max(axis=0) < 2.0).all(), xtrack.max(axis=0)          # inside the corridor's half-width
    out = metrics.compute()
    assert (out["completion"] > 0.0).all() and (out["distance"] > 2.0).all() and out["events"].tolist() == [0, 0]


def test_a_scene_that_ends_mid_drive_stands_still_while_the_other_goes_on(model):
    """A disc of radius 3 comes down scene 0's route towards the ego (scene 1's slot is empty); with stop_on_collision the scene
    ends at the contact.  From then on its vehicle is held and its record frozen; scene 1 drives on."""
    m, cfg, sch, img = model
    sampler, nav, ctl, veh, metrics = _stack(m, cfg, sch, stop_on_collision=True, r_ego=1.0)
    route, pose = _routes()
    ahead = route[0, 6] - route[0, 0]                                      # 12 m down the route
    unit = ahead / np.linalg.norm(ahead)
    discs = np.zeros((S, 1, 5))
    discs[0, 0] = [*(route[0, 0] + ahead), *(-8.0 * unit), 3.0]           # 2 m per tick towards the start: contact by tick 5
    discs[1, 0] = [0.0, 0.0, 0.0, 0.0, -1.0]
    world = World(discs=torch.from_numpy(discs).to(DEV))
    assert drive(sampler, veh, metrics, ticks=6, image=img, world=world, guide_fn=lambda t, frame, w: None) == 6
    assert metrics.done.tolist() == [2, 0]
    rec, state = metrics.words(), veh.state_snapshot()
    f = DriveMetrics.fields(rec)
    assert 1 <= f["first_tick"][0] <= 5 and f["ticks"][0] == f["first_tick"][0] and f["events"][0] == 1 and f["first_slot"][0] == 0
    assert veh.speed[0].item() == 0.0 and veh.velocity[0].item() == 0.0    # held since the tick after the contact
    assert abs(world.discs[0, 0, 0].item() - (discs[0, 0, 0] + 6 * DT * discs[0, 0, 2])) < 1e-12      # the world moved on by six ticks
    # all scenes done is what check_every looks for: not yet, so the six ticks all run
    assert drive(sampler, veh, metrics, ticks=6, image=img, world=world, guide_fn=lambda t, frame, w: None, check_every=2) == 6
    assert torch.equal(metrics.words()[0], rec[0]) and torch.equal(veh.state[0], state[0])
    g = DriveMetrics.fields(metrics.words())
    assert g["ticks"].tolist() == [int(f["ticks"][0]), 12] and g["progress_max"][1] >= f["progress_max"][1] and metrics.done.tolist()[0] == 2
    assert not torch.equal(veh.state[1], state[1])
    # ... and once every scene is done (scene 1 marked by hand, in its record and in `done`) the runner stops at the next check
    metrics.state[1, 2] = 5
    metrics.done.fill_(5)
    assert drive(sampler, veh, metrics, ticks=6, image=img, check_every=2) == 2
