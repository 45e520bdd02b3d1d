"""CPU: the closed loop composed from the restatements (tests/closed_loop_ref.py) -- no device, no kernel.  A drive with a synthetic
candidate source against what is known in closed form, which pins the frames, scales and signs BETWEEN the restatements (the
navigator's window is what the plans are drawn on, the controller's mirrored metres are what the vehicle's steer sign expects,
the guide's ego-frame obstacles are what stops the plan the metrics then see halt); and the power of the replay's checks: a
transcript of that drive replayed under each planted wiring defect fails, under `drive`'s own wiring it passes.  The GPU test
(tests/test_gpu_closed_loop_ref.py) sends the device's transcript through the same `replay`."""
import numpy as np
import pytest

import closed_loop_ref as CL
import drive_ref as DR
import vehicle_ref as V

TICKS = 40
STEP = 1.4 / CL.XY_SCALE                            # 1.4 m between waypoints: 2.8 m/s at the controller's 0.5 s per waypoint
LOOK = (9, 6, 7, 8)                                 # the window point each candidate heads for
DR_DONE_COLLISION = 2                               # drive metrics v1: done = 2 is a collision
OFFSET = (0.18, 0.0, -0.10, 0.14)                    # its lateral offset at the last waypoint, model units: candidate 0 is the worst


def source(t, pose, nav):
    """K straight plans per scene in this tick's ego frame, model units: from the ego towards a point of the navigator's window,
    1.4 m per waypoint, drifting sideways by the candidate's offset."""
    out = np.zeros((CL.K, CL.S, CL.H, CL.D), np.float32)
    h = np.arange(CL.H, dtype=np.float64)[:, None]
    for s in range(CL.S):
        for k in range(CL.K):
            p = nav["window"][s, LOOK[k]].astype(np.float64)
            u = p / np.linalg.norm(p)
            n = np.array([-u[1], u[0]])
            out[k, s, :, :2] = u * (STEP * h) + n * (OFFSET[k] * h / (CL.H - 1))
    assert np.abs(out).max() <= 1.0
    return out


def _cfg():
    from autonomous_driving_with_diffusion_model_amd.config import create_cfg
    return create_cfg()


@pytest.fixture(scope="module", params=[None, 0.5], ids=["waypoint_dt = dt", "waypoint_dt = 0.5"])
def transcript(request):
    setup = CL.setup(_cfg(), request.param)
    route, pose = CL.routes()
    discs, boxes = CL.world(route)
    return CL.roll(setup, pose, discs, boxes, source, TICKS)


def _fields(tr, name):
    return np.array([[rec[name] for rec in DR.unpack(r["met_words_after"])] for r in tr["ticks"]])      # [T, S]


def test_the_composed_drive_does_what_its_geometry_says(transcript):
    ticks, setup = transcript["ticks"], transcript["setup"]
    route, _ = CL.routes()
    discs, _ = CL.world(route)
    pre = CL.preconditions(transcript)
    print("CPU drive:", pre)
    progress, xtrack = _fields(transcript, "progress_max"), _fields(transcript, "xtrack")
    speed = np.array([V.unpack_state(r["veh_words_after"])["speed"] for r in ticks])
    pose = np.array([r["pose_after"] for r in ticks])
    # scene 2 drives free: it left its first segments, its progress grows at every tick once under way, it stays on the route
    assert pre["ended"][2] is None and progress[-1, 2] > 20.0 and (np.diff(progress[3:, 2]) > 0.0).all()
    assert xtrack[:, 2].max() < 1.0, xtrack[:, 2].max()
    assert all(r["f_status"][2] == 0 for r in ticks)
    # scene 0 halts short of its disc: re-timed from the first tick on, at rest at the end, never in contact, and closer than it began
    gap = np.linalg.norm(pose[:, 0, :2] - discs[0, 0, :2], axis=1) - discs[0, 0, 4] - setup.metrics["r_ego"]
    assert all(r["f_status"][0] != 0 for r in ticks) and all(r["c_blocked"][0] == 1 for r in ticks)
    assert pre["ended"][0] is None and speed[-5:, 0].max() == 0.0 and gap.min() > 0.5 and gap[-1] < gap[0] - 5.0, (gap[0], gap[-1])
    assert _fields(transcript, "events")[-1, 0] == 0
    # scene 1 ends at the contact with the oncoming disc and stands still from the next tick on, its record frozen
    end = pre["ended"][1]
    assert end == 2 and pre["done"][1] == DR_DONE_COLLISION
    assert (speed[end + 1:, 1] == 0.0).all() and all(np.array_equal(pose[t, 1], pose[end, 1]) for t in range(end + 1, TICKS))
    assert all(np.array_equal(r["met_words_after"][1], ticks[end]["met_words_after"][1]) for r in ticks[end:])
    assert speed[end, 1] > 0.0 or end == 0                  # the hold is the PREVIOUS tick's done: the contact tick itself still moved
    # the drive is not vacuous: the fallback re-timed, the selector did not always pick 0, the controls changed, the obstacles moved
    assert pre["retimed"] > 0 and pre["nonzero_selected"] > 0 and pre["control_changes"] > pre["of"] // 2 and pre["obstacles_moved"]



def test_the_replay_passes_its_own_drive_and_fails_every_planted_defect(transcript):
    """The power check (the idiom of test_power_check_planted_defects_fail_the_bars in test_gpu_resnet_conditioned.py): the default
    wiring is clean; each defect is caught by at least one stage or wiring check.  Defect (h) needs a waypoint_dt that differs."""
    setup = transcript["setup"]
    rep = CL.replay(transcript)
    print("default wiring:", rep.summary())
    assert rep.ok, rep.failures[:5]
    assert rep.decisions == len(CL.DROPPABLE) * CL.S * TICKS and len(rep.dropped) <= 0.1 * rep.decisions, rep.dropped
    assert len(CL.DEFECTS) == 8
    for name, wiring in CL.DEFECTS.items():
        bad = CL.replay(transcript, wiring)
        stages = sorted({f[1] for f in bad.failures})
        print(f"defect {name}: {len(bad.failures)} failing checks in {stages}")
        if name.startswith("h") and setup.waypoint_dt == setup.vehicle["dt"]:
            assert bad.ok, (name, bad.failures[:3])         # the two dt are the same number: there is nothing to catch
            continue
        assert not bad.ok, name
        assert not [f for f in bad.failures if f[1] == "carry"], name      # a wiring defect is caught where it acts


def test_a_defect_in_a_recorded_value_is_caught_too(transcript):
    """Not wiring but values: one ulp on a control, another committed index, one ulp on the returned trajectory."""
    import copy
    for key, scene, change in (("control", 2, lambda a: np.nextafter(a, np.float32(2))), ("c_index", 0, lambda a: (a + 1) % CL.K),
                               ("traj", 0, lambda a: np.nextafter(a, np.float32(2)))):
        tr = dict(setup=transcript["setup"], ticks=copy.deepcopy(transcript["ticks"]))
        r = tr["ticks"][7]
        r[key] = r[key].copy()
        r[key][scene] = change(r[key][scene])
        assert not CL.replay(tr).ok, key
