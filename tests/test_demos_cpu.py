"""CPU: the hindsight labels of `Demonstrations` (demos.py) through their NumPy restatement (tests/demos_ref.py) on hand-written
logs with numbers in closed form -- a straight drive, a quarter turn, a wrap across +-pi, a `done` in the middle, the off-by-one of
the action column --, the package's own validity index against the restatement's, and what `Demonstrations` does without a device:
recording through a stand-in sampler, the refusal past `capacity`, and the refusals of its constructor."""
import numpy as np
import pytest
import torch

import demos_ref as DR

K = 20.0            # xy_scale
H = 4


def _log(T, S=1):
    return dict(pose=np.zeros((T, S, 3)), velocity=np.zeros((T, S), np.float32), target=np.zeros((T, S, 2), np.float32),
                control=np.zeros((T, S, 3), np.float32), done=np.zeros((T, S), np.int32))


def _labels(log, horizon=H, stride=1, speed_scale=10.0):
    return DR.labels(log["pose"], log["velocity"], log["target"], log["control"], log["done"], horizon=horizon, stride=stride,
                     speed_scale=speed_scale, xy_scale=K)


def test_a_straight_drive_at_constant_speed_gives_rows_at_known_spacing():
    """Compass pi / 2: forward is world +x (ego frame v1).  2 m per tick, stride 2: rows 4 m = 0.2 units apart along +y."""
    T = 12
    log = _log(T)
    log["pose"][:, 0, 0], log["pose"][:, 0, 2] = 3.0 + 2.0 * np.arange(T), np.pi / 2
    log["velocity"][:] = 4.0
    log["target"][:, 0] = np.stack([np.arange(T), -np.arange(T)], axis=1)
    index, wps, bound, target = _labels(log, stride=2)
    assert index.tolist() == [[t, 0] for t in range(T - 8)]                              # t + H * stride <= T - 1
    for i, t in enumerate(index[:, 0]):
        assert np.abs(wps[i, :, 0]).max() < 1e-6 and np.allclose(wps[i, :, 1], 0.2 * np.arange(H), atol=1e-6)
        assert wps[i, 0, 0] == 0.0 and wps[i, 0, 1] == 0.0                               # row 0 is the origin
        assert (wps[i, :, 2] == 0.0).all() and (wps[i, :, 3] == np.float32(0.4)).all()
        assert target[i].tolist() == [float(t), -float(t)]                               # the target of tick t, unclipped
    assert (bound > 0).all() and bound.max() < 1e-6


def test_a_quarter_turn_brings_the_yaw_column_to_a_half_and_a_wrap_across_pi_adds_or_subtracts_two():
    T = H + 1
    log = _log(T)
    log["pose"][:, 0, 2] = np.linspace(0.0, np.pi / 2, T)                                 # a quarter turn over the horizon + 1
    _, wps, _, _ = _labels(log)
    assert np.allclose(wps[0, :, 2], np.linspace(0.0, 0.5, T)[:H], atol=1e-7) and wps[0, 0, 2] == 0.0
    log["pose"][:, 0, 2] = np.pi / 2 * np.arange(T)                                       # a quarter turn per tick
    assert _labels(log)[1][0, :, 2].tolist() == [0.0, 0.5, 1.0, -0.5]                     # 1.5 wraps to -0.5
    # from compass 3 (just short of pi) on to -3 (just beyond -pi): the difference -6 / pi = -1.91 wraps to +0.09, not to -0.91
    log["pose"][:, 0, 2] = [3.0, 3.1, -3.1, -3.0, -2.9]
    want = np.array([0.0, 0.1, 2 * np.pi - 6.1, 2 * np.pi - 6.0]) / np.pi
    got = _labels(log)[1][0, :, 2]
    assert np.allclose(got, want, atol=1e-7) and (got >= 0).all()
    log["pose"][:, 0, 2] = [-3.0, -3.1, 3.1, 3.0, 2.9]                                    # and the other way round
    assert np.allclose(_labels(log)[1][0, :, 2], -want, atol=1e-7)


def test_a_done_in_the_middle_invalidates_exactly_the_samples_whose_horizon_crosses_it():
    T, S = 20, 2
    log = _log(T, S)
    log["done"][9, 1] = 2                                                                 # scene 1, tick 9 only
    index = _labels(log)[0]
    span = H
    want = [[t, s] for t in range(T - span) for s in range(S) if not (s == 1 and t <= 9 <= t + span)]
    assert index.tolist() == want
    assert [t for t, s in index.tolist() if s == 1] == [0, 1, 2, 3, 4] + list(range(10, 16))
    from autonomous_driving_with_diffusion_model_amd import Demonstrations
    for stride in (1, 2, 3):
        ref = _labels(log, stride=stride)[0]
        got = Demonstrations.valid_index(torch.from_numpy(log["done"]), horizon=H, stride=stride)
        assert got.dtype == torch.int64 and got.tolist() == ref.tolist(), stride
    assert Demonstrations.valid_index(torch.zeros(H, 2, dtype=torch.int32), horizon=H, stride=1).shape == (0, 2)      # too short a log
    assert Demonstrations.valid_index(torch.zeros(H + 1, 2, dtype=torch.int32), horizon=H, stride=1).tolist() == [[0, 0], [0, 1]]


def test_the_action_of_row_k_is_the_control_of_the_row_after_it():
    T = 12
    log = _log(T)
    log["control"][:, 0, 0] = 0.01 * np.arange(T)                                         # throttle = tick / 100
    log["control"][:, 0, 1] = -0.01 * np.arange(T)
    log["control"][:, 0, 2] = np.arange(T) % 2
    index, wps, _, _ = _labels(log, stride=2)
    for i, t in enumerate(index[:, 0]):
        ticks = t + 2 * (np.arange(H) + 1)                                                # t + (k + 1) * stride
        assert wps[i, :, 4].tolist() == (0.01 * ticks).astype(np.float32).tolist()
        assert wps[i, :, 5].tolist() == (-0.01 * ticks).astype(np.float32).tolist() and wps[i, :, 6].tolist() == (ticks % 2).astype(np.float32).tolist()


def test_every_word_is_clipped_and_the_target_is_not():
    log = _log(H + 1)
    log["pose"][:, 0, 0], log["pose"][:, 0, 2] = 30.0 * np.arange(H + 1), np.pi / 2      # 30 m = 1.5 units per tick
    log["velocity"][:], log["control"][:, 0, 0], log["target"][:] = 25.0, 9.0, 3.0
    _, wps, _, target = _labels(log)
    assert wps[0, :, 1].tolist() == [0.0, 1.0, 1.0, 1.0] and (wps[0, :, 3] == 1.0).all() and (wps[0, :, 4] == 1.0).all()
    assert target.tolist() == [[3.0, 3.0]]


# ---- the recorder without a device --------------------------------------------------------------------------------------------------
class _Sampler:
    model = None

    def __init__(self, S):
        self.last_control, self.calls = None, 0

    def __call__(self, image, *, pose, velocity, guide=None):
        self.calls += 1
        self.last_control = torch.full((pose.shape[0], 3), float(self.calls))
        return "plan"


class _Camera:
    def __init__(self, S):
        self.frames = torch.zeros(S, 8, 12, 3, dtype=torch.uint8)


def _navigator(S=2):
    from autonomous_driving_with_diffusion_model_amd import Navigator
    return Navigator(torch.zeros(S, 4, 2, dtype=torch.float64), torch.zeros(S, 4, dtype=torch.int32), torch.full((S,), 4, dtype=torch.int32),
                     xy_scale=K, device="cpu")


def test_the_recorder_forwards_appends_and_refuses_past_its_capacity():
    from autonomous_driving_with_diffusion_model_amd import Demonstrations
    S = 2
    nav, cam, smp, done = _navigator(S), _Camera(S), _Sampler(S), torch.zeros(S, dtype=torch.int32)
    demo = Demonstrations(smp, cam, nav, done=done, capacity=3, horizon=4, stride=1, speed_scale=10.0)
    assert demo.frames_log.shape == (3, S, 8, 12, 3) and demo.count == 0 and "recorded=0 of 3 ticks" in repr(demo)
    pose, vel = torch.zeros(S, 3, dtype=torch.float64), torch.zeros(S)
    for t in range(3):
        pose[:, 0], vel[:], done[1] = float(t), 0.5 * t, t
        cam.frames.fill_(t + 1)
        nav.target.fill_(10.0 + t)
        assert demo(None, pose=pose, velocity=vel, guide="ignored") == "plan" and demo.last_control is smp.last_control
    assert demo.count == 3 and smp.calls == 3
    assert demo.pose_log[:, 0, 0].tolist() == [0.0, 1.0, 2.0] and demo.velocity_log[:, 1].tolist() == [0.0, 0.5, 1.0]
    assert demo.frames_log[:, 0, 0, 0, 0].tolist() == [1, 2, 3] and demo.target_log[:, 0, 0].tolist() == [10.0, 11.0, 12.0]
    assert demo.control_log[:, 0, 0].tolist() == [1.0, 2.0, 3.0] and demo.done_log[:, 1].tolist() == [0, 1, 2]      # done as it stood
    with pytest.raises(IndexError, match="the logs hold 3 ticks and are full"):
        demo(None, pose=pose, velocity=vel)
    assert smp.calls == 3                                                                 # refused before the sampler ran
    assert len(demo) == 0 and demo.labels()[1].shape == (0, 4, 7)                         # three ticks hold no sample of horizon 4
    demo.clear()
    assert demo.count == 0
    with pytest.raises(ValueError, match="pose must be float64"):
        demo(None, pose=pose.float(), velocity=vel)


def test_the_recorder_refuses_what_it_cannot_record():
    from autonomous_driving_with_diffusion_model_amd import Demonstrations
    nav, cam, smp, done = _navigator(), _Camera(2), _Sampler(2), torch.zeros(2, dtype=torch.int32)
    kw = dict(done=done, capacity=4, stride=1, speed_scale=10.0)
    with pytest.raises(TypeError, match="sampler must be callable"):
        Demonstrations(object(), cam, nav, **kw)
    with pytest.raises(TypeError, match="navigator must be a Navigator"):
        Demonstrations(smp, cam, object(), **kw)
    with pytest.raises(TypeError, match="camera must be a Camera with uint8 frames"):
        Demonstrations(smp, object(), nav, **kw)
    with pytest.raises(ValueError, match="the camera's frames are"):
        Demonstrations(smp, _Camera(3), nav, **kw)
    with pytest.raises(ValueError, match="done must be int32"):
        Demonstrations(smp, cam, nav, **dict(kw, done=torch.zeros(2)))
    with pytest.raises(ValueError, match="capacity, horizon and stride must be >= 1"):
        Demonstrations(smp, cam, nav, **dict(kw, stride=0))
    with pytest.raises(ValueError, match="speed_scale must be finite and > 0"):
        Demonstrations(smp, cam, nav, **dict(kw, speed_scale=0.0))
    doc = Demonstrations.__doc__
    assert "subtracts or adds 1 where 2 is meant" in doc and "FABRICATES" in doc
