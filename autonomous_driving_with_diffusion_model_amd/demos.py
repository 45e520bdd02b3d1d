"""A drive recorded as training samples, on the device: the frame a tick saw, the 16 x 7 hindsight trajectory in that tick's ego
frame, and the target point -- the format `TrajDataset` (dataset/carla_dataset.py) reads and the training step consumes.

The reference's writer is misc/data_collect.py:152-212: it drives CARLA with an expert, and every `save_every_n_frame` frames it
appends (position, compass / pi, speed / scale, control) to a list until 17 entries are there, then writes the first 16 in the
first entry's frame, each with the control of the entry after it.  `Demonstrations` does the same in hindsight over logs that
stay on the device: it wraps a sampler of `drive` (an `Expert`, or any other), forwards every call, and appends what the tick
saw to preallocated logs -- no allocation, no synchronisation per tick.  `labels()` then forms every sample at once with torch
indexing and one launch of ego frame v1 (`EgoFrame.points`); there is no new kernel here.
"""
from __future__ import annotations

import math
import os

import torch

from .navigation import MAX_SCENES, EgoFrame, Navigator, _describe, _positive

ROW_WIDTH = 7      # x, y, yaw / pi, speed / speed_scale, throttle, steer, brake


class Demonstrations:
    """A sampler for `drive` that records: `drive(Demonstrations(Expert(...), camera, navigator, done=metrics.done, ...), vehicle,
    metrics, image=camera, world=world)`.

    `sampler`: what drives (anything `drive` takes: callable with `pose=`, `velocity=`, with a `last_control`); `camera`: the
    `Camera` whose static `frames` show this tick (`drive` renders through `image=camera` before it calls the sampler);
    `navigator`: the `Navigator` the sampler steps, whose `target` and `xy_scale` are recorded; `done`: `metrics.done`, int32
    `[S]`, read as it stands at the call, so it records the hold this tick's vehicle step will see; `capacity`: the ticks the
    logs hold -- a call beyond it raises; `horizon` = H rows per sample; `stride`: the ticks between two rows; `speed_scale`: what
    a speed in m/s is divided by (the reference's 'speed / scale' state column).

    Every call forwards to `sampler` and then copies `camera.frames`, `pose`, `velocity`, `navigator.target`,
    `sampler.last_control` and `done` into row `count` of the device logs `frames_log` uint8 `[capacity, S, h, w, 3]`,
    `pose_log` float64 `[capacity, S, 3]`, `velocity_log` float32 `[capacity, S]`, `target_log` float32 `[capacity, S, 2]`,
    `control_log` float32 `[capacity, S, 3]` and `done_log` int32 `[capacity, S]`.

    `labels()`: the sample index int64 `[n, 2]` = (tick, scene), `waypoints` float32 `[n, H, 7]` clipped to [-1, 1] and `target`
    float32 `[n, 2]`.  Row k of sample (t, s) describes the state at tick t + k * stride:
      x, y     the position then, in the ego frame of tick t: `EgoFrame(pose_t, xy_scale).points`, ego frame v1's `point`, so
               row 0 is (0, 0);
      yaw      d = (compass_k - compass_0) / pi in fp64, d - 2 when d > 1, d + 2 when d < -1, rounded to fp32;
      speed    (double)velocity_k / speed_scale, rounded to fp32;
      action   the control recorded at tick t + (k + 1) * stride: what was applied between this row and the next.
    A sample is VALID when every tick from t to t + H * stride was recorded and the scene's `done` was 0 at all of them.
    The samples come in (tick, scene) order.

    Two deviations from the reference's writer, on purpose.  Its wrap of the yaw column subtracts or adds 1 where 2 is meant (the
    column is in units of pi, a turn is 2), which maps a wrap across +-pi onto the wrong angle; here it is 2.  And it has a
    red-light special case that FABRICATES a sample of 16 standing rows with full brake when a sample starts at a red light;
    here nothing is fabricated: a vehicle that waits at a light is recorded as it stands, tick by tick."""

    def __init__(self, sampler, camera, navigator: Navigator, *, done: torch.Tensor, capacity: int, horizon: int = 16, stride: int,
                 speed_scale: float):
        if not callable(sampler):
            raise TypeError(f"Demonstrations: sampler must be callable like a sampler of drive, got {type(sampler).__name__}")
        if not isinstance(navigator, Navigator):
            raise TypeError(f"Demonstrations: navigator must be a Navigator, got {type(navigator).__name__}")
        frames = getattr(camera, "frames", None)
        if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise TypeError(f"Demonstrations: camera must be a Camera with uint8 frames [S, h, w, 3], got {_describe(frames)}")
        S, dev = navigator.scenes, navigator.device
        if frames.shape[0] != S or frames.device != dev:
            raise ValueError(f"Demonstrations: the camera's frames are {_describe(frames)}, the navigator holds {S} scenes on {dev}")
        if not torch.is_tensor(done) or done.dtype != torch.int32 or tuple(done.shape) != (S,) or done.device != dev:
            raise ValueError(f"Demonstrations: done must be int32 [{S}] on {dev} (DriveMetrics.done), got {_describe(done)}")
        capacity, horizon, stride = int(capacity), int(horizon), int(stride)
        if capacity < 1 or horizon < 1 or stride < 1:
            raise ValueError(f"Demonstrations: capacity, horizon and stride must be >= 1, got {capacity}, {horizon} and {stride}")
        self.sampler, self.camera, self.navigator, self.done = sampler, camera, navigator, done
        self.scenes, self.device, self.capacity, self.horizon, self.stride = S, dev, capacity, horizon, stride
        self.speed_scale = _positive(speed_scale, "Demonstrations: speed_scale")
        self.xy_scale = navigator.xy_scale
        self.model = getattr(sampler, "model", None)      # drive reads the xy scale of its sampler's model
        h, w = int(frames.shape[1]), int(frames.shape[2])
        self.frames_log = torch.zeros((capacity, S, h, w, 3), dtype=torch.uint8, device=dev)
        self.pose_log = torch.zeros((capacity, S, 3), dtype=torch.float64, device=dev)
        self.velocity_log = torch.zeros((capacity, S), dtype=torch.float32, device=dev)
        self.target_log = torch.zeros((capacity, S, 2), dtype=torch.float32, device=dev)
        self.control_log = torch.zeros((capacity, S, 3), dtype=torch.float32, device=dev)
        self.done_log = torch.zeros((capacity, S), dtype=torch.int32, device=dev)
        self.count = 0
        self._labels = None

    @property
    def last_control(self):
        return self.sampler.last_control

    def __call__(self, image=None, *, pose: torch.Tensor, velocity: torch.Tensor, **kw):
        """Forward to the sampler, then append this tick to the logs (six device copies, no allocation, no synchronisation)."""
        t, S = self.count, self.scenes
        if t >= self.capacity:
            raise IndexError(f"Demonstrations: the logs hold {self.capacity} ticks and are full")
        if not torch.is_tensor(pose) or pose.dtype != torch.float64 or tuple(pose.shape) != (S, 3) or pose.device != self.device:
            raise ValueError(f"Demonstrations: pose must be float64 [{S}, 3] on {self.device}, got {_describe(pose)}")
        if not torch.is_tensor(velocity) or velocity.dtype != torch.float32 or tuple(velocity.shape) != (S,) or velocity.device != self.device:
            raise ValueError(f"Demonstrations: velocity must be float32 [{S}] on {self.device}, got {_describe(velocity)}")
        out = self.sampler(image, pose=pose, velocity=velocity, **kw)
        control = self.sampler.last_control
        if control is None:
            raise ValueError("Demonstrations: the sampler produced no control; build it with a controller")
        self.frames_log[t].copy_(self.camera.frames)
        self.pose_log[t].copy_(pose)
        self.velocity_log[t].copy_(velocity)
        self.target_log[t].copy_(self.navigator.target)
        self.control_log[t].copy_(control)
        self.done_log[t].copy_(self.done)
        self.count, self._labels = t + 1, None
        return out

    def clear(self) -> None:
        """Forget the recorded ticks (the logs keep their storage)."""
        self.count, self._labels = 0, None

    @staticmethod
    def valid_index(done: torch.Tensor, *, horizon: int, stride: int) -> torch.Tensor:
        """int64 `[n, 2]` = (tick, scene) of the valid samples of a `done` log `[T, S]`, in that order: t + H * stride <= T - 1
        and `done` 0 at every tick from t to t + H * stride.  Plain torch, any device."""
        T, S = int(done.shape[0]), int(done.shape[1])
        span = int(horizon) * int(stride)
        last = T - 1 - span                                                             # the last tick a sample can start at
        if last < 0:
            return torch.zeros((0, 2), dtype=torch.int64, device=done.device)
        bad = torch.cat([torch.zeros((1, S), dtype=torch.int64, device=done.device), (done != 0).to(torch.int64).cumsum(0)])      # [T + 1, S]
        return ((bad[span + 1:span + last + 2] - bad[:last + 1]) == 0).nonzero()

    @staticmethod
    def form_labels(pose, velocity, target, control, done, *, horizon: int, stride: int, speed_scale: float, xy_scale: float):
        """`labels()` on given logs `[T, S, ...]` on one device (the recorded ticks only): the same rules, so a hand-written log
        can be labelled.  Returns (index int64 `[n, 2]`, waypoints float32 `[n, H, 7]`, target float32 `[n, 2]`); only the x and
        y columns launch a kernel (`EgoFrame.points`) -- with n = 0 nothing does."""
        H, st, dev = int(horizon), int(stride), pose.device
        index = Demonstrations.valid_index(done, horizon=H, stride=st)
        n = int(index.shape[0])
        t0, sc = index[:, 0], index[:, 1]
        ticks = t0[:, None] + st * torch.arange(H, device=dev)[None, :]                   # [n, H]
        scn = sc[:, None].expand(-1, H)
        wps = torch.zeros((n, H, ROW_WIDTH), dtype=torch.float32, device=dev)
        if n:
            pose0 = pose[t0, sc].contiguous()                                            # [n, 3]
            pts = pose[ticks, scn][..., 0:2].contiguous()                                # [n, H, 2]
            for a in range(0, n, MAX_SCENES):                                            # ego frame v1 takes 65535 scenes a launch
                b = min(a + MAX_SCENES, n)
                wps[a:b, :, 0:2] = EgoFrame(pose0[a:b].contiguous(), xy_scale).points(pts[a:b].contiguous())
            # the divisors are device tensors: by a host scalar torch multiplies with the reciprocal, which is not the division
            pi, scale = (torch.full((), v, dtype=torch.float64, device=dev) for v in (math.pi, float(speed_scale)))
            d = (pose[ticks, scn][..., 2] - pose0[:, 2:3]) / pi
            d = torch.where(d > 1.0, d - 2.0, torch.where(d < -1.0, d + 2.0, d))
            wps[:, :, 2] = d.to(torch.float32)
            wps[:, :, 3] = (velocity[ticks, scn].to(torch.float64) / scale).to(torch.float32)
            wps[:, :, 4:7] = control[ticks + st, scn]
        return index, wps.clip(-1, 1), target[t0, sc].clone()

    def labels(self):
        """(index, waypoints, target) of every valid sample recorded so far, on the device (cached until the next call records)."""
        if self._labels is None:
            T = self.count
            self._labels = self.form_labels(self.pose_log[:T], self.velocity_log[:T], self.target_log[:T], self.control_log[:T],
                                            self.done_log[:T], horizon=self.horizon, stride=self.stride, speed_scale=self.speed_scale,
                                            xy_scale=self.xy_scale)
        return self._labels

    def __len__(self) -> int:
        return int(self.labels()[0].shape[0])

    def batch(self, indices):
        """Samples `indices` (a sequence or tensor of positions in `labels()`'s order) as device tensors shaped like a collated
        batch of `TrajDataset`: frames uint8 `[n, h, w, 3]`, waypoints float32 `[n, H, 7]`, target float32 `[n, 2]`."""
        index, wps, target = self.labels()
        idx = torch.as_tensor(indices, dtype=torch.int64, device=self.device).reshape(-1)
        n = int(index.shape[0])
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
            raise IndexError(f"Demonstrations.batch: indices must lie in 0..{n - 1}")
        return self.frames_log[index[idx, 0], index[idx, 1]], wps[idx], target[idx]

    def save(self, root: str, start: int = 0) -> int:
        """Write every valid sample under `root` in the reference's on-disk format, numbered from `start`:
        `front/%06d.png` and `waypoints/%06d.txt` (line 1 the target, then H lines of 7 numbers), so that
        `TrajDataset(root, horizon=H)` reads the same samples back.  Every float is written through `repr(float(x))`, which
        round-trips an fp32 value exactly.  Returns the samples written."""
        from PIL import Image
        index, wps, target = self.labels()
        os.makedirs(os.path.join(root, "front"), exist_ok=True)
        os.makedirs(os.path.join(root, "waypoints"), exist_ok=True)
        idx, wps, target = index.cpu(), wps.cpu().numpy(), target.cpu().numpy()
        frames = self.frames_log[index[:, 0], index[:, 1]].cpu().numpy() if len(idx) else None
        for i in range(len(idx)):
            name = f"{int(start) + i:06d}"
            Image.fromarray(frames[i]).save(os.path.join(root, "front", name + ".png"))
            with open(os.path.join(root, "waypoints", name + ".txt"), "w") as f:
                f.write(" ".join(repr(float(v)) for v in target[i]) + "\n")
                for row in wps[i]:
                    f.write(" ".join(repr(float(v)) for v in row) + "\n")
        return len(idx)

    def __repr__(self):
        return (f"Demonstrations(scenes={self.scenes}, recorded={self.count} of {self.capacity} ticks, horizon={self.horizon}, "
                f"stride={self.stride}, speed_scale={self.speed_scale}, frames={tuple(self.frames_log.shape[2:4])}, device={self.device})")
