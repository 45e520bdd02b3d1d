"""The front camera of a closed loop, rendered on the device: an analytic ray caster over exactly the primitives the loop already
holds -- the ground with its roads and stop lines, the world's boxes and discs, the lamps and poles of its signals.

The reference closes its loop through CARLA's RGB sensor (e2e_driving/diffusion_agent.py: sensors(): 900 x 256, fov 100 degrees,
1.5 m behind the vehicle centre, 2.0 m up, pitch 0).  This package rules the simulator out, so the renderer is its
own: `Camera.render(pose)` is one call of `adx_camera_render` (csrc/camera.hip, "camera v1" of include/adx.h) -- a small stage
launch that puts every primitive into the camera frame, and the render launch that writes the frame the encoder reads.

`drive(sampler, vehicle, metrics, image=camera, world=world)` is then a loop in which perception is in the loop: a light that turns
red and a car that brakes in front of the ego change the pixels the ResNet sees.  THE FRAMES ARE FLAT-SHADED GEOMETRY, NOT A TOWN:
no textures, no lighting, no fog (the contract's "differs"), and CARLA-trained weights do not transfer.  What a score says about
driving is still a property of weights.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .navigation import MAX_SCENES, _describe, _device, _positive
from .ops import IMAGENET_MEAN, IMAGENET_STD
from .simulation import MAX_SLOTS, World, _no_cpu, _nonneg, _static

MAX_PATHS, MAX_PATH_POINTS, PALETTE_ROWS, FACES = 8, 64, 20, 5
HEADER_WORDS, OBJECT_WORDS, GROUND_WORDS = 16, 16, 8
CLASSES = ("sky", "ground", "road", "marking", "stop line", "box", "disc", "lamp", "pole")
# the committed default of adx_camera_default_palette (csrc/camera.hip), so that an object on a CPU device shows it too
DEFAULT_PALETTE = ((135, 190, 235), (96, 128, 72), (120, 140, 110), (70, 70, 74), (230, 230, 225), (250, 250, 250),
                   (200, 40, 40), (40, 80, 200), (230, 200, 40), (240, 240, 240), (30, 30, 30), (40, 160, 80), (150, 90, 170),
                   (230, 130, 40), (150, 110, 70), (60, 60, 60), (30, 220, 60), (250, 210, 30), (240, 30, 30), (250, 120, 20))
DEFAULT_SHADE = (200, 232, 168, 184, 255)


def _finite(v, what: str) -> float:
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"{what} must be finite, got {v}")
    return v


class Camera:
    """The front cameras of S scenes ("camera v1" of include/adx.h) and the static outputs of `render`.

    `width`, `height` (8..2048, 8..1024), `fov_deg` (the horizontal field of view, below 3 rad), `mount_back` and `cam_height`:
    the eye at ego (0, mount_back, cam_height) metres; the defaults are the reference's sensor.  `world`: a `World` whose `boxes`,
    `discs`, `signals.records` and `signals.phase` are read IN PLACE at every render, so the camera sees traffic and lights as of
    their last step (None: an empty world).  `roads` float64 `[S, Q, G, 2]` world metres with `road_lengths` int `[S, Q]`, Q in
    1..8 polylines of G in 2..64 points -- `Traffic`'s path layout; `Camera.roads_from(traffic, navigator)` builds them; host
    values are uploaded once, device tensors are read in place.  `half_width`, `mark`: a road is the ground within half_width of
    a polyline, its outer `mark` metres the edge marking; `line_half`: half the painted width of a stop line; `far`: beyond it
    the ground is one flat colour; `box_height`, `disc_height`, `lamp_radius`, `lamp_height`, `lamp_setback` (metres beyond its
    stop line along the driving direction), `pole_radius` (0: no pole); `palette` uint8 `[20, 3]` and `shade` uint8 `[5]` (None:
    the committed default); `mean`, `std`: the normalisation of `image`.
    All static, the same storage at every call, so a captured graph and a `GraphedSampler` can hold them:
      `frames` uint8 `[S, H, W, 3]`   `forward_frames`' format
      `image`  float32 `[S, 3, H, W]` bit for bit `ops.image_transform(frames, mean, std)`
      `ids`    int32 `[S, H, W]`      face << 16 | class << 8 | slot            (with `ids=True`)
      `depth`  float32 `[S, H, W]`    the forward depth in metres, +inf for sky  (with `depth=True`)
      `prims`  float32                the primitive table of the last render
    An object on a CPU device can be built and inspected; its launches refuse (there is no CPU path)."""

    def __init__(self, scenes: int, device, *, width: int = 900, height: int = 256, fov_deg: float = 100.0, mount_back: float = -1.5,
                 cam_height: float = 2.0, world: Optional[World] = None, roads=None, road_lengths=None, half_width: float = 1.75,
                 mark: float = 0.15, line_half: float = 0.2, near: float = 0.1, far: float = 150.0, box_height: float = 1.6,
                 disc_height: float = 1.8, lamp_radius: float = 0.35, lamp_height: float = 4.0, lamp_setback: float = 12.0,
                 pole_radius: float = 0.1, palette=None, shade=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, ids: bool = False,
                 depth: bool = False):
        S, W, H, dev = int(scenes), int(width), int(height), _device(device)
        if not 1 <= S <= MAX_SCENES:
            raise ValueError(f"Camera: scenes must be 1..{MAX_SCENES}, got {S}")
        if not (8 <= W <= 2048 and 8 <= H <= 1024):
            raise ValueError(f"Camera: width must be 8..2048 and height 8..1024, got {W} x {H}")
        fov = math.radians(_positive(fov_deg, "Camera: fov_deg"))
        if not fov < 3.0:
            raise ValueError(f"Camera: fov_deg must be below {math.degrees(3.0):.3f} (3 rad), got {fov_deg}")
        self.scenes, self.width, self.height, self.device, self.fov = S, W, H, dev, fov
        self.mount_back, self.lamp_setback = _finite(mount_back, "Camera: mount_back"), _finite(lamp_setback, "Camera: lamp_setback")
        for name, v in (("cam_height", cam_height), ("near", near), ("far", far), ("half_width", half_width), ("line_half", line_half),
                        ("box_height", box_height), ("disc_height", disc_height), ("lamp_radius", lamp_radius), ("lamp_height", lamp_height)):
            setattr(self, name, _positive(v, f"Camera: {name}"))
        self.mark, self.pole_radius = _nonneg(mark, "Camera: mark"), _nonneg(pole_radius, "Camera: pole_radius")
        if not self.far > self.near:
            raise ValueError(f"Camera: far must exceed near, got {self.far} and {self.near}")
        if not self.mark <= self.half_width:
            raise ValueError(f"Camera: mark must not exceed half_width, got {self.mark} and {self.half_width}")
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if len(self.mean) != 3 or len(self.std) != 3 or not all(math.isfinite(v) for v in self.mean + self.std) or 0.0 in self.std:
            raise ValueError(f"Camera: mean and std must be three finite values each, std not 0, got {mean} and {std}")
        self.palette = np.array(DEFAULT_PALETTE if palette is None else palette, dtype=np.uint8)
        self.shade = np.array(DEFAULT_SHADE if shade is None else shade, dtype=np.uint8)
        if self.palette.shape != (PALETTE_ROWS, 3) or self.shade.shape != (FACES,):
            raise ValueError(f"Camera: palette must be uint8 [{PALETTE_ROWS}, 3] and shade uint8 [{FACES}], got {self.palette.shape} and "
                             f"{self.shade.shape}")
        # ---- the world, read in place ----
        if world is not None and not isinstance(world, World):
            raise TypeError(f"Camera: world must be a World, got {type(world).__name__}")
        self.world = world
        self.n_boxes = self.n_discs = self.n_signals = 0
        if world is not None:
            for name, t in (("boxes", world.boxes), ("discs", world.discs)):
                if t is not None and (t.shape[0] != S or t.device != dev):
                    raise ValueError(f"Camera: the world's {name} are {_describe(t)}, the camera holds {S} scenes on {dev}")
            if world.signals is not None and (world.signals.scenes != S or world.signals.device != dev):
                raise ValueError(f"Camera: the world's signals hold {world.signals.scenes} scenes on {world.signals.device}, the camera "
                                 f"{S} on {dev}")
            self.n_boxes = 0 if world.boxes is None else int(world.boxes.shape[1])
            self.n_discs = 0 if world.discs is None else int(world.discs.shape[1])
            self.n_signals = 0 if world.signals is None else world.signals.n_signals
        # ---- the roads ----
        self.roads = self.road_lengths = None
        self.n_paths = self.n_points = 0
        if (roads is None) != (road_lengths is None):
            raise ValueError("Camera: roads and road_lengths come together")
        if roads is not None:
            self.roads = self._upload(roads, torch.float64, "roads")
            self.road_lengths = self._upload(road_lengths, torch.int32, "road_lengths")
            if self.roads.dim() != 4 or self.roads.shape[0] != S or self.roads.shape[3] != 2 or not 1 <= self.roads.shape[1] <= MAX_PATHS \
                    or not 2 <= self.roads.shape[2] <= MAX_PATH_POINTS:
                raise ValueError(f"Camera: roads must be [{S}, 1..{MAX_PATHS}, 2..{MAX_PATH_POINTS}, 2] world metres, got "
                                 f"{tuple(self.roads.shape)}")
            self.n_paths, self.n_points = int(self.roads.shape[1]), int(self.roads.shape[2])
            if tuple(self.road_lengths.shape) != (S, self.n_paths):
                raise ValueError(f"Camera: road_lengths must be [{S}, {self.n_paths}], got {tuple(self.road_lengths.shape)}")
        self._cfg = L.CameraCfg(S, W, H, self.n_boxes, self.n_discs, self.n_signals, self.n_paths, self.n_points, fov, self.mount_back,
                                self.cam_height, self.near, self.far, self.half_width, self.mark, self.line_half, self.box_height,
                                self.disc_height, self.lamp_radius, self.lamp_height, self.lamp_setback, self.pole_radius,
                                (C.c_float * 3)(*self.mean), (C.c_float * 3)(*self.std), (C.c_uint8 * 60)(*self.palette.reshape(-1).tolist()),
                                (C.c_uint8 * 5)(*self.shade.tolist()))
        self.n_objects = self.n_boxes + self.n_discs + 2 * self.n_signals
        self.n_ground = self.n_signals + self.n_paths * max(self.n_points - 1, 0)
        self.scene_words = HEADER_WORDS + OBJECT_WORDS * self.n_objects + GROUND_WORDS * self.n_ground
        nbytes = int(L.lazy("adx_camera_prims_bytes")(C.byref(self._cfg)))
        if nbytes != 4 * S * self.scene_words:
            raise L.AdxError(f"adx_camera_prims_bytes = {nbytes}: not the table of camera v1 ({4 * S * self.scene_words})")
        self.prims = torch.zeros((S, self.scene_words), dtype=torch.float32, device=dev)
        self.frames = torch.zeros((S, H, W, 3), dtype=torch.uint8, device=dev)
        self.image = torch.zeros((S, 3, H, W), dtype=torch.float32, device=dev)
        self.ids = torch.zeros((S, H, W), dtype=torch.int32, device=dev) if ids else None
        self.depth = torch.zeros((S, H, W), dtype=torch.float32, device=dev) if depth else None

    def _upload(self, t, dtype, name: str) -> torch.Tensor:
        if torch.is_tensor(t) and t.is_cuda:
            if t.dtype != dtype or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"Camera: {name} on the device are read in place and must be contiguous {dtype} on {self.device}, got "
                                 f"{_describe(t)}")
            return t
        try:
            host = torch.as_tensor(np.asarray(t.detach().numpy() if torch.is_tensor(t) else t)).to(dtype)
        except (TypeError, ValueError) as e:
            raise TypeError(f"Camera: {name} must be numeric values, got {type(t).__name__}") from e
        return host.to(self.device, copy=True).contiguous()

    @staticmethod
    def roads_from(traffic=None, navigator=None):
        """(`roads` float64 `[S, Q, G, 2]`, `road_lengths` int32 `[S, Q]`) on the device: the traffic's paths and / or the
        navigator's route as one more path (a route of more than 64 points does not fit a path: decimate it first).  With both, the
        shorter rows are padded to the longer G with their last point; the lengths say what counts."""
        parts = []
        if traffic is not None:
            parts.append((traffic.paths, traffic.lengths.to(torch.int32)))
        if navigator is not None:
            r = navigator.route_m
            if r.shape[1] > MAX_PATH_POINTS:
                raise ValueError(f"Camera.roads_from: the navigator's route holds {r.shape[1]} points, a path at most {MAX_PATH_POINTS}")
            if r.shape[1] < 2:
                raise ValueError("Camera.roads_from: a route of one point is no road")
            parts.append((r[:, None].to(torch.float64), navigator.lengths.to(torch.int32)[:, None]))
        if not parts:
            raise ValueError("Camera.roads_from: give traffic=, navigator= or both")
        G = max(p.shape[2] for p, _ in parts)
        padded = [p if p.shape[2] == G else torch.cat([p, p[:, :, -1:].expand(-1, -1, G - p.shape[2], -1)], dim=2) for p, _ in parts]
        roads, lengths = torch.cat(padded, dim=1).contiguous(), torch.cat([n for _, n in parts], dim=1).contiguous()
        if roads.shape[1] > MAX_PATHS:
            raise ValueError(f"Camera.roads_from: {roads.shape[1]} paths, the camera draws at most {MAX_PATHS}")
        return roads, lengths

    def key(self) -> tuple:
        """What a captured launch bakes in."""
        w = self.world
        return (self.scenes, self.width, self.height, self.fov, self.mount_back, self.cam_height, self.near, self.far, self.half_width,
                self.mark, self.line_half, self.box_height, self.disc_height, self.lamp_radius, self.lamp_height, self.lamp_setback,
                self.pole_radius, self.mean, self.std, self.palette.tobytes(), self.shade.tobytes(), self.n_boxes, self.n_discs,
                self.n_signals, self.n_paths, self.n_points,
                L.ptr(None if w is None else w.boxes), L.ptr(None if w is None else w.discs),
                L.ptr(None if w is None or w.signals is None else w.signals.records),
                L.ptr(None if w is None or w.signals is None else w.signals.phase), L.ptr(self.roads), L.ptr(self.road_lengths),
                self.prims.data_ptr(), self.frames.data_ptr(), self.image.data_ptr(), L.ptr(self.ids), L.ptr(self.depth))

    def render(self, pose: torch.Tensor, hold: Optional[torch.Tensor] = None) -> "Camera":
        """One C call (two launches) on the current stream, no allocation, no synchronisation: `pose` float64 `[S, 3]` as ego
        frame v1 takes it (a `KinematicVehicle`'s static output); `hold` int32 `[S]` or None: a held scene's table and outputs are
        left as they are.  The world's boxes, discs, signal records and phases are read as they stand; the phases of signals that
        have never stepped are all 0, which draws no lamp and no stop line."""
        S, dev, w = self.scenes, self.device, self.world
        _static(pose, (S, 3), torch.float64, dev, "Camera: pose")
        if hold is not None:
            _static(hold, (S,), torch.int32, dev, "Camera: hold")
        _no_cpu(dev, "the camera")
        boxes = None if w is None else w.boxes
        discs = None if w is None else w.discs
        signals = None if w is None else w.signals
        if (0 if boxes is None else int(boxes.shape[1])) != self.n_boxes or (0 if discs is None else int(discs.shape[1])) != self.n_discs:
            raise ValueError("Camera: the world's boxes or discs changed shape since the camera was built")
        L.check(L.lazy("adx_camera_render")(C.byref(self._cfg), pose.data_ptr(), L.ptr(boxes), L.ptr(discs),
                                            L.ptr(None if signals is None else signals.records),
                                            L.ptr(None if signals is None else signals.phase), L.ptr(self.roads), L.ptr(self.road_lengths),
                                            L.ptr(hold), self.prims.data_ptr(), self.frames.data_ptr(), self.image.data_ptr(),
                                            L.ptr(self.ids), L.ptr(self.depth), L.stream_ptr(dev)), "adx_camera_render")
        return self

    def __call__(self, tick: int, pose: torch.Tensor) -> torch.Tensor:
        """`drive`'s `image=callable(tick, pose)`: renders and returns the static `image`.  `drive` primes the world's signals (one
        step on the start pose) before it asks for the first image, so tick 0 already shows the right lamps; at tick t the frame
        shows the traffic and the lights as of the step that followed tick t - 1's vehicle step -- the world at this tick's pose."""
        return self.render(pose).image

    def __repr__(self):
        return (f"Camera(scenes={self.scenes}, {self.width} x {self.height}, fov={math.degrees(self.fov):.1f} deg, boxes={self.n_boxes}, "
                f"discs={self.n_discs}, signals={self.n_signals}, roads={self.n_paths} x {self.n_points}, device={self.device})")
