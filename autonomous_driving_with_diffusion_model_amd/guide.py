"""Guide: where a sampling tick must NOT go ("cost guidance v1", include/adx.h) -- and, since v4, where the road is.

A guide is what the caller knows of the scene's obstacles -- moving discs (a parked car, a crossing pedestrian) and half-planes (a
stop line, a lane edge) -- per scene, in the model's own units (the units of `target` and of the clamped result before xy
scaling) and in THIS tick's ego frame.  Every sampler step moves the xy of its predicted clean trajectory down the gradient of
the cost of those constraints, inside the step kernel, and derives the rest of the step from the moved x0: analytic cost guidance
as Diffuser-style planners use it, and how the reference's classifier guidance acts for its own PRED_TYPE = "sample".

    discs    [S, M, 5] = (cx, cy, vx, vy, r), M <= 32: at waypoint h the centre is (cx + h * vx, cy + h * vy); a slot with
             r <= 0 (or NaN) is empty, so scenes with fewer obstacles pad with zeros.
    planes   [S, P, 3] = (nx, ny, b), P <= 8: the half-plane nx * x + ny * y <= b is allowed.
    scale    the step size; `schedule` "variance" multiplies it by the step's noise variance (guidance fades as the sample gets
             clean, Diffuser's Sigma-scaling), "constant" uses it as it is.
    cap      the largest move of one coordinate in one iteration (inf: none); `iters`: gradient iterations per step, 1..8.

A guide may also hold a FIELD ("cost guidance v2"): `field=CostField(cells, origin, cell, weight)`, a cost raster [S, Gy, Gx] a
perception stack produces (drivable area, kerbs, parked-car blobs), read bilinearly at every waypoint after the discs and planes.
`CostField.from_occupancy` makes one from a binary occupancy raster in one launch ("cost field from occupancy v1").  A guide
without a field is cost guidance v1, bit for bit.

A guide may also hold MOTION LIMITS ("cost guidance v3"): `motion=MotionLimits(limits)`, per scene `(s_max, a_max)`: no segment of
the plan longer than s_max, no second difference longer than a_max, in the model's units per waypoint interval.  For this model
speed IS the spacing of the waypoints (the controller derives its desired speed from it), so these are a speed and an acceleration
limit; `MotionLimits.from_physical` converts from m/s and m/s^2.  The terms couple neighbouring waypoints: a step with limits
runs the row-wise step kernel (one wave per row, H <= 64).  A guide without limits is v1 / v2, bit for bit.

A guide may also hold a ROUTE ("cost guidance v4"): `route=Route(points, half_width)`, per scene a polyline of R <= 32 points and a
half-width: a waypoint further than the half-width from the polyline pays for it and is pulled back -- "stay in this lane / on this
route", the one thing the reference's own driver has in hand every tick (its route planner's future waypoints).  The term is
point-wise, so it runs in whichever step kernel the guide's other terms pick; `Route.from_physical` converts from metres.  A guide
without a route is v1 / v2 / v3, bit for bit.

A guide may also hold CAPSULES ("cost guidance v5"): `capsules=Capsules(slots)`, per scene up to 32 moving segments with a radius
-- the other road users as a perception stack reports them, oriented boxes with a heading, which one disc fits badly.  The
potential is the disc's around the nearest point of the segment, so a disc is the capsule of zero length.  The term is point-wise,
like the route; `Capsules.from_boxes` converts boxes on the device in one launch, `Capsules.boxes_from_physical` prepares them from
metres, m/s and a yaw angle.  A guide without capsules is v1 .. v4, bit for bit.

No reference counterpart as a caller-facing object: the reference names the idea (GUIDANCE.LOSS_LIST) and has one entry, under
CLASSIFIER_GUIDANCE only.  Whether guided plans drive better is a property of trained weights and is not measured in this
repository.
"""
from __future__ import annotations

import ctypes as C
import math
import operator
from typing import Optional, Tuple

import torch

from . import _lib as L

SCHEDULES = ("variance", "constant")
MAX_DISCS, MAX_PLANES, MAX_ITERS = 32, 8, 8
MIN_NODES, MAX_NODES, MAX_RADIUS = 2, 256, 16
MIN_ROUTE_POINTS, MAX_ROUTE_POINTS = 2, 32
MAX_CAPSULES = 32


def _f32(v: float) -> float:
    """The fp32 number nearest v, as a Python float."""
    return C.c_float(v).value


def _pair(v, name: str) -> Tuple[float, float]:
    try:
        a, b = v
        return float(a), float(b)
    except (TypeError, ValueError):
        raise ValueError(f"CostField: {name} must be a pair of numbers, got {v!r}") from None


def _geometry(origin, cell) -> Tuple[float, float, float, float]:
    """(x_min, y_min, dx, dy) of a raster, or a refusal: a finite origin, finite cell sizes > 0 whose fp32 reciprocals are finite."""
    (x_min, y_min), (dx, dy) = _pair(origin, "origin"), _pair(cell, "cell")
    if not (math.isfinite(x_min) and math.isfinite(y_min)):
        raise ValueError(f"CostField: origin must be finite, got ({x_min}, {y_min})")
    for name, d in (("dx", dx), ("dy", dy)):
        if not (math.isfinite(d) and d > 0.0 and math.isfinite(_f32(1.0 / d)) and _f32(1.0 / d) > 0.0):
            raise ValueError(f"CostField: cell {name} must be finite and > 0 with a finite fp32 reciprocal, got {d}")
    return x_min, y_min, dx, dy


def _raster(t, what: str) -> None:
    if not torch.is_tensor(t):
        raise TypeError(f"CostField: {what} must be a tensor, got {type(t).__name__}")
    if t.dim() != 3 or t.shape[0] < 1:
        raise ValueError(f"CostField: {what} must be [S, Gy, Gx], got {tuple(t.shape)}")
    if not (MIN_NODES <= t.shape[1] <= MAX_NODES and MIN_NODES <= t.shape[2] <= MAX_NODES):
        raise ValueError(f"CostField: {what} holds {t.shape[1]} x {t.shape[2]} nodes (Gy x Gx), supported {MIN_NODES}..{MAX_NODES} each")
    if t.dtype != torch.float32:
        raise TypeError(f"CostField: {what} must be float32, got {t.dtype}")


class _Record:
    """What the record classes of a guide share.  Each declares, as class attributes, what `Guide` and its consumers walk (RECORDS
    below holds the classes in version order, the order of the exports' arguments):

        ATTR       its attribute of a Guide, the keyword of `Guide.__init__` and `Guide.like`
        NOUN       what a refusal about it calls it ("the field"); EARLIER: what a refusal about a later record calls it ("field")
        SUFFIX     of the exports whose last record it is (`adx_ddim_step_<SUFFIX>`, ...)
        POINTWISE  whether its term names places (the stop-short fallback looks for those)
        TENSORS    the names of its tensors, in the order `like` takes them; the first, the lead tensor, says how many scenes the
                   record holds and where they live
    """
    ATTR = NOUN = EARLIER = SUFFIX = ""
    POINTWISE = False
    TENSORS: Tuple[str, ...] = ()

    def __init_subclass__(cls):
        cls._PATHS = tuple((name, f"guide.{cls.ATTR}.{name}") for name in cls.TENSORS)      # what a refusal calls each tensor

    @property
    def lead(self) -> torch.Tensor:
        return getattr(self, self.TENSORS[0])

    @property
    def scenes(self) -> int:
        return int(self.lead.shape[0])

    @property
    def device(self) -> torch.device:
        return self.lead.device

    def tensors(self) -> tuple:
        """((name, tensor), ...) in the order of TENSORS."""
        return tuple((name, getattr(self, name)) for name in self.TENSORS)

    def clone(self):
        """The same settings over clones of the tensors."""
        return self.like(*(t.clone() for _, t in self.tensors()))

    def _on_device_of(self, x: torch.Tensor) -> None:
        """Every tensor a float32 GPU tensor on the device of the sample `x`, or a refusal."""
        dev = x.device                      # this runs on every step of an eager tick
        for name, path in self._PATHS:
            t = getattr(self, name)
            if L.require_gpu_f32(t, path).device != dev:
                raise ValueError(f"{path} lives on {t.device}, the sample on {dev}")


class CostField(_Record):
    """The field of "cost guidance v2" (include/adx.h): `cells` float32 `[S, Gy, Gx]`, 2 <= Gy, Gx <= 256, node `[i][j]` at
    `(x_min + j * dx, y_min + i * dy)` in the model's units and this tick's ego frame; `origin` = (x_min, y_min), `cell` =
    (dx, dy), `weight` >= 0.  A waypoint inside the raster pays `weight` times the bilinear interpolant where that is positive;
    outside the raster the field says nothing (add planes for "off the map is forbidden").  The cells are read at every step:
    new values need no new object (and, in a GraphedSampler, no new capture); shape, geometry and weight are baked."""
    ATTR, NOUN, EARLIER, SUFFIX, POINTWISE, TENSORS = "field", "the field", "field", "field", True, ("cells",)

    def __init__(self, cells: torch.Tensor, origin=(0.0, 0.0), cell=(1.0, 1.0), weight: float = 1.0):
        _raster(cells, "cells")
        self.x_min, self.y_min, self.dx, self.dy = _geometry(origin, cell)
        weight = float(weight)
        if not weight >= 0.0:
            raise ValueError(f"CostField: weight must be >= 0, got {weight}")
        self.cells, self.weight = cells.contiguous(), weight

    def key(self) -> tuple:
        """What a captured graph bakes: everything but the values of the cells."""
        return (int(self.cells.shape[1]), int(self.cells.shape[2]), self.x_min, self.y_min, self.dx, self.dy, self.weight)

    def like(self, cells: torch.Tensor) -> "CostField":
        """The same geometry and weight over other cells."""
        return CostField(cells, (self.x_min, self.y_min), (self.dx, self.dy), self.weight)

    def desc(self, x: torch.Tensor) -> L.FieldDesc:
        """The `adx_guide_field` of a launch on `x` [B, H, D].  The struct holds an address: keep this object alive until the
        launch is enqueued."""
        self._on_device_of(x)
        f = L.FieldDesc()
        S, Gy, Gx = self.cells.shape
        f.cells, f.scene_rows, f.gy, f.gx = self.cells.data_ptr(), S, Gy, Gx
        f.x_min, f.y_min, f.inv_dx, f.inv_dy, f.weight = self.x_min, self.y_min, 1.0 / self.dx, 1.0 / self.dy, self.weight
        return f

    @staticmethod
    def from_occupancy(occ: torch.Tensor, origin, cell, margin: float, weight: float = 1.0,
                       out: Optional[torch.Tensor] = None) -> "CostField":
        """A field from a binary occupancy raster `occ` float32 [S, Gy, Gx] (occupied iff > 0.5), one launch of
        `adx_cost_field_from_occupancy` ("cost field from occupancy v1"): 0.5 on an occupied node, falling to 0 at distance
        `margin` from the nearest one -- the disc potential of cost guidance v1 around it.  The search window is
        ceil(margin / dx) x ceil(margin / dy) nodes, at most 16 each.  `out`: cells to write (a static buffer of a captured
        graph); None allocates."""
        _raster(occ, "occ")
        x_min, y_min, dx, dy = _geometry(origin, cell)
        margin = float(margin)
        if not (math.isfinite(margin) and margin > 0.0):
            raise ValueError(f"CostField.from_occupancy: margin must be finite and > 0, got {margin}")
        rx, ry = math.ceil(margin / dx), math.ceil(margin / dy)
        if rx > MAX_RADIUS or ry > MAX_RADIUS:
            raise ValueError(f"CostField.from_occupancy: margin {margin} spans {ry} x {rx} cells (dy {dy}, dx {dx}), at most "
                             f"{MAX_RADIUS} each: use a coarser raster or a smaller margin")
        occ = L.require_gpu_f32(occ, "occ")
        if out is None:
            out = torch.empty_like(occ)
        else:
            _raster(out, "out")
            if out.shape != occ.shape or out.device != occ.device or not out.is_contiguous():
                raise ValueError(f"CostField.from_occupancy: out must be contiguous {tuple(occ.shape)} on {occ.device}, got "
                                 f"{tuple(out.shape)} on {out.device}")
        S, Gy, Gx = occ.shape
        L.check(L.lazy("adx_cost_field_from_occupancy")(occ.data_ptr(), out.data_ptr(), S, Gy, Gx, dx, dy, 1.0 / (margin * margin), ry, rx,
                                                        L.stream_ptr(occ.device)), "adx_cost_field_from_occupancy")
        return CostField(out, (x_min, y_min), (dx, dy), weight)

    def __repr__(self):
        return (f"CostField(cells={tuple(self.cells.shape)}, origin=({self.x_min}, {self.y_min}), cell=({self.dx}, {self.dy}), "
                f"weight={self.weight})")


class MotionLimits(_Record):
    """The motion limits of "cost guidance v3" (include/adx.h): `limits` float32 `[S, 2]` = per scene `(s_max, a_max)` in the
    model's own units (the clamped result before xy scaling) per waypoint interval.  `s_max` caps the length of a segment
    `|p[i+1] - p[i]|`, `a_max` the length of a second difference `|p[i+1] - 2 p[i] + p[i-1]|`; `inf` switches a term off for that
    scene (a NaN does too), `s_max = 0` means "do not move".  A plan over a limit pays `w * (excess of the squared length)^2 / 2`;
    `w_speed`, `w_accel` >= 0, and a weight of exactly 0 switches its term off everywhere.  The squared excess is small in the
    model's units: weights that make the terms dimensionless are `1 / s_ref**4` and `1 / a_ref**4` for a typical segment `s_ref`
    and second difference `a_ref` (an excess of s_ref^2 then costs 1/2, like a waypoint on a disc's centre).  The first waypoint,
    the ego's present pose, is never moved by these terms.  The limits are read at every step: new values need no new object
    (and, in a GraphedSampler, no new capture); the weights are baked.

    With `TrajectorySelector(hard=True)` the limits inherit v1's property: a candidate that sits one ulp over a limit is "not
    free".  A separate tolerance for selection does not exist."""
    ATTR, NOUN, EARLIER, SUFFIX, POINTWISE, TENSORS = "motion", "the motion limits", "motion limits", "motion", False, ("limits",)

    def __init__(self, limits: torch.Tensor, w_speed: float = 1.0, w_accel: float = 1.0):
        if not torch.is_tensor(limits):
            raise TypeError(f"MotionLimits: limits must be a tensor, got {type(limits).__name__}")
        if limits.dim() != 2 or limits.shape[1] != 2 or limits.shape[0] < 1:
            raise ValueError(f"MotionLimits: limits must be [S, 2] = (s_max, a_max) per scene, got {tuple(limits.shape)}")
        if limits.dtype != torch.float32:
            raise TypeError(f"MotionLimits: limits must be float32, got {limits.dtype}")
        w_speed, w_accel = float(w_speed), float(w_accel)
        for name, w in (("w_speed", w_speed), ("w_accel", w_accel)):
            if not w >= 0.0:
                raise ValueError(f"MotionLimits: {name} must be >= 0, got {w}")
        self.limits, self.w_speed, self.w_accel = limits.contiguous(), w_speed, w_accel

    def key(self) -> tuple:
        """What a captured graph bakes: everything but the values of the limits."""
        return (self.w_speed, self.w_accel)

    def like(self, limits: torch.Tensor) -> "MotionLimits":
        """The same weights over other limits."""
        return MotionLimits(limits, self.w_speed, self.w_accel)

    def desc(self, x: torch.Tensor) -> L.MotionDesc:
        """The `adx_guide_motion` of a launch on `x` [B, H, D].  The struct holds an address: keep this object alive until the
        launch is enqueued."""
        self._on_device_of(x)
        m = L.MotionDesc()
        m.limits, m.scene_rows, m.w_speed, m.w_accel = self.limits.data_ptr(), self.limits.shape[0], self.w_speed, self.w_accel
        return m

    @staticmethod
    def from_physical(v_max, a_max, dt: float, xy_scale: float, w_speed: float = 1.0, w_accel: float = 1.0,
                      device=None) -> "MotionLimits":
        """Limits from physical ones, on the host: `v_max` (m/s) and `a_max` (m/s^2) are numbers or sequences of S numbers (one
        per scene; a number stands for all), `dt` the seconds between two waypoints, `xy_scale` the metres of one model unit
        (`model.magic_num`).  s_max = v_max * dt / xy_scale and a_max = a_max * dt * dt / xy_scale, formed in double and rounded
        to fp32 once.  `inf` stays `inf`."""
        dt, xy_scale = float(dt), float(xy_scale)
        if not (math.isfinite(dt) and dt > 0.0 and math.isfinite(xy_scale) and xy_scale > 0.0):
            raise ValueError(f"MotionLimits.from_physical: dt and xy_scale must be finite and > 0, got {dt} and {xy_scale}")
        v = [float(t) for t in (v_max if hasattr(v_max, "__len__") else [v_max])]
        a = [float(t) for t in (a_max if hasattr(a_max, "__len__") else [a_max])]
        S = max(len(v), len(a))
        if len(v) not in (1, S) or len(a) not in (1, S) or S < 1:
            raise ValueError(f"MotionLimits.from_physical: v_max holds {len(v)} scenes, a_max {len(a)}")
        v, a = v * (S // len(v)), a * (S // len(a))
        for name, t in (("v_max", v), ("a_max", a)):
            if not all(q >= 0.0 for q in t):
                raise ValueError(f"MotionLimits.from_physical: {name} must be >= 0 (inf: no limit), got {t}")
        rows = [[v[i] * dt / xy_scale, a[i] * dt * dt / xy_scale] for i in range(S)]
        return MotionLimits(torch.tensor(rows, dtype=torch.float64).to(torch.float32).to(device or "cpu"), w_speed, w_accel)

    def __repr__(self):
        return f"MotionLimits(limits={tuple(self.limits.shape)}, w_speed={self.w_speed}, w_accel={self.w_accel})"


class Route(_Record):
    """The route corridor of "cost guidance v4" (include/adx.h): `points` float32 `[S, R, 2]` = per scene a polyline of R points
    (x, y), 2 <= R <= 32, in the model's own units (the clamped result before xy scaling) and THIS tick's ego frame; segment i
    joins point i and point i + 1, and a scene with fewer points pads by repeating its last one.  `half_width` float32 `[S]`, or a
    number that stands for every scene: a waypoint whose squared distance d2 to the nearest segment exceeds `half_width**2` pays
    `weight * (d2 - half_width**2)**2 / 2` and is pulled straight back toward the polyline; `inf` switches the term off for that
    scene (a NaN does too), `0` means "pull onto the route".  `weight` >= 0; exactly 0 switches the term off everywhere.  The
    squared excess is small in the model's units: a weight that makes the term dimensionless is `1 / w_ref**4` for a typical
    half-width `w_ref` (an excess of w_ref^2 then costs 1/2, like a waypoint on a disc's centre).  The points and widths are read
    at every step: new values need no new object (and, in a GraphedSampler, no new capture); R and the weight are baked.

    With `TrajectorySelector(hard=True)` a candidate that leaves the corridor, by one ulp, is "not free"."""
    ATTR, NOUN, EARLIER, SUFFIX, POINTWISE, TENSORS = "route", "the route", "route", "route", True, ("points", "half_width")

    def __init__(self, points: torch.Tensor, half_width, weight: float = 1.0):
        if not torch.is_tensor(points):
            raise TypeError(f"Route: points must be a tensor, got {type(points).__name__}")
        if points.dim() != 3 or points.shape[2] != 2 or points.shape[0] < 1:
            raise ValueError(f"Route: points must be [S, R, 2] = (x, y) per scene, got {tuple(points.shape)}")
        if not MIN_ROUTE_POINTS <= points.shape[1] <= MAX_ROUTE_POINTS:
            raise ValueError(f"Route: {points.shape[1]} points per scene, supported {MIN_ROUTE_POINTS}..{MAX_ROUTE_POINTS}")
        if points.dtype != torch.float32:
            raise TypeError(f"Route: points must be float32, got {points.dtype}")
        S = int(points.shape[0])
        if not torch.is_tensor(half_width):
            try:
                half_width = torch.full((S,), float(half_width), dtype=torch.float32, device=points.device)
            except (TypeError, ValueError):
                raise TypeError(f"Route: half_width must be a tensor [S] or a number, got {type(half_width).__name__}") from None
        if half_width.dim() != 1 or half_width.shape[0] != S:
            raise ValueError(f"Route: half_width must be [S] = [{S}] (or a number), got {tuple(half_width.shape)}")
        if half_width.dtype != torch.float32:
            raise TypeError(f"Route: half_width must be float32, got {half_width.dtype}")
        if half_width.device != points.device:
            raise ValueError(f"Route: points live on {points.device}, half_width on {half_width.device}")
        weight = float(weight)
        if not weight >= 0.0:
            raise ValueError(f"Route: weight must be >= 0, got {weight}")
        self.points, self.half_width, self.weight = points.contiguous(), half_width.contiguous(), weight

    @property
    def R(self) -> int:
        return int(self.points.shape[1])

    def key(self) -> tuple:
        """What a captured graph bakes: everything but the values of the points and widths."""
        return (self.R, self.weight)

    def like(self, points: torch.Tensor, half_width) -> "Route":
        """The same weight over other points and widths."""
        return Route(points, half_width, self.weight)

    def desc(self, x: torch.Tensor) -> L.RouteDesc:
        """The `adx_guide_route` of a launch on `x` [B, H, D].  The struct holds addresses: keep this object alive until the
        launch is enqueued."""
        self._on_device_of(x)
        r = L.RouteDesc()
        r.points, r.half_width = self.points.data_ptr(), self.half_width.data_ptr()
        r.scene_rows, r.n_points, r.weight = self.points.shape[0], self.points.shape[1], self.weight
        return r

    @staticmethod
    def from_physical(points_m, half_width_m, xy_scale: float, weight: float = 1.0, device=None) -> "Route":
        """A route from metres, on the host: `points_m` [S, R, 2] (a tensor or nested sequences) in metres in this tick's ego
        frame, `half_width_m` a number or a sequence of S numbers (one per scene; a number stands for all), `xy_scale` the metres
        of one model unit (`model.magic_num`).  Each coordinate and width is divided by `xy_scale` in double and rounded to fp32
        once.  `inf` stays `inf`."""
        xy_scale = float(xy_scale)
        if not (math.isfinite(xy_scale) and xy_scale > 0.0):
            raise ValueError(f"Route.from_physical: xy_scale must be finite and > 0, got {xy_scale}")
        pts = torch.as_tensor(points_m).detach().to("cpu", torch.float64)
        if pts.dim() != 3 or pts.shape[2] != 2 or pts.shape[0] < 1:
            raise ValueError(f"Route.from_physical: points_m must be [S, R, 2], got {tuple(pts.shape)}")
        S = int(pts.shape[0])
        w = [float(t) for t in (half_width_m if hasattr(half_width_m, "__len__") else [half_width_m])]
        if len(w) not in (1, S):
            raise ValueError(f"Route.from_physical: points_m hold {S} scenes, half_width_m {len(w)}")
        w = w * (S // len(w))
        if not all(q >= 0.0 for q in w):
            raise ValueError(f"Route.from_physical: half_width_m must be >= 0 (inf: no corridor), got {w}")
        dev = device or "cpu"
        return Route((pts / xy_scale).to(torch.float32).to(dev),
                     (torch.tensor(w, dtype=torch.float64) / xy_scale).to(torch.float32).to(dev), weight)

    def __repr__(self):
        return f"Route(points={tuple(self.points.shape)}, half_width={tuple(self.half_width.shape)}, weight={self.weight})"


class Capsules(_Record):
    """The moving capsules of "cost guidance v5" (include/adx.h): `slots` float32 `[S, C, 7]` = per scene C slots
    `(ax, ay, bx, by, vx, vy, r)`, 1 <= C <= 32, in the model's own units (the clamped result before xy scaling) and THIS tick's
    ego frame: the segment from a to b with radius r, both ends moving by `(vx, vy)` per waypoint.  A waypoint closer than r to
    the moved segment pays `weight * (1 - d2 / r^2)^2 / 2` -- v1's disc potential around the nearest point of the axis -- and is
    pushed straight away from it; a slot with `r <= 0` (or NaN) is empty, so scenes with fewer vehicles pad with zeros, and
    `a == b` is a disc.  `weight` >= 0; exactly 0 switches the term off everywhere.  The slots are read at every step: new values
    need no new object (and, in a GraphedSampler, no new capture); C and the weight are baked.

    `Capsules.from_boxes` makes the slots from oriented boxes in one launch ("capsules from boxes v1"); the capsule is a box's
    INSCRIBED stadium, so its corners stick out by up to `(sqrt(2) - 1) * width / 2`: cover that, and the ego's own radius, with
    `inflate`.  With `TrajectorySelector(hard=True)` a candidate inside a capsule, by one ulp, is "not free"."""
    ATTR, NOUN, EARLIER, SUFFIX, POINTWISE, TENSORS = "capsules", "the capsules", "capsules", "capsule", True, ("slots",)

    def __init__(self, slots: torch.Tensor, weight: float = 1.0):
        if not torch.is_tensor(slots):
            raise TypeError(f"Capsules: slots must be a tensor, got {type(slots).__name__}")
        if slots.dim() != 3 or slots.shape[2] != 7 or slots.shape[0] < 1:
            raise ValueError(f"Capsules: slots must be [S, C, 7] = (ax, ay, bx, by, vx, vy, r) per slot, got {tuple(slots.shape)}")
        if not 1 <= slots.shape[1] <= MAX_CAPSULES:
            raise ValueError(f"Capsules: {slots.shape[1]} slots per scene, supported 1..{MAX_CAPSULES}")
        if slots.dtype != torch.float32:
            raise TypeError(f"Capsules: slots must be float32, got {slots.dtype}")
        weight = float(weight)
        if not weight >= 0.0:
            raise ValueError(f"Capsules: weight must be >= 0, got {weight}")
        self.slots, self.weight = slots.contiguous(), weight

    @property
    def C(self) -> int:
        return int(self.slots.shape[1])

    def key(self) -> tuple:
        """What a captured graph bakes: everything but the values of the slots."""
        return (self.C, self.weight)

    def like(self, slots: torch.Tensor) -> "Capsules":
        """The same weight over other slots."""
        return Capsules(slots, self.weight)

    def desc(self, x: torch.Tensor) -> L.CapsuleDesc:
        """The `adx_guide_capsules` of a launch on `x` [B, H, D].  The struct holds an address: keep this object alive until the
        launch is enqueued."""
        self._on_device_of(x)
        c = L.CapsuleDesc()
        c.capsules, c.scene_rows, c.n_capsules, c.weight = self.slots.data_ptr(), self.slots.shape[0], self.slots.shape[1], self.weight
        return c

    @staticmethod
    def _boxes(t, what: str, last: int) -> None:
        if not torch.is_tensor(t):
            raise TypeError(f"Capsules.from_boxes: {what} must be a tensor, got {type(t).__name__}")
        if t.dim() != 3 or t.shape[2] != last or t.shape[0] < 1:
            raise ValueError(f"Capsules.from_boxes: {what} must be [S, N, {last}], got {tuple(t.shape)}")
        if not 1 <= t.shape[1] <= MAX_CAPSULES:
            raise ValueError(f"Capsules.from_boxes: {t.shape[1]} boxes per scene, supported 1..{MAX_CAPSULES}")
        if t.dtype != torch.float32:
            raise TypeError(f"Capsules.from_boxes: {what} must be float32, got {t.dtype}")

    @staticmethod
    def from_boxes(boxes: torch.Tensor, inflate: float = 0.0, weight: float = 1.0, out: Optional[torch.Tensor] = None) -> "Capsules":
        """Capsules from oriented boxes `boxes` float32 [S, N, 8] = (cx, cy, vx, vy, ux, uy, length, width), one launch of
        `adx_capsules_from_boxes` ("capsules from boxes v1"): `(ux, uy)` is the UNIT heading along `length` (the caller
        normalises it; `boxes_from_physical` does), everything in the model's units.  Box j becomes slot j: the inscribed stadium
        along the longer side with radius `shorter / 2 + inflate`; a box with a size <= 0 or NaN becomes an empty slot.
        `inflate`: finite and >= 0, the ego's own radius (and the corners' overhang).  `out`: slots [S, N, 7] to write (a static
        buffer of a captured graph); None allocates."""
        Capsules._boxes(boxes, "boxes", 8)
        inflate = float(inflate)
        if not (math.isfinite(inflate) and inflate >= 0.0):
            raise ValueError(f"Capsules.from_boxes: inflate must be finite and >= 0, got {inflate}")
        weight = float(weight)
        if not weight >= 0.0:
            raise ValueError(f"Capsules: weight must be >= 0, got {weight}")
        boxes = L.require_gpu_f32(boxes, "boxes").contiguous()
        S, N, _ = boxes.shape
        if out is None:
            out = torch.empty((S, N, 7), dtype=torch.float32, device=boxes.device)
        else:
            Capsules._boxes(out, "out", 7)
            if out.shape[:2] != boxes.shape[:2] or out.device != boxes.device or not out.is_contiguous():
                raise ValueError(f"Capsules.from_boxes: out must be contiguous {(S, N, 7)} on {boxes.device}, got "
                                 f"{tuple(out.shape)} on {out.device}")
        L.check(L.lazy("adx_capsules_from_boxes")(boxes.data_ptr(), out.data_ptr(), S, N, inflate, L.stream_ptr(boxes.device)),
                "adx_capsules_from_boxes")
        return Capsules(out, weight)

    @staticmethod
    def boxes_from_physical(boxes_m, dt: float, xy_scale: float, device=None) -> torch.Tensor:
        """The `[S, N, 8]` device format of `from_boxes` from a detector's boxes, on the host: `boxes_m` [S, N, 7] =
        (cx, cy, vx, vy, yaw, length, width) (a tensor or nested sequences) with positions and sizes in metres in this tick's ego
        frame, speeds in m/s and yaw in radians; `dt` the seconds between two waypoints, `xy_scale` the metres of one model unit
        (`model.magic_num`).  Positions and sizes are divided by `xy_scale`, speeds multiplied by `dt / xy_scale`, the heading is
        `(cos yaw, sin yaw)`; all in double, rounded to fp32 once."""
        dt, xy_scale = float(dt), float(xy_scale)
        if not (math.isfinite(xy_scale) and xy_scale > 0.0):
            raise ValueError(f"Capsules.boxes_from_physical: xy_scale must be finite and > 0, got {xy_scale}")
        if not (math.isfinite(dt) and dt > 0.0):
            raise ValueError(f"Capsules.boxes_from_physical: dt must be finite and > 0, got {dt}")
        # nested sequences of Python floats are doubles: read them as such, not through torch's default float32
        b = boxes_m.detach().to("cpu", torch.float64) if torch.is_tensor(boxes_m) else torch.as_tensor(boxes_m, dtype=torch.float64)
        if b.dim() != 3 or b.shape[2] != 7 or b.shape[0] < 1:
            raise ValueError(f"Capsules.boxes_from_physical: boxes_m must be [S, N, 7] = (cx, cy, vx, vy, yaw, length, width), got "
                             f"{tuple(b.shape)}")
        out = torch.empty(b.shape[:2] + (8,), dtype=torch.float64)
        out[..., 0:2] = b[..., 0:2] / xy_scale
        out[..., 2:4] = b[..., 2:4] * (dt / xy_scale)
        out[..., 4] = torch.cos(b[..., 4])
        out[..., 5] = torch.sin(b[..., 4])
        out[..., 6:8] = b[..., 5:7] / xy_scale
        return out.to(torch.float32).to(device or "cpu")

    def __repr__(self):
        return f"Capsules(slots={tuple(self.slots.shape)}, weight={self.weight})"


RECORDS = (CostField, MotionLimits, Route, Capsules)        # version order: the order of the exports' arguments and suffixes
_records_of = operator.attrgetter(*(kind.ATTR for kind in RECORDS))


class Guide:
    """`discs` float32 `[S, M, 5]` and / or `planes` float32 `[S, P, 3]` on one device (None: no such constraint); `scale`,
    `schedule`, `cap`, `iters` as the module docstring says; `field`: a CostField or None, `motion`: a MotionLimits or None,
    `route`: a Route or None, `capsules`: a Capsules or None (all keyword only; RECORDS holds their classes in this order, and
    everything below that treats the records alike walks it).  The tensors are read at every step: new values need no new object
    (and, in a GraphedSampler, no new capture)."""

    def __init__(self, discs: Optional[torch.Tensor] = None, planes: Optional[torch.Tensor] = None, scale: float = 1.0,
                 schedule: str = "variance", cap: float = float("inf"), iters: int = 1, *, field: Optional[CostField] = None,
                 motion: Optional[MotionLimits] = None, route: Optional[Route] = None, capsules: Optional[Capsules] = None):
        for name, t, last, most in (("discs", discs, 5, MAX_DISCS), ("planes", planes, 3, MAX_PLANES)):
            if t is None:
                continue
            if not torch.is_tensor(t):
                raise TypeError(f"Guide: {name} must be a tensor or None, got {type(t).__name__}")
            if t.dim() != 3 or t.shape[2] != last or t.shape[0] < 1:
                raise ValueError(f"Guide: {name} must be [S, {'M' if last == 5 else 'P'}, {last}], got {tuple(t.shape)}")
            if t.shape[1] > most:
                raise ValueError(f"Guide: at most {most} {name} per scene, got {t.shape[1]}")
            if t.dtype != torch.float32:
                raise TypeError(f"Guide: {name} must be float32, got {t.dtype}")
        if discs is not None and planes is not None:
            if discs.device != planes.device:
                raise ValueError(f"Guide: discs live on {discs.device}, planes on {planes.device}")
            if discs.shape[0] != planes.shape[0]:
                raise ValueError(f"Guide: discs hold {discs.shape[0]} scenes, planes {planes.shape[0]}")
        # each record agrees with everything before it: the discs and planes that hold a constraint, then the earlier records
        earlier = [(name, t) for name, t in (("discs", discs), ("planes", planes)) if t is not None and t.shape[1] > 0]
        for kind, rec in zip(RECORDS, (field, motion, route, capsules)):
            if rec is None:
                continue
            if not isinstance(rec, kind):
                raise TypeError(f"Guide: {kind.ATTR} must be a {kind.__name__} or None, got {type(rec).__name__}")
            for name, t in earlier:
                if t.device != rec.device:
                    raise ValueError(f"Guide: {name} live on {t.device}, {kind.NOUN} on {rec.device}")
                if t.shape[0] != rec.scenes:
                    raise ValueError(f"Guide: {name} hold {t.shape[0]} scenes, {kind.NOUN} {rec.scenes}")
            earlier.append((kind.EARLIER, rec.lead))
        if schedule not in SCHEDULES:
            raise ValueError(f"Guide: schedule must be one of {SCHEDULES}, got {schedule!r}")
        scale, cap = float(scale), float(cap)
        if math.isnan(scale):
            raise ValueError("Guide: scale is NaN")
        if not cap >= 0.0:
            raise ValueError(f"Guide: cap must be >= 0 (inf: no cap), got {cap}")
        if int(iters) != iters or not 1 <= int(iters) <= MAX_ITERS:
            raise ValueError(f"Guide: iters must be an integer in 1..{MAX_ITERS}, got {iters!r}")
        self.discs = None if discs is None else discs.contiguous()
        self.planes = None if planes is None else planes.contiguous()
        self.scale, self.schedule, self.cap, self.iters = scale, schedule, cap, int(iters)
        self.field, self.motion, self.route, self.capsules = field, motion, route, capsules

    # ---- shape ----
    @property
    def M(self) -> int:
        return 0 if self.discs is None else int(self.discs.shape[1])

    @property
    def P(self) -> int:
        return 0 if self.planes is None else int(self.planes.shape[1])

    @property
    def scenes(self) -> Optional[int]:
        """S of the tensors; None for a guide without any (which fits every batch)."""
        t = self._first()
        return None if t is None else int(t.shape[0])

    @property
    def device(self) -> Optional[torch.device]:
        t = self._first()
        return None if t is None else t.device

    def records(self) -> tuple:
        """The records in the order of RECORDS, None where the guide holds none of that kind."""
        return _records_of(self)

    def pointwise(self) -> tuple:
        """The records whose terms name places, in order, None where absent: what `adx_stop_short` takes after the guide."""
        return tuple(r for kind, r in zip(RECORDS, self.records()) if kind.POINTWISE)

    def _held(self) -> tuple:
        """The records up to the last one held: what the key spells out and what the narrowest export that fits takes."""
        records = _records_of(self)
        held = len(records)
        while held and records[held - 1] is None:
            held -= 1
        return records[:held]

    def tensors(self) -> tuple:
        """((name, tensor), ...) of every tensor the guide holds: `discs`, `planes`, then `<attribute>.<name>` per record."""
        own = tuple((name, t) for name, t in (("discs", self.discs), ("planes", self.planes)) if t is not None)
        return own + tuple((f"{r.ATTR}.{name}", t) for r in self.records() if r is not None for name, t in r.tensors())

    def _first(self) -> Optional[torch.Tensor]:
        """The tensor that says how many scenes the guide holds and where: the first of `tensors()`."""
        if self.discs is not None:
            return self.discs
        if self.planes is not None:
            return self.planes
        return next((r.lead for r in self.records() if r is not None), None)

    def key(self) -> tuple:
        """What a captured graph bakes: everything but the values of the tensors.  The 6-tuple of cost guidance v1, then the keys
        of the records up to the last one held, None for an absent one in between: a guide keeps the key it had before the
        kinds of record it does not hold existed."""
        return ((self.M, self.P, self.scale, self.schedule, self.cap, self.iters) +
                tuple(None if r is None else r.key() for r in self._held()))

    def like(self, discs: Optional[torch.Tensor], planes: Optional[torch.Tensor], field: Optional[CostField] = None,
             motion: Optional[MotionLimits] = None, route: Optional[Route] = None, capsules: Optional[Capsules] = None) -> "Guide":
        """The same settings over other tensors."""
        return Guide(discs, planes, self.scale, self.schedule, self.cap, self.iters, field=field, motion=motion, route=route,
                     capsules=capsules)

    def clone(self) -> "Guide":
        """The same guide over clones of its tensors: the static buffers of a captured graph."""
        return self.like(None if self.discs is None else self.discs.clone(), None if self.planes is None else self.planes.clone(),
                         *(None if r is None else r.clone() for r in self.records()))

    def copy_(self, src: "Guide") -> "Guide":
        """The values of `src`, a guide of the same key and shapes, copied into this one's tensors.  Tensors meet by name, and one
        without elements is skipped: of two guides with equal keys one may hold `discs=None` and the other an empty [S, 0, 5]."""
        if src.key() != self.key():
            raise ValueError(f"Guide.copy_: the keys differ, {src.key()} into {self.key()}")
        mine = dict(self.tensors())
        for name, t in src.tensors():
            if t.numel() > 0:
                mine[name].copy_(t)
        return self

    # ---- launches ----
    def desc(self, x: torch.Tensor, lam: float = 0.0) -> L.GuideDesc:
        """The `adx_guide` of a launch on `x` [B, H, D] with lambda = `lam` (a scheduler's `guide_level`).  The struct holds
        addresses: keep this object alive until the launch is enqueued."""
        first, dev = self._first(), x.device        # `self.scenes` without the property's hop: this runs on every step of an eager tick
        S = None if first is None else int(first.shape[0])
        for name, t in (("guide.discs", self.discs), ("guide.planes", self.planes)):
            if t is not None and (L.require_gpu_f32(t, name).device != dev):
                raise ValueError(f"{name} lives on {t.device}, the sample on {dev}")
        if x.dim() != 3 or x.shape[2] < 2 or (S is not None and x.shape[0] % S != 0):
            raise ValueError(f"the guide holds {S} scenes; the sample is {tuple(x.shape)}: [B, H, D] with D >= 2 and rows a multiple "
                             "of the guide's scenes")
        g = L.GuideDesc()
        g.discs, g.planes = L.ptr(self.discs), L.ptr(self.planes)
        t = self.discs if self.discs is not None else self.planes
        g.scene_rows, g.n_discs, g.n_planes = 1 if t is None else int(t.shape[0]), self.M, self.P
        g.iters, g.lambda_, g.cap = self.iters, float(lam), self.cap
        return g

    def field_desc(self, x: torch.Tensor) -> Optional[L.FieldDesc]:
        """The `adx_guide_field` of a launch on `x`, or None for a guide without a field."""
        return None if self.field is None else self.field.desc(x)

    def motion_desc(self, x: torch.Tensor) -> Optional[L.MotionDesc]:
        """The `adx_guide_motion` of a launch on `x`, or None for a guide without motion limits."""
        return None if self.motion is None else self.motion.desc(x)

    def route_desc(self, x: torch.Tensor) -> Optional[L.RouteDesc]:
        """The `adx_guide_route` of a launch on `x`, or None for a guide without a route."""
        return None if self.route is None else self.route.desc(x)

    def capsule_desc(self, x: torch.Tensor) -> Optional[L.CapsuleDesc]:
        """The `adx_guide_capsules` of a launch on `x`, or None for a guide without capsules."""
        return None if self.capsules is None else self.capsules.desc(x)

    def descs(self, x: torch.Tensor, lam: float = 0.0):
        """`(export suffix, byref arguments, the structs)` of a guided launch on `x`: the narrowest export that fits.  The suffix
        is the SUFFIX of the last record held ("guide" with none); the arguments are what that export takes after the pin, in
        its order: the `adx_guide`, then the records up to that one, None for an absent one.  Keep the structs alive until the
        launch is enqueued."""
        g, held, byref = self.desc(x, lam), self._held(), C.byref
        structs, refs = [g], [byref(g)]
        for r in held:                      # this runs on every step of an eager tick: one plain loop
            s = None if r is None else r.desc(x)
            structs.append(s)
            refs.append(None if s is None else byref(s))
        return held[-1].SUFFIX if held else "guide", tuple(refs), tuple(structs)

    def cost(self, traj: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """What a plan still violates, one launch of `adx_guide_cost`: `(cost [rows] float32, active [rows] int32)` of `traj`
        [rows, H, D] -- the contract's cost summed over a row's waypoints and the number of active (waypoint, constraint) pairs.
        `traj` is in the MODEL's units: a result before xy scaling (`scale_xy=False`, `warm.prev`), row r against scene r % S."""
        traj = L.require_gpu_f32(traj, "traj")
        suffix, refs, _alive = self.descs(traj)
        rows, H, D = traj.shape
        cost = torch.empty(rows, dtype=torch.float32, device=traj.device)
        active = torch.empty(rows, dtype=torch.int32, device=traj.device)
        name = "adx_guide_cost" + ("" if suffix == "guide" else "_" + suffix)
        L.check(L.lazy(name)(traj.data_ptr(), *refs, cost.data_ptr(), active.data_ptr(), rows, H, D, L.stream_ptr(traj.device)), name)
        return cost, active

    def __repr__(self):
        return ", ".join([f"Guide(discs={None if self.discs is None else tuple(self.discs.shape)}, "
                          f"planes={None if self.planes is None else tuple(self.planes.shape)}, scale={self.scale}, "
                          f"schedule={self.schedule!r}, cap={self.cap}, iters={self.iters}"] +
                         [f"{r.ATTR}={r!r}" for r in self.records() if r is not None]) + ")"
