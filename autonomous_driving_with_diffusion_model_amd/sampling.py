"""The callers' sampling loops, restated over the drop-in model/scheduler objects.

`generate_traj` mirrors `interact.Agent.generate_traj` (interact.py:115-168) ==
`DiffusionAgent.generate_traj` (e2e_driving/diffusion_agent.py:179-232); `evaluate_sample` mirrors
the loop of `train.evaluate` (train.py:62-90).  They exist so that parity tests and the benchmark can
drive the exact call sequence the reference's callers issue: model.forward + scheduler.step per
timestep, `trajs[:, 0, :3] = 0` before the loop and after every step, final clamp and xy scaling.

Differences from the callers, both optional and numerically identical:
  * `target` may be [B, 2] (one goal per scene) instead of one [2] goal repeated over the batch;
  * `fuse=True` folds the classifier-free combine and the `[:, 0, :3] = 0` write into the scheduler's
    step kernel instead of issuing them as separate torch ops.
A third option changes WHICH noise a stochastic sampler sees, not the arithmetic: `noise=DeviceNoise(...)` draws the initial
trajectory and every step's noise from the counter-based stream of noise.py inside the step kernel, where the callers draw
`torch.randn` tensors -- the same loop then also runs as one HIP graph (`GraphedSampler(..., noise=...)`).
A fourth has no counterpart in the callers: `candidates=K` draws K trajectories per scene in one loop of K * S rows (the encoder
still runs once per scene) and keeps the one a device-side cost prefers (control/select.py, "selection cost v1" of include/adx.h).
A fifth has none either: `warm=WarmStart(steps=m)` starts a tick from the previous tick's result -- advanced, re-based, clamped
and re-noised on the device ("warm start v1" of include/adx.h) -- and runs only the last m steps of the schedule.
A sixth closes the tick: `controller=DeviceController(...)` turns the result into (throttle, steer, brake) per scene on the device
("control v1" of include/adx.h, control/device.py), where the callers hand `traj[0, :4, :2]` to a host `Controller`.
A seventh makes the loop's one hard-coded constraint general: `pin=Pin(known, mask)` holds waypoints the caller has already
decided through the tick, inside the step kernels ("pinned waypoints v1" of include/adx.h, pin.py), where the callers can only
say `trajs[:, 0, :3] = 0`.
An eighth says where NOT to go: `guide=Guide(discs, planes, ...)` bends every step's predicted clean trajectory away from the
caller's obstacles, inside the step kernels ("cost guidance v1" of include/adx.h, guide.py).
The fourth and the eighth meet in the selector: one with `w_guide` or `hard` (`TrajectorySelector.uses_guide`) is handed the
tick's guide and scores every candidate against the obstacles in the select launch itself ("selection cost v2" of include/adx.h):
with `hard` a candidate that violates nothing beats every candidate that violates something, and `Selection.blocked` says per scene
whether the chosen plan is still blocked.  A plain selector on a guided tick runs as it always did.
A ninth reads the scene as a perception stack draws it: `guide=Guide(..., field=CostField(cells, origin, cell))` adds a cost raster
to the guide ("cost guidance v2" of include/adx.h), read bilinearly at every waypoint by the same routine of the same kernels, so
the steps, `Guide.cost`, the guided selector, the warm state, the controller and the graph all see it;
`CostField.from_occupancy` makes the raster from an occupancy grid in one launch ("cost field from occupancy v1").
A tenth says how fast to go: `guide=Guide(..., motion=MotionLimits(limits))` caps the length of a segment and of a second difference
per scene ("cost guidance v3"); every step then runs the row-wise step kernel, one wave per row.
An eleventh says where the road is: `guide=Guide(..., route=Route(points, half_width))` keeps the plan within a half-width of a
per-scene polyline ("cost guidance v4"), a point-wise term of the same routine, so it runs in whichever step kernel the rest picks.
A twelfth says where the other vehicles are: `guide=Guide(..., capsules=Capsules(slots))` steers around per-scene moving capsules
("cost guidance v5"), point-wise like the route; `Capsules.from_boxes` makes them from oriented boxes in one capturable launch.
A thirteenth is the last resort when the plan a tick ends with still runs into something: `fallback=StopShort(params)` keeps its
path and re-times it to brake to a halt before its first conflict with the guide ("stop-short fallback v1", control/fallback.py),
one launch between selection and control; the controller and the caller get the re-timed plan, the warm state the sampler's own.
A fourteenth says what the K candidates contain: `modes=TrajectoryModes(...)` clusters them per scene into the manoeuvres they
stand for and counts the sample mass behind each ("trajectory modes v1", control/modes.py), one launch directly after selection
that alters nothing the tick returns; the result is left in `modes.last`.
A fifteenth keeps the plan from flickering between two manoeuvres of nearly equal cost: `commit=ManoeuvreCommit(...)` holds the
manoeuvre the previous tick chose unless the selector's new choice is clearly better ("manoeuvre commitment v1",
control/commit.py), one launch directly after selection whose state lives on the device; everything after it -- the warm state,
the fallback, the controller, the caller -- follows the committed plan, the selector's own choice stays in `commit.selected`.
A sixteenth supplies what the callers compute on the host before every tick: `navigator=Navigator(...)` with `pose=` walks the
global plan, rotates the next waypoint into the ego frame and derives the odometry in one launch in front of the tick ("route
planner v1", navigation.py), and the tick reads `navigator.target` and `navigator.motion`.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Callable, Optional, Tuple

import torch

from . import _lib as L
from ._lib import AdxRangeError
from .control.device import DeviceController
from .control.fallback import MAX_HORIZON as FALLBACK_MAX_HORIZON, NO_POINTWISE_TERM, StopResult, StopShort, pointwise
from .control.commit import MAX_HORIZON as COMMIT_MAX_HORIZON, CommitResult, ManoeuvreCommit
from .control.modes import MAX_HORIZON as MODES_MAX_HORIZON, ModeSet, TrajectoryModes
from .control.select import MAX_CANDIDATES, Selection, TrajectorySelector
from .misc.constant import GuidanceType
from .noise import DeviceNoise
from .guide import Guide
from .navigation import Navigator
from .pin import Pin, pin_apply


def _targets(target: Optional[torch.Tensor], batch: int) -> Optional[torch.Tensor]:
    if target is None:
        return None
    t = target.reshape(-1, 2)
    if t.shape[0] == 1:
        t = t.repeat(batch, 1)   # interact.py:120
    if t.shape[0] != batch:
        raise ValueError(f"target must be [2] or [{batch}, 2], got {tuple(target.shape)}")
    return t.contiguous()


class WarmStart:
    """Receding-horizon warm starting: the state one agent carries from tick to tick.

    `steps` = m: a warm tick runs the last m of the EVAL.SAMPLE_STEPS = n steps, from the previous result noised to the level
    of `timesteps[n - m]`; `shift`: the waypoints the vehicle passed between two ticks.  Left at None they read EVAL.WARM_STEPS
    (0 = off: every tick is cold and this object is never touched) and EVAL.WARM_SHIFT (1).  `prev` is the static [S, H, D]
    buffer of the last result in the model's own units (clamped, before xy scaling; the winners at K > 1), allocated on first
    use and never re-allocated -- captured graphs read and write it; `valid` says on the host whether it holds one.  `reset()`
    makes the next tick cold: call it after a scene cut or a teleport.  How good a plan m steps give is a property of the
    trained weights and is not measured in this repository."""

    def __init__(self, steps: Optional[int] = None, shift: Optional[int] = None):
        self.steps, self.shift = steps, shift
        self.prev: Optional[torch.Tensor] = None
        self.valid = False

    def reset(self) -> None:
        self.valid = False

    def resolve(self, cfg) -> Tuple[int, int]:
        m = int(getattr(cfg.EVAL, "WARM_STEPS", 0) if self.steps is None else self.steps)
        shift = int(getattr(cfg.EVAL, "WARM_SHIFT", 1) if self.shift is None else self.shift)
        if m < 0:
            raise ValueError(f"WarmStart: steps must be >= 0, got {m}")
        return m, shift

    def _store(self, result: torch.Tensor) -> None:
        if self.prev is None:
            self.prev = torch.empty_like(result)
        self.prev.copy_(result)
        self.valid = True

    def __repr__(self):
        shape = None if self.prev is None else tuple(self.prev.shape)
        return f"WarmStart(steps={self.steps}, shift={self.shift}, valid={self.valid}, prev={shape})"


def warm_init(prev: torch.Tensor, rows: int, shift: int, level: Tuple[float, float], noise: DeviceNoise,
              motion: Optional[torch.Tensor] = None, zero_first: bool = True) -> torch.Tensor:
    """One launch of `adx_warm_init` ("warm start v1", include/adx.h): [rows, H, D] from prev [prev_rows, H, D] under the
    stream's current tick; `level` = `scheduler.noise_level(tau)`; row r draws logical row `noise.row_offset + r`."""
    prev = L.require_gpu_f32(prev, "prev")
    if prev.dim() != 3:
        raise ValueError(f"prev must be [rows, H, D], got {tuple(prev.shape)}")
    if motion is not None:
        motion = L.require_gpu_f32(motion, "motion")
        if tuple(motion.shape) != (prev.shape[0], 3):
            raise ValueError(f"motion must be [{prev.shape[0]}, 3], got {tuple(motion.shape)}")
    P, H, D = prev.shape
    out = torch.empty((int(rows), H, D), dtype=torch.float32, device=prev.device)
    L.check(L.lib().adx_warm_init(prev.data_ptr(), P, L.ptr(motion), out.data_ptr(), int(rows), H, D, int(shift), float(level[0]),
                                  float(level[1]), noise.state_ptr(), noise.row_offset, int(bool(zero_first)),
                                  L.stream_ptr(prev.device)), "adx_warm_init")
    return out


@dataclass(frozen=True, eq=False)
class TickPlan:
    """Every decision of one sampling tick, made once by `plan_tick` and only read afterwards: by `generate_traj`, which runs it,
    and by `GraphedSampler`, which keys its captured graphs on `key()`.  Each field says how a captured graph sees it: "baked"
    (a host value that becomes part of a graph node: it belongs in `key()`), "buffer" (a tensor whose values travel through a
    static buffer: new values replay, they never capture again) or "derived" (a function of baked fields alone)."""
    # ---- shapes ----
    S: int                  # baked.  Scenes = image.shape[0]
    # baked.  Candidates per scene: the argument, or EVAL.CANDIDATES when it is left at 1 (absent key: 1).  K > 1 is best-of-K
    # sampling: the loop runs on K * S rows in candidate-major order (candidate k of scene s is row k * S + s and draws logical row
    # k * S + s of the noise stream), the targets are tiled K times, the conditioning table keeps the image batch at S (the encoder
    # runs once per scene) and after the final clamp `selector` picks the [S, H, D] winners.  Needs `hoisted` and an unsharded noise
    K: int
    # baked (its weights, and `hard`).  At K > 1: the argument, or TrajectorySelector(*EVAL.SELECT) -- 3, 4 or 5 values: w_goal,
    # w_smooth, w_consensus[, w_guide[, hard]].  One with `uses_guide` is called with the tick's `guide` (whose static buffers a
    # graph's select node then reads: new obstacle values replay); any other is called without, guide or no guide
    selector: Optional[TrajectorySelector]
    rows: int               # baked.  Rows of the loop: init_trajs.shape[0] when init_trajs is given, else K * S
    H: int                  # baked.  MODEL.HORIZON
    D: int                  # baked.  MODEL.TRANSITION_DIM
    # ---- guidance and loop switches ----
    n: int                  # baked.  EVAL.SAMPLE_STEPS
    use: GuidanceType       # baked.  GUIDANCE.USE_COND
    free_scale: Optional[float]    # baked.  GUIDANCE.FREE_SCALE under FREE_GUIDANCE, else None
    fuse: bool              # baked.  The classifier-free combine and `[:, 0, :3] = 0` run inside the step kernel
    # baked.  What the UNet derives from (t, target, image feature) alone does not change inside the loop: with the perception memo
    # on (the product default) it is computed for all timesteps in one pass, and each step then starts at the first convolution.
    # The reference-faithful mode (cache_perception = False) keeps the reference's per-step recomputation
    hoisted: bool
    table_rows: int         # derived.  Rows of the conditioning table: `rows`, twice that under FREE_GUIDANCE
    is_ddpm: bool           # baked.  The step takes an injected `variance_noise`: the DDPM schedulers (a deterministic solver has none)
    pair_identity: bool     # derived.  One row and a table: the table's rows make the classifier-free pair, not a cat
    # ---- the noise of the tick ----
    # by address.  The call is one tick of the stream: every step draws inside its kernel at the slot of its timestep -- no noise
    # tensor, no torch generator -- and a graph node reads the stream's state through its pointer
    noise: Optional[DeviceNoise]
    step_noise: Optional[Callable[[int, tuple], torch.Tensor]]     # eager only.  Injected tensors for the DDPM steps
    # ---- how the tick starts ----
    # baked.  "warm": `adx_warm_init` from warm.prev; "init": a clone of init_trajs; "stream": the noise stream's INIT_SLOT draw;
    # "randn": torch.randn (a GraphedSampler draws it outside the graph and hands it in as init_trajs: "init" to a graph)
    start: str
    # ---- warm start ----
    # baked.  m > 0: the tick ends by copying the clamped, unscaled [S, H, D] result (the winners at K > 1) into warm.prev.
    # 0: no `warm`, or one that is off -- the loop as it was
    m_warm: int
    shift: int              # baked.  Waypoints the vehicle passed between two ticks
    # baked.  warm.valid, as the plan found it.  A warm tick builds its `rows` start rows from warm.prev (row r from scene r % S) and
    # `motion` at the noise level of timesteps[i0], sets the scheduler's begin index to i0 and runs timesteps[i0:] only; clamp,
    # selection, scaling and the copy into warm.prev follow as on a cold tick
    is_warm: bool
    motion: Optional[torch.Tensor]    # buffer; whether it is there is baked.  [S, 3] = (tx, ty, phi) per scene, on a warm tick only
    i0: int                 # derived.  n - m_warm on a warm tick, else 0
    # ---- controller ----
    # baked (identity, state address, every setting).  The tick ends with one launch of `controller.step` on the clamped, unscaled
    # [S, H, D] result (the winners at K > 1) with xy_scale = model.magic_num and the scenes' targets ([S, 2] in the model's units;
    # None: the waypoint after the controller's last stands in)
    controller: Optional[DeviceController]
    velocity: Optional[torch.Tensor]  # buffer; whether it is there is baked.  [S], the scenes' current speeds
    # ---- pin ----
    # known and mask: buffers; presence, mode and shape: baked.  The pin with its mode resolved.  Every `scheduler.step` of the loop
    # gets it (fused or not, all three guidance branches) and blends inside its kernel; the K * S rows read the [S, H, D] pin
    # directly (row r reads scene r % S), nothing is tiled.  Cells with mask 1 equal `known` in the result wherever |known| <= 1,
    # outside `[:, 0, :3]`
    pin: Optional[Pin]
    # derived.  `clean` mode also blends the start rows once at loop entry (`adx_pin_apply` -- on the cold draw, init_trajs or a warm
    # start's output -- between two writes of `[:, 0, :3] = 0`); `repaint` mode has no entry blend, its first step is the entry
    entry_blend: bool
    # ---- guide ----
    # discs and planes: buffers; presence, M, P, scale, schedule, cap and iters: baked (lambda, which scale and schedule give per
    # timestep, is a by-value argument of every step node).  Every `scheduler.step` of the loop gets it (fused or not, all three
    # guidance branches) and moves its x0 inside its kernel; the K * S rows read the [S, ..] obstacles directly (row r reads scene
    # r % S), nothing is tiled.  A guide's records (guide.py, RECORDS) travel the same way: their tensors (`Guide.tensors()`) are
    # buffers; presence and what each record's `key()` holds are baked (by-value arguments of every step node), through `Guide.key()`
    guide: Optional[Guide]
    # ---- modes ----
    # baked (max_modes, radius, h0: by-value arguments of the node).  At K > 1, directly after selection: one launch of
    # `modes(trajs, S)` on the clamped, unscaled K * S candidates.  It reads them and writes buffers of its own: nothing the tick
    # returns changes.  The ModeSet is left in `modes.last`, in model units whatever `scale_xy` says
    modes: Optional[TrajectoryModes] = None
    # ---- commit ----
    # baked (every setting and the state's address: `commit.key()`, and the resolved `commit_shift`); the state itself is read and
    # advanced through its address.  At K > 1, directly after selection and before the modes: one launch of `commit(trajs, S, sel,
    # commit_motion, commit_shift)` on the clamped, unscaled K * S candidates.  Past it `best`, `Selection.index` and
    # `Selection.blocked` are the committed ones: warm.prev, the fallback, the controller and the caller all follow the plan the
    # vehicle follows.  The CommitResult without `best` is left in `commit.last`; the selector's own index is kept as
    # `commit.selected` (it differs from the committed `commit.last.index` exactly where `commit.last.status` is HELD)
    commit: Optional[ManoeuvreCommit] = None
    commit_shift: int = 0   # baked.  commit.shift, or EVAL.WARM_SHIFT (1) where that is None
    # buffer; whether it is there is baked.  The tick's `motion` as given, on every tick (`motion` above is None on a cold one)
    commit_motion: Optional[torch.Tensor] = None
    # ---- fallback ----
    # params: a buffer; presence: baked.  After selection and the copy into warm.prev, one launch of `fallback(best, guide)`
    # re-times the [S, H, D] result (the winners at K > 1) in place, against the tick's guide and before the control launch: the
    # controller and the caller get the re-timed plan, warm.prev keeps the sampler's own winner (a warm start from a stopped plan
    # would teach the next tick to stop).  Needs a guide with a point-wise term, H <= 64, D >= 2 and no `source="action"` controller
    fallback: Optional[StopShort] = None

    def key(self) -> tuple:
        """Everything baked, as a hashable: two plans with equal keys capture the same graph over the same shapes.  A plan without
        a fallback keeps the key it had, and so does one without modes and one without a commit."""
        sel, ctl, pin, guide = self.selector, self.controller, self.pin, self.guide
        weights = None if sel is None else (sel.w_goal, sel.w_smooth, sel.w_consensus)
        if sel is not None and sel.uses_guide:
            weights += (sel.w_guide, sel.hard)
        key = (self.S, self.K, weights, self.rows, self.H, self.D,
               self.n, self.use, self.free_scale, self.fuse, self.hoisted, self.is_ddpm,
               "init" if self.start == "randn" else self.start,
               self.m_warm, self.shift, self.is_warm, self.motion is None,
               None if ctl is None else (id(ctl), ctl.state.data_ptr(), ctl.key(), self.velocity is None),
               None if pin is None else (pin.mode, tuple(pin.known.shape)), None if guide is None else guide.key())
        key = key if self.fallback is None else key + (self.fallback.key(),)
        key = key if self.modes is None else key + (self.modes.key(),)
        return key if self.commit is None else key + ((self.commit.key(), self.commit_shift, self.commit_motion is None),)


def _hoists(model) -> bool:
    return bool(getattr(model, "cache_perception", False)) and hasattr(model, "time_conditioning")


def _pin_plan(cfg, pin: Optional[Pin], image, scheduler, noise, step_noise=None, graphed: bool = False) -> Optional[Pin]:
    """The pin section of `plan_tick`: the pin with its mode resolved (None without one), or a refusal."""
    if pin is None:
        return None
    want = (int(image.shape[0]), int(cfg.MODEL.HORIZON), int(cfg.MODEL.TRANSITION_DIM))
    if not isinstance(pin, Pin):
        raise TypeError(f"generate_traj: `pin` must be a Pin, got {type(pin).__name__}")
    for name, t in (("known", pin.known), ("mask", pin.mask)):
        if tuple(t.shape) != want or t.device != image.device or t.dtype != torch.float32:
            raise ValueError(f"pin.{name} must be a float32 tensor {want} = (scenes, MODEL.HORIZON, MODEL.TRANSITION_DIM) on "
                             f"{image.device}, got {tuple(t.shape)}, {t.dtype} on {t.device}")
    pin = pin.with_mode(pin.resolve(cfg))          # refuses an unknown EVAL.PIN_MODE
    if not getattr(scheduler, "supports_pin", False):
        raise ValueError(f"{type(scheduler).__name__}.step takes no pin: use GuidanceDDIMScheduler, GuidanceDDPMScheduler or "
                         "GuidanceDPMSolverMultistepScheduler")
    if pin.mode == "repaint":
        if step_noise is not None:
            raise ValueError("generate_traj: a `repaint` pin shares each step's own noise; `step_noise` injects tensors for the "
                             "DDPM steps alone -- use noise=DeviceNoise(...) or a `clean` pin")
        if getattr(scheduler, "deterministic", False) and not isinstance(noise, DeviceNoise):
            raise ValueError("generate_traj: a `repaint` pin on the DPM-Solver++ sampler needs noise=DeviceNoise(...): the solver "
                             "has no noise of its own, the pin's is drawn inside the step kernel")
        if graphed and noise is None:
            raise ValueError("GraphedSampler: a `repaint` pin needs noise=DeviceNoise(...) at construction: a noise tensor drawn "
                             "during the capture would replay on every tick")
    return pin


def _guide_plan(cfg, guide: Optional[Guide], image, scheduler) -> Optional[Guide]:
    """The guide section of `plan_tick`: the guide (None without one), or a refusal."""
    if guide is None:
        return None
    if not isinstance(guide, Guide):
        raise TypeError(f"generate_traj: `guide` must be a Guide, got {type(guide).__name__}")
    S = int(image.shape[0])
    for name, t in guide.tensors():
        if int(t.shape[0]) != S or t.device != image.device:
            raise ValueError(f"guide.{name} must hold {S} scenes (image.shape[0]) on {image.device}, got {tuple(t.shape)} on {t.device}")
    if int(cfg.MODEL.TRANSITION_DIM) < 2:
        raise ValueError(f"generate_traj: a guide moves (x, y) and needs MODEL.TRANSITION_DIM >= 2, got {int(cfg.MODEL.TRANSITION_DIM)}")
    if guide.motion is not None and int(cfg.MODEL.HORIZON) > 64:
        raise ValueError(f"generate_traj: motion limits give a row to a wave and need MODEL.HORIZON <= 64, got {int(cfg.MODEL.HORIZON)}")
    if not getattr(scheduler, "supports_guide", False):
        raise ValueError(f"{type(scheduler).__name__}.step takes no guide: use GuidanceDDIMScheduler, GuidanceDDPMScheduler or "
                         "GuidanceDPMSolverMultistepScheduler")
    return guide


def _fallback_plan(cfg, fallback: Optional[StopShort], guide: Optional[Guide], controller: Optional[DeviceController],
                   image) -> Optional[StopShort]:
    """The fallback section of `plan_tick`: the fallback (None without one), or a refusal."""
    if fallback is None:
        return None
    if not isinstance(fallback, StopShort):
        raise TypeError(f"generate_traj: `fallback` must be a StopShort, got {type(fallback).__name__}")
    if guide is None:
        raise ValueError("generate_traj: a fallback re-times the plan against a guide; pass guide=Guide(...) for the tick")
    if not pointwise(guide):
        raise ValueError(NO_POINTWISE_TERM)
    H, D, S = int(cfg.MODEL.HORIZON), int(cfg.MODEL.TRANSITION_DIM), int(image.shape[0])
    if H > FALLBACK_MAX_HORIZON:
        raise ValueError(f"generate_traj: a fallback gives a row to a wave and needs MODEL.HORIZON <= {FALLBACK_MAX_HORIZON}, got {H}")
    if D < 2:
        raise ValueError(f"generate_traj: a fallback re-times (x, y) and needs MODEL.TRANSITION_DIM >= 2, got {D}")
    if fallback.scenes != S or fallback.device != image.device:
        raise ValueError(f"fallback.params must hold {S} scenes (image.shape[0]) on {image.device}, got "
                         f"{tuple(fallback.params.shape)} on {fallback.device}")
    if controller is not None and controller.source == "action":
        raise ValueError("generate_traj: a controller with source='action' reads the model's action columns and would not see a "
                         "re-timing; use source='pid' with a fallback")
    return fallback


def _modes_plan(cfg, modes: Optional[TrajectoryModes], K: int) -> Optional[TrajectoryModes]:
    """The modes section of `plan_tick`: the modes (None without them), or a refusal."""
    if modes is None:
        return None
    if not isinstance(modes, TrajectoryModes):
        raise TypeError(f"generate_traj: `modes` must be a TrajectoryModes, got {type(modes).__name__}")
    if K == 1:
        raise ValueError("generate_traj: `modes` clusters a scene's candidates and needs candidates > 1 (or EVAL.CANDIDATES > 1)")
    H = int(cfg.MODEL.HORIZON)
    if H > MODES_MAX_HORIZON:
        raise ValueError(f"generate_traj: modes stage a scene's candidates in LDS and need MODEL.HORIZON <= {MODES_MAX_HORIZON}, got {H}")
    if modes.h0 > H - 1:
        raise ValueError(f"generate_traj: modes.h0 = {modes.h0} leaves no waypoint of MODEL.HORIZON = {H} to score")
    return modes


def _commit_plan(cfg, commit: Optional[ManoeuvreCommit], K: int, image) -> Tuple[Optional[ManoeuvreCommit], int]:
    """The commit section of `plan_tick`: (the commit, its resolved shift) -- (None, 0) without one --, or a refusal."""
    if commit is None:
        return None, 0
    if not isinstance(commit, ManoeuvreCommit):
        raise TypeError(f"generate_traj: `commit` must be a ManoeuvreCommit, got {type(commit).__name__}")
    if K == 1:
        raise ValueError("generate_traj: `commit` chooses among a scene's candidates and needs candidates > 1 (or EVAL.CANDIDATES > 1)")
    H, S = int(cfg.MODEL.HORIZON), int(image.shape[0])
    if H > COMMIT_MAX_HORIZON:
        raise ValueError(f"generate_traj: a commit stages a scene's candidates in LDS and needs MODEL.HORIZON <= {COMMIT_MAX_HORIZON}, "
                         f"got {H}")
    if commit.scenes != S:
        raise ValueError(f"the ManoeuvreCommit holds the state of {commit.scenes} scenes, this tick has {S} (image.shape[0]); use a "
                         "commit of its own for another batch")
    if commit.horizon != H:
        raise ValueError(f"the ManoeuvreCommit holds plans of {commit.horizon} waypoints, MODEL.HORIZON is {H}")
    if commit.device != image.device:
        raise ValueError(f"the ManoeuvreCommit lives on {commit.device}, the image on {image.device}")
    shift = commit.resolve_shift(cfg)
    if not 0 <= shift <= H - 1:
        raise ValueError(f"ManoeuvreCommit: shift = {shift} must be in 0..{H - 1} (MODEL.HORIZON = {H})")
    return commit, shift


def plan_tick(model, scheduler, cfg, image: torch.Tensor, target: Optional[torch.Tensor] = None,
              init_trajs: Optional[torch.Tensor] = None, *, fuse: bool = True, set_timesteps: bool = True,
              noise: Optional[DeviceNoise] = None, step_noise=None, candidates: int = 1,
              selector: Optional[TrajectorySelector] = None, warm: Optional[WarmStart] = None,
              motion: Optional[torch.Tensor] = None, controller: Optional[DeviceController] = None,
              velocity: Optional[torch.Tensor] = None, pin: Optional[Pin] = None, guide: Optional[Guide] = None,
              fallback: Optional[StopShort] = None, graphed: bool = False, modes: Optional[TrajectoryModes] = None,
              commit: Optional[ManoeuvreCommit] = None) -> TickPlan:
    """The TickPlan of a `generate_traj` call with these arguments (`graphed`: of a GraphedSampler call).  Pure: no launch, no device
    allocation (but one: a strided `motion` is packed, as it always was), no tick of the noise stream, nothing written to the
    scheduler, `warm` or the controller -- so every refusal comes before any of those and before a capture opens, in the order
    candidates, `noise` / `step_noise`, warm, control, pin, guide, a selector that needs a guide, fallback, modes, commit.  `scheduler` is read for
    a warm tick on the caller's own timesteps (`set_timesteps=False`), for a pin and for a guide; `is_ddpm` asks it with defaults."""
    use = GuidanceType[cfg.GUIDANCE.USE_COND]
    S, device = int(image.shape[0]), image.device
    hoisted = bool(fuse) and _hoists(model)
    # ---- candidates: the keyword arguments left at their defaults read EVAL.CANDIDATES / EVAL.SELECT ----
    K = int(candidates) if int(candidates) != 1 else int(getattr(cfg.EVAL, "CANDIDATES", 1))
    if not 1 <= K <= MAX_CANDIDATES:
        raise ValueError(f"candidates must be 1..{MAX_CANDIDATES}, got {K}")
    if K > 1:
        if selector is None:
            select = tuple(getattr(cfg.EVAL, "SELECT", (1.0, 0.0, 0.0)))
            if not 3 <= len(select) <= 5:
                raise ValueError("EVAL.SELECT holds 3, 4 or 5 values (w_goal, w_smooth, w_consensus[, w_guide[, hard]]), got "
                                 f"{len(select)}")
            selector = TrajectorySelector(*select)
        if not hoisted:
            raise ValueError("generate_traj: candidates > 1 needs the hoisted conditioning path: fuse=True and "
                             "model.cache_perception on (the per-step path would run the encoder on K * S rows)")
        if noise is not None and noise.row_offset > 0:
            raise ValueError("generate_traj: candidates > 1 does not take a sharded DeviceNoise (row_offset "
                             f"{noise.row_offset}): scene sharding and candidate-major rows do not compose")
        if init_trajs is not None and init_trajs.shape[0] != K * S:
            raise ValueError(f"init_trajs must have candidates * scenes = {K * S} rows, got {tuple(init_trajs.shape)}")
    if noise is not None and step_noise is not None:
        raise ValueError("generate_traj: pass `noise` (the in-kernel stream) or `step_noise` (injected tensors), not both")
    n, H, D = int(cfg.EVAL.SAMPLE_STEPS), int(cfg.MODEL.HORIZON), int(cfg.MODEL.TRANSITION_DIM)
    # ---- warm ----
    if motion is not None:
        if warm is None and commit is None:
            raise ValueError("generate_traj: `motion` is the odometry of a warm start; pass warm=WarmStart(...) with it")
        # checked on every tick it is given, cold ones included (which do not read it): a wrong shape shows on the first call
        motion = L.require_gpu_f32(motion, "motion")
        if tuple(motion.shape) != (S, 3) or motion.device != device:
            raise ValueError(f"motion must be [{S}, 3] = (tx, ty, phi) per scene on {device}, got {tuple(motion.shape)} "
                             f"on {motion.device}")
    given_motion = motion          # checked; a commit reads it on every tick, a warm start on a warm one
    m_warm, shift = (0, 0) if warm is None else warm.resolve(cfg)
    is_warm = False
    if m_warm == 0:
        shift = 0
    else:
        if m_warm > n:
            raise ValueError(f"WarmStart: steps = {m_warm} is more than EVAL.SAMPLE_STEPS = {n}")
        if not 0 <= shift < H:
            raise ValueError(f"WarmStart: shift = {shift} must be in 0..{H - 1} (MODEL.HORIZON = {H})")
        if not isinstance(noise, DeviceNoise):
            raise ValueError("WarmStart needs noise=DeviceNoise(...): the re-noise is drawn inside the warm-start kernel")
        if noise.device != device:
            raise ValueError(f"the DeviceNoise lives on {noise.device}, the image on {device}")
        if warm.prev is not None and (tuple(warm.prev.shape) != (S, H, D) or warm.prev.device != device):
            raise ValueError(f"WarmStart: the state holds {tuple(warm.prev.shape)} on {warm.prev.device}, this tick is "
                             f"{(S, H, D)} on {device}; use a new WarmStart for another batch shape or device")
        is_warm = bool(warm.valid)
    if is_warm:
        if init_trajs is not None:
            raise ValueError("generate_traj: `init_trajs` and a valid warm state both name the tick's start; warm.reset() first "
                             "for a cold tick from init_trajs")
        if not set_timesteps and len(scheduler.timesteps) != n:    # a caller that keeps its own timesteps
            raise ValueError(f"the scheduler holds {len(scheduler.timesteps)} timesteps, EVAL.SAMPLE_STEPS is {n}")
    else:
        motion = None
    # ---- control ----
    if controller is None:
        if velocity is not None:
            raise ValueError("generate_traj: `velocity` is the speed a controller reads; pass controller=DeviceController(...) with it")
    else:
        if controller.scenes != S or controller.device != device:
            raise ValueError(f"the DeviceController holds the windows of {controller.scenes} scenes on {controller.device}, this tick "
                             f"is {S} scenes on {device}; use a controller of its own for another batch or device")
        controller.check(H, D, target is not None)
        if velocity is None:
            if controller.source != "action":
                raise ValueError("generate_traj: a controller with source='pid' needs `velocity` [S], the scenes' current speeds")
        elif not torch.is_tensor(velocity) or tuple(velocity.shape) != (S,) or velocity.device != device or \
                velocity.dtype != torch.float32:
            what = (tuple(velocity.shape), velocity.dtype, velocity.device) if torch.is_tensor(velocity) else type(velocity).__name__
            raise ValueError(f"velocity must be a float32 tensor [{S}] on {device}, got {what}")
    pin = _pin_plan(cfg, pin, image, scheduler, noise, step_noise, graphed)
    guide = _guide_plan(cfg, guide, image, scheduler)
    if K > 1 and selector.uses_guide and guide is None:
        raise ValueError(f"generate_traj: {selector!r} scores the candidates against a guide; pass guide=Guide(...) for the tick")
    fallback = _fallback_plan(cfg, fallback, guide, controller, image)
    modes = _modes_plan(cfg, modes, K)
    commit, commit_shift = _commit_plan(cfg, commit, K, image)
    rows = K * S if init_trajs is None else int(init_trajs.shape[0])
    free = use == GuidanceType.FREE_GUIDANCE
    return TickPlan(S=S, K=K, selector=selector if K > 1 else None, rows=rows, H=H, D=D, n=n, use=use,
                    free_scale=float(cfg.GUIDANCE.FREE_SCALE) if free else None, fuse=bool(fuse), hoisted=hoisted,
                    table_rows=2 * rows if free else rows, pair_identity=rows == 1 and hoisted, noise=noise, step_noise=step_noise,
                    is_ddpm=not getattr(scheduler, "_is_ddim", False) and not getattr(scheduler, "deterministic", False),
                    start="warm" if is_warm else "init" if init_trajs is not None else "randn" if noise is None else "stream",
                    m_warm=m_warm, shift=shift, is_warm=is_warm, motion=motion, i0=n - m_warm if is_warm else 0,
                    controller=controller, velocity=velocity, pin=pin, entry_blend=pin is not None and pin.mode == "clean",
                    guide=guide, fallback=fallback, modes=modes, commit=commit, commit_shift=commit_shift,
                    commit_motion=given_motion if commit is not None else None)


def generate_traj(model, scheduler, cfg, image: torch.Tensor, target: Optional[torch.Tensor] = None,
                  init_trajs: Optional[torch.Tensor] = None, *, fuse: bool = True, scale_xy: bool = True,
                  step_noise: Optional[Callable[[int, tuple], torch.Tensor]] = None,
                  set_timesteps: bool = True, noise: Optional[DeviceNoise] = None, candidates: int = 1,
                  selector: Optional[TrajectorySelector] = None, return_selection: bool = False,
                  warm: Optional[WarmStart] = None, motion: Optional[torch.Tensor] = None,
                  controller: Optional[DeviceController] = None, velocity: Optional[torch.Tensor] = None,
                  pin: Optional[Pin] = None, guide: Optional[Guide] = None, fallback: Optional[StopShort] = None,
                  modes: Optional[TrajectoryModes] = None, commit: Optional[ManoeuvreCommit] = None,
                  navigator: Optional[Navigator] = None, pose=None):
    """One sampling tick: `plan_tick` decides (what each argument means is written on the TickPlan field it becomes), this
    function runs the plan.  With S = image.shape[0] scenes:

    `target` [2] or [S, 2]; `init_trajs` [K * S, H, D] or None (a draw); `noise`: a DeviceNoise, of which the call is one tick
    (`begin_tick()` first); `step_noise`: injected DDPM noise tensors instead; `candidates` = K and `selector`: best-of-K;
    `warm` and `motion`: warm start; `controller` and `velocity`: the device controller; `pin`: pinned waypoints; `guide`: cost guidance;
    `fallback`: the stop-short fallback (its report of this tick is `fallback.last`, a StopResult without `traj`); `modes`:
    trajectory modes of the K candidates (K > 1; the tick's ModeSet is `modes.last`, in model units; nothing returned changes);
    `commit`: manoeuvre commitment (K > 1; it takes `motion` with or without a `warm`, on every tick); `fuse`, `set_timesteps`,
    `scale_xy`: as the module docstring says.  `navigator` and `pose` (both or neither; `target` and `motion` must then be None):
    the call runs `navigator.step(pose)` on the current stream once the tick is planned and before anything reads a tensor, and
    proceeds exactly as if the caller had passed `target=navigator.target` and, where a `warm` or a `commit` reads the odometry,
    `motion=navigator.motion`; a guide built on `navigator.route(...)` sees the new window.  The step is a launch in front of the
    tick, not part of its plan: there is no TickPlan field for it and no graph key changes; weaving it into a captured graph as a
    node is a later step.

    The order at the end of a tick is fixed: clamp, selection (K > 1), the commit, the modes, the copy into `warm.prev`, the
    fallback, the control launch, xy scaling -- so the warm state sees the clamped, unscaled, pinned, guided result, and the
    controller and the caller that result re-timed by the fallback (when there is one).  Past the commit node `traj`,
    `Selection.index` and `Selection.blocked` are the COMMITTED ones -- `warm.prev`, the fallback, the controller and the caller all
    follow the plan the vehicle follows --; the selector's own choice stays readable as `commit.selected` beside `Selection.cost`
    and `commit.last.index` (`commit.last`: the tick's CommitResult without `best`, which is what the call returns).

    Returns `traj` [S, H, D] (the winners at K > 1); `(traj, selection)` with `return_selection=True` (a Selection whose
    `candidates` is the [K, S, H, D] tensor scaled like `traj`; None at K = 1, where no selector runs); with a controller
    `control` [S, 3] = (throttle, steer, brake) comes last: `(traj, control)` or `(traj, selection, control)`.  `traj` is bit for
    bit what the call without a controller returns."""
    target, motion = _navigator_inputs(navigator, pose, image, target, motion, warm is not None or commit is not None)
    plan = plan_tick(model, scheduler, cfg, image, target, init_trajs, fuse=fuse, set_timesteps=set_timesteps, noise=noise,
                     step_noise=step_noise, candidates=candidates, selector=selector, warm=warm, motion=motion,
                     controller=controller, velocity=velocity, pin=pin, guide=guide, fallback=fallback, modes=modes, commit=commit)
    if navigator is not None:
        navigator.step(pose)       # fills the static target / motion / window the plan already points at
    model.eval()
    device, K, S = image.device, plan.K, plan.S
    noise, controller = plan.noise, plan.controller    # from here on the plan is the one source
    if noise is not None:
        noise.begin_tick()
    if plan.start == "warm":
        if set_timesteps:
            scheduler.set_timesteps(plan.n, device=device)
        # zero_first: the kernel writes the `[:, 0, :3] = 0` of the loop's entry itself
        trajs = warm_init(warm.prev, plan.rows, plan.shift, scheduler.noise_level(scheduler.timesteps[plan.i0]), noise, plan.motion)
    else:
        if plan.start != "init":
            shape = (plan.rows, plan.H, plan.D)
            init_trajs = torch.randn(shape, device=device) if plan.start == "randn" else noise.normal(DeviceNoise.INIT_SLOT, shape)
        trajs = init_trajs.clone().detach()
    # the scenes' targets, and the rows': at K = 1 a row is its own scene
    scene_tgt = _targets(target, plan.rows if K == 1 else S)
    tgt = scene_tgt if K == 1 or scene_tgt is None else scene_tgt.repeat(K, 1)
    free = tgt is not None and plan.use == GuidanceType.FREE_GUIDANCE
    cond = torch.cat([tgt, torch.zeros_like(tgt)], dim=0) if free else None   # interact.py:121-127
    if plan.start != "warm":
        trajs[:, 0, :3] = 0.0
        if set_timesteps:
            scheduler.set_timesteps(plan.n, device=device)
    if plan.entry_blend:
        # where the callers write their one pinned cell group before the loop; waypoint 0 keeps the last word
        trajs = pin_apply(trajs if trajs.is_contiguous() else trajs.contiguous(), plan.pin)
        trajs[:, 0, :3] = 0.0
    # a warm tick's table holds the suffix only; table row r reads image feature r % S: with candidate-major rows its own scene
    tc = _conditioning_table(model, scheduler, image, plan.table_rows, cond, plan.i0) if plan.hoisted else None
    # nothing in this loop writes `image`: say so, so that the reference-faithful per-step encoder pass of a batched tick may run
    # beside the previous step's temporal stack (modeling/perception.py:frozen_image; a no-op for holders without the method)
    frozen = getattr(getattr(model, "perception", None), "frozen_image", None)
    if plan.is_warm:
        scheduler.set_begin_index(plan.i0)
    try:
        with (frozen(image) if frozen is not None else contextlib.nullcontext()):
            trajs = _tick_loop(model, scheduler, plan, image, trajs, tgt, cond, tc)
    finally:
        if plan.is_warm:
            scheduler.set_begin_index(0)       # the begin index belongs to this tick: a later loop on the scheduler starts at 0
    trajs = trajs.to(torch.float32).clamp(-1, 1)
    best, sel = trajs, None                            # at K = 1 the trajectory is its own winner
    if K > 1:
        # the cost is taken in the model's own units (the units of `target` and of the guide)
        sel = plan.selector(trajs, S, scene_tgt, plan.guide) if plan.selector.uses_guide else plan.selector(trajs, S, scene_tgt)
        best = sel.best
        if plan.commit is not None:
            # reads the candidates and the selector's outputs, advances its own state; from here on the committed plan is the plan
            res = plan.commit(trajs, S, sel, plan.commit_motion, plan.commit_shift)
            plan.commit.selected = sel.index
            plan.commit.last = CommitResult(None, *res[1:])      # `best` is the tick's result: later nodes re-time and scale it in place
            best = res.best
            sel = Selection(best, res.index, sel.cost, None, sel.active, sel.blocked if res.blocked is None else res.blocked)
        if plan.modes is not None:
            plan.modes.last = plan.modes(trajs, S)      # reads the candidates, writes buffers of its own
    if plan.m_warm > 0:
        warm._store(best)
    if plan.fallback is not None:
        # in place: warm.prev already holds its own copy of the sampler's winner
        res = plan.fallback(best, plan.guide, out=best if best.is_contiguous() else None)
        best, plan.fallback.last = res.traj, StopResult(None, *res[1:])
    control = None if controller is None else controller.step(best, plan.velocity, scene_tgt, xy_scale=model.magic_num)
    if scale_xy:
        best[..., :2] *= model.magic_num
    if K > 1 and return_selection:
        cands = trajs.reshape(K, S, trajs.shape[1], trajs.shape[2])
        if scale_xy:
            cands[..., :2] *= model.magic_num
        sel = Selection(best, sel.index, sel.cost, cands, sel.active, sel.blocked)
    return _tick_result(best, sel, control, return_selection, controller is not None)


def _navigator_inputs(navigator: Optional[Navigator], pose, image, target, motion, reads_motion: bool):
    """(target, motion) of a tick: the caller's without a navigator; with one its static `target` and -- where a warm start or a
    commit reads the odometry -- `motion`, which `navigator.step(pose)` fills AFTER the tick is planned and before anything reads
    them.  No launch here: every refusal, the plan's included, comes before the walk moves."""
    if navigator is None:
        if pose is not None:
            raise ValueError("generate_traj: `pose` is what a navigator reads; pass navigator=Navigator(...) with it")
        return target, motion
    if not isinstance(navigator, Navigator):
        raise TypeError(f"generate_traj: `navigator` must be a Navigator, got {type(navigator).__name__}")
    if pose is None:
        raise ValueError("generate_traj: a navigator needs `pose` [S, 3] = (x, y, compass), the scenes' world poses of this tick")
    if target is not None or motion is not None:
        raise ValueError("generate_traj: with a navigator `target` and `motion` are its outputs; pass neither")
    if navigator.scenes != int(image.shape[0]) or navigator.device != image.device:
        raise ValueError(f"the Navigator holds the plans of {navigator.scenes} scenes on {navigator.device}, this tick is "
                         f"{int(image.shape[0])} scenes on {image.device}; use a navigator of its own for another batch or device")
    return navigator.target, navigator.motion if reads_motion else None


def _tick_result(traj, selection, control, return_selection: bool, controlled: bool):
    """traj | (traj, selection) | (traj, control) | (traj, selection, control)"""
    out = (traj,) + ((selection,) if return_selection else ()) + ((control,) if controlled else ())
    return traj if len(out) == 1 else out


def _conditioning_table(model, scheduler, image, rows: int, cond=None, begin: int = 0):
    """What `model.time_conditioning` gives for `scheduler.timesteps[begin:]`: one pass for all the steps of a loop (`_hoists`)."""
    ts = scheduler.timesteps
    ts = ts.tensor if hasattr(ts, "tensor") else torch.as_tensor(ts)
    if begin > 0:
        ts = ts[begin:]         # the loop indexes the table relative to `begin`
    with torch.no_grad():
        return model.time_conditioning(image, ts.to(image.device), cond=cond, rows=rows)


def _tick_loop(model, scheduler, plan: TickPlan, image, trajs, tgt, cond, tc):
    """The steps `timesteps[plan.i0:]`; `i` (the row of the conditioning table) counts from there."""
    use, fuse, B = plan.use, plan.fuse, plan.rows
    extra = {} if plan.noise is None else {"generator": plan.noise}
    if plan.pin is not None:
        extra["pin"] = plan.pin
    if plan.guide is not None:
        extra["guide"] = plan.guide
    action = None
    for i, t in enumerate(scheduler.timesteps if plan.i0 == 0 else list(scheduler.timesteps)[plan.i0:]):
        tck = None if tc is None else (tc, i)
        if plan.is_ddpm and plan.step_noise is not None:
            extra["variance_noise"] = plan.step_noise(i, tuple(trajs.shape)).to(image.device)
        if use == GuidanceType.FREE_GUIDANCE:
            with torch.no_grad():
                out = model(trajs if plan.pair_identity else torch.cat([trajs, trajs], dim=0), image, t.reshape(-1), cond=cond,
                            time_cond=tck)
            if fuse:
                trajs = scheduler.step(out, t, trajs, cfg_scale=plan.free_scale, zero_first=True, **extra).prev_sample
                continue
            c, u = out.chunk(2, dim=0)
            model_output = u + plan.free_scale * (c - u)
            trajs = scheduler.step(model_output, t, trajs, **extra).prev_sample
        elif use == GuidanceType.CLASSIFIER_GUIDANCE:
            with torch.no_grad():
                action, time_embed = model(trajs, image, t.reshape(-1).repeat(B), return_action_and_time_only=True,
                                           time_cond=tck)
            guided = getattr(scheduler, "use_classifier_guidance", False) and tgt is not None
            if fuse and guided and scheduler.guidance_loss.guidance_step == 1:
                # one launch: state_pred forward + TargetGuidance + its gradient through state_pred + update + clip
                model_output = model.state_pred.guided_output(action, time_embed, tgt, scheduler.guidance_std(t),
                                                              scheduler.guidance_loss.scale)
                trajs = scheduler.step(model_output, t, trajs, zero_first=True, **extra).prev_sample
                continue
            action = action.detach().requires_grad_()
            with torch.enable_grad():
                state = model.state_pred(action[:, :-1], time_embed)
                state = torch.cat([torch.zeros_like(state[:, :1]), state], dim=1)
                model_output = torch.cat([state, action], dim=-1)
            trajs = scheduler.step(model_output, t, trajs, target=tgt, action=action, **extra).prev_sample.detach()
        else:
            with torch.no_grad():
                model_output = model(trajs, image, t.reshape(-1).repeat(B), time_cond=tck)
            if fuse:
                trajs = scheduler.step(model_output, t, trajs, zero_first=True, **extra).prev_sample
                continue
            trajs = scheduler.step(model_output, t, trajs, **extra).prev_sample
        trajs[:, 0, :3] = 0.0
    return trajs


@torch.no_grad()
def evaluate_sample(model, noise_scheduler, image: torch.Tensor, init_trajs: Optional[torch.Tensor], n_steps: int,
                    step_noise: Optional[Callable[[int, tuple], torch.Tensor]] = None,
                    noise: Optional[DeviceNoise] = None) -> torch.Tensor:
    """train.evaluate's loop: stock DDPM scheduler, B copies of one image, fresh/injected noise.  `noise`: as in
    `generate_traj` (one tick of the noise stream; `init_trajs` may then be None: one trajectory per image row)."""
    model.eval()
    if noise is not None:
        if step_noise is not None:
            raise ValueError("evaluate_sample: pass `noise` (the in-kernel stream) or `step_noise` (injected tensors), not both")
        noise.begin_tick()
    if init_trajs is None:
        if noise is None:
            raise ValueError("evaluate_sample: init_trajs is required without `noise`")
        init_trajs = noise.normal(DeviceNoise.INIT_SLOT, (image.shape[0], model.horizon, model.transition_dim))
    B = init_trajs.shape[0]
    trajs = init_trajs.clone()
    trajs[:, 0, :3] = 0
    noise_scheduler.set_timesteps(n_steps, device=image.device)
    tc = _conditioning_table(model, noise_scheduler, image, B) if _hoists(model) else None
    for i, t in enumerate(noise_scheduler.timesteps):
        out = model(trajs, image, t.reshape(-1).repeat(B), time_cond=None if tc is None else (tc, i))
        kw = {} if noise is None else {"generator": noise}
        if step_noise is not None:
            kw["variance_noise"] = step_noise(i, tuple(trajs.shape)).to(image.device)
        trajs = noise_scheduler.step(out, t, trajs, **kw).prev_sample
        trajs[:, 0, :3] = 0
    return trajs


class GraphedSampler:
    """`generate_traj` captured once as a HIP graph and replayed per tick.

    The loop is a fixed sequence of ~50 launches per denoising step with no host decision inside it (the timestep
    values travel as kernel arguments, the guidance rule runs on the device), so for the small batches of real driving
    (one scene, B = 1 or 2 with classifier-free guidance) the host's launch work is a visible part of the tick: at
    B = 1 the 50-step DDIM loop takes 29.2 ms eagerly and 26.4 ms as one graph launch on an MI355X
    (tools/graph_probe.py; at B = 64 the GPU is the bound either way).  Results are bit-identical to the eager loop.

    Without `noise`: deterministic samplers only (DDIM with eta = 0, or a scheduler that says `deterministic = True` of itself:
    the DPM-Solver++ multistep sampler, whose x0 history is allocated by its steps inside the capture and so lives in the graph's
    pool; a DDPM loop would replay its captured noise tensors).
    With `noise=DeviceNoise(...)` the DDPM scheduler is accepted too: `begin_tick()`, the initial draw (when `init_trajs`
    is not passed) and every step's in-kernel draw are nodes of the graph and read the stream's state from device memory,
    so replay k of a fresh object samples under tick k -- bit for bit what the eager `generate_traj(noise=...)` gives there.
    Eval mode, fused step path.  Inputs are copied into static buffers; the camera frame's perception pass is part of
    the graph, so every replay sees the new frame.
    `candidates=K` > 1 (or EVAL.CANDIDATES when left at 1): best-of-K sampling as in `generate_traj`; the select kernel is a
    node of the graph, the call returns the [S, H, D] winners and `last_selection` the last replay's index and cost (and, when the
    selector scores against the call's guide, `active` and `blocked`: the select node reads the guide's static buffers).
    `warm=WarmStart(...)` (or EVAL.WARM_STEPS > 0 when left at None): warm starting as in `generate_traj`.  The sampler then holds
    two graphs, a cold and a warm one, and picks by the host flag `warm.valid`; both end with the copy into the static
    `warm.prev`, so replay k + 1 starts from replay k's result without leaving the device.  `motion` travels through a static
    buffer like `target`.  Up to `MAX_GRAPHS` captured graphs stay alive (keyed by shapes, K, warm state ...): alternating
    between them replays, it does not capture again.
    `controller=DeviceController(...)`: the control launch is the graph's last kernel node (`generate_traj(controller=...)`);
    `velocity` travels through a static buffer like `target` and `motion`, the call still returns the trajectory and
    `last_control` the [S, 3] controls of the last replay.  The controller's windows live in its own device buffer, which the
    graph reads and advances through its address: replay k of a fresh sampler sees the windows k eager ticks leave (the
    capture's warm-up pass, a real tick, gives its sample back).
    `pin=Pin(...)` per call: pinned waypoints as in `generate_traj`.  `known` and `mask` travel through static buffers like
    `target`, `motion` and `velocity`; presence, mode and shape are part of the graph key, new values never capture again.  A
    `repaint` pin needs `noise=DeviceNoise(...)` at construction (a captured noise tensor would replay) and is refused without.
    `guide=Guide(...)` per call: cost guidance as in `generate_traj`.  `discs` and `planes` travel through static buffers; presence,
    M, P, scale, schedule, cap and iters are part of the graph key (every step node holds its lambda by value), new obstacle values
    never capture again.  A guide's records (guide.py, RECORDS) travel the same way: their tensors through static buffers
    (`Guide.clone`, `Guide.copy_`), their presence and what each one's `key()` holds through the key.
    `fallback=StopShort(...)`: the stop-short launch is a node of the graph after selection and before control
    (`generate_traj(fallback=...)`).  Its params are copied into a static buffer at every call, so new values never capture again;
    its presence is part of the graph key.  The call returns the re-timed plan and `last_fallback` the report of the last replay.
    `modes=TrajectoryModes(...)`: the modes launch is a node of the graph directly after selection (`generate_traj(modes=...)`); its
    settings are part of the graph key.  The call returns what it returns without it and `last_modes` the ModeSet of the last replay.
    `commit=ManoeuvreCommit(...)`: the commit launch is a node of the graph between selection and the modes
    (`generate_traj(commit=...)`); its settings and the address of its state are part of the graph key.  The state lives in the
    commit's own device buffer, which the graph reads and advances through its address: the first tick and every later one are the
    same graph, and replay k of a fresh sampler sees the state k eager ticks leave (the capture's warm-up pass, a real tick, is
    undone).  `motion` is copied into its static buffer at every call and reaches the node on every tick, with or without a `warm`.
    The call returns the committed plan, `last_selection` the committed index and `last_commit` the CommitResult of the last replay.
    `navigator=Navigator(...)` with `pose=` per call (`generate_traj(navigator=...)`): `navigator.step(pose)` is a launch IN FRONT of
    the graph, not a node of it -- it runs on the current stream before anything is copied into the static buffers, and the call
    proceeds as if `target=navigator.target` (and `motion=navigator.motion` with a warm start or a commit) had been passed.  No
    graph key changes; weaving the step in as a node is a later step.  The capture's warm-up pass does not run the step; the
    navigator's state is snapshotted and restored around it all the same, like the controller's and the commit's.
    """

    MAX_GRAPHS = 4

    def __init__(self, model, scheduler, cfg, *, scale_xy: bool = True, noise: Optional[DeviceNoise] = None,
                 candidates: int = 1, selector: Optional[TrajectorySelector] = None, warm: Optional[WarmStart] = None,
                 controller: Optional[DeviceController] = None, fallback: Optional[StopShort] = None,
                 modes: Optional[TrajectoryModes] = None, commit: Optional[ManoeuvreCommit] = None,
                 navigator: Optional[Navigator] = None):
        if navigator is not None and not isinstance(navigator, Navigator):
            raise TypeError(f"GraphedSampler: `navigator` must be a Navigator, got {type(navigator).__name__}")
        deterministic = getattr(scheduler, "_is_ddim", False) or getattr(scheduler, "deterministic", False)
        if float(getattr(cfg.EVAL, "ETA", 0) or 0) != 0.0 or (noise is None and not deterministic):
            raise ValueError("GraphedSampler needs a deterministic sampler (DDIM with eta = 0, DPM-Solver++), or a DeviceNoise for "
                             "the DDPM sampler (noise=...)")
        if warm is None and int(getattr(cfg.EVAL, "WARM_STEPS", 0)) > 0:
            warm = WarmStart()                 # a sampler carries state from tick to tick: the config keys are enough
        if warm is not None and warm.resolve(cfg)[0] > 0 and noise is None:
            raise ValueError("GraphedSampler: WarmStart needs noise=DeviceNoise(...): the re-noise is drawn inside the warm-start kernel")
        self.model, self.scheduler, self.cfg, self.scale_xy, self.noise = model, scheduler, cfg, scale_xy, noise
        self.candidates, self.selector, self.warm = int(candidates), selector, warm
        self.controller = controller
        self.fallback = fallback
        self.modes = modes
        self.commit = commit
        self.navigator = navigator
        self._graphs = {}                      # key -> the captured graph and its static buffers
        self._key = None
        self._graph = None                     # the graph of the last call
        self._sel = None
        self._ctl = None
        self._fb = None
        self._modes = None
        self._commit = None

    def _capture(self, image, target, init_trajs, motion, velocity=None, pin=None, guide=None):
        dev = image.device
        warm = self.warm
        self.model.eval()
        self.scheduler.set_timesteps(self.cfg.EVAL.SAMPLE_STEPS, device=dev)   # host tables + device timesteps, once
        g = SimpleNamespace()
        # the graph reads these device tensors on every replay: keep them alive even if somebody calls
        # scheduler.set_timesteps() again (which replaces the scheduler's own references)
        g.timesteps = list(self.scheduler.timesteps)
        g.img, g.init = image.clone(), None if init_trajs is None else init_trajs.clone()
        g.tgt = None if target is None else target.clone()
        g.motion = None if motion is None else motion.clone()
        g.vel = None if velocity is None else velocity.clone()
        g.pin = None if pin is None else Pin(pin.known.clone(), pin.mask.clone(), pin.mode)
        g.guide = None if guide is None else guide.clone()
        ctl = self.controller
        g.fb = None if self.fallback is None else self.fallback.like(self.fallback.params.clone())
        run = lambda: generate_traj(self.model, self.scheduler, self.cfg, g.img, g.tgt, g.init,  # noqa: E731
                                    fuse=True, scale_xy=self.scale_xy, set_timesteps=False, noise=self.noise,
                                    candidates=self.candidates, selector=self.selector, return_selection=True,
                                    warm=warm, motion=g.motion, controller=ctl, velocity=g.vel, pin=g.pin, guide=g.guide,
                                    fallback=g.fb, modes=self.modes, commit=self.commit)
        tick = None if self.noise is None else self.noise.tick()
        # the warm-up pass below is a real tick: it moves the noise stream on and overwrites the warm state.  Both are given
        # back, so that the first replay is the next tick and starts from the result of the tick before it
        valid = warm is not None and warm.valid
        prev = warm.prev.clone() if valid else None
        windows = None if ctl is None else ctl.state_snapshot()       # ... and pushes a sample into every PID window
        held = None if self.commit is None else self.commit.state_snapshot()      # ... and moves the commit state on one tick
        walk = None if self.navigator is None else self.navigator.state_snapshot()      # the step ran in front: keep what it left
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):          # warm-up off the capture: lazy packs, workspaces, tile tables (and warm.prev)
            run()
        torch.cuda.current_stream(dev).wait_stream(side)
        if tick is not None:
            self.noise.seek(tick)              # the warm-up consumed a tick: give it back, so that the first replay is the next one
        if warm is not None:
            warm.valid = valid
            if prev is not None:
                warm.prev.copy_(prev)
        if windows is not None:
            ctl.state_restore(windows)
        if held is not None:
            self.commit.state_restore(held)
        if walk is not None:
            self.navigator.state_restore(walk)
        self.model._feat_cache = None          # the perception pass must be IN the graph (new frame every tick)
        g.graph = torch.cuda.CUDAGraph()
        # thread-local capture mode: a process group's watchdog thread (multi-rank runs) may query events while this
        # thread captures; in the default global mode that would invalidate the capture
        with torch.cuda.graph(g.graph, capture_error_mode="thread_local"):
            g.out, g.sel, g.ctl = run() if ctl is not None else (*run(), None)
        g.fbres = None if g.fb is None else g.fb.last      # the static first, status, stop_at and active_after of the stop-short node
        g.modes = None if self.modes is None else self.modes.last      # the static outputs of the modes node
        g.commit = None if self.commit is None else self.commit.last   # ... and of the commit node
        g.selected = None if self.commit is None else self.commit.selected
        self.model._feat_cache = None          # the memo now points at the static frame buffer: drop it
        g.pointers = self._model_pointers()
        return g

    def _model_pointers(self):
        """Addresses of the model-owned buffers the captured launches read and write (workspaces, packed weight images and
        the range status words).  The model re-allocates them lazily (a later eager forward at a larger batch or image size, a
        weight re-pack, a move to another device); a replay over stale addresses would touch freed memory, so `__call__`
        re-captures when any moved."""
        m = self.model
        owners = [m, getattr(m, "perception", None), getattr(m, "state_pred", None)]
        return tuple(None if t is None else t.data_ptr()
                     for o in owners if o is not None
                     for t in (getattr(o, "_ws", None), getattr(o, "_packed", None), getattr(o, "_range_words", None)))

    def reset(self) -> None:
        """Forget the captured graphs (call after the model's weights changed: the weight images are packed outside
        the graph, during the warm-up pass of the next capture).  The warm state is the WarmStart's: `warm.reset()`."""
        self._graphs = {}
        self._key, self._graph, self._sel, self._ctl, self._fb, self._modes = None, None, None, None, None, None
        self._commit = None

    @property
    def captured(self) -> int:
        """How many graphs are alive."""
        return len(self._graphs)

    @property
    def last_selection(self) -> Optional[Selection]:
        """Clones of the static `index` [S] and `cost` [S, K] buffers as the last replay left them, and of `active` [S, K] and
        `blocked` [S] when the selector ran against a guide (`best` and `candidates` are not kept: the call returned the winners);
        None before the first call and at one candidate per scene."""
        if self._sel is None:
            return None
        clone = lambda t: None if t is None else t.clone()  # noqa: E731
        return Selection(None, self._sel.index.clone(), self._sel.cost.clone(), None, clone(self._sel.active), clone(self._sel.blocked))

    @property
    def last_candidates(self) -> Optional[torch.Tensor]:
        """A clone of the static [K, S, H, D] candidates as the last replay left them (scaled like the result: `scale_xy`); None
        before the first call and at one candidate per scene.  What `evaluation.OpenLoopMetrics` scores after a replay."""
        return None if self._sel is None or self._sel.candidates is None else self._sel.candidates.clone()

    @property
    def last_control(self) -> Optional[torch.Tensor]:
        """A clone of the static control [S, 3] = (throttle, steer, brake) as the last replay left it; None before the first
        call and without a controller."""
        return None if self._ctl is None else self._ctl.clone()

    @property
    def last_fallback(self) -> Optional[StopResult]:
        """Clones of the static `first`, `status`, `stop_at` and `active_after` [S] as the last replay left them (`traj` is not
        kept: the call returned the re-timed plan); None before the first call and without a fallback."""
        return None if self._fb is None else StopResult(None, *(t.clone() for t in self._fb[1:]))

    @property
    def last_modes(self) -> Optional[ModeSet]:
        """Clones of the static `modes` [M, S, H, D], `index`, `mass`, `assign` and `count` as the last replay left them, in model
        units; None before the first call and without modes."""
        return None if self._modes is None else ModeSet(*(None if t is None else t.clone() for t in self._modes))

    @property
    def last_commit(self) -> Optional[CommitResult]:
        """Clones of the static `index`, `status`, `follower`, `dist2` and `blocked` as the last replay left them (`best` is not
        kept: the call returned the committed plan); None before the first call and without a commit."""
        return None if self._commit is None else CommitResult(*(None if t is None else t.clone() for t in self._commit))

    @torch.no_grad()
    def __call__(self, image: torch.Tensor, target: Optional[torch.Tensor] = None,
                 init_trajs: Optional[torch.Tensor] = None, motion: Optional[torch.Tensor] = None,
                 velocity: Optional[torch.Tensor] = None, pin: Optional[Pin] = None, guide: Optional[Guide] = None,
                 pose=None) -> torch.Tensor:
        warm = self.warm
        target, motion = _navigator_inputs(self.navigator, pose, image, target, motion, warm is not None or self.commit is not None)
        plan = plan_tick(self.model, self.scheduler, self.cfg, image, target, init_trajs, noise=self.noise,
                         candidates=self.candidates, selector=self.selector, warm=warm, motion=motion,
                         controller=self.controller, velocity=velocity, pin=pin, guide=guide, fallback=self.fallback, graphed=True,
                         modes=self.modes, commit=self.commit)
        if self.navigator is not None:
            self.navigator.step(pose)          # in front of the graph: before anything below is copied into a static buffer
        # one static buffer serves the warm start (warm ticks) and the commit node (every tick)
        motion, pin, guide = plan.motion if plan.commit_motion is None else plan.commit_motion, plan.pin, plan.guide
        if plan.start == "randn":
            init_trajs = torch.randn((plan.rows, plan.H, plan.D), device=image.device)
        # init_trajs None (with a DeviceNoise): the initial trajectory is drawn inside the graph, from INIT_SLOT
        # the sampler's own part (the shapes of the static buffers, the device, whose warm state the graph writes), then the plan's
        key = (tuple(image.shape), None if target is None else tuple(target.shape),
               None if init_trajs is None else tuple(init_trajs.shape), image.device, id(warm), plan.key())
        g = self._graphs.get(key)
        if g is None or g.pointers != self._model_pointers():
            self._graphs.pop(key, None)
            while len(self._graphs) >= self.MAX_GRAPHS:
                self._graphs.pop(next(iter(self._graphs)))        # the oldest capture
            g = self._graphs[key] = self._capture(image, target, init_trajs, motion, velocity, pin, guide)
        else:
            g.img.copy_(image)
            if init_trajs is not None:
                g.init.copy_(init_trajs)
            if target is not None:
                g.tgt.copy_(target)
            if motion is not None:
                g.motion.copy_(motion)
            if velocity is not None:
                g.vel.copy_(velocity)
            if pin is not None:
                g.pin.known.copy_(pin.known)
                g.pin.mask.copy_(pin.mask)
            if guide is not None:
                g.guide.copy_(guide)
            if g.fb is not None:
                g.fb.params.copy_(self.fallback.params)
        self._key, self._graph, self._sel, self._ctl, self._fb, self._modes = key, g.graph, g.sel, g.ctl, g.fbres, g.modes
        if self.modes is not None:
            self.modes.last = g.modes          # the static buffers of the graph that replays now (`last_modes` hands out clones)
        self._commit = g.commit
        if self.commit is not None:
            self.commit.last, self.commit.selected = g.commit, g.selected
        # range_guard = "raise": what an eager forward does around its pass (clear, run, read), here around the replay -- the
        # check is skipped while the graph is captured
        guard = getattr(self.model, "range_guard", "off") == "raise"
        if guard:
            self.model.clear_range_status()
        g.graph.replay()
        if plan.m_warm > 0:
            warm.valid = True                  # the replay ended with the copy into warm.prev
        if guard:
            bad = self.model.range_status()
            if bad:
                raise AdxRangeError(bad)
        return g.out.clone()
