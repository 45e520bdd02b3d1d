"""MI355X-native diffusion trajectory denoiser (drop-in for the hot path of
Justin900429/autonomous_driving_with_diffusion_model).

Public surface mirrors the reference's packages:
    modeling.build_model(cfg)                         (reference: modeling/__init__.py)
    scheduler.{GuidanceDDIM,GuidanceDDPM,InpaintingDDIM,InpaintingDDPM}Scheduler, DDPMScheduler
    scheduler.GuidanceDPMSolverMultistepScheduler     (no reference counterpart: what `EVAL.SCHEDULER: dpm` names, scheduler/dpm.py)
    control.GuidanceLoss
    DeviceNoise                                       (no reference counterpart: in-kernel sampler noise, noise.py)
    TrajectorySelector, Selection                     (no reference counterpart: best-of-K sampling, control/select.py)
    WarmStart                                         (no reference counterpart: receding-horizon warm starting, sampling.py)
    Pin                                               (no reference counterpart: waypoints held through a tick, pin.py)
    Guide                                             (no reference counterpart: obstacles a tick steers around, guide.py)
    CostField                                         (no reference counterpart: a cost raster in a Guide, guide.py)
    MotionLimits                                      (no reference counterpart: speed and acceleration limits in a Guide, guide.py)
    Route                                             (no reference counterpart: a route corridor in a Guide, guide.py)
    Capsules                                          (no reference counterpart: moving capsules in a Guide, guide.py)
    StopShort, StopResult                             (no reference counterpart: re-time a blocked plan to halt before its
                                                       conflict, control/fallback.py)
    TrajectoryModes, ModeSet                          (no reference counterpart: the manoeuvres a scene's K candidates contain and
                                                       the sample mass behind each, control/modes.py)
    ManoeuvreCommit, CommitResult                     (no reference counterpart: hold the previous tick's manoeuvre unless the
                                                       selector's new choice is clearly better, control/commit.py)
    Navigator, EgoFrame                               (planner.RoutePlanner.run_step, process_next_waypoint, get_future_waypoints
                                                       and agent_to_world for all scenes on the device, and the odometry a
                                                       warm start takes, navigation.py)
    OpenLoopMetrics, evaluate_open_loop               (no reference counterpart: ADE / FDE, minADE_K / minFDE_K and miss rates
                                                       against logged waypoints, on the device, evaluation.py)
    KinematicVehicle, DriveMetrics, World, drive,     (no reference counterpart -- the reference drives CARLA --: a kinematic
    evaluate_closed_loop                               bicycle, the closed-loop criteria of a drive and the runner that strings
                                                       navigator, tick, vehicle and metrics together, on the device, simulation.py)
    Signals                                           (no reference counterpart -- the reference asks CARLA --: traffic lights and
                                                       stop signs as the guide's stop lines, and the RunRedLight / RunStopSign
                                                       criteria, on the device, signals.py)
    Traffic                                           (no reference counterpart -- the reference's traffic is CARLA's autopilot and
                                                       BasicAgent --: car-following agents on caller-laid paths that queue, stop at
                                                       the lights and yield to the ego, on the device, traffic.py)
    Camera                                            (no reference counterpart -- the reference reads CARLA's RGB sensor --: the
                                                       front camera as an analytic ray caster over the world's primitives, the
                                                       frames `drive(image=)` feeds the encoder, on the device, camera.py)
    Expert                                            (no reference counterpart -- the reference collects with CARLA's autopilot and
                                                       a Roach expert --: a privileged driver that follows the route, queues, stops
                                                       at lights and slows for bends, on the device, expert.py)
    Demonstrations                                    (misc/data_collect.py's writer: a drive recorded as the frames, hindsight
                                                       waypoints and targets TrajDataset reads, demos.py)
    DeviceController                                  (control.Controller + post_process_control for all scenes in one launch,
                                                       control/device.py)
    misc.constant.GuidanceType, misc.load_param.copy_parameters
All compute runs in libadx.so (hand-written HIP for gfx950); there is no CPU fallback.
"""
import os as _os

# Kernel arguments in DEVICE memory (ROCm's HIP_FORCE_DEV_KERNARG, AMD's recommended setting for MI300-class parts): every
# eagerly launched kernel otherwise fetches its argument block from host memory when it starts -- 1-2 us in front of kernels that
# run for 5-10 us.  The reference's own loops launch eagerly (interact.py:131-164): measured on the deployed tick (one scene,
# 50 DDIM steps) 17.5 -> 14.5 ms; HIP-graph replays keep their arguments on the device either way (profiles/README.md,
# round 6).  The runtime reads the variable when it initialises, i.e. at the process's first GPU call: set here unless the
# user decided otherwise; a process that has already touched the GPU before importing this package keeps what it had.
_os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

from . import _lib  # noqa: F401,E402
from .noise import DeviceNoise  # noqa: E402
from .scheduler import GuidanceDPMSolverMultistepScheduler  # noqa: E402
from .control.select import Selection, TrajectorySelector  # noqa: E402
from .control.device import DeviceController  # noqa: E402
from .control.fallback import StopResult, StopShort  # noqa: E402
from .control.modes import ModeSet, TrajectoryModes  # noqa: E402
from .control.commit import CommitResult, ManoeuvreCommit  # noqa: E402
from .pin import Pin  # noqa: E402
from .guide import Capsules, CostField, Guide, MotionLimits, Route  # noqa: E402
from .navigation import EgoFrame, Navigator  # noqa: E402
from .sampling import WarmStart  # noqa: E402
from .evaluation import MetricsBatch, OpenLoopMetrics, evaluate_open_loop  # noqa: E402
from .simulation import DriveMetrics, EagerTick, KinematicVehicle, World, drive, evaluate_closed_loop  # noqa: E402
from .signals import Signals  # noqa: E402
from .traffic import Traffic  # noqa: E402
from .camera import Camera  # noqa: E402
from .expert import Expert  # noqa: E402
from .demos import Demonstrations  # noqa: E402

__all__ = ["modeling", "scheduler", "control", "misc", "config", "sampling", "DeviceNoise", "GuidanceDPMSolverMultistepScheduler",
           "TrajectorySelector", "Selection", "WarmStart", "DeviceController", "Pin", "Guide", "CostField", "MotionLimits",
           "Route", "Capsules", "StopShort", "StopResult", "TrajectoryModes", "ModeSet", "ManoeuvreCommit", "CommitResult",
           "OpenLoopMetrics", "MetricsBatch", "evaluate_open_loop", "Navigator", "EgoFrame",
           "KinematicVehicle", "DriveMetrics", "World", "EagerTick", "drive", "evaluate_closed_loop", "Signals", "Traffic", "Camera",
           "Expert", "Demonstrations"]
