from .controller import Controller, post_process_control
from .device import DeviceController
from .guidance import GuidanceLoss
from .guidance_loss import TargetGuidance
from .pid import PIDController
from .fallback import StopResult, StopShort
from .commit import CommitResult, ManoeuvreCommit
from .modes import ModeSet, TrajectoryModes
from .select import Selection, TrajectorySelector

__all__ = ["GuidanceLoss", "TargetGuidance", "Controller", "PIDController", "post_process_control", "Selection",
           "TrajectorySelector", "DeviceController", "StopShort", "StopResult", "TrajectoryModes", "ModeSet", "ManoeuvreCommit",
           "CommitResult"]
