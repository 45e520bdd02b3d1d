from .base import DDIMScheduler, DDPMScheduler, SchedulerOutput, TimestepSequence
from .dpm import GuidanceDPMSolverMultistepScheduler
from .guidance import GuidanceDDIMScheduler, GuidanceDDPMScheduler
from .inpainting import InpaintingDDIMScheduler, InpaintingDDPMScheduler

__all__ = [
    "GuidanceDDIMScheduler",
    "GuidanceDDPMScheduler",
    "GuidanceDPMSolverMultistepScheduler",
    "InpaintingDDIMScheduler",
    "InpaintingDDPMScheduler",
    "DDPMScheduler",
    "DDIMScheduler",
]
