"""GuidanceDDIMScheduler / GuidanceDDPMScheduler (reference: scheduler/guidance_ddim_scheduler.py,
scheduler/guidance_ddpm_scheduler.py): same constructor (`cfg=` + diffusers kwargs) and
`step(model_output, t, sample, ..., target=None, action=None)`; the elementwise math of one step is
one HIP kernel launch.  Deviation, documented: `GuidanceDDPMScheduler(thresholding=True)` raises
NameError in the reference (`np` is not imported, guidance_ddpm_scheduler.py:41); here it performs
the thresholding the code intended, which for sample_max_value = 1 is clamp(-1, 1)."""
from __future__ import annotations

import torch

from ..misc.constant import GuidanceType
from .base import DDIMScheduler, DDPMScheduler, timestep_to_int


def _wants_classifier_guidance(cfg) -> bool:
    return cfg.GUIDANCE.USE_COND == GuidanceType.CLASSIFIER_GUIDANCE.name and cfg.GUIDANCE.LOSS_LIST is not None


class GuidanceDDIMScheduler(DDIMScheduler):
    supports_pin = True
    supports_guide = True

    def __init__(self, cfg, **kwargs):
        super().__init__(**kwargs)
        self.use_classifier_guidance = _wants_classifier_guidance(cfg)
        if self.use_classifier_guidance:
            from ..control import GuidanceLoss
            self.guidance_loss = GuidanceLoss(cfg)

    def guidance_std(self, timestep) -> float:
        """model_std = exp(0.5 * variance) handed to GuidanceLoss (guidance_ddim_scheduler.py:87-91)."""
        t = timestep_to_int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        return float(torch.exp(0.5 * self._get_variance(t, prev_t)))

    def step(self, model_output, timestep, sample, eta: float = 0.0, use_clipped_model_output: bool = False,
             generator=None, variance_noise=None, return_dict: bool = True, target=None, action=None,
             cfg_scale=None, zero_first: bool = False, pin=None, guide=None):
        """`cfg_scale` / `zero_first` are optional fusions (classifier-free combine of a [2B] model
        output, interact.py:142-144, and `prev[:, 0, :3] = 0`, interact.py:164); leaving them at their
        defaults gives exactly the reference signature and behaviour.

        `pin`: a Pin ("pinned waypoints v1", include/adx.h): the finished prev_sample is blended with the pin's known values
        under its mask in the same kernel, before `zero_first`.  A `repaint` pin shares the step's own noise (eta > 0); with
        eta = 0 it draws from `generator` when that is a DeviceNoise, else a tensor as the step's noise would be drawn
        (`variance_noise`, or torch.randn from `generator`).  None is the call as it was.

        `guide`: a Guide ("cost guidance v1", include/adx.h, guide.py): the xy of the clipped pred_original_sample move down the
        gradient of the guide's cost inside the same kernel, a moved element's eps is re-derived from its x0 (the
        `use_clipped_model_output` arithmetic) and `pred_original_sample` returns the guided value.  None is the call as it was."""
        t = timestep_to_int(timestep)
        c = self._ddim_coef(t, eta, use_clipped_model_output)
        if self.use_classifier_guidance and target is not None:
            prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
            with torch.enable_grad():
                model_std = torch.exp(0.5 * self._get_variance(t, prev_t))
                model_output = self.guidance_loss(model_output, action, target, model_std)
        mo, x = self._check_step_inputs(model_output, sample, cfg_scale is not None)
        self._fuse(c, cfg_scale, zero_first)
        z = None
        if eta > 0:
            if variance_noise is not None and generator is not None:
                raise ValueError("Cannot pass both generator and variance_noise. Please make sure that either "
                                 "`generator` or `variance_noise` stays `None`.")
            z = self._noise(x.shape, generator, x.device, x.dtype, variance_noise)
        p, p_noise = self._pin_desc(pin, t, x)
        if p_noise and z is None:
            z = self._noise(x.shape, generator, x.device, x.dtype, variance_noise)
        prev, x0 = self._launch(False, c, mo, x, z, None, None, slot=t, pin=p, guide=self._guide_desc(guide, t, x))
        return self._result(prev, x0, return_dict)


class GuidanceDDPMScheduler(DDPMScheduler):
    supports_pin = True
    supports_guide = True

    def __init__(self, cfg, **kwargs):
        super().__init__(**kwargs)
        self.use_classifier_guidance = _wants_classifier_guidance(cfg)
        if self.use_classifier_guidance:
            from ..control import GuidanceLoss
            self.guidance_loss = GuidanceLoss(cfg)

    def guidance_std(self, timestep) -> float:
        """model_std = exp(0.5 * variance) handed to GuidanceLoss (guidance_ddpm_scheduler.py:94-99)."""
        return float(torch.exp(0.5 * self._get_variance(timestep_to_int(timestep))))

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True, target=None,
             action=None, variance_noise=None, cfg_scale=None, zero_first: bool = False, pin=None, guide=None):
        """`pin`: as in GuidanceDDIMScheduler.step; a `repaint` pin shares the step's noise (both exist exactly when t > 0).
        `guide`: as in GuidanceDDIMScheduler.step; a moved x0 enters `c_x0 * x0 + c_x * x`."""
        t = timestep_to_int(timestep)
        c = self._ddpm_coef(t)
        if self.use_classifier_guidance and target is not None:
            with torch.enable_grad():
                model_std = torch.exp(0.5 * self._get_variance(t))
                model_output = self.guidance_loss(model_output, action, target, model_std)
        mo, x = self._check_step_inputs(model_output, sample, cfg_scale is not None)
        self._fuse(c, cfg_scale, zero_first)
        z = self._noise(x.shape, generator, x.device, x.dtype, variance_noise) if t > 0 else None
        p, _ = self._pin_desc(pin, t, x)
        prev, x0 = self._launch(True, c, mo, x, z, None, None, slot=t, pin=p, guide=self._guide_desc(guide, t, x))
        return self._result(prev, x0, return_dict)
