"""GuidanceDPMSolverMultistepScheduler: the deterministic DPM-Solver++ multistep sampler, order 2 (midpoint; "2M") with order 1
selectable.  What `EVAL.SCHEDULER: dpm` names in the reference's callers (interact.py:92-93 and
e2e_driving/diffusion_agent.py:86-87 set its `lambda_min_clipped` keyword) without ever constructing it: `SCHEDULER_FUNC`
has no "dpm" entry there.  INTEGRATION.md shows the one line that adds it.

Host arithmetic restated from the published `diffusers==0.28.0` DPMSolverMultistepScheduler (`algorithm_type="dpmsolver++"`,
`solver_type="midpoint"`, `timestep_spacing="linspace"`, `final_sigmas_type="zero"`): fp32 tables built with torch and numpy
on the host, per-step scalars as 0-dim fp32 CPU tensors in that code's operation order, handed BY VALUE to the fused step
kernel (csrc/sched.hip, adx_dpm_step), as base.py does for DDIM.  PARITY UNPINNED: diffusers is not a dependency and the
reference has no vectors for this sampler.

The solver has one step of memory: a second-order step reads the x0 the previous step produced.  The scheduler keeps a
reference to that tensor and to the index of the call that wrote it; the index of a call is found from the timestep's VALUE
(not counted), index 0 never reads history, so loops may be run any number of times -- and captured into a graph -- without
a reset between them.  `set_begin_index(i0)` moves that first, history-free step to index i0: step i0 is then first order,
the steps after it are what they are in the full schedule.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from .. import _lib as L
from ..noise import DeviceNoise
from .base import PRED, SchedulerBase, TimestepSequence, timestep_to_int
from .guidance import _wants_classifier_guidance


class GuidanceDPMSolverMultistepScheduler(SchedulerBase):
    _is_ddim = False
    deterministic = True        # no step draws noise: a captured loop replays exactly (sampling.GraphedSampler)
    supports_pin = True
    supports_guide = True

    def __init__(self, cfg=None, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, solver_order=2, prediction_type="epsilon", thresholding=False,
                 dynamic_thresholding_ratio=0.995, sample_max_value=1.0, algorithm_type="dpmsolver++",
                 solver_type="midpoint", lower_order_final=True, euler_at_final=False, use_karras_sigmas=False,
                 use_lu_lambdas=False, final_sigmas_type="zero", lambda_min_clipped=-float("inf"), variance_type=None,
                 timestep_spacing="linspace", steps_offset=0, rescale_betas_zero_snr=False):
        if cfg is not None and _wants_classifier_guidance(cfg):
            raise ValueError("classifier guidance needs the step's variance (model_std = exp(0.5 * variance)), which an ODE "
                             "solver does not have: use GuidanceDDIMScheduler / GuidanceDDPMScheduler, or NO / FREE guidance")
        if solver_order not in (1, 2):
            raise NotImplementedError(f"solver_order={solver_order}: only orders 1 and 2 (DPM-Solver++ 2M) are implemented")
        if algorithm_type != "dpmsolver++":
            raise NotImplementedError(f"algorithm_type={algorithm_type!r}: only the deterministic 'dpmsolver++' is implemented")
        if solver_type != "midpoint":
            raise NotImplementedError(f"solver_type={solver_type!r}: only 'midpoint' is implemented")
        if lower_order_final is not True:
            raise NotImplementedError("lower_order_final=False has no effect with final_sigmas_type='zero' (the last step is "
                                      "always first order); only True is accepted")
        if euler_at_final:
            raise NotImplementedError("euler_at_final=True is implied by final_sigmas_type='zero'; only False is accepted")
        if use_karras_sigmas or use_lu_lambdas:
            raise NotImplementedError("Karras sigmas / Lu lambdas are not implemented: the schedule is the linspace one")
        if final_sigmas_type != "zero":
            raise NotImplementedError(f"final_sigmas_type={final_sigmas_type!r}: only 'zero' is implemented")
        if variance_type is not None:
            raise NotImplementedError("variance_type: a model that predicts a variance is not supported")
        if timestep_spacing != "linspace":
            raise NotImplementedError(f"timestep_spacing={timestep_spacing!r}: only 'linspace' (the DPM-Solver default) is "
                                      "implemented")
        if steps_offset != 0:
            raise NotImplementedError("steps_offset is not used by 'linspace' spacing; only 0 is accepted")
        # the DDIM/DDPM base checks 'leading' spacing: hand it its own default and record the real value afterwards
        super().__init__(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas, False, prediction_type,
                         thresholding, dynamic_thresholding_ratio, 1.0, sample_max_value, "leading", 0,
                         rescale_betas_zero_snr)
        self.config = SimpleNamespace(
            num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
            trained_betas=trained_betas, solver_order=solver_order, prediction_type=prediction_type,
            thresholding=thresholding, dynamic_thresholding_ratio=dynamic_thresholding_ratio,
            sample_max_value=sample_max_value, algorithm_type=algorithm_type, solver_type=solver_type,
            lower_order_final=lower_order_final, euler_at_final=euler_at_final, use_karras_sigmas=use_karras_sigmas,
            use_lu_lambdas=use_lu_lambdas, final_sigmas_type=final_sigmas_type, lambda_min_clipped=lambda_min_clipped,
            variance_type=variance_type, timestep_spacing=timestep_spacing, steps_offset=steps_offset,
            rescale_betas_zero_snr=rescale_betas_zero_snr)
        self.use_classifier_guidance = False
        self.alpha_t = torch.sqrt(self.alphas_cumprod)
        self.sigma_t = torch.sqrt(1 - self.alphas_cumprod)
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)
        self.sigmas = ((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5
        self._index = {}
        self._last = None        # (index, x0 tensor) of the previous step() call

    # -- schedule ----------------------------------------------------------------------------------
    def set_timesteps(self, num_inference_steps: int, device=None):
        n_train = self.config.num_train_timesteps
        clipped_idx = torch.searchsorted(torch.flip(self.lambda_t, [0]), self.config.lambda_min_clipped)
        last = int((n_train - clipped_idx).numpy().item())
        ts = np.linspace(0, last - 1, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
        if len(set(ts.tolist())) != len(ts):
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} rounds to repeated timesteps on the {last} usable "
                             f"train timesteps (lambda_min_clipped = {self.config.lambda_min_clipped}); at most {last - 1}")
        sigmas = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        sigmas = np.interp(ts, np.arange(0, len(sigmas)), sigmas)
        sigmas = np.concatenate([sigmas, [0]]).astype(np.float32)
        self.sigmas = torch.from_numpy(sigmas)
        self.num_inference_steps = num_inference_steps
        self.timesteps = TimestepSequence(ts.tolist(), device=device)
        self._index = {t: i for i, t in enumerate(ts.tolist())}
        self._last = None
        self.begin_index = 0

    def previous_timestep(self, timestep):
        raise NotImplementedError("the multistep solver steps along `timesteps`, not by a fixed stride")

    @staticmethod
    def _sigma_to_alpha_sigma_t(sigma):
        alpha_t = 1 / ((sigma ** 2 + 1) ** 0.5)
        sigma_t = sigma * alpha_t
        return alpha_t, sigma_t

    def step_index(self, timestep) -> int:
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the "
                             "scheduler")
        t = timestep_to_int(timestep)
        if t not in self._index:
            raise ValueError(f"timestep {t} is not one of this schedule's timesteps {self.timesteps.tolist()}")
        return self._index[t]

    def _dpm_coef(self, i: int) -> L.DpmCoef:
        """The scalars of step i (sigmas[i] -> sigmas[i + 1]) in the operation order of diffusers' convert_model_output,
        dpm_solver_first_order_update and multistep_dpm_solver_second_order_update."""
        pt = self.config.prediction_type
        if pt not in PRED:
            raise ValueError(f"prediction_type given as {pt} must be one of `epsilon`, `sample`, or `v_prediction`")
        n = len(self.timesteps)
        c = L.DpmCoef()
        c.prediction_type = PRED[pt]
        c.clip, c.clip_range = (1, 1.0) if self.config.thresholding else (0, 0.0)   # sample_max_value is 1: clamp(-1, 1)
        sigma_t, sigma_s0 = self.sigmas[i + 1], self.sigmas[i]
        alpha_t, sigma_t = self._sigma_to_alpha_sigma_t(sigma_t)
        alpha_s0, sigma_s0 = self._sigma_to_alpha_sigma_t(sigma_s0)
        lambda_t = torch.log(alpha_t) - torch.log(sigma_t)
        lambda_s0 = torch.log(alpha_s0) - torch.log(sigma_s0)
        h = lambda_t - lambda_s0
        k = alpha_t * (torch.exp(-h) - 1.0)
        c.alpha_s, c.sigma_s = float(alpha_s0), float(sigma_s0)
        c.r = float(sigma_t / sigma_s0)
        c.k = float(k)
        c.half_k = float(0.5 * k)
        # the first executed step (set_begin_index; 0 unless the schedule begins in the middle) has no history: first order
        second = self.config.solver_order == 2 and self.begin_index < i < n - 1
        c.second_order = int(second)
        if second:
            alpha_s1, sigma_s1 = self._sigma_to_alpha_sigma_t(self.sigmas[i - 1])
            lambda_s1 = torch.log(alpha_s1) - torch.log(sigma_s1)
            h_0 = lambda_s0 - lambda_s1
            r0 = h_0 / h
            c.inv_r0 = float(1.0 / r0)
        return c

    def _guide_sb(self, timestep) -> float:
        return self._dpm_coef(self.step_index(timestep)).sigma_s

    def _repaint_level(self, timestep):
        """alpha and sigma * alpha of sigmas[i + 1], as `_dpm_coef` forms alpha_t and sigma_t; no noise on the last step."""
        i = self.step_index(timestep)
        alpha_t, sigma_t = self._sigma_to_alpha_sigma_t(self.sigmas[i + 1])
        return float(alpha_t), float(sigma_t), i < len(self.timesteps) - 1

    # -- step --------------------------------------------------------------------------------------
    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True, target=None, action=None,
             cfg_scale=None, zero_first: bool = False, pin=None, guide=None):
        """One solver step.  `target` and `action` are accepted for the callers' common signature and unused (classifier
        guidance is refused at construction); so is `generator` without a pin: no step draws noise.  `cfg_scale` /
        `zero_first`: the fusions of GuidanceDDIMScheduler.step; `pred_original_sample` is never zeroed (it is the next step's
        history).

        `pin`: a Pin ("pinned waypoints v1", include/adx.h), blended into prev_sample before `zero_first`;
        `pred_original_sample` is never pinned.  A `repaint` pin is the one thing that makes this step draw: it needs
        `generator=DeviceNoise(...)` (the draw happens in the kernel, at the slot of the timestep) and raises ValueError without.

        `guide`: a Guide ("cost guidance v1", include/adx.h): a moved x0 enters the first- and second-order terms and is the
        `pred_original_sample` the next step reads as history."""
        i = self.step_index(timestep)
        stream = isinstance(generator, DeviceNoise)
        if pin is not None and pin.resolve() == "repaint" and not stream:
            raise ValueError("a `repaint` pin needs generator=DeviceNoise(...) on the DPM-Solver++ sampler: the solver has no noise "
                             "of its own, the pin's is drawn inside the step kernel")
        c = self._dpm_coef(i)
        history = None
        if c.second_order:
            ok = (self._last is not None and self._last[0] == i - 1 and torch.is_tensor(sample)
                  and self._last[1].shape == sample.shape and self._last[1].device == sample.device)
            if not ok:
                was = "no step" if self._last is None else f"step {self._last[0]} on {tuple(self._last[1].shape)}, {self._last[1].device}"
                raise ValueError(f"step {i} (timestep {timestep_to_int(timestep)}) is second order and needs the x0 of step "
                                 f"{i - 1} on a sample of the same shape and device; the previous call was {was}")
            history = self._last[1]
        mo, x = self._check_step_inputs(model_output, sample, cfg_scale is not None)
        self._fuse(c, cfg_scale, zero_first)
        B, H, D = x.shape
        p, _ = self._pin_desc(pin, timestep, x)
        g = self._guide_desc(guide, timestep, x)
        prev, x0 = torch.empty_like(x), torch.empty_like(x)
        if g is not None:
            suffix, guides, _alive = g                                                     # as guide.py's `Guide.descs` chooses them
            _, state, row_offset = self._noise_args(generator if stream else None, x)      # the stream or nothing
            L.check(L.lazy("adx_dpm_step_" + suffix)(
                C.byref(c), mo.data_ptr(), x.data_ptr(), L.ptr(history), state, timestep_to_int(timestep), row_offset,
                None if p is None else C.byref(p), *guides, prev.data_ptr(), x0.data_ptr(), B, H, D, L.stream_ptr(x.device)),
                "scheduler step")
        elif p is None:
            L.check(L.lib().adx_dpm_step(C.byref(c), mo.data_ptr(), x.data_ptr(), L.ptr(history), prev.data_ptr(), x0.data_ptr(),
                                         B, H, D, L.stream_ptr(x.device)), "scheduler step")
        else:
            _, state, row_offset = self._noise_args(generator if stream else None, x)      # the stream or nothing
            L.check(L.lazy("adx_dpm_step_pin")(C.byref(c), mo.data_ptr(), x.data_ptr(), L.ptr(history), state,
                                               timestep_to_int(timestep), row_offset, C.byref(p), prev.data_ptr(), x0.data_ptr(),
                                               B, H, D, L.stream_ptr(x.device)), "scheduler step")
        self._last = (i, x0)
        return self._result(prev, x0, return_dict)

