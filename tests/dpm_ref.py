"""Test infrastructure: CPU restatement of the deterministic DPM-Solver++ multistep sampler (orders 1 and 2, midpoint) that
scheduler/dpm.py and csrc/sched.hip (adx_dpm_step) implement, written from the published `diffusers==0.28.0`
DPMSolverMultistepScheduler (`algorithm_type="dpmsolver++"`, `timestep_spacing="linspace"`, `final_sigmas_type="zero"`).
diffusers is not installed and the reference never constructs this scheduler, so parity with diffusers is UNPINNED; what
this file pins is (a) the solver's order of accuracy on a problem with a closed-form answer and (b) that the package computes
exactly this arithmetic.

Every step exists in two forms that share one function: with fp32 scalars (0-dim CPU tensors, the operation order of the
package's host side; applied op by op to fp32 tensors on any device) and with fp64 scalars and tensors throughout.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from oracle import unet as U
from oracle.diffusers_base import make_betas
from oracle.resnet import resnet34_forward

MAGIC_NUM = 23.315
SCALARS = ("alpha_s", "sigma_s", "r", "k", "half_k", "inv_r0")


def alphas_cumprod(n_train=100, beta_schedule="squaredcos_cap_v2", beta_start=1e-4, beta_end=0.02) -> torch.Tensor:
    """fp32, as every scheduler of the package builds it."""
    return torch.cumprod(1.0 - make_betas(beta_schedule, n_train, beta_start, beta_end), dim=0)


def schedule(ac: torch.Tensor, n: int, lambda_min_clipped: float = -math.inf, dtype=np.float32):
    """-> (timesteps int64 [n], sigmas `dtype` [n + 1], the last one 0)."""
    N = ac.shape[0]
    alpha_t, sigma_t = torch.sqrt(ac), torch.sqrt(1 - ac)
    lambda_t = torch.log(alpha_t) - torch.log(sigma_t)
    clipped_idx = int(torch.searchsorted(torch.flip(lambda_t, [0]), lambda_min_clipped))
    last = N - clipped_idx
    timesteps = np.linspace(0, last - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
    table = (((1 - ac) / ac) ** 0.5).numpy()
    sigmas = np.interp(timesteps, np.arange(0, N), table)
    return timesteps, np.concatenate([sigmas, [0.0]]).astype(dtype)


def _alpha_sigma(sigma):
    alpha = 1 / ((sigma ** 2 + 1) ** 0.5)
    return alpha, sigma * alpha


def _lam(sigma):
    alpha, sig = _alpha_sigma(sigma)
    return torch.log(alpha) - torch.log(sig)


def step_order(i: int, n: int, solver_order: int) -> int:
    """First order at index 0, at the last index and when the solver is first order; second order everywhere else."""
    return 1 if (i == 0 or i == n - 1 or solver_order == 1) else 2


def coefficients(sigmas: torch.Tensor, i: int, solver_order: int = 2) -> dict:
    """The scalars of step i as 0-dim tensors of `sigmas`' dtype.  `inv_r0` exists on second-order steps only; it is 0 on
    the others (nothing reads it there)."""
    n = sigmas.shape[0] - 1
    alpha_s, sigma_s = _alpha_sigma(sigmas[i])
    alpha_n, sigma_n = _alpha_sigma(sigmas[i + 1])
    h = _lam(sigmas[i + 1]) - _lam(sigmas[i])
    k = alpha_n * (torch.exp(-h) - 1.0)
    co = dict(alpha_s=alpha_s, sigma_s=sigma_s, r=sigma_n / sigma_s, k=k, half_k=0.5 * k, inv_r0=torch.zeros_like(k),
              second_order=step_order(i, n, solver_order) == 2)
    if co["second_order"]:
        r0 = (_lam(sigmas[i]) - _lam(sigmas[i - 1])) / h
        co["inv_r0"] = 1.0 / r0
    return co


def step(co: dict, prediction_type: str, thresholding: bool, m: torch.Tensor, x: torch.Tensor,
         prev_x0: Optional[torch.Tensor] = None):
    """One solver step, one torch op per arithmetic operation, left to right.  -> (prev_sample, x0)"""
    a, s = co["alpha_s"], co["sigma_s"]
    if prediction_type == "epsilon":
        x0 = (x - s * m) / a
    elif prediction_type == "sample":
        x0 = m
    elif prediction_type == "v_prediction":
        x0 = a * x - s * m
    else:
        raise ValueError(prediction_type)
    if thresholding:                       # sample_max_value = 1: the dynamic threshold is clamp(-1, 1)
        x0 = x0.clamp(-1, 1)
    prev = co["r"] * x - co["k"] * x0
    if co["second_order"]:
        prev = prev - co["half_k"] * (co["inv_r0"] * (x0 - prev_x0))
    return prev, x0


def on_device(co: dict, device) -> dict:
    """The step's scalars as one-element tensors on `device`, so that every product is a tensor-tensor op there."""
    return {k: (torch.full((1,), float(v), dtype=v.dtype, device=device) if torch.is_tensor(v) else v) for k, v in co.items()}


class Solver:
    """The sampler as a loop object: `for i in range(n): x = solver.step(i, model_output, x)`."""

    def __init__(self, n_steps: int, *, n_train=100, beta_schedule="squaredcos_cap_v2", beta_start=1e-4, beta_end=0.02,
                 prediction_type="sample", thresholding=False, solver_order=2, lambda_min_clipped=-math.inf,
                 dtype=torch.float32):
        self.prediction_type, self.thresholding, self.solver_order, self.dtype = prediction_type, thresholding, solver_order, dtype
        ac = alphas_cumprod(n_train, beta_schedule, beta_start, beta_end)
        self.timesteps, sig = schedule(ac, n_steps, lambda_min_clipped, np.float32 if dtype == torch.float32 else np.float64)
        self.sigmas = torch.from_numpy(sig)
        self.n = n_steps
        self.x0 = None

    def coefficients(self, i):
        return coefficients(self.sigmas, i, self.solver_order)

    def step(self, i, model_output, x):
        prev, self.x0 = step(self.coefficients(i), self.prediction_type, self.thresholding, model_output, x,
                             self.x0 if i > 0 else None)
        return prev


# -- the problem with a closed-form answer -------------------------------------------------------------------------------
def linear_denoiser(x, alpha, sigma, s):
    """E[x0 | x_t] for per-element data ~ N(0, s^2) and x_t = alpha x0 + sigma eps."""
    return (alpha * s * s / (alpha * alpha * s * s + sigma * sigma)) * x


def exact_end(x_T, alpha_T, sigma_T, s):
    """Along the probability-flow ODE x_t / sqrt(alpha_t^2 s^2 + sigma_t^2) is constant; at the end alpha = 1, sigma = 0."""
    return x_T * s / (alpha_T * alpha_T * s * s + sigma_T * sigma_T) ** 0.5


def analytic_error(n_steps: int, solver_order: int, s: float, x_T: Optional[torch.Tensor] = None) -> float:
    """Relative error of the fp64 restatement at the end of an n-step loop on the linear problem (N = 100 squaredcos_cap_v2,
    lambda_min_clipped = -5.1, `sample` prediction, no thresholding)."""
    sol = Solver(n_steps, solver_order=solver_order, lambda_min_clipped=-5.1, dtype=torch.float64)
    x = torch.ones(1, dtype=torch.float64) if x_T is None else x_T.double()
    a_T, s_T = _alpha_sigma(sol.sigmas[0])
    want = exact_end(x, a_T, s_T, s)
    for i in range(n_steps):
        a, sg = _alpha_sigma(sol.sigmas[i])
        x = sol.step(i, linear_denoiser(x, a, sg, s), x)
    return float((x - want).norm() / want.norm())


# -- the callers' loop on the CPU oracle ---------------------------------------------------------------------------------
def generate_traj(sd, image, init_trajs, target, *, use_cond: str, n_steps: int, free_scale: float = 1.0,
                  prediction_type="sample", thresholding=True, solver_order=2, lambda_min_clipped=-math.inf, n_train=100,
                  dim: int = 64, dim_mults: Sequence[int] = (1, 2, 4, 8), scale_xy: bool = True) -> torch.Tensor:
    """The agent's sampling loop (as oracle/sampling.py:generate_traj drives it) on the fp32 restatement, NO and FREE guidance."""
    assert use_cond in (U.NO_GUIDANCE, U.FREE_GUIDANCE)
    sol = Solver(n_steps, n_train=n_train, prediction_type=prediction_type, thresholding=thresholding,
                 solver_order=solver_order, lambda_min_clipped=lambda_min_clipped)
    trajs = init_trajs.clone().detach()
    cond = None
    if target is not None and use_cond == U.FREE_GUIDANCE:
        tg = target if target.dim() > 1 else target.repeat(trajs.size(0), 1)
        cond = torch.cat([tg, torch.zeros_like(tg)], dim=0)
    feat = resnet34_forward(sd, "perception.", image)
    trajs[:, 0, :3] = 0.0
    with torch.no_grad():
        for i, t in enumerate(torch.from_numpy(sol.timesteps)):
            if use_cond == U.FREE_GUIDANCE:
                out = U.unet_forward(sd, torch.cat([trajs, trajs], dim=0), image, t.reshape(-1), cond, use_cond=use_cond, dim=dim,
                                     dim_mults=dim_mults, img_feature=feat)
                c, u = out.chunk(2, dim=0)
                model_output = u + free_scale * (c - u)
            else:
                model_output = U.unet_forward(sd, trajs, image, t.reshape(-1).repeat(trajs.shape[0]), use_cond=use_cond, dim=dim, dim_mults=dim_mults,
                                              img_feature=feat)
            trajs = sol.step(i, model_output, trajs)
            trajs[:, 0, :3] = 0.0
    trajs = trajs.to(torch.float32).clamp(-1, 1)
    if scale_xy:
        trajs[..., :2] *= MAGIC_NUM
    return trajs
