"""Samplers of the denoising loop: the step plan, pure host arithmetic, and the specification of the fused
DPM-Solver++(2M) step (step_reference below: torch, on whatever device the tensors live; the GPU path is csrc/sampler.hip).

The reference samples with first-order EDM Euler ("euler": model_diffusion_renderer.py:30-82, this project's default, whose loop
and kernels this file does not touch).  "dpmpp_2m" is DPM-Solver++(2M) (Lu et al. 2022; k-diffusion's sample_dpmpp_2m): an
exponential integrator of the data-prediction ODE that keeps ONE history tensor, the previous step's denoised estimate D, and
costs one model evaluation per step like Euler.  With t = -log(sigma), h = log(sigma / sigma_next), e = -expm1(-h) = 1 -
sigma_next / sigma and r = h_last / h = log(sigma_prev / sigma) / h:

    first step          x' = (sigma_next / sigma) x + e D                                   (first order: Euler's own step)
    middle step         x' = (sigma_next / sigma) x + e ((1 + 1 / 2r) D - (1 / 2r) D_prev)
    sigma_next == 0     x' = D                                                              (Euler's last step)

D is the EDM-preconditioned estimate c_skip x + c_out m of the network output m, with the scheduler's own fp32 scalars, so it
has Euler's bits.  The loop keeps x in bf16, as the reference does, and D in fp32.
"""
import math
from typing import List, NamedTuple, Optional

import torch

SAMPLERS = ("euler", "dpmpp_2m")


class Step(NamedTuple):
    c_in: float                  # the scheduler's fp32 scalars of this step (CleanEDMEulerScheduler.step_scalars) ...
    c_skip: float
    c_out: float
    a: float                     # ... and x' = state_dtype(a x + b1 D + b0 D_prev): float64 arithmetic, rounded to fp32 once
    b1: float
    b0: float
    has_hist: bool               # whether D_prev is read at all (b0 is 0 where it is not)
    c_in_next: Optional[float]   # c_in of the following step (the fused step writes that step's model input); None on the last


def check_sampler(sampler, tile_join="pixel"):
    """ValueError for a sampler that does not exist or cannot be honoured, from settings alone (so before any GPU work)."""
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler must be one of {SAMPLERS}, got {sampler!r}")
    if sampler != "euler" and tile_join == "latent":
        raise ValueError(f"tile_join = 'latent' with sampler = {sampler!r} is not implemented (every tile would need a history of "
                         "its own): set sampler = 'euler' or tile_join = 'pixel'")


def _f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float64).to(torch.float32))


def plan_steps(sigmas, sigma_data: float, kind: str = "dpmpp_2m") -> List[Step]:
    """One Step per denoising step of the scheduler's fp32 table `sigmas` (strictly decreasing, positive, then the trailing 0).
    kind "dpmpp_2m": the rules above.  kind "euler": every step first order - (sigma_next / sigma, 1 - sigma_next / sigma, 0), the
    EDM Euler step written in this file's form - which is what the convergence table compares against; the loop under
    sampler = "euler" never asks for a plan."""
    if kind not in SAMPLERS:
        raise ValueError(f"sampler must be one of {SAMPLERS}, got {kind!r}")
    table = torch.as_tensor(sigmas, dtype=torch.float32).detach().to("cpu").reshape(-1)
    sg = [float(v) for v in table]
    if len(sg) < 2 or sg[-1] != 0.0 or not all(math.isfinite(v) and v > 0 for v in sg[:-1]) \
            or any(b >= a for a, b in zip(sg, sg[1:])):
        raise ValueError(f"sigmas must be a strictly decreasing positive table with a trailing 0, got {sg}")
    sd = sigma_data
    scal = []
    for sigma in table[:-1]:
        # the scheduler's own fp32 torch expressions (CleanEDMEulerScheduler.step_scalars)
        c_in = 1 / torch.sqrt(sigma ** 2 + sd ** 2)
        c_skip = sd ** 2 / (sigma ** 2 + sd ** 2)
        c_out = (sigma * sd) / torch.sqrt(sigma ** 2 + sd ** 2)
        scal.append((float(c_in), float(c_skip), float(c_out)))
    plan = []
    for i in range(len(sg) - 1):
        s, sn = sg[i], sg[i + 1]
        if sn == 0.0:
            a, b1, b0, has_hist = 0.0, 1.0, 0.0, False
        else:
            a = sn / s
            h = math.log(s / sn)
            e = -math.expm1(-h)
            if kind == "euler":
                b1, b0, has_hist = 1.0 - sn / s, 0.0, False
            elif i == 0:
                b1, b0, has_hist = e, 0.0, False
            else:
                r = math.log(sg[i - 1] / s) / h
                b1, b0, has_hist = e * (1.0 + 1.0 / (2.0 * r)), -e / (2.0 * r), True
        plan.append(Step(*scal[i], _f32(a), _f32(b1), _f32(b0), has_hist, scal[i + 1][0] if i + 2 < len(sg) else None))
    return plan


def _step_torch(cond, uncond, guidance, x, hist, coef: Step, copies, state_dtype):
    """The specification.  state_dtype bf16: fp32 arithmetic, every operation rounded on its own (torch never fuses two ops), the
    bf16 roundings of cfg_kernel's chain, one rounding of the new latent, the scaled input from the ROUNDED latent.  state_dtype
    float64: the same expressions in float64 with no bf16 rounding anywhere."""
    if state_dtype == torch.float64:
        wide, rnd = (lambda t: t.to(torch.float64)), (lambda t: t)
    else:
        wide, rnd = (lambda t: t.to(torch.float32)), (lambda t: t.to(torch.bfloat16).to(torch.float32))
    c = wide(cond)
    m = c
    if uncond is not None:
        d = rnd(c - wide(uncond))
        gd = rnd(d * float(guidance))
        m = rnd(c + gd)
    xf = wide(x)
    D = xf * coef.c_skip + m * coef.c_out
    s = D * coef.b1
    if coef.has_hist:
        s = s + wide(hist) * coef.b0
    x_new = (xf * coef.a + s).to(state_dtype)
    scaled = None
    if coef.c_in_next is not None:
        one = (wide(x_new) * coef.c_in_next).to(state_dtype)
        scaled = torch.cat([one] * copies, 0).contiguous()
    return x_new, D, scaled


def step_reference(cond: torch.Tensor, uncond: Optional[torch.Tensor], guidance: float, x: torch.Tensor,
                   hist: Optional[torch.Tensor], coef: Step, copies: int = 1, state_dtype: torch.dtype = torch.bfloat16,
                   backend: str = "auto", hist_out: Optional[torch.Tensor] = None):
    """One step of the plan: cond (and uncond, or None for no CFG) the network's outputs and x the latent, all [P, ...] of
    state_dtype; hist the previous step's denoised estimate (fp32; float64 under state_dtype float64), never read where
    coef.has_hist is false (None is fine there).  -> (the new latent, the denoised estimate = the next step's history, the next
    step's model input [copies * P, ...] = the new latent times coef.c_in_next, `copies` (1, or 2 under CFG) times along the batch,
    or None on the last step).  hist_out: a tensor that receives the denoised estimate and is returned as such; it may be `hist`.

    backend: 'auto' = the HIP kernel (drn_sampler_step_2m, one launch) on GPU tensors and torch on CPU tensors; 'torch' / 'hip'
    force a path ('hip' needs GPU tensors and the bf16 state).  The torch path is the specification and what CPU devices run."""
    if backend not in ("auto", "torch", "hip"):
        raise ValueError(f"unknown backend {backend!r}")
    if state_dtype not in (torch.bfloat16, torch.float64):
        raise ValueError(f"state_dtype is torch.bfloat16 (the loop's) or torch.float64 (no rounding), got {state_dtype}")
    if copies not in (1, 2):
        raise ValueError(f"copies must be 1 or 2, got {copies}")
    if coef.has_hist and hist is None:
        raise ValueError("this step reads the previous denoised estimate: hist is needed")
    for name, t in (("cond", cond), ("uncond", uncond), ("hist", hist if coef.has_hist else None), ("hist_out", hist_out)):
        if t is not None and (tuple(t.shape) != tuple(x.shape) or t.device != x.device):
            raise ValueError(f"{name} {tuple(t.shape)} on {t.device} and x {tuple(x.shape)} on {x.device} are not one latent on "
                             "one device")
    if backend == "hip" and not x.is_cuda:
        raise ValueError(f"backend='hip' needs a GPU tensor, got one on {x.device} (the torch path is what CPU devices run)")
    if backend == "hip" and state_dtype != torch.bfloat16:
        raise ValueError("backend='hip' steps the bf16 state (the float64 form is the torch specification's)")
    if backend == "torch" or not x.is_cuda or state_dtype != torch.bfloat16:
        x_new, D, scaled = _step_torch(cond, uncond, guidance, x, hist, coef, copies, state_dtype)
        if hist_out is not None:
            D = hist_out.copy_(D)
        return x_new, D, scaled
    from . import native
    if hist_out is None:
        hist_out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    x_new, scaled = native.sampler_step_2m(cond.contiguous(), None if uncond is None else uncond.contiguous(), float(guidance),
                                           x.contiguous(), hist.contiguous() if coef.has_hist else None, hist_out, coef.c_skip,
                                           coef.c_out, coef.a, coef.b1, coef.b0, coef.c_in_next, copies)
    return x_new, hist_out, scaled
