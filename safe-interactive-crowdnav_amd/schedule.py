"""Diffusion noise schedule and the DDIM step table (host side).

Follows ``VarianceSchedule`` (``sicnav_diffusion/JMID/MID/models/diffusion.py:12-64``) as
built by ``MID._build_model`` (``MID/mid.py:1281-1283``: ``num_steps=100, beta_1=1e-4,
beta_T=5e-2, mode="linear"``), including its fp32 sequential accumulation of
``log(alpha)`` (``diffusion.py:36-39``), and the step enumeration of
``DiffusionTraj.sample_sicnav_inference`` (``diffusion.py:507-528``).

torch is used only for bit-identical fp32 ``linspace``/``log``/``exp`` on the host.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import numpy as np
import torch


@dataclass(frozen=True)
class VarianceSchedule:
    betas: np.ndarray        # [num_steps+1] f32, betas[0] = 0 (padding)
    alphas: np.ndarray       # [num_steps+1] f32
    alpha_bars: np.ndarray   # [num_steps+1] f32
    num_steps: int
    sigmas_inflex: np.ndarray = None   # [num_steps+1] f32 (DDPM, flexibility 0; diffusion.py:41-47)
    sigmas_flex: np.ndarray = None     # [num_steps+1] f32 = sqrt(betas) (flexibility 1; diffusion.py:41)

    @classmethod
    def linear(cls, num_steps: int = 100, beta_1: float = 1e-4, beta_T: float = 5e-2) -> "VarianceSchedule":
        betas = torch.linspace(beta_1, beta_T, steps=num_steps)
        betas = torch.cat([torch.zeros([1]), betas], dim=0)
        alphas = 1 - betas
        log_alphas = torch.log(alphas)
        for i in range(1, log_alphas.size(0)):
            log_alphas[i] += log_alphas[i - 1]
        alpha_bars = log_alphas.exp()
        sigmas_flex = torch.sqrt(betas)
        sigmas_inflex = torch.zeros_like(betas)
        for i in range(1, betas.size(0)):
            sigmas_inflex[i] = ((1 - alpha_bars[i - 1]) / (1 - alpha_bars[i])) * betas[i]
        sigmas_inflex = torch.sqrt(sigmas_inflex)
        return cls(betas.numpy().copy(), alphas.numpy().copy(), alpha_bars.numpy().copy(), num_steps,
                   sigmas_inflex.numpy().copy(), sigmas_flex.numpy().copy())


def loss_tables(sched: VarianceSchedule):
    """The forward process per timestep, as ``DiffusionTraj.get_loss`` reads it (``diffusion.py:453-457``): ``(beta, c0, c1)`` float32
    [num_steps + 1] with ``c0 = sqrt(alpha_bar)``, ``c1 = sqrt(1 - alpha_bar)`` in torch fp32; index = timestep, entry 0 the padding
    entry.  What ``jmid_set_loss_schedule`` takes."""
    ab = torch.from_numpy(np.ascontiguousarray(sched.alpha_bars, dtype=np.float32))
    return (np.ascontiguousarray(sched.betas, dtype=np.float32), torch.sqrt(ab).numpy().copy(), torch.sqrt(1 - ab).numpy().copy())


@dataclass(frozen=True)
class DDIMStep:
    t: int
    beta: np.float32
    # x0 = (x - e*c_e)/c_x ; x_next = n_x*x0 + n_e*e
    c_e: np.float32    # sqrt(1 - abar_t)
    c_x: np.float32    # sqrt(abar_t)
    n_x: np.float32    # sqrt(abar_{t-stride})
    n_e: np.float32    # sqrt(1 - abar_{t-stride})


def ddim_steps(sched: VarianceSchedule, step: int) -> List[DDIMStep]:
    """Steps of the reverse loop for ``step`` (the reference's ``step_size`` config key).

    ``stride = int(100 / step)`` and ``t = num_steps, num_steps-stride, ... > 0``
    (``diffusion.py:507-508``).  Configs whose stride does not divide ``num_steps``
    would index ``alpha_bars[t - stride]`` with a negative index in the reference
    (Python wrap-around); they are rejected here.
    """
    if step <= 0:
        raise ValueError("step must be positive")
    stride = int(100 / step)
    if stride <= 0 or sched.num_steps % stride != 0:
        raise ValueError(
            f"step={step} gives stride {stride}, which does not divide num_steps={sched.num_steps}; "
            "the reference would wrap alpha_bars[t-stride] around (undefined schedule)"
        )
    out = []
    ab = torch.from_numpy(sched.alpha_bars)
    for t in range(sched.num_steps, 0, -stride):
        a_t, a_n = ab[t], ab[t - stride]
        out.append(
            DDIMStep(
                t=t,
                beta=np.float32(sched.betas[t]),
                c_e=np.float32((1 - a_t).sqrt().item()),
                c_x=np.float32(a_t.sqrt().item()),
                n_x=np.float32(a_n.sqrt().item()),
                n_e=np.float32((1 - a_n).sqrt().item()),
            )
        )
    return out


@dataclass(frozen=True)
class DDPMStep:
    t: int
    beta: np.float32
    c0: np.float32       # 1/sqrt(alpha_t)
    c1: np.float32       # (1 - alpha_t)/sqrt(1 - abar_t)
    sigma: np.float32    # get_sigmas(t, flexibility) (diffusion.py:59-64)
    noise: bool          # z ~ N(0,1) is used (t > 1), else zeros     (diffusion.py:509)


def ddpm_steps(sched: VarianceSchedule, step: int, flexibility: float = 0.0) -> List[DDPMStep]:
    """x_next = c0*(x - c1*e) + sigma*z  (``sampling="ddpm"``, diffusion.py:509-522), same step enumeration as DDIM;
    sigma = sigmas_flex[t]*flexibility + sigmas_inflex[t]*(1 - flexibility) (``get_sigmas``, diffusion.py:59-64)."""
    if not 0.0 <= flexibility <= 1.0:
        raise ValueError("flexibility must be in [0, 1]")
    if step <= 0:
        raise ValueError("step must be positive")
    stride = int(100 / step)
    if stride <= 0 or sched.num_steps % stride != 0:
        raise ValueError(f"step={step}: stride {stride} does not divide num_steps={sched.num_steps}")
    al, ab = torch.from_numpy(sched.alphas), torch.from_numpy(sched.alpha_bars)
    sg = torch.from_numpy(sched.sigmas_flex) * flexibility + torch.from_numpy(sched.sigmas_inflex) * (1 - flexibility)
    out = []
    for t in range(sched.num_steps, 0, -stride):
        out.append(DDPMStep(t=t, beta=np.float32(sched.betas[t]), c0=np.float32((1.0 / torch.sqrt(al[t])).item()),
                            c1=np.float32(((1 - al[t]) / torch.sqrt(1 - ab[t])).item()), sigma=np.float32(sg[t].item()),
                            noise=t > 1))
    return out


def guidance_weights(scale: float = 0.02, step: int = 50, sched: VarianceSchedule = None, table: str = "alpha_bar") -> np.ndarray:
    """The per-entry weights of guided sampling (``jmid_denoise_guided``: metres, one per entry of the DDIM table of ``step``) -> float64
    [n_steps].  ``table="alpha_bar"`` (the default): ``weights[i] = scale * alpha_bar`` of the timestep the state is at AFTER entry i
    (``t - stride``) - about 0 on pure noise, where integrated noise is not a path worth pushing, and ``scale`` behind the last entry
    (alpha_bar[0] = 1).  ``table="last_half"``: 0 behind the first half of the entries, ``scale`` behind the rest.  ``table="flat"``:
    ``scale`` everywhere.  ``scale`` defaults to the repair's step, 0.02 m."""
    if not (np.isfinite(scale) and scale >= 0.0):
        raise ValueError("scale must be finite and >= 0")
    sched = sched or VarianceSchedule.linear()
    tab = ddim_steps(sched, step)
    stride = int(100 / step)
    n = len(tab)
    if table == "alpha_bar":
        w = [float(scale) * float(sched.alpha_bars[s.t - stride]) for s in tab]
    elif table == "last_half":
        w = [0.0 if i < n // 2 else float(scale) for i in range(n)]
    elif table == "flat":
        w = [float(scale)] * n
    else:
        raise ValueError("table must be 'alpha_bar', 'last_half' or 'flat'")
    return np.asarray(w, dtype=np.float64)
