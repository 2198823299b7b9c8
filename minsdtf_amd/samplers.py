"""Multistep and ancestral samplers of the denoise loop: DPM++ 2M, DPM++ 2M SDE and Euler ancestral, optionally on Karras
sigmas (``generate_image(..., sampler="dpmpp_2m_karras")``).

These are k-diffusion's algorithms (sample_dpmpp_2m, sample_dpmpp_2m_sde with eta 1 and the midpoint correction,
sample_euler_ancestral with eta 1) rewritten for the variance-preserving latent this code keeps, x = alpha * x_k.  For the
executed evaluation i, with k-diffusion sigma s_i, alpha_i = 1 / sqrt(1 + s_i^2), sigma_i = s_i alpha_i (the VP signal and
noise rates: Scheduler.signal_rates[t] / noise_rates[t] at integer t), s = 0 after the last evaluation,
lambda = -log s, h_i = lambda_{i+1} - lambda_i, r_i = h_{i-1} / h_i:

    D  = (x - sigma_i e) / alpha_i            e: the UNet's guided (CFG + rescale) noise prediction
    x' = c_x x + c_D D + c_P P + c_z z        P: the previous evaluation's D;  z: this step's N(0,1) draw;  then P <- D

and the fp32 row the device kernel (msd_sampler_step) indexes with its step counter is {alpha_i, sigma_i, c_x, c_D, c_P, c_z, 0, 0}.
Every coefficient is computed here in float64 ("Samplers", has the table).  On the last row every sampler gives
x' = D.  The per-step draws are made on the host for the global batch, sample-major (``draw_step_noise``): with a seed they
come from ``default_rng([seed, 1])``, so a picture does not depend on the batch size or the number of ranks; they are not
k-diffusion's Brownian-tree draws, so pictures do not match k-diffusion's for the same seed.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

KINDS = ("dpmpp_2m", "dpmpp_2m_sde", "euler_a")
STOCHASTIC = ("dpmpp_2m_sde", "euler_a")
KARRAS_RHO = 7.0
ROW = 8   # coefficient row width: {alpha, sigma, c_x, c_D, c_P, c_z, 0, 0}


@dataclass(frozen=True)
class SamplerSpec:
    name: str      # as given: "<kind>" or "<kind>_karras"
    kind: str      # one of KINDS
    karras: bool

    @property
    def stochastic(self) -> bool:
        return self.kind in STOCHASTIC


def names():
    """Every accepted sampler name."""
    return [k + s for k in KINDS for s in ("", "_karras")]


def parse(name) -> Optional[SamplerSpec]:
    """None -> None (the default sampler); a known name -> its spec; anything else raises ValueError."""
    if name is None:
        return None
    if isinstance(name, SamplerSpec):
        return name
    if not isinstance(name, str):
        raise ValueError(f"sampler must be a string or None, not {type(name).__name__}")
    karras = name.endswith("_karras")
    kind = name[:-len("_karras")] if karras else name
    if kind not in KINDS:
        raise ValueError(f"unknown sampler {name!r}: choose one of {', '.join(names())} (or None for the default)")
    return SamplerSpec(name, kind, karras)


def training_sigmas(scheduler) -> np.ndarray:
    """k-diffusion sigma of every training timestep, float64: noise_rate / signal_rate = sqrt((1 - abar) / abar)."""
    return np.asarray(scheduler.noise_rates, dtype=np.float64) / np.asarray(scheduler.signal_rates, dtype=np.float64)


def karras_sigmas(n: int, s_min: float, s_max: float, rho: float = KARRAS_RHO) -> np.ndarray:
    """Karras et al. (2022) eq. 5: s_i = (s_max^(1/rho) + i/(n-1) (s_min^(1/rho) - s_max^(1/rho)))^rho, i = 0 .. n-1."""
    ramp = np.linspace(0.0, 1.0, n) if n > 1 else np.zeros(1)
    hi, lo = s_max ** (1.0 / rho), s_min ** (1.0 / rho)
    return (hi + ramp * (lo - hi)) ** rho


def sigma_to_t(sigmas, train_sigmas) -> np.ndarray:
    """Fractional timestep of each sigma: piecewise-linear interpolation of log sigma over the training log-sigmas (increasing
    with t), as k-diffusion's DiscreteSchedule.sigma_to_t; clamped to [0, len - 1]."""
    ls = np.log(np.asarray(train_sigmas, dtype=np.float64))
    return np.interp(np.log(np.asarray(sigmas, dtype=np.float64)), ls, np.arange(len(ls), dtype=np.float64))


@dataclass(frozen=True)
class Schedule:
    spec: SamplerSpec
    timesteps: np.ndarray   # float64 [n]: the UNet's time input per evaluation (fractional for Karras)
    sigmas: np.ndarray      # float64 [n + 1]: k-diffusion sigma per evaluation, then 0

    @property
    def num_steps(self) -> int:
        return len(self.timesteps)

    @property
    def alphas(self) -> np.ndarray:   # [n + 1]
        return 1.0 / np.sqrt(1.0 + self.sigmas ** 2)

    @property
    def noise_rates(self) -> np.ndarray:   # [n + 1]
        return self.sigmas * self.alphas

    def entry_latent(self, k: int, encoded, noise) -> np.ndarray:
        """img2img / inpaint: the latent at the first executed evaluation k, alpha_k encoded + sigma_k noise (k-diffusion's
        convention; the default sampler keeps the reference's)."""
        a, s = float(self.alphas[k]), float(self.noise_rates[k])
        B = noise.shape[0]
        return a * np.repeat(np.asarray(encoded), B // np.asarray(encoded).shape[0], axis=0) + s * np.asarray(noise)


def schedule(spec: SamplerSpec, scheduler, num_steps: int) -> Schedule:
    """Plain names: the reference's own timesteps (Scheduler.set_timesteps: linspace(0, 1000, n, endpoint=False), descending)
    and their sigmas.  `_karras`: Karras sigmas between s(999) and s(0) of the training schedule, at fractional timesteps."""
    n = int(num_steps)
    if n < 1:
        raise ValueError("num_steps must be >= 1")
    train = training_sigmas(scheduler)
    if spec.karras:
        s = karras_sigmas(n, float(train[0]), float(train[-1]))
        t = sigma_to_t(s, train)
    else:
        t = np.linspace(0, len(train), n, dtype=np.int32, endpoint=False)[::-1].astype(np.float64)
        s = train[t.astype(np.int64)]
    return Schedule(spec, np.ascontiguousarray(t), np.append(s, 0.0))


def rows(sched: Schedule, start: int = 0) -> np.ndarray:
    """float64 [n][8] = {alpha_i, sigma_i, c_x, c_D, c_P, c_z, 0, 0} for a run whose first executed evaluation is `start`
    (that row never reads P; rows before it are never executed and are left with alpha 1, everything else 0)."""
    n, kind = sched.num_steps, sched.spec.kind
    s, a, sg = sched.sigmas, sched.alphas, sched.noise_rates
    out = np.zeros((n, ROW), dtype=np.float64)
    out[:start, 0] = 1.0
    h_prev = None
    for i in range(start, n):
        out[i, 0], out[i, 1] = a[i], sg[i]
        if i == n - 1:   # s_{i+1} = 0: x' = D for every sampler
            out[i, 3] = 1.0
            continue
        h = np.log(s[i]) - np.log(s[i + 1])
        first = h_prev is None
        if kind == "dpmpp_2m":
            phi = -a[i + 1] * np.expm1(-h)
            cx, cd, cp, cz = sg[i + 1] / sg[i], phi, 0.0, 0.0
            if not first:
                r = h_prev / h
                cd, cp = phi * (1.0 + 1.0 / (2.0 * r)), -phi / (2.0 * r)
        elif kind == "dpmpp_2m_sde":
            psi = -a[i + 1] * np.expm1(-2.0 * h)
            cx, cd, cp = (sg[i + 1] / sg[i]) * np.exp(-h), psi, 0.0
            if not first:
                r = h_prev / h
                cd, cp = psi * (1.0 + 1.0 / (2.0 * r)), -psi / (2.0 * r)
            cz = sg[i + 1] * np.sqrt(-np.expm1(-2.0 * h))
        else:   # euler_a
            s_up = min(s[i + 1], np.sqrt(s[i + 1] ** 2 * (s[i] ** 2 - s[i + 1] ** 2) / s[i] ** 2))
            s_dn = np.sqrt(s[i + 1] ** 2 - s_up ** 2)
            cx, cd, cp, cz = (a[i + 1] / a[i]) * (s_dn / s[i]), a[i + 1] * (1.0 - s_dn / s[i]), 0.0, a[i + 1] * s_up
        out[i, 2:6] = (cx, cd, cp, cz)
        h_prev = h
    return out


def coefficient_table(sched: Schedule, start: int = 0) -> np.ndarray:
    """The fp32 [n][8] table msd_sampler_step indexes with the device step counter."""
    return rows(sched, start).astype(np.float32)


def host_step(row, x, e, prev, z=None):
    """One step in float64 on host arrays (the host_loop=True path): returns (x', D).  `prev` is the previous D (ignored
    where c_P = 0), `z` this step's draw (ignored where c_z = 0)."""
    alpha, sigma, cx, cd, cp, cz = (float(v) for v in row[:6])
    x = np.asarray(x, dtype=np.float64)
    d = (x - sigma * np.asarray(e, dtype=np.float64)) / alpha
    out = cx * x + cd * d
    if cp != 0.0:
        out = out + cp * prev
    if cz != 0.0 and z is not None:
        out = out + cz * np.asarray(z, dtype=np.float64)
    return out, d


def draw_step_noise(batch: int, num_steps: int, h: int, w: int, seed=None, stream_key: int = 1) -> np.ndarray:
    """The stochastic samplers' N(0,1) draws for the GLOBAL batch, sample-major: (batch, num_steps, h, w, 4) float32, one
    block per row of the table (executed or not).  With a seed: default_rng([seed, stream_key]) (1: a job's own loop; 3: the
    second pass of a hires job; 2 is the hires re-noise draw, hires.draw_noise); without: numpy's global stream (as the TCD
    sampler's).  Sample b's draws are the b-th block whatever the batch size."""
    shape = (int(batch), int(num_steps), int(h), int(w), 4)
    if seed is None:
        return np.random.randn(*shape).astype(np.float32)
    return np.random.default_rng([int(seed), int(stream_key)]).standard_normal(shape).astype(np.float32)
