"""Hires fix: two-pass text-to-image with an on-device latent upscale (``generate_image(..., hires=...)``).

Pass 1 denoises at the pipeline's own size, the latent is resampled to the target size and re-noised part of the way in one
launch (``msd_latent_resample``), pass 2 finishes the denoising at the target size.  This module is the host side of it and
needs no GPU: the job description (``HiresSpec`` / ``parse``), the resampler's tap tables (``taps`` / ``pack_rows``) and the
pass-2 entry point (``entry``).

Resampling follows ``torch.nn.functional.interpolate(x, size=..., mode=..., align_corners=False)`` exactly (upscaling only, so
antialiasing would change nothing and is not offered): per output coordinate of an axis, up to four source indices (already
clamped to the source: replicate border, clamped per tap) and their weights, computed here in float64.  The device reads them
as fp32 rows ``{int32 idx[4], float w[4]}``; unused taps carry weight 0.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

UPSCALERS = ("nearest", "nearest-exact", "bilinear", "bicubic")
TAPS = 4             # taps per output coordinate and axis
ROW_BYTES = 32       # one device row: int32 idx[4], float w[4]  (MsdResampleRow)
BICUBIC_A = -0.75    # torch's cubic convolution coefficient


@dataclass(frozen=True)
class HiresSpec:
    """A hires job: the target size as ``scale`` (of the pipeline's own size) or as ``size = (height, width)`` in pixels,
    ``steps`` of the pass-2 schedule (None: the job's num_steps), of which the last int(steps * strength + 0.5) run, and the
    latent ``upscaler`` (one of UPSCALERS)."""
    scale: Optional[float] = None
    size: Optional[Tuple[int, int]] = None
    steps: Optional[int] = None
    strength: float = 0.6
    upscaler: str = "bilinear"


@dataclass(frozen=True)
class HiresJob:
    """A HiresSpec resolved against a pipeline size and a job's num_steps."""
    height: int
    width: int
    steps: int
    strength: float
    upscaler: str

    @property
    def run_steps(self) -> int:
        return int(self.steps * self.strength + 0.5)


def parse(hires, base_height: int, base_width: int, num_steps: int) -> Optional[HiresJob]:
    """None -> None; a HiresSpec or a dict of its fields -> the resolved job.  ValueError for an unknown upscaler, a target
    that is not a multiple of 64, is smaller than the base in either dimension or equals the base (nothing to upscale: the
    two engines and the hand-off's source and destination would be the same), a strength outside (0, 1), steps < 1."""
    if hires is None:
        return None
    if isinstance(hires, dict):
        unknown = set(hires) - {"scale", "size", "steps", "strength", "upscaler"}
        if unknown:
            raise ValueError(f"hires: unknown field(s) {sorted(unknown)}")
        hires = HiresSpec(**hires)
    if not isinstance(hires, HiresSpec):
        raise ValueError(f"hires must be a HiresSpec, a dict or None, not {type(hires).__name__}")
    if hires.upscaler not in UPSCALERS:
        raise ValueError(f"hires: unknown upscaler {hires.upscaler!r}: choose one of {', '.join(UPSCALERS)}")
    if (hires.scale is None) == (hires.size is None):
        raise ValueError("hires: give the target as exactly one of `scale` and `size` = (height, width)")
    if hires.size is not None:
        try:
            th, tw = (int(v) for v in hires.size)
        except (TypeError, ValueError) as e:
            raise ValueError(f"hires: size must be (height, width), got {hires.size!r}") from e
        if (th, tw) != tuple(hires.size):
            raise ValueError(f"hires: size must be whole pixels, got {hires.size!r}")
    else:
        fh, fw = float(hires.scale) * base_height, float(hires.scale) * base_width
        th, tw = int(round(fh)), int(round(fw))
        if abs(fh - th) > 1e-6 or abs(fw - tw) > 1e-6:
            raise ValueError(f"hires: scale {hires.scale} of {base_height}x{base_width} is not a whole number of pixels")
    if th % 64 or tw % 64:
        raise ValueError(f"hires: the target {th}x{tw} must be a multiple of 64 in both dimensions")
    if th < base_height or tw < base_width:
        raise ValueError(f"hires: the target {th}x{tw} is smaller than the base {base_height}x{base_width} (upscaling only)")
    if (th, tw) == (base_height, base_width):
        raise ValueError(f"hires: the target {th}x{tw} is the pipeline's own size: nothing to upscale (run the plain job)")
    strength = float(hires.strength)
    if not 0.0 < strength < 1.0:
        raise ValueError(f"hires: strength {hires.strength} is outside (0, 1)")
    steps = int(num_steps if hires.steps is None else hires.steps)
    if steps < 1:
        raise ValueError(f"hires: steps {steps} < 1")
    return HiresJob(th, tw, steps, strength, hires.upscaler)


def _cubic_inner(x, a=BICUBIC_A):   # |x| <= 1
    return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0


def _cubic_outer(x, a=BICUBIC_A):   # 1 < |x| < 2
    return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a


def taps(n_in: int, n_out: int, mode: str):
    """The tap table of one axis: (idx int32 [n_out][4], w float64 [n_out][4]) with
    out[o] = sum_j w[o][j] * in[idx[o][j]]  ==  interpolate(in, size=n_out, mode=mode, align_corners=False) along that axis.
    Every index lies in [0, n_in); unused taps repeat a valid index with weight 0; the weights of a row sum to 1."""
    n_in, n_out = int(n_in), int(n_out)
    if mode not in UPSCALERS:
        raise ValueError(f"unknown upscaler {mode!r}: choose one of {', '.join(UPSCALERS)}")
    if n_in < 1 or n_out < n_in:
        raise ValueError(f"taps: {n_in} -> {n_out} (upscaling only)")
    idx = np.zeros((n_out, TAPS), dtype=np.int64)
    w = np.zeros((n_out, TAPS), dtype=np.float64)
    o = np.arange(n_out)
    if mode in ("nearest", "nearest-exact"):
        # torch computes the source index in fp32: floor(o * scale) (the legacy rule) / floor((o + 0.5) * scale), scale = in / out
        scale = np.float32(n_in) / np.float32(n_out)
        pos = o.astype(np.float32) + (np.float32(0.5) if mode == "nearest-exact" else np.float32(0.0))
        src = np.minimum(np.floor(pos * scale).astype(np.int64), n_in - 1)
        idx[:] = src[:, None]
        w[:, 0] = 1.0
    else:
        scale = n_in / n_out
        src = scale * (o + 0.5) - 0.5
        if mode == "bilinear":
            src = np.maximum(src, 0.0)
            i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
            i1 = np.minimum(i0 + 1, n_in - 1)
            lam = np.clip(src - i0, 0.0, 1.0)
            idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3] = i0, i1, i1, i1
            w[:, 0], w[:, 1] = 1.0 - lam, lam
        else:   # bicubic: four taps around floor(src), each clamped to the source on its own
            i0 = np.floor(src).astype(np.int64)
            t = src - i0
            for j in range(TAPS):
                idx[:, j] = np.clip(i0 - 1 + j, 0, n_in - 1)
            w[:, 0], w[:, 1] = _cubic_outer(t + 1.0), _cubic_inner(t)
            w[:, 2], w[:, 3] = _cubic_inner(1.0 - t), _cubic_outer(2.0 - t)
    return idx.astype(np.int32), w


def pack_rows(idx: np.ndarray, w: np.ndarray) -> np.ndarray:
    """The device form of a tap table: int32 [n][8], row = {idx[4], the fp32 bits of w[4]} (MsdResampleRow, 32 bytes)."""
    n = idx.shape[0]
    out = np.empty((n, 2 * TAPS), dtype=np.int32)
    out[:, :TAPS] = idx
    out[:, TAPS:] = np.ascontiguousarray(w, dtype=np.float32).view(np.int32)
    return out


def resample_host(x: np.ndarray, h_out: int, w_out: int, mode: str) -> np.ndarray:
    """float64 resample of an NHWC array through the tap tables (the host restatement of msd_latent_resample's sum)."""
    x = np.asarray(x, dtype=np.float64)
    iy, wy = taps(x.shape[1], h_out, mode)
    ix, wx = taps(x.shape[2], w_out, mode)
    rows = sum(wx[None, None, :, j, None] * x[:, :, ix[:, j], :] for j in range(TAPS))
    return sum(wy[None, :, j, None, None] * rows[:, iy[:, j], :, :] for j in range(TAPS))


def entry(scheduler, spec, steps: int, strength: float):
    """Where pass 2 enters its schedule of `steps` steps: (a, s, start, run) with the latent a * upsampled + s * noise in front
    of evaluation `start` and `run` = int(steps * strength + 0.5) steps to go.  The convention is image_to_image's for the same
    steps and strength.  Default sampler (`spec` None; `scheduler` is left set to `steps` timesteps): the reference's rule, the
    signal / noise rates of t = ascending[run].  A named sampler (a samplers.SamplerSpec): its Schedule's alphas[start] /
    noise_rates[start], start = steps - run."""
    from . import samplers as smp

    steps = int(steps)
    run = int(steps * strength + 0.5)
    if run < 1:
        raise ValueError(f"hires: strength {strength} leaves no step of the {steps}-step second pass to run")
    start = steps - run
    if spec is None:
        if run >= steps:
            raise ValueError(f"hires: strength {strength} with {steps} steps enters the second pass in front of its first timestep; "
                             "lower the strength or use more steps")
        scheduler.set_timesteps(steps)
        t = scheduler.timesteps[::-1][run]
        return float(scheduler.signal_rates[t]), float(scheduler.noise_rates[t]), start, run
    sched = smp.schedule(spec, scheduler, steps)
    return float(sched.alphas[start]), float(sched.noise_rates[start]), start, run


def draw_noise(batch: int, h: int, w: int, seed=None) -> np.ndarray:
    """The re-noise draw of the GLOBAL batch, sample-major: (batch, h, w, 4) float32; with a seed from default_rng([seed, 2])
    (sample b's block does not depend on the batch size), without one from numpy's global stream."""
    shape = (int(batch), int(h), int(w), 4)
    if seed is None:
        return np.random.randn(*shape).astype(np.float32)
    return np.random.default_rng([int(seed), 2]).standard_normal(shape).astype(np.float32)
