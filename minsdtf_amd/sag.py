"""Self-attention guidance (SAG, Hong et al. 2023: "Improving Sample Quality of Diffusion Models Using Self-Attention Guidance"):
``generate_image(..., sag=...)``, after diffusers' ``StableDiffusionSAGPipeline``.

Every step the UNet runs twice, the second pass depending on the first.  With rows u (unconditional) and c (conditional),
guidance g and SAG scale s:

1. pass 1 is the usual forward; in ``mid_block.attentions.0`` attn1 the u rows also produce the map
   ``A[b][j] = (1 / heads) * sum_h sum_i softmax_j(q_h k_h^T)[i][j]`` (``msdx_attention_colsum``), the attention key j receives;
2. the latent is degraded where that map exceeds the threshold: ``x0 = (x - sigma_t e_u) / alpha_t`` is blurred (9-tap Gaussian,
   reflect borders) and noised back, ``x~ = alpha_t blur(x0) + sigma_t e_u``; elsewhere ``x~ = x`` (``msdx_sag_degrade``);
3. pass 2 is ``d = UNet(x~, t, unconditional context)``;
4. ``eps = u + g (c - u) + s (u - d)``, realised as ``c' = k u + c - k d`` with ``k = s / g`` in front of the unchanged guidance /
   sampler step on (u, c').  Without guidance (g <= 0) the only rows are c: the map, x0 and pass 2's context come from them and
   ``eps = (1 + s) c - s d``.

This module is the host side and needs no GPU: the job description (``SagSpec`` / ``parse``), the uploads (``taps``, ``params``,
``weights``) and the float64 / fp32 host statements of the two device steps for the host loop (``degrade_host``, ``combine_host``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import regions

RADIUS = 4   # 9 taps, diffusers' kernel_size = 9


@dataclass
class SagSpec:
    """``scale``: s > 0; ``blur_sigma``: the Gaussian's sigma in latent pixels, in (0, 3]; ``threshold``: a key is degraded where
    the attention it receives exceeds this (1.0 = the mean over the keys).  The defaults are diffusers'."""
    scale: float = 0.75
    blur_sigma: float = 1.0
    threshold: float = 1.0


@dataclass(frozen=True)
class Resolved:
    """A SagSpec checked: three finite floats in their ranges."""
    scale: float
    blur_sigma: float
    threshold: float


def _number(name, value, ok, rule) -> float:
    try:
        v = float(value)
    except (TypeError, ValueError) as e:
        raise ValueError(f"sag: {name} = {value!r} must be {rule}") from e
    if isinstance(value, bool) or not np.isfinite(v) or not ok(v):
        raise ValueError(f"sag: {name} = {value!r} must be {rule}")
    return v


def parse(sag) -> Optional[Resolved]:
    """None -> None; True -> the defaults; a SagSpec or a dict of its fields -> the checked description.  ValueError for an unknown
    field, a scale that is not a finite float > 0, a blur_sigma outside (0, 3] or a threshold that is not finite."""
    if sag is None:
        return None
    if isinstance(sag, Resolved):
        return sag
    if sag is True:
        sag = SagSpec()
    if isinstance(sag, dict):
        unknown = set(sag) - {"scale", "blur_sigma", "threshold"}
        if unknown:
            raise ValueError(f"sag: unknown field(s) {sorted(unknown)}")
        sag = SagSpec(**sag)
    if not isinstance(sag, SagSpec):
        raise ValueError(f"sag must be a SagSpec, a dict, True or None, not {type(sag).__name__}")
    return Resolved(_number("scale", sag.scale, lambda v: v > 0.0, "a finite float > 0"),
                    _number("blur_sigma", sag.blur_sigma, lambda v: 0.0 < v <= 3.0, "a finite float in (0, 3]"),
                    _number("threshold", sag.threshold, lambda v: True, "a finite float"))


def taps(blur_sigma: float) -> np.ndarray:
    """The 9 Gaussian taps exp(-0.5 ((i - 4) / blur_sigma)^2), normalised in float64, as the fp32 values the device reads."""
    i = np.arange(2 * RADIUS + 1, dtype=np.float64) - RADIUS
    t = np.exp(-0.5 * (i / float(blur_sigma)) ** 2)
    return (t / t.sum()).astype(np.float32)


def params(spec: Resolved) -> np.ndarray:
    """msdx_sag_degrade's `params` upload, fp32 [10]: the 9 taps, then the threshold."""
    return np.concatenate([taps(spec.blur_sigma), np.asarray([spec.threshold], dtype=np.float32)]).astype(np.float32)


def factor(scale: float, guidance: float) -> float:
    """k of c' = k u + c - k d, in float64: s / g with guidance; without, s of c' = (1 + s) c - s d."""
    scale, guidance = float(scale), float(guidance)
    return scale / guidance if guidance > 0.0 else scale


def weights(scale: float, guidance: float, h: int, w: int) -> np.ndarray:
    """The constant planes of the combine (msd_region_combine), fp32: with guidance (3, h, w) = fp32(k), 1, fp32(-k) over the row
    groups (u, c, d); without (2, h, w) = fp32(1 + s), fp32(-s) over (c, d).  k is rounded once from float64."""
    k = factor(scale, guidance)
    vals = (k, 1.0, -k) if float(guidance) > 0.0 else (1.0 + k, -k)
    out = np.empty((len(vals), int(h), int(w)), dtype=np.float32)
    for i, v in enumerate(vals):
        out[i] = np.float32(v)
    return out


def mask_host(A, map_hw, h: int, w: int, threshold: float) -> np.ndarray:
    """bool (B, h, w): A[b][(y * mh // h) * mw + (x * mw // w)] > threshold - the integer nearest upsample of the map (torch's
    'nearest' where h % mh == 0 and w % mw == 0).  The comparison is made on the fp32 values the device holds."""
    mh, mw = (int(v) for v in map_hw)
    A = np.asarray(A, dtype=np.float32).reshape(-1, mh, mw)
    ys = (np.arange(int(h)) * mh) // int(h)
    xs = (np.arange(int(w)) * mw) // int(w)
    return A[:, ys][:, :, xs] > np.float32(threshold)


def degrade_host(x, e, alpha, sigma, A, map_hw, taps, threshold) -> np.ndarray:
    """msdx_sag_degrade in float64: x, e (B, h, w, 4); alpha, sigma the step's rates; A (B, mh * mw) the map; `taps` the 9 values
    the device reads.  Where the mask is set alpha * blur((x - sigma e) / alpha) + sigma * e, elsewhere x itself."""
    x = np.asarray(x, dtype=np.float64)
    e = np.asarray(e, dtype=np.float64)
    alpha, sigma = float(alpha), float(sigma)
    t = np.asarray(taps, dtype=np.float64)
    if t.shape != (2 * RADIUS + 1,):
        raise ValueError(f"degrade_host: {t.shape} taps, expected ({2 * RADIUS + 1},)")
    B, h, w, _c = x.shape
    if h <= RADIUS or w <= RADIUS:
        raise ValueError(f"degrade_host: a {h} x {w} latent (reflect padding of {RADIUS} needs at least {RADIUS + 1} per side)")
    x0 = (x - sigma * e) / alpha
    pad = np.pad(x0, ((0, 0), (0, 0), (RADIUS, RADIUS), (0, 0)), mode="reflect")
    hor = sum(t[i] * pad[:, :, i:i + w] for i in range(2 * RADIUS + 1))
    pad = np.pad(hor, ((0, 0), (RADIUS, RADIUS), (0, 0), (0, 0)), mode="reflect")
    blur = sum(t[i] * pad[:, i:i + h] for i in range(2 * RADIUS + 1))
    m = mask_host(A, map_hw, h, w, threshold)[..., None]
    return np.where(m, alpha * blur + sigma * e, x)


def combine_host(u, c, d, w) -> np.ndarray:
    """c' on the host, for the host loop, in msd_region_combine's order in fp32 (regions.combine_host): with guidance the product
    w[0] * u, then fma(w[1], c, .), then fma(w[2], d, .); without (u is None) w[0] * c, then fma(w[1], d, .)."""
    return regions.combine_host([c, d], w) if u is None else regions.combine_host([u, c, d], w)
