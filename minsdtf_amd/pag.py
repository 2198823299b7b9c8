"""Perturbed-attention guidance (PAG, Ahn et al. 2024: "Self-Rectifying Diffusion Sampling with Perturbed-Attention Guidance"):
``generate_image(..., pag=...)``.

Every step the UNet evaluates the conditional context a second time with the self-attention map of the selected blocks replaced
by the identity - those layers' output is V itself (``msd_attention_identity``) - and the prediction is pushed away from that
structure-less one.  With rows u (unconditional), c (conditional), p (conditional context, perturbed self-attention), guidance g
and PAG scale s:

    eps = u + g (c - u) + s (c - p)

The engine realises it as c' = (1 + k) c - k p written in place over the c rows, followed by the unchanged guidance / sampler
step on (u, c'):  k = s / g for g > 0 (then u + g (c' - u) is the line above), k = s for g = 0 (no u rows: the step sees c'
alone).  The p rows are further batch rows of the one denoise engine, behind the c rows; the combine is ``msd_region_combine``
with two constant weight planes, fp32(1 + k) and fp32(-k).  ``guidance_rescale`` therefore measures its reference std on c'
(diffusers measures it on c; with guidance_rescale = 0 the two agree).

This module is the host side and needs no GPU: the job description (``PagSpec`` / ``parse``), the two weight planes
(``weights``) and the kernel's arithmetic on the host for the host loop (``combine_host``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, FrozenSet, Optional

import numpy as np

from . import regions

ALIASES = {"mid": "mid_block.attentions.0"}


def layer_names():
    """The 16 attention blocks a job may select, in forward order (engine.PAG_LAYERS: the blocks behind engine.UNET_ATTN_LAYERS)."""
    from . import engine

    return engine.PAG_LAYERS


@dataclass
class PagSpec:
    """``scale``: s >= 0 (0: the plain job); ``layers``: one attention block name or a sequence of them - "mid" is
    mid_block.attentions.0, the other names are "down_blocks.L.attentions.R" (L 0..2, R 0..1) and "up_blocks.U.attentions.R"
    (U 1..3, R 0..2)."""
    scale: float = 3.0
    layers: Any = "mid"


@dataclass(frozen=True)
class Resolved:
    """A PagSpec checked: scale a finite float >= 0, layers a non-empty frozenset of block names."""
    scale: float
    layers: FrozenSet[str]

    @property
    def key(self) -> tuple:
        """The layer set in a fixed order: what an engine is keyed by (never the scale)."""
        return tuple(sorted(self.layers))


def parse(pag) -> Optional[Resolved]:
    """None -> None; a PagSpec or a dict of its fields -> the checked description.  ValueError for an unknown field, a scale that
    is not a finite float >= 0, an empty layer set or an unknown layer name."""
    if pag is None:
        return None
    if isinstance(pag, Resolved):
        return pag
    if isinstance(pag, dict):
        unknown = set(pag) - {"scale", "layers"}
        if unknown:
            raise ValueError(f"pag: unknown field(s) {sorted(unknown)}")
        pag = PagSpec(**pag)
    if not isinstance(pag, PagSpec):
        raise ValueError(f"pag must be a PagSpec, a dict or None, not {type(pag).__name__}")
    try:
        scale = float(pag.scale)
    except (TypeError, ValueError) as e:
        raise ValueError(f"pag: scale = {pag.scale!r} must be a finite float >= 0") from e
    if not np.isfinite(scale) or scale < 0.0:
        raise ValueError(f"pag: scale = {pag.scale!r} must be a finite float >= 0")
    names = [pag.layers] if isinstance(pag.layers, str) else list(pag.layers if pag.layers is not None else ())
    if not names:
        raise ValueError("pag: no layer selected")
    valid = layer_names()
    layers = set()
    for n in names:
        n = ALIASES.get(n, n) if isinstance(n, str) else n
        if n not in valid:
            raise ValueError(f"pag: unknown layer {n!r}: one of 'mid', {', '.join(valid)}")
        layers.add(n)
    return Resolved(scale, frozenset(layers))


def factor(scale: float, guidance: float) -> float:
    """k of c' = (1 + k) c - k p, in float64: s / g with guidance, s without."""
    scale, guidance = float(scale), float(guidance)
    return scale / guidance if guidance > 0.0 else scale


def weights(scale: float, guidance: float, h: int, w: int) -> np.ndarray:
    """The two constant planes of the combine, fp32 (2, h, w): fp32(1 + k) for the c rows, fp32(-k) for the p rows, k rounded
    once from float64."""
    k = factor(scale, guidance)
    out = np.empty((2, int(h), int(w)), dtype=np.float32)
    out[0] = np.float32(1.0 + k)
    out[1] = np.float32(-k)
    return out


def combine_host(c, p, w) -> np.ndarray:
    """c' on the host, for the host loop: msd_region_combine's sum over the two row groups in its order, in fp32 - the product
    w[0] * c, then one fused multiply-add of w[1] * p (regions.combine_host)."""
    return regions.combine_host([c, p], w)
