"""Regional prompting (Latent Couple / MultiDiffusion region control): one prompt per masked region of the picture
(``generate_image(..., regions=...)``).

Every step the UNet evaluates the conditional half once per region prompt - the regions are further batch rows of the one denoise
engine, region-major behind the unconditional rows - and one launch (``msd_region_combine``) in front of the guidance / sampler
step replaces the conditional eps of every latent pixel by the weighted sum of the regions' predictions for it.  The step
kernels then see the [2B][n] layout they always have.  This module is the host side of it and needs no GPU: the job description
(``RegionSpec`` / ``Regions`` / ``parse``), the normalised per-pixel weights (``weights``), the common binary masks (``boxes``) and
a float64 statement of the kernel (``combine_reference``).

Weights: w_r = weight_r * mask_r / sum_q weight_q * mask_q per latent pixel, computed in float64 and rounded once to fp32, so
a pixel covered by one region alone has exactly 1.0 there and 0.0 elsewhere, and the kernel copies that region's eps bit for bit.
With ``base_weight`` > 0 the job's own prompt joins as region 0 with the constant mask ``base_weight``; with 0 it is not
evaluated at all.

``mode="attention"`` ("attention couple") applies the masks where the prompts enter the network instead: the UNet runs the plain
job's rows, and in every attn2 the conditional rows compute out(q) = sum_r w_r(q) softmax(q K_r^T) V_r in one launch
(``msd_region_attention``).  Its host side is here too: the weight planes of the UNet's four resolution levels
(``Resolved.level_weights``: float64 block means of the weighted masks, normalised over the regions, rounded once), their packing
into the one array an engine uploads (``pack_levels``) and a float64 statement of the kernel (``attention_reference``).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np

MAX_REGIONS = 16   # MSD_REGION_MAX


@dataclass
class RegionSpec:
    """One region: ``prompt`` (anything encode_text accepts, or an encoded (T, 768) array), ``mask`` (2-D, values >= 0, at
    latent resolution (h, w) or image resolution (H, W) = (8 h, 8 w)) and ``weight`` (> 0)."""
    prompt: Any = None
    mask: Any = None
    weight: float = 1.0


@dataclass
class Regions:
    """A regional job: the RegionSpecs in order and the weight of the job's own prompt (0: it is not evaluated)."""
    regions: Sequence[RegionSpec] = field(default_factory=list)
    base_weight: float = 0.0
    mode: str = "latent"   # "latent": one UNet row per region, msd_region_combine; "attention": the masks applied in every attn2


@dataclass(frozen=True)
class Resolved:
    """A Regions description resolved against a pipeline size.  prompts: the region prompts in order (without the base prompt);
    masks: float64 (len(prompts), h, w) at latent resolution, the regions' weights multiplied in; base_weight: >= 0."""
    prompts: Tuple[Any, ...]
    masks: np.ndarray
    base_weight: float
    mode: str = "latent"

    @property
    def count(self) -> int:
        """Evaluated region prompts: the base prompt counts when its weight is positive."""
        return len(self.prompts) + (1 if self.base_weight > 0.0 else 0)

    def weights(self) -> np.ndarray:
        """fp32 (count, h, w), the base prompt's constant mask first when it takes part."""
        m = self.masks
        if self.base_weight > 0.0:
            m = np.concatenate([np.full((1,) + m.shape[1:], self.base_weight, dtype=np.float64), m], axis=0)
        return _normalise(m)

    def level_weights(self, levels) -> List[np.ndarray]:
        """The weight planes of an attention-mode job: one fp32 (count, h_l, w_l) per UNet resolution level, ``levels`` being the
        (h_l, w_l) of the levels as the engine records them ((h, w) of the latent first, every further level ceil-halved).
        Pixel (y, x) of level l stands for the latent pixels [y 2^l, min((y + 1) 2^l, h)) x [x 2^l, min((x + 1) 2^l, w)): its
        weights are the float64 means of the weighted masks over that (clipped) block - the base prompt's plane is the
        constant base_weight - normalised over the regions and rounded once to fp32.  Level 0 is weights() bit for bit."""
        h, w = self.masks.shape[1:]
        out = []
        for l, (hl, wl) in enumerate(levels):
            f = 1 << l
            hl, wl = int(hl), int(wl)
            if (hl, wl) != (-(-h // f), -(-w // f)):
                raise ValueError(f"regions: level {l} is {(hl, wl)}, expected {(-(-h // f), -(-w // f))} for a latent of {(h, w)}")
            pad = np.zeros((self.masks.shape[0], hl * f, wl * f), dtype=np.float64)
            pad[:, :h, :w] = self.masks
            rows = np.minimum(f, h - f * np.arange(hl)).astype(np.float64)   # latent rows / columns of each (clipped) block
            cols = np.minimum(f, w - f * np.arange(wl)).astype(np.float64)
            m = pad.reshape(-1, hl, f, wl, f).sum(axis=(2, 4)) / (rows[:, None] * cols[None, :])[None]
            if self.base_weight > 0.0:
                m = np.concatenate([np.full((1, hl, wl), self.base_weight, dtype=np.float64), m], axis=0)
            out.append(_normalise(m))
        return out


def pack_levels(planes) -> np.ndarray:
    """The level planes of level_weights() as the ONE flat fp32 array an attention-mode engine uploads: level l's (count, h_l, w_l)
    row-major at level_offsets()[l], every level starting on a multiple of 4 floats (16 bytes)."""
    planes = [np.ascontiguousarray(p, dtype=np.float32) for p in planes]
    offs = level_offsets(planes[0].shape[0], [p.shape[1:] for p in planes])
    out = np.zeros(offs[-1], dtype=np.float32)
    for p, o in zip(planes, offs):
        out[o:o + p.size] = p.reshape(-1)
    return out


def level_offsets(count: int, levels) -> List[int]:
    """Float offsets of the levels' planes in pack_levels' array, and behind them its length."""
    offs = [0]
    for hl, wl in levels:
        offs.append(offs[-1] + (int(count) * int(hl) * int(wl) + 3) // 4 * 4)
    return offs


def boxes(h: int, w: int, rows: int, cols: int) -> List[np.ndarray]:
    """The rows * cols binary rectangle masks (h, w) of a grid, row-major; cell i of an axis of length L with k cells covers
    [i * L // k, (i + 1) * L // k).  Every pixel lies in exactly one of them."""
    h, w, rows, cols = int(h), int(w), int(rows), int(cols)
    if not (1 <= rows <= h and 1 <= cols <= w):
        raise ValueError(f"regions: a {rows} x {cols} grid on {h} x {w} pixels")
    out = []
    for r in range(rows):
        for c in range(cols):
            m = np.zeros((h, w), dtype=np.float32)
            m[r * h // rows:(r + 1) * h // rows, c * w // cols:(c + 1) * w // cols] = 1.0
            out.append(m)
    return out


def latent_mask(mask, h: int, w: int, what: str = "mask") -> np.ndarray:
    """A mask at latent (h, w) or image (8 h, 8 w) resolution -> float64 (h, w); an image-resolution mask is reduced by the
    float64 mean over 8 x 8 blocks.  ValueError for another shape, a negative or a non-finite entry."""
    m = np.asarray(mask, dtype=np.float64)
    if m.ndim != 2 or tuple(m.shape) not in ((h, w), (8 * h, 8 * w)):
        raise ValueError(f"regions: {what} has shape {tuple(m.shape)}: expected the latent's {(h, w)} or the image's {(8 * h, 8 * w)}")
    if not np.all(np.isfinite(m)):
        raise ValueError(f"regions: {what} has a non-finite entry")
    if m.min() < 0.0:
        raise ValueError(f"regions: {what} has a negative entry")
    if tuple(m.shape) != (h, w):
        m = m.reshape(h, 8, w, 8).mean(axis=(1, 3))
    return m


def _normalise(m: np.ndarray) -> np.ndarray:
    total = m.sum(axis=0)
    if total.min() <= 0.0:
        y, x = np.argwhere(total <= 0.0)[0]
        raise ValueError(f"regions: no region covers latent pixel (y, x) = ({int(y)}, {int(x)}): every mask is zero there")
    return (m / total[None]).astype(np.float32)


def weights(masks, region_weights=None, base_weight: float = 0.0, h: Optional[int] = None, w: Optional[int] = None) -> np.ndarray:
    """The normalised per-pixel weights fp32 (R, h, w): weight_r * mask_r / sum in float64, rounded once.  masks: a sequence of
    2-D masks (latent or image resolution; h, w default to the first mask's shape taken as the latent's); region_weights:
    one float > 0 per mask (default 1); base_weight > 0 puts a constant mask of that value in front."""
    masks = list(masks)
    if not masks:
        raise ValueError("regions: no region")
    if h is None or w is None:
        h, w = np.shape(masks[0])
    ws = [1.0] * len(masks) if region_weights is None else [float(v) for v in region_weights]
    if len(ws) != len(masks):
        raise ValueError(f"regions: {len(ws)} weights for {len(masks)} masks")
    return _resolve([RegionSpec(None, m, v) for m, v in zip(masks, ws)], base_weight, int(h), int(w)).weights()


MODES = ("latent", "attention")


def _resolve(specs, base_weight, h: int, w: int, mode: str = "latent") -> Resolved:
    if mode not in MODES:
        raise ValueError(f"regions: mode = {mode!r}: one of {MODES}")
    base_weight = float(base_weight)
    if not np.isfinite(base_weight) or base_weight < 0.0:
        raise ValueError(f"regions: base_weight = {base_weight!r} must be a finite float >= 0")
    specs = list(specs)
    if not specs:
        raise ValueError("regions: no region")
    count = len(specs) + (1 if base_weight > 0.0 else 0)
    if count > MAX_REGIONS:
        raise ValueError(f"regions: {count} evaluated prompts (the base prompt included), at most MAX_REGIONS = {MAX_REGIONS}")
    out = []
    for i, s in enumerate(specs):
        wt = float(s.weight)
        if not np.isfinite(wt) or wt <= 0.0:
            raise ValueError(f"regions: region {i} has weight {s.weight!r}: a finite float > 0")
        if s.mask is None:
            raise ValueError(f"regions: region {i} has no mask")
        out.append(wt * latent_mask(s.mask, h, w, f"the mask of region {i}"))
    res = Resolved(tuple(s.prompt for s in specs), np.stack(out, axis=0), base_weight, mode)
    res.weights()   # (ValueError for an uncovered pixel, now rather than in the middle of the job)
    return res


def parse(regions, img_height: int, img_width: int) -> Optional[Resolved]:
    """None -> None; a Regions object or a dict {"regions": [RegionSpec or dict of its fields, ...], "base_weight": 0.0,
    "mode": "latent" or "attention"} -> the description resolved at the pipeline's size.  ValueError for an unknown field or
    mode, a bad mask or weight, a pixel no region covers,
    more than MAX_REGIONS evaluated prompts."""
    if regions is None:
        return None
    if isinstance(regions, Resolved):
        if regions.mode not in MODES:
            raise ValueError(f"regions: mode = {regions.mode!r}: one of {MODES}")
        if tuple(regions.masks.shape[1:]) != (img_height // 8, img_width // 8):
            raise ValueError(f"regions: masks of {tuple(regions.masks.shape[1:])} on a latent of {(img_height // 8, img_width // 8)}")
        return regions
    if isinstance(regions, dict):
        unknown = set(regions) - {"regions", "base_weight", "mode"}
        if unknown:
            raise ValueError(f"regions: unknown field(s) {sorted(unknown)}")
        regions = Regions(**regions)
    if not isinstance(regions, Regions):
        raise ValueError(f"regions must be a Regions, a dict or None, not {type(regions).__name__}")
    if img_height % 8 or img_width % 8:
        raise ValueError(f"regions: the image {img_height}x{img_width} must be a multiple of 8 in both dimensions")
    specs = []
    for i, s in enumerate(regions.regions):
        if isinstance(s, dict):
            unknown = set(s) - {"prompt", "mask", "weight"}
            if unknown:
                raise ValueError(f"regions: region {i}: unknown field(s) {sorted(unknown)}")
            s = RegionSpec(**s)
        if not isinstance(s, RegionSpec):
            raise ValueError(f"regions: region {i} must be a RegionSpec or a dict, not {type(s).__name__}")
        if s.prompt is None:
            raise ValueError(f"regions: region {i} has no prompt")
        specs.append(s)
    return _resolve(specs, regions.base_weight, img_height // 8, img_width // 8, regions.mode)


def combine_reference(eps, w) -> np.ndarray:
    """float64 statement of msd_region_combine: eps (R * B, h, w, C) region-major (row r * B + b), w (R, h, w) ->
    (B, h, w, C) = sum_r w[r] * eps[r * B + b], w shared by the batch and the channels."""
    eps, w = np.asarray(eps, dtype=np.float64), np.asarray(w, dtype=np.float64)
    R = w.shape[0]
    if eps.ndim != 4 or w.ndim != 3 or eps.shape[0] % R or tuple(eps.shape[1:3]) != tuple(w.shape[1:]):
        raise ValueError(f"regions: eps of shape {eps.shape} with weights of shape {w.shape}")
    e = eps.reshape((R, eps.shape[0] // R) + eps.shape[1:])
    out = np.zeros(e.shape[1:], dtype=np.float64)
    for r in range(R):
        out += w[r][None, :, :, None] * e[r]
    return out


def combine_host(eps_list, w) -> np.ndarray:
    """The kernel's arithmetic on the host, for the host loop: fp32 (B, h, w, C) from one fp32 (B, h, w, C) per region, in the
    kernel's order - a product, then one fused multiply-add per further region (the exact fp32 product added in float64 and
    rounded to fp32)."""
    w = np.asarray(w, dtype=np.float32)
    v = w[0][None, :, :, None] * np.asarray(eps_list[0], dtype=np.float32)
    for r in range(1, len(eps_list)):
        prod = w[r].astype(np.float64)[None, :, :, None] * np.asarray(eps_list[r], dtype=np.float32).astype(np.float64)
        v = (prod + v.astype(np.float64)).astype(np.float32)
    return v


def attention_reference(q, k, v, w, heads: int) -> np.ndarray:
    """float64 statement of msd_region_attention: q (B, S, C) carrying scale * log2(e), k and v (R * B, T, C) region-major (row
    r * B + b), w (R, S), C = heads * d -> (B, S, C) = sum_r w[r][i] * softmax2(q_h k_rh^T) v_rh per head h, the softmax to base
    2.  A region takes part at a query only where its weight is positive, so the K / V of a region that is nowhere positive may
    hold anything."""
    q, k, v, w = (np.asarray(x, dtype=np.float64) for x in (q, k, v, w))
    R = w.shape[0]
    if q.ndim != 3 or k.ndim != 3 or k.shape != v.shape or w.ndim != 2 or k.shape[0] != R * q.shape[0] or w.shape[1] != q.shape[1] \
            or q.shape[2] != k.shape[2] or q.shape[2] % heads:
        raise ValueError(f"regions: q {q.shape}, k {k.shape}, v {v.shape}, w {w.shape}, {heads} heads")
    B, S, C = q.shape
    d = C // heads
    out = np.zeros((B, S, C), dtype=np.float64)
    for r in range(R):
        on = w[r] > 0.0
        if not on.any():
            continue
        for b in range(B):
            for h in range(heads):
                c = slice(h * d, (h + 1) * d)
                s = q[b, on, c] @ k[r * B + b, :, c].T
                p = np.exp2(s - s.max(axis=1, keepdims=True))
                out[b, on, c] += w[r, on, None] * ((p / p.sum(axis=1, keepdims=True)) @ v[r * B + b, :, c])
    return out
