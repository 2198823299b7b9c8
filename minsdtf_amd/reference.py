"""Reference-only control: self-attention over a reference image (the ``reference_only`` preprocessor of the A1111 ControlNet
extension; diffusers' community ``StableDiffusionReferencePipeline`` with ``reference_attn=True``).

Every step the UNet runs one more batch row r, the reference latent noised to the step's level,

    x_r = a_i * z_ref + b_i * n_ref            (a_i, b_i): the signal / noise rate at which evaluation i sees its latent

and in the selected attention blocks the generated rows' self-attention also attends to r's keys:

    r:  plain self-attention
    c:  joint = softmax(q [K_own ; K_r]^T) [V_own ; V_r]
    u:  fidelity * plain + (1 - fidelity) * joint          (diffusers' style_fidelity)

which is one ``msd_attention_joint`` launch per block (the blend is the online softmax's state at the segment boundary).  One
stated deviation from diffusers: n_ref is ONE draw (not a fresh one per step) and r runs once, with the conditional context of
sample 0 (not with both contexts), so the result is a function of the arguments and the cost is one row.

Reference AdaIN (the extension's ``reference_adain`` and ``reference_adain+attn`` preprocessors; diffusers' ``reference_adain``)
is the field ``adain``: at a chosen set of block outputs (``ADAIN_SITES``) each generated row's feature map is renormalised,
channel by channel, to the mean and standard deviation the reference row has at the same place (one ``msd_reference_adain``
launch per site, blended by the same ``mix``).  Attention carries the subject, AdaIN the palette and contrast.

This module is the host side and needs no GPU: the job description (``ReferenceSpec`` / ``parse``), the rate table (``rates``),
the reference noise (``draw_noise``), the AdaIN site table (``ADAIN_SITES`` / ``adain_sites``) and float64 statements of the
kernels (``joint_attention_reference``, ``adain_reference``).
"""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction
from typing import Any, FrozenSet, Optional, Tuple

import numpy as np

ALIASES = {"mid": "mid_block.attentions.0"}
FIELDS = ("image", "latent", "fidelity", "layers", "noise", "adain")
NOISE_STREAM = 3   # default_rng([seed, 3]): the convention of hires_noise (1: a job's step draws, 2: the hires re-noise draw)


_ADAIN_DOWN = ("down_blocks.1.attentions.0", "down_blocks.1.attentions.1", "down_blocks.2.attentions.0", "down_blocks.2.attentions.1",
               "down_blocks.3.resnets.0", "down_blocks.3.resnets.1")
_ADAIN_UP = ("up_blocks.0.resnets.0", "up_blocks.0.resnets.1", "up_blocks.0.upsamplers.0.conv", "up_blocks.1.attentions.0",
             "up_blocks.1.attentions.1", "up_blocks.1.upsamplers.0.conv", "up_blocks.2.attentions.0", "up_blocks.2.attentions.1")
# The fifteen AdaIN sites in forward order: (the name of the call whose output is the site, its position weight gw).  gw is
# 2 (1 - i / 6) down the encoder, 0 at the mid block and 2 i / 8 up the decoder, kept as exact fractions of the integer
# positions: a site applies when gw < weight, strictly.  No site at the first level and none on a downsampler; where a block
# ends in an upsampler the site is the upsampler conv's output.
ADAIN_SITES: Tuple[Tuple[str, Fraction], ...] = (
    tuple((n, Fraction(2 * (6 - i), 6)) for i, n in enumerate(_ADAIN_DOWN)) + (("mid_block.resnets.1", Fraction(0)),)
    + tuple((n, Fraction(2 * i, 8)) for i, n in enumerate(_ADAIN_UP)))
ADAIN_DEFAULT_WEIGHT = 1.0   # the extension's default: seven sites, all at C = 1280


def adain_sites(weight) -> FrozenSet[str]:
    """The sites with gw < weight (strictly; the comparison is exact: gw is a fraction of the integer position and a float is a
    dyadic rational).  ValueError for a weight that is not a finite float in (0, 2] - every such weight selects the mid block."""
    try:
        w = float(weight)
    except (TypeError, ValueError) as e:
        raise ValueError(f"reference_only: adain = {weight!r} must be a weight in (0, 2]") from e
    if not 0.0 < w <= 2.0:   # (NaN fails both comparisons)
        raise ValueError(f"reference_only: adain = {weight!r} must be a weight in (0, 2]")
    sites = frozenset(n for n, gw in ADAIN_SITES if gw < Fraction(w))
    if not sites:
        raise ValueError(f"reference_only: adain = {weight!r} selects no site")
    return sites


def _adain(value) -> Optional[FrozenSet[str]]:
    """The `adain` field -> a non-empty frozenset of site names, or None (off)."""
    if value is None:
        return None
    names = dict(ADAIN_SITES)
    if isinstance(value, str):
        if value == "auto":
            return adain_sites(ADAIN_DEFAULT_WEIGHT)
        if value == "all":
            return frozenset(names)
        value = [value]
    elif isinstance(value, (bool, np.bool_)):
        raise ValueError(f"reference_only: adain = {value!r} must be None, 'auto', 'all', a weight in (0, 2] or site names")
    elif isinstance(value, (int, float, np.integer, np.floating)):
        return adain_sites(value)
    try:
        value = list(value)
    except TypeError as e:
        raise ValueError(f"reference_only: adain = {value!r} must be None, 'auto', 'all', a weight in (0, 2] or site names") from e
    if not value:
        raise ValueError("reference_only: adain selects no site")
    for n in value:
        if not isinstance(n, str) or n not in names:
            raise ValueError(f"reference_only: adain: unknown site {n!r}: 'auto', 'all', a weight or of {', '.join(names)}")
    return frozenset(value)


def layer_names():
    """The 16 attention blocks a job may select, in forward order (engine.PAG_LAYERS)."""
    from . import engine

    return engine.PAG_LAYERS


@dataclass
class ReferenceSpec:
    """Exactly one of ``image`` (anything ``preprocessed_image`` takes; encoded by the VAE encoder) and ``latent`` (a
    (1, h, w, 4) array, used as is); ``fidelity`` in [0, 1]: the share of the plain self-attention in the unconditional rows;
    ``layers``: "all", "mid" or attention block names (engine.PAG_LAYERS); ``noise``: the (1, h, w, 4) draw n_ref, or None for
    ``draw_noise``; ``adain``: None (off), "auto" (weight 1.0), "all" (the fifteen ADAIN_SITES), a weight in (0, 2] selecting the
    sites with gw < weight, or site names - reference AdaIN at those block outputs.  With ``adain`` given, ``layers`` may be
    empty ([] or None): AdaIN without the attention part."""
    image: Any = None
    latent: Any = None
    fidelity: float = 0.5
    layers: Any = "all"
    noise: Any = None
    adain: Any = None


@dataclass(frozen=True)
class Resolved:
    """A ReferenceSpec checked: one of image / latent, fidelity a float in [0, 1], layers a frozenset of block names (empty only
    next to AdaIN sites), adain a non-empty frozenset of site names or None."""
    image: Any
    latent: Optional[np.ndarray]
    fidelity: float
    layers: FrozenSet[str]
    noise: Optional[np.ndarray]
    adain: Optional[FrozenSet[str]] = None

    @property
    def key(self) -> tuple:
        """The layer set in a fixed order: what an engine is keyed by (never the image, the draw or the fidelity).  With AdaIN
        sites it also holds their sorted tuple, as one last element."""
        layers = tuple(sorted(self.layers))
        return layers if self.adain is None else layers + (("adain",) + tuple(sorted(self.adain)),)

    @property
    def adain_key(self) -> Optional[tuple]:
        """The AdaIN sites in a fixed order, or None."""
        return None if self.adain is None else tuple(sorted(self.adain))


def _latent(x, what):
    a = np.asarray(x, dtype=np.float32)
    if a.ndim != 4 or a.shape[0] != 1 or a.shape[3] != 4:
        raise ValueError(f"reference_only: {what} must have shape (1, h, w, 4), not {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"reference_only: {what} holds a value that is not finite")
    return np.ascontiguousarray(a)


def parse(ref) -> Optional[Resolved]:
    """None -> None; a ReferenceSpec or a dict of its fields -> the checked description.  ValueError for an unknown field, both or
    neither of image / latent, a latent or noise of another shape than (1, h, w, 4) (or two different ones), a fidelity outside
    [0, 1], an empty layer set (unless `adain` selects sites) or an unknown layer name, and for an `adain` that is none of None,
    "auto", "all", a weight in (0, 2] that selects a site, a site name or a non-empty iterable of site names."""
    if ref is None:
        return None
    if isinstance(ref, Resolved):
        return ref
    if isinstance(ref, dict):
        unknown = set(ref) - set(FIELDS)
        if unknown:
            raise ValueError(f"reference_only: unknown field(s) {sorted(unknown)}")
        ref = ReferenceSpec(**ref)
    if not isinstance(ref, ReferenceSpec):
        raise ValueError(f"reference_only must be a ReferenceSpec, a dict or None, not {type(ref).__name__}")
    if (ref.image is None) == (ref.latent is None):
        raise ValueError("reference_only: give exactly one of 'image' and 'latent'")
    try:
        fidelity = float(ref.fidelity)
    except (TypeError, ValueError) as e:
        raise ValueError(f"reference_only: fidelity = {ref.fidelity!r} must be a float in [0, 1]") from e
    if not 0.0 <= fidelity <= 1.0:   # (NaN fails both comparisons)
        raise ValueError(f"reference_only: fidelity = {ref.fidelity!r} must be a float in [0, 1]")
    valid = layer_names()
    if isinstance(ref.layers, str) and ref.layers == "all":
        names = list(valid)
    else:
        names = [ref.layers] if isinstance(ref.layers, str) else list(ref.layers if ref.layers is not None else ())
    adain = _adain(ref.adain)
    if not names and adain is None:
        raise ValueError("reference_only: no layer selected")
    layers = set()
    for n in names:
        n = ALIASES.get(n, n) if isinstance(n, str) else n
        if n not in valid:
            raise ValueError(f"reference_only: unknown layer {n!r}: 'all', 'mid' or of {', '.join(valid)}")
        layers.add(n)
    latent = None if ref.latent is None else _latent(ref.latent, "latent")
    noise = None if ref.noise is None else _latent(ref.noise, "noise")
    if latent is not None and noise is not None and latent.shape != noise.shape:
        raise ValueError(f"reference_only: noise {noise.shape} and latent {latent.shape} differ in shape")
    return Resolved(ref.image, latent, fidelity, frozenset(layers), noise, adain)


def draw_noise(h: int, w: int, seed=None) -> np.ndarray:
    """n_ref, (1, h, w, 4) float32: default_rng([seed, 3]) with a seed, numpy's global stream without (as hires_noise)."""
    shape = (1, int(h), int(w), 4)
    if seed is None:
        return np.random.randn(*shape).astype(np.float32)
    return np.random.default_rng([int(seed), NOISE_STREAM]).standard_normal(shape).astype(np.float32)


def rates(sched, start_index: int = 0) -> np.ndarray:
    """float64 [num_steps][2] = (a_i, b_i): the signal and noise rate at which evaluation i's UNet call sees its latent.  `sched`
    is the default step's Scheduler after set_timesteps (signal_rates[t_i], noise_rates[t_i]) or a samplers.Schedule (alpha_i,
    sigma_i * alpha_i).  Rows before `start_index` are never executed and are left (1, 0), as samplers.rows leaves its own."""
    start = int(start_index)
    if hasattr(sched, "sigmas"):   # samplers.Schedule
        n = sched.num_steps
        a, b = np.asarray(sched.alphas, dtype=np.float64)[:n], np.asarray(sched.noise_rates, dtype=np.float64)[:n]
    else:
        ts = np.asarray(sched.timesteps, dtype=np.int64)
        a = np.asarray(sched.signal_rates, dtype=np.float64)[ts]
        b = np.asarray(sched.noise_rates, dtype=np.float64)[ts]
    out = np.stack([a, b], axis=1).astype(np.float64)
    out[:start] = (1.0, 0.0)
    return out


def reference_latent_host(z_ref, n_ref, row) -> np.ndarray:
    """x_r on the host, for the host loop: msd_reference_latent's arithmetic in fp32 - the product a * z, then one fused
    multiply-add of b * n (emulated in float64: a product of two fp32 values is exact there, and so is the sum before the one
    rounding)."""
    a, b = np.float32(row[0]), np.float32(row[1])
    z, n = np.asarray(z_ref, dtype=np.float32), np.asarray(n_ref, dtype=np.float32)
    az = (z.astype(np.float64) * np.float64(a)).astype(np.float32)
    return (n.astype(np.float64) * np.float64(b) + az.astype(np.float64)).astype(np.float32)


def joint_attention_reference(q, k, v, k_ref, v_ref, mix, heads: int) -> np.ndarray:
    """float64 statement of msd_attention_joint.  q (B, S, C) carrying scale * log2(e), k / v (B, T, C), k_ref / v_ref (T_ref, C),
    mix (B,) or None, C = heads * d.  Returns (B, S, C): mix * softmax2(q k^T) v + (1 - mix) * softmax2(q [k ; k_ref]^T) [v ; v_ref]
    with softmax2 the base-2 softmax.  A sample with mix == 1 does not look at k_ref / v_ref."""
    q, k, v = (np.asarray(x, dtype=np.float64) for x in (q, k, v))
    k_ref, v_ref = np.asarray(k_ref, dtype=np.float64), np.asarray(v_ref, dtype=np.float64)
    B, S, C = q.shape
    T, Tr = k.shape[1], k_ref.shape[0]
    d = C // heads
    mix = np.zeros(B) if mix is None else np.asarray(mix, dtype=np.float64).reshape(B)

    def attend(qh, kh, vh):   # (H, S, d), (H, T, d) -> (H, S, d)
        s = np.einsum("hsd,htd->hst", qh, kh)
        p = np.exp2(s - s.max(-1, keepdims=True))
        return np.einsum("hst,htd->hsd", p / p.sum(-1, keepdims=True), vh)

    def heads_of(x, n):
        return x.reshape(n, heads, d).transpose(1, 0, 2)

    out = np.empty((B, S, C), dtype=np.float64)
    for b in range(B):
        qh, kh, vh = heads_of(q[b], S), heads_of(k[b], T), heads_of(v[b], T)
        f = float(mix[b])
        plain = attend(qh, kh, vh)
        if f == 1.0:
            o = plain
        else:
            joint = attend(qh, np.concatenate([kh, heads_of(k_ref, Tr)], 1), np.concatenate([vh, heads_of(v_ref, Tr)], 1))
            o = joint if f == 0.0 else f * plain + (1.0 - f) * joint
        out[b] = o.transpose(1, 0, 2).reshape(S, C)
    return out


def adain_reference(x, ref, mix=None, eps: float = 1e-6) -> np.ndarray:
    """float64 statement of msd_reference_adain.  x (rows, hw, C), ref (hw, C), mix (rows,) or None (all 0).  Returns (rows, hw, C):

        mean, var = var_mean(x[b], over the pixels, correction=0)        std = sqrt(max(var, 0) + eps)
        mean_acc, std_acc likewise from ref
        y = ((x[b] - mean) / std) * std_acc + mean_acc                   out[b] = mix[b] * x[b] + (1 - mix[b]) * y

    which is diffusers' ``reference_adain`` (torch.var_mean(..., correction=0), ((x - mean) / std) * std_acc + mean_acc) with
    its ``style_fidelity`` blend of the unconditional rows.  A row with mix == 1 is returned as it is, whatever it holds."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rows = x.shape[0]
    mix = np.zeros(rows) if mix is None else np.asarray(mix, dtype=np.float64).reshape(rows)
    mean_r = ref.mean(axis=0)
    std_r = np.sqrt(np.maximum(((ref - mean_r) ** 2).mean(axis=0), 0.0) + eps)
    out = np.empty_like(x)
    for b in range(rows):
        f = float(mix[b])
        if f == 1.0:
            out[b] = x[b]
            continue
        mean = x[b].mean(axis=0)
        std = np.sqrt(np.maximum(((x[b] - mean) ** 2).mean(axis=0), 0.0) + eps)
        y = (x[b] - mean) * (std_r / std) + mean_r
        out[b] = y if f == 0.0 else f * x[b] + (1.0 - f) * y
    return out
