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

This module is the host side and needs no GPU: the job description (``ReferenceSpec`` / ``parse``), the rate table (``rates``),
the reference noise (``draw_noise``) and a float64 statement of the kernel (``joint_attention_reference``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, FrozenSet, Optional

import numpy as np

ALIASES = {"mid": "mid_block.attentions.0"}
FIELDS = ("image", "latent", "fidelity", "layers", "noise")
NOISE_STREAM = 3   # default_rng([seed, 3]): the convention of hires_noise (1: a job's step draws, 2: the hires re-noise draw)


def layer_names():
    """The 16 attention blocks a job may select, in forward order (engine.PAG_LAYERS)."""
    from . import engine

    return engine.PAG_LAYERS


@dataclass
class ReferenceSpec:
    """Exactly one of ``image`` (anything ``preprocessed_image`` takes; encoded by the VAE encoder) and ``latent`` (a
    (1, h, w, 4) array, used as is); ``fidelity`` in [0, 1]: the share of the plain self-attention in the unconditional rows;
    ``layers``: "all", "mid" or attention block names (engine.PAG_LAYERS); ``noise``: the (1, h, w, 4) draw n_ref, or None for
    ``draw_noise``."""
    image: Any = None
    latent: Any = None
    fidelity: float = 0.5
    layers: Any = "all"
    noise: Any = None


@dataclass(frozen=True)
class Resolved:
    """A ReferenceSpec checked: one of image / latent, fidelity a float in [0, 1], layers a non-empty frozenset of block names."""
    image: Any
    latent: Optional[np.ndarray]
    fidelity: float
    layers: FrozenSet[str]
    noise: Optional[np.ndarray]

    @property
    def key(self) -> tuple:
        """The layer set in a fixed order: what an engine is keyed by (never the image, the draw or the fidelity)."""
        return tuple(sorted(self.layers))


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
    [0, 1], an empty layer set or an unknown layer name."""
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
    if not names:
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
    return Resolved(ref.image, latent, fidelity, frozenset(layers), noise)


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
