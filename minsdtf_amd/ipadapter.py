"""IP-Adapter image prompts (Ye et al. 2023; diffusers' ``load_ip_adapter`` / ``ip_adapter_image_embeds``, ComfyUI's IPAdapter
nodes, the ``ip-adapter`` preprocessor of the A1111 ControlNet extension): ``generate_image(..., ip_adapter=...)``.

An adapter adds, to every cross-attention of the UNet, a second attention of the same query over N image tokens, with its own
``to_k_ip`` / ``to_v_ip`` projections, decoupled from the text attention:

    out(q) = softmax(q K_text^T) V_text + s(i, layer) * softmax(q K_ip^T) V_ip
    s(i, layer) = weight * keep(i) * factor(weight_type)[layer]
    keep(i)     = 0.0 if (i / num_steps < start or (i + 1) / num_steps > end) else 1.0      (control.keep: diffusers' rule)

for step row i and attention block `layer` (engine.PAG_LAYERS order).  The image tokens are the adapter's projection of the CLIP
image embedding, ``LayerNorm(Linear(embeds).reshape(N, 768))``; the unconditional rows of a guidance pair get the tokens of the ZERO
embedding (diffusers' and the extension's negative).

This module is the host side and needs no GPU: the description (``IPAdapterSpec`` / ``parse``), the per-call uploads (``table``,
``project``), the checkpoint map (``read_state``), what an image-prompt job refuses (``REFUSED`` / ``refuse``) and the float64
statement of the launch (``attention_reference``).  The device side is msdi_attention_decoupled
(include/minsdtf_hip_ipadapter.h); the weights live in ``models.IPAdapter``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, fields
from typing import Dict, Optional, Tuple

import numpy as np

from .control import keep

LAYERS = 16            # MSDI_LAYERS: the UNet's attention blocks (engine.PAG_LAYERS)
KEYS = 96              # MSDI_KEYS: roundup8(T) + N keys share one tile
MAX_TOKENS = 16        # MSDI_MAX_TOKENS
EMBED_DIM = 1024       # CLIP ViT-H/14 image embedding
CONTEXT_DIM = 768
WEIGHT_TYPES = ("linear", "style", "composition")
LN_EPS = 1e-5          # torch.nn.LayerNorm's default, the adapter's image_proj.norm

# what a job with an image prompt cannot be combined with, in the order a refusal names them: generate_image's arguments, then states
REFUSED = (("regions", "pag", "sag", "reference_only", "hypertile", "tiled", "hires"), ("denoise_streams = 2",))


def layer_names() -> Tuple[str, ...]:
    from .engine import PAG_LAYERS

    return PAG_LAYERS


# diffusers' attn_processors order of the 16 cross-attentions - the down blocks, then the UP blocks, then the mid block - as indices
# into engine.PAG_LAYERS (forward order: down, mid, up); entry j belongs to ip_adapter.<2 j + 1>
CHECKPOINT_ORDER = tuple(range(6)) + tuple(range(7, 16)) + (6,)
CHECKPOINT_WIDTHS = (320, 320, 640, 640, 1280, 1280) + (1280,) * 3 + (640,) * 3 + (320,) * 3 + (1280,)


@dataclass
class IPAdapterSpec:
    """Exactly one of ``embeds`` (the (1024,) CLIP image embedding), ``tokens`` ((N, 768) image tokens, past the projection: the
    entry for "plus" adapters) and ``image`` (a picture, through StableDiffusion.image_prompt_encoder or the pipeline's own
    clip_vision tower); ``weight``: a finite float;
    ``start`` / ``end``: the share of the steps the adapter acts on, 0 <= start <= end <= 1; ``weight_type``: one of WEIGHT_TYPES or
    a dict {attention block name: factor}; at most one of ``path`` (an IP-Adapter checkpoint) and ``model`` (a models.IPAdapter).
    ``negative_tokens``: with ``tokens``, the (N, 768) tokens of the unconditional rows (default: zeros)."""
    embeds: object = None
    tokens: object = None
    image: object = None
    weight: float = 1.0
    start: float = 0.0
    end: float = 1.0
    weight_type: object = "linear"
    path: Optional[str] = None
    model: object = None
    negative_tokens: object = None


_FIELDS = tuple(f.name for f in fields(IPAdapterSpec))


def _number(what, value, ok, rule) -> float:
    try:
        v = float(value)
    except (TypeError, ValueError) as e:
        raise ValueError(f"ip_adapter: {what} = {value!r} must be {rule}") from e
    if isinstance(value, bool) or not math.isfinite(v) or not ok(v):
        raise ValueError(f"ip_adapter: {what} = {value!r} must be {rule}")
    return v


def _array(what, value, shape_ok, rule) -> np.ndarray:
    try:
        a = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"ip_adapter: {what} must be {rule}") from e
    if not shape_ok(a.shape) or not np.isfinite(a).all():
        raise ValueError(f"ip_adapter: {what} of shape {a.shape} must be {rule}")
    return a


def block_factors(weight_type) -> np.ndarray:
    """float64 [16]: the factor of every attention block, in engine.PAG_LAYERS order."""
    names = layer_names()
    if isinstance(weight_type, dict):
        unknown = [k for k in weight_type if k not in names]
        if unknown:
            raise ValueError(f"ip_adapter: weight_type names unknown attention block(s) {sorted(map(str, unknown))} (engine.PAG_LAYERS)")
        f = np.zeros(LAYERS, dtype=np.float64)
        for k, v in weight_type.items():
            f[names.index(k)] = _number(f"weight_type[{k!r}]", v, lambda x: True, "a finite float")
        return f
    if not isinstance(weight_type, str) or weight_type not in WEIGHT_TYPES:
        raise ValueError(f"ip_adapter: weight_type = {weight_type!r} must be one of {WEIGHT_TYPES} or a dict of block factors")
    if weight_type == "linear":
        return np.ones(LAYERS, dtype=np.float64)
    if weight_type == "style":   # InstantStyle's style blocks for SD 1.5
        return np.asarray([1.0 if n.startswith("up_blocks.1.attentions.") else 0.0 for n in names], dtype=np.float64)
    return np.asarray([1.0 if n == "down_blocks.2.attentions.1" else 0.0 for n in names], dtype=np.float64)


def parse(ip_adapter) -> Optional[IPAdapterSpec]:
    """None -> None; an IPAdapterSpec or a dict of its fields -> the checked spec (numbers as floats, arrays as float64).
    ValueError naming the field for anything else."""
    if ip_adapter is None:
        return None
    s = ip_adapter
    if isinstance(s, dict):
        unknown = set(s) - set(_FIELDS)
        if unknown:
            raise ValueError(f"ip_adapter: unknown field(s) {sorted(unknown)}")
        s = IPAdapterSpec(**s)
    if not isinstance(s, IPAdapterSpec):
        raise ValueError(f"ip_adapter is {type(s).__name__}, expected an ipadapter.IPAdapterSpec or a dict of its fields")
    given = [n for n in ("embeds", "tokens", "image") if getattr(s, n) is not None]
    if len(given) != 1:
        raise ValueError(f"ip_adapter: exactly one of `embeds`, `tokens` and `image` is needed, got {given or 'none'}")
    embeds = tokens = negative = None
    if s.embeds is not None:
        embeds = _array("embeds", s.embeds, lambda sh: sh in ((EMBED_DIM,), (1, EMBED_DIM)), f"a finite ({EMBED_DIM},) array").reshape(EMBED_DIM)
    if s.tokens is not None:
        tokens = _array("tokens", s.tokens, lambda sh: len(sh) == 2 and 1 <= sh[0] <= MAX_TOKENS and sh[1] == CONTEXT_DIM,
                        f"a finite (N, {CONTEXT_DIM}) array, 1 <= N <= {MAX_TOKENS}")
    if s.negative_tokens is not None:
        if tokens is None:
            raise ValueError("ip_adapter: `negative_tokens` goes with `tokens` (an embedding's negative is the zero embedding's tokens)")
        negative = _array("negative_tokens", s.negative_tokens, lambda sh: sh == tokens.shape, f"a finite array of the tokens' shape {tokens.shape}")
    weight = _number("weight", s.weight, lambda x: True, "a finite float")
    start = _number("start", s.start, lambda x: 0.0 <= x <= 1.0, "a float in [0, 1]")
    end = _number("end", s.end, lambda x: 0.0 <= x <= 1.0, "a float in [0, 1]")
    if start > end:
        raise ValueError(f"ip_adapter: start = {start!r} > end = {end!r} (0 <= start <= end <= 1)")
    block_factors(s.weight_type)   # (ValueError for an unknown type or block)
    if s.path is not None and s.model is not None:
        raise ValueError("ip_adapter: `path` and `model` should not both be given")
    if s.path is not None and not isinstance(s.path, str):
        raise ValueError(f"ip_adapter: path = {s.path!r} must be a checkpoint file name")
    wt = dict(s.weight_type) if isinstance(s.weight_type, dict) else s.weight_type
    return IPAdapterSpec(embeds, tokens, s.image, weight, start, end, wt, s.path, s.model, negative)


def table(spec, num_steps: int) -> np.ndarray:
    """The per-call upload: fp32 [num_steps][16], built in float64 and rounded once.  Row i is the row of the job's coefficient
    table (the device step counter), whatever step the job enters at; column l is attention block engine.PAG_LAYERS[l]."""
    spec = parse(spec)
    num_steps = int(num_steps)
    if num_steps < 1:
        raise ValueError(f"ip_adapter: num_steps = {num_steps} (>= 1)")
    f = block_factors(spec.weight_type) * spec.weight
    t = np.zeros((num_steps, LAYERS), dtype=np.float64)
    for i in range(num_steps):
        t[i] = f * keep(i, num_steps, spec.start, spec.end)
    return t.astype(np.float32)


def project(embeds, proj_w, proj_b, norm_w, norm_b, tokens: int) -> np.ndarray:
    """The adapter's image projection on the host: LayerNorm(768)(Linear(1024 -> N * 768)(embeds).reshape(N, 768)) in float64,
    rounded once to fp32 (N, 768).  proj_w (N * 768, 1024) and norm_w (768,) as torch stores them."""
    x = np.asarray(embeds, dtype=np.float64).reshape(EMBED_DIM)
    y = (np.asarray(proj_w, dtype=np.float64) @ x + np.asarray(proj_b, dtype=np.float64)).reshape(int(tokens), CONTEXT_DIM)
    mean = y.mean(axis=-1, keepdims=True)
    var = ((y - mean) ** 2).mean(axis=-1, keepdims=True)
    out = (y - mean) / np.sqrt(var + LN_EPS) * np.asarray(norm_w, dtype=np.float64) + np.asarray(norm_b, dtype=np.float64)
    return out.astype(np.float32)


# ---- the public IP-Adapter file layout ----------------------------------------------------------------------------------------
def read_state(state) -> Dict[str, np.ndarray]:
    """A loaded IP-Adapter checkpoint - the nested dict {"image_proj": {...}, "ip_adapter": {...}} of a .bin or flat prefixed keys
    ("image_proj.proj.weight", "ip_adapter.1.to_k_ip.weight", ...) - as {"proj.weight", "proj.bias", "norm.weight", "norm.bias",
    "<attention block>.to_k_ip", "<attention block>.to_v_ip"} float32 arrays, the block names engine.PAG_LAYERS'.  The map from the
    checkpoint's odd indices 1 .. 31 (diffusers' attn_processors order) is verified by shape; any mismatch raises.
    A "plus" checkpoint - one with `image_proj.latents` - has a Resampler in place of the projection: its keys come back as
    "resampler.<key>" (resampler.read_state's, verified there) and there is no "proj.*" / "norm.*" entry."""
    flat = {}
    for k, v in dict(state).items():
        if isinstance(v, dict):
            for k2, v2 in v.items():
                flat[f"{k}.{k2}"] = v2
        else:
            flat[k] = v

    def arr(key):
        if key not in flat:
            raise ValueError(f"ip_adapter: the checkpoint has no {key!r}")
        v = flat[key]
        v = v.detach().to("cpu").float().numpy() if hasattr(v, "detach") else np.asarray(v)
        return np.ascontiguousarray(v, dtype=np.float32)

    out = {}
    if "image_proj.latents" in flat:   # a "plus" checkpoint: its image_proj is a Resampler (resampler.read_state verifies it)
        from . import resampler as resampler_mod

        for key, a in resampler_mod.read_state(flat).items():
            out["resampler." + key] = a
        return _read_kv(flat, arr, out)
    pw = arr("image_proj.proj.weight")
    if pw.ndim != 2 or pw.shape[1] != EMBED_DIM or pw.shape[0] % CONTEXT_DIM or not 1 <= pw.shape[0] // CONTEXT_DIM <= MAX_TOKENS:
        raise ValueError(f"ip_adapter: image_proj.proj.weight has shape {pw.shape}, expected (N * {CONTEXT_DIM}, {EMBED_DIM}) with "
                         f"1 <= N <= {MAX_TOKENS} (a \"plus\" adapter's resampler is not supported: pass its `tokens`)")
    out["proj.weight"] = pw
    for key, shape in (("proj.bias", (pw.shape[0],)), ("norm.weight", (CONTEXT_DIM,)), ("norm.bias", (CONTEXT_DIM,))):
        out[key] = arr("image_proj." + key)
        if out[key].shape != shape:
            raise ValueError(f"ip_adapter: image_proj.{key} has shape {out[key].shape}, expected {shape}")
    return _read_kv(flat, arr, out)


def _read_kv(flat, arr, out) -> Dict[str, np.ndarray]:
    """The 32 to_k_ip / to_v_ip matrices of a checkpoint's `ip_adapter` part into `out` (read_state: both layouts share them)."""
    names = layer_names()
    for j, (layer, width) in enumerate(zip(CHECKPOINT_ORDER, CHECKPOINT_WIDTHS)):
        for m in ("to_k_ip", "to_v_ip"):
            key = f"ip_adapter.{2 * j + 1}.{m}.weight"
            w = arr(key)
            if w.shape != (width, CONTEXT_DIM):
                raise ValueError(f"ip_adapter: {key} has shape {w.shape}, {names[layer]} takes ({width}, {CONTEXT_DIM})")
            out[f"{names[layer]}.{m}"] = w
    extra = [k for k in flat if k.startswith("ip_adapter.") and k.split(".")[1].isdigit() and not (int(k.split(".")[1]) % 2 and int(k.split(".")[1]) <= 31)]
    if extra:
        raise ValueError(f"ip_adapter: unexpected checkpoint keys {sorted(extra)[:4]}")
    return out


# ---- what does not go together --------------------------------------------------------------------------------------------------
def refuse(given: dict, streams=None) -> None:
    """ValueError naming every argument of `given` (generate_image's, by name) that is set and every state that holds which a job
    with an image prompt cannot take."""
    arguments, states = REFUSED
    holds = {"denoise_streams = 2": streams == 2}
    refused = [n for n in arguments if given.get(n) is not None] + [s for s in states if holds[s]]
    if refused:
        raise ValueError(f"ip_adapter: an image prompt acts on the plain UNet rows of one stream: it cannot be combined with {', '.join(refused)}")


def check_context(t: int, tokens: int) -> None:
    """ValueError when a text context of t tokens and the image tokens do not fit the one key tile."""
    if (int(t) + 7) // 8 * 8 + int(tokens) > KEYS:
        raise ValueError(f"ip_adapter: a text context of {t} tokens and {tokens} image tokens exceed the {KEYS} keys of one tile "
                         f"(roundup8(T) + N <= {KEYS}): prompts longer than 77 tokens cannot be combined with an image prompt")


# ---- the float64 statement of the launch ----------------------------------------------------------------------------------------
def attention_reference(q, k, v, k_ip, v_ip, scale, heads: int) -> np.ndarray:
    """msdi_attention_decoupled in float64: q (B, S, C) carrying head_dim^-0.5 * log2(e), k / v (B, T, C), k_ip / v_ip (B, N, C)
    (v and v_ip NOT transposed), scale the table entry; returns (B, S, C).  Per head: softmax2(q k^T) v + scale * softmax2(q k_ip^T)
    v_ip with softmax2(x) = 2^x / sum 2^x; scale == 0 drops the image term whatever it holds."""
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    B, S, C = q.shape
    d = C // heads

    def part(kk, vv):
        kk, vv = np.asarray(kk, dtype=np.float64), np.asarray(vv, dtype=np.float64)
        qh = q.reshape(B, S, heads, d).transpose(0, 2, 1, 3)
        kh = kk.reshape(B, -1, heads, d).transpose(0, 2, 1, 3)
        vh = vv.reshape(B, -1, heads, d).transpose(0, 2, 1, 3)
        x = qh @ kh.transpose(0, 1, 3, 2)
        p = np.exp2(x - x.max(axis=-1, keepdims=True))
        p = p / p.sum(axis=-1, keepdims=True)
        return (p @ vh).transpose(0, 2, 1, 3).reshape(B, S, C)

    out = part(k, v)
    if float(scale) != 0.0:
        out = out + float(scale) * part(k_ip, v_ip)
    return out
