"""The Resampler of the IP-Adapter "plus" checkpoints (``ip-adapter-plus_sd15``, ``ip-adapter-plus-face_sd15``; the Perceiver
resampler of IP-Adapter's ``resampler.py``, diffusers' ``IPAdapterPlusImageProjection``): from the CLIP ViT-H/14 tower's penultimate
hidden states (B, 257, 1280) to the N = 16 image tokens (B, N, 768) the decoupled cross-attention takes.

    x       = proj_in(hidden)                                        Linear 1280 -> 768 with bias
    latents = the learned (1, N, 768) parameter, repeated over B
    for each of `depth` layers:
        xn = LayerNorm1(x);  ln = LayerNorm2(latents)
        q = to_q(ln);  k, v = to_kv(concat(xn, ln) along tokens)     no bias; 257 + N keys, the x keys first
        w = softmax((q * 64**-0.25) (k * 64**-0.25)^T) per head of 64, over all 257 + N keys
        latents = to_out(w v) + latents
        latents = W2 gelu_erf(W1 LayerNorm(latents)) + latents       768 -> 3072 -> 768, no bias
    tokens  = LayerNorm_out(proj_out(latents))                       Linear 768 -> 768 with bias

``x`` is never updated; only ``latents`` moves through the layers.  This module is the host side and needs no GPU: the checkpoint
map (``read_state``), the float64 statement (``forward_host``, ``attention_reference``) and the seeded synthetic state
(``synthetic_state``).  The device side is ``models.IPResampler`` over ``engine.emit_ip_resampler``, whose attention is
msdr_perceiver_attention (include/minsdtf_hip_resampler.h).
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np

EMBED_DIM = 1280       # the tower's hidden width (weights.VIT_DIM)
DIM = 768              # the resampler's width = the UNet's context width
HEADS, HEAD_DIM = 12, 64
FF_MULT = 4
MAX_TOKENS = 16        # ipadapter.MAX_TOKENS = MSDR_MAX_QUERIES
DEPTH = 4              # the SD 1.5 plus adapters
MAX_DEPTH = 16
LN_EPS = 1e-5          # torch.nn.LayerNorm's default
PREFIX = "image_proj."
LAYER_KEYS = (("0.norm1.weight", (DIM,)), ("0.norm1.bias", (DIM,)), ("0.norm2.weight", (DIM,)), ("0.norm2.bias", (DIM,)),
              ("0.to_q.weight", (DIM, DIM)), ("0.to_kv.weight", (2 * DIM, DIM)), ("0.to_out.weight", (DIM, DIM)),
              ("1.0.weight", (DIM,)), ("1.0.bias", (DIM,)), ("1.1.weight", (FF_MULT * DIM, DIM)), ("1.3.weight", (DIM, FF_MULT * DIM)))


def key_shapes(depth: int, tokens: int = MAX_TOKENS) -> Dict[str, Tuple[int, ...]]:
    """Every key of a resampler with `depth` layers and `tokens` queries (without the `image_proj.` prefix) -> its shape as torch
    stores it, in checkpoint order."""
    out = {"latents": (1, int(tokens), DIM), "proj_in.weight": (DIM, EMBED_DIM), "proj_in.bias": (DIM,),
           "proj_out.weight": (DIM, DIM), "proj_out.bias": (DIM,), "norm_out.weight": (DIM,), "norm_out.bias": (DIM,)}
    for i in range(int(depth)):
        for k, shape in LAYER_KEYS:
            out[f"layers.{i}.{k}"] = shape
    return out


def read_state(state) -> Dict[str, np.ndarray]:
    """The `image_proj` part of a loaded plus checkpoint - the nested dict {"image_proj": {...}, ...} of a .bin or flat prefixed keys
    ("image_proj.latents", "image_proj.layers.0.0.to_q.weight", ...); fp16 files load - as float32 arrays under the keys of
    key_shapes().  `depth` is inferred from the keys (the layers present must be 0 .. depth - 1) and N from `latents`; every shape
    is verified - the inner width must be 768 = 12 heads of 64, because the head count is not in the file - and a missing key or a
    wrong shape raises ValueError naming the key."""
    flat = {}
    for k, v in dict(state).items():
        if isinstance(v, dict):
            for k2, v2 in v.items():
                flat[f"{k}.{k2}"] = v2
        else:
            flat[k] = v

    def arr(key):
        if PREFIX + key not in flat:
            raise ValueError(f"ip_adapter: the checkpoint has no {PREFIX + key!r}")
        v = flat[PREFIX + key]
        v = v.detach().to("cpu").float().numpy() if hasattr(v, "detach") else np.asarray(v)
        return np.ascontiguousarray(v, dtype=np.float32)

    lat = arr("latents")
    if lat.ndim != 3 or lat.shape[0] != 1 or not 1 <= lat.shape[1] <= MAX_TOKENS or lat.shape[2] != DIM:
        raise ValueError(f"ip_adapter: {PREFIX}latents has shape {lat.shape}, expected (1, N, {DIM}) with 1 <= N <= {MAX_TOKENS}")
    layers = set()
    for k in flat:
        parts = k.split(".")
        if k.startswith(PREFIX + "layers.") and len(parts) > 2 and parts[2].isdigit():
            layers.add(int(parts[2]))
    depth = len(layers)
    if not 1 <= depth <= MAX_DEPTH or layers != set(range(depth)):
        raise ValueError(f"ip_adapter: {PREFIX}layers has the indices {sorted(layers)}, expected 0 .. depth - 1 with 1 <= depth <= {MAX_DEPTH}")
    tq = arr("layers.0.0.to_q.weight")
    if tq.ndim != 2 or tq.shape[0] != HEADS * HEAD_DIM:
        raise ValueError(f"ip_adapter: {PREFIX}layers.0.0.to_q.weight has shape {tq.shape}: an inner width of {HEADS * HEAD_DIM} = "
                         f"{HEADS} heads of {HEAD_DIM} is the one that is built (the head count is not in the file)")
    out = {}
    for key, shape in key_shapes(depth, lat.shape[1]).items():
        a = arr(key)
        if a.shape != shape:
            raise ValueError(f"ip_adapter: {PREFIX + key} has shape {a.shape}, expected {shape}")
        out[key] = a
    return out


def depth_of(named) -> int:
    """The number of layers of a read_state() / synthetic_state() result."""
    return len({k.split(".")[1] for k in named if k.startswith("layers.")})


# ---- the float64 statement ------------------------------------------------------------------------------------------------------
def _ln(x, g, b):
    mean = x.mean(axis=-1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
    return (x - mean) / np.sqrt(var + LN_EPS) * g + b


_erf = np.vectorize(math.erf, otypes=[np.float64])


def forward_host(state, hidden, depth: int = None) -> np.ndarray:
    """The Resampler in float64, the formula of the module docstring literally (the two 64**-0.25 factors included): `state` is
    read_state()'s result (or synthetic_state()'s), `hidden` (B, 257, 1280) or (257, 1280) - any token count >= 1 is taken;
    returns (B, N, 768) float64."""
    if any(isinstance(v, dict) or str(k).startswith(PREFIX) for k, v in dict(state).items()):   # (the checkpoint's own layout)
        state = read_state(state)
    s = {k: np.asarray(v, dtype=np.float64) for k, v in state.items()}
    depth = depth_of(s) if depth is None else int(depth)
    h = np.asarray(hidden, dtype=np.float64)
    h = h[None] if h.ndim == 2 else h
    if h.ndim != 3 or h.shape[2] != EMBED_DIM or h.shape[1] < 1:
        raise ValueError(f"ip_resampler: hidden states of shape {h.shape} ((B, 257, {EMBED_DIM}): the tower's `penultimate`)")
    B = h.shape[0]
    x = h @ s["proj_in.weight"].T + s["proj_in.bias"]
    lat = np.broadcast_to(s["latents"], (B,) + s["latents"].shape[1:]).copy()
    N = lat.shape[1]
    f = HEAD_DIM ** -0.25
    for i in range(depth):
        p = f"layers.{i}."
        xn = _ln(x, s[p + "0.norm1.weight"], s[p + "0.norm1.bias"])
        ln = _ln(lat, s[p + "0.norm2.weight"], s[p + "0.norm2.bias"])
        q = ln @ s[p + "0.to_q.weight"].T
        kv = np.concatenate([xn, ln], axis=1) @ s[p + "0.to_kv.weight"].T
        k, v = kv[..., :DIM], kv[..., DIM:]
        qh = q.reshape(B, N, HEADS, HEAD_DIM).transpose(0, 2, 1, 3)
        kh = k.reshape(B, -1, HEADS, HEAD_DIM).transpose(0, 2, 1, 3)
        vh = v.reshape(B, -1, HEADS, HEAD_DIM).transpose(0, 2, 1, 3)
        w = (qh * f) @ (kh * f).transpose(0, 1, 3, 2)
        w = np.exp(w - w.max(axis=-1, keepdims=True))
        w = w / w.sum(axis=-1, keepdims=True)
        o = (w @ vh).transpose(0, 2, 1, 3).reshape(B, N, DIM)
        lat = o @ s[p + "0.to_out.weight"].T + lat
        y = _ln(lat, s[p + "1.0.weight"], s[p + "1.0.bias"]) @ s[p + "1.1.weight"].T
        y = 0.5 * y * (1.0 + _erf(y / math.sqrt(2.0)))
        lat = y @ s[p + "1.3.weight"].T + lat
    return _ln(lat @ s["proj_out.weight"].T + s["proj_out.bias"], s["norm_out.weight"], s["norm_out.bias"])


def attention_reference(q, k_x, v_x, k_l, v_l, scale, heads: int) -> np.ndarray:
    """msdr_perceiver_attention in float64: q (B, N, C), k_x / v_x (B, T, C), k_l / v_l (B, N, C) (the V operands NOT transposed),
    `scale` the launch's (it carries log2(e): the softmax is base 2); returns (B, N, C).  One softmax over the T + N keys per head."""
    q = np.asarray(q, dtype=np.float64)
    k = np.concatenate([np.asarray(k_x, dtype=np.float64), np.asarray(k_l, dtype=np.float64)], axis=1)
    v = np.concatenate([np.asarray(v_x, dtype=np.float64), np.asarray(v_l, dtype=np.float64)], axis=1)
    B, N, C = q.shape
    d = C // heads
    qh = q.reshape(B, N, heads, d).transpose(0, 2, 1, 3)
    kh = k.reshape(B, -1, heads, d).transpose(0, 2, 1, 3)
    vh = v.reshape(B, -1, heads, d).transpose(0, 2, 1, 3)
    x = float(scale) * (qh @ kh.transpose(0, 1, 3, 2))
    p = np.exp2(x - x.max(axis=-1, keepdims=True))
    p = p / p.sum(axis=-1, keepdims=True)
    return (p @ vh).transpose(0, 2, 1, 3).reshape(B, N, C)


# ---- the seeded synthetic resampler -----------------------------------------------------------------------------------------------
def synthetic_state(seed: int = 0, depth: int = DEPTH, tokens: int = MAX_TOKENS) -> Dict[str, np.ndarray]:
    """A seeded synthetic resampler under the checkpoint's flat keys ("image_proj. ..."), float32: Glorot-uniform matrices,
    LayerNorm gains in [0.8, 1.2], biases and offsets in [-0.1, 0.1], latents N(0, 1) / sqrt(768) (the reference's initialisation)."""
    rng = np.random.Generator(np.random.PCG64([int(seed), 0x9E5A]))
    state = {}
    for key, shape in key_shapes(depth, tokens).items():
        if key == "latents":
            w = rng.standard_normal(size=shape) / math.sqrt(DIM)
        elif len(shape) == 2:
            lim = math.sqrt(6.0 / (shape[0] + shape[1]))
            w = rng.uniform(-lim, lim, size=shape)
        elif "norm" in key.split(".")[-2] and key.endswith(".weight") or key.endswith(".1.0.weight"):
            w = rng.uniform(0.8, 1.2, size=shape)
        else:
            w = rng.uniform(-0.1, 0.1, size=shape)
        state[PREFIX + key] = w.astype(np.float32)
    return state
