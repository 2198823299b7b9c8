"""Host side of the CLIP ViT-H/14 vision tower (models.ClipVisionEncoder): the picture -> pixels preprocessing of an image prompt and
the float64 restatement of the tower the tests and tools compare the device against.

``preprocess`` is CLIPImageProcessor's rule - shortest edge to 224 (the long edge ``int(long * 224 / short)``), centre crop,
bicubic - with the resampling evaluated in floating point: Pillow's bicubic filter (antialiased, a = -0.5) as
``torch.nn.functional.interpolate(mode="bicubic", antialias=True)`` computes it in float64, clamped to 0 .. 255.  That is
Pillow's mode-"F" resize to 3e-5 levels; Pillow's 8-bit path rounds and clips between its two passes and differs from it by at
most one level on smooth pictures.  The normalisation (mean / std) is NOT applied here: the pixels stay on the
0 .. 255 scale and msdv_patch_embed applies ``pixel_affine()`` in one fma.

``forward_host`` is plain torch on the CPU: the same formulas as the launch plan (engine.emit_clip_vision), nothing rounded.
"""
from __future__ import annotations

import hashlib
from typing import Dict, Tuple

import numpy as np
import torch

from . import weights as wtab

SIZE = wtab.VIT_IMAGE
MEAN = (0.48145466, 0.4578275, 0.40821073)    # OPENAI_CLIP_MEAN
STD = (0.26862954, 0.26130258, 0.27577711)    # OPENAI_CLIP_STD
EPS = 1e-5                                    # CLIPVisionConfig.layer_norm_eps


def pixel_affine() -> Tuple[Tuple[float, float, float], Tuple[float, float, float]]:
    """(scale, shift) per channel, float64: x = pixel * scale + shift is (pixel / 255 - mean) / std."""
    return tuple(1.0 / (255.0 * s) for s in STD), tuple(-m / s for m, s in zip(MEAN, STD))


def zero_normalised_pixels() -> np.ndarray:
    """The (224, 224, 3) float32 picture, on the 0 .. 255 scale, whose normalised pixels are zero: pixel = -shift / scale = 255 * mean
    per channel, rounded once to fp32 (so pixel * scale + shift is zero to fp32 rounding).  The negative of a "plus" IP-Adapter."""
    scale, shift = pixel_affine()
    row = np.asarray([-b / a for a, b in zip(scale, shift)], dtype=np.float64)
    return np.ascontiguousarray(np.broadcast_to(row.astype(np.float32), (SIZE, SIZE, 3)))


def resize_size(h: int, w: int) -> Tuple[int, int]:
    """(rows, columns) after the resize: the shortest edge becomes 224, the long edge int(long * 224 / short)."""
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(long * SIZE / short)
    return (new_long, SIZE) if w <= h else (SIZE, new_long)


def _pixels(picture) -> np.ndarray:
    if type(picture) is str:
        from PIL import Image

        with Image.open(picture) as im:
            return np.array(im.convert("RGB"))
    if isinstance(picture, torch.Tensor):
        picture = picture.detach().cpu().numpy()
    return np.array(picture)


def preprocess(picture) -> np.ndarray:
    """A picture - uint8 / float HxWx3 (or 1xHxWx3, HxW grey, HxWx4 with its alpha dropped) on the 0 .. 255 scale, or a file path -
    -> (224, 224, 3) float32 on the 0 .. 255 scale.  A 224 x 224 picture passes unchanged."""
    px = _pixels(picture)
    if px.ndim == 4 and px.shape[0] == 1:
        px = px[0]
    if px.ndim == 2:
        px = np.repeat(px[..., None], 3, axis=-1)
    if px.ndim != 3 or px.shape[-1] not in (3, 4) or min(px.shape[:2]) < 1:
        raise ValueError(f"clip_vision: a picture of shape {px.shape} (HxWx3 on the 0 .. 255 scale)")
    px = np.asarray(px[..., :3], dtype=np.float64)
    if not np.isfinite(px).all():
        raise ValueError("clip_vision: the picture holds NaN / Inf")
    h, w = px.shape[:2]
    nh, nw = resize_size(h, w)
    if (nh, nw) != (h, w):
        t = torch.from_numpy(np.ascontiguousarray(px)).permute(2, 0, 1)[None]
        t = torch.nn.functional.interpolate(t, size=(nh, nw), mode="bicubic", antialias=True, align_corners=False)
        px = t[0].permute(1, 2, 0).clamp_(0.0, 255.0).numpy()
    top, left = (nh - SIZE) // 2, (nw - SIZE) // 2
    return np.ascontiguousarray(px[top:top + SIZE, left:left + SIZE], dtype=np.float32)


def digest(pixels: np.ndarray) -> str:
    """What the pipeline keys its last embedding by: SHA-256 of the preprocessed fp32 pixels."""
    return hashlib.sha256(np.ascontiguousarray(pixels, dtype=np.float32).tobytes()).hexdigest()


def _ln(x, g, b):
    mean = x.mean(dim=-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(dim=-1, keepdim=True)
    return d / torch.sqrt(var + EPS) * g + b


def forward_host(weights, pixels, layers: int = wtab.VIT_LAYERS, dtype=torch.float64) -> Dict[str, np.ndarray]:
    """The tower in plain torch on the CPU.  weights: the checkpoint's state (key -> array / tensor, PyTorch layout, the key names of
    wtab.clip_vision_table); pixels (B, 224, 224, 3) or (224, 224, 3) on the 0 .. 255 scale.  Returns `image_embeds` (B, 1024),
    `last_hidden_state` (B, 257, 1280: the output of the last layer, before the post-LayerNorm) and `penultimate` (B, 257, 1280: the
    input of the last layer, diffusers' hidden_states[-2]) as arrays of `dtype`."""
    W = lambda k: torch.as_tensor(np.asarray(weights[k].detach().float().cpu() if hasattr(weights[k], "detach") else weights[k])).to(dtype)  # noqa: E731
    px = torch.as_tensor(np.asarray(pixels)).to(dtype)
    px = px[None] if px.dim() == 3 else px
    B, C, T, P, G = px.shape[0], wtab.VIT_DIM, wtab.VIT_TOKENS, wtab.VIT_PATCH, wtab.VIT_IMAGE // wtab.VIT_PATCH
    if tuple(px.shape[1:]) != (SIZE, SIZE, 3):
        raise ValueError(f"clip_vision: pixels of shape {tuple(px.shape)} ((B, {SIZE}, {SIZE}, 3))")
    scale, shift = pixel_affine()
    x = px * torch.tensor(scale, dtype=dtype) + torch.tensor(shift, dtype=dtype)
    # patches: [B][py][ky][px][kx][c] -> [B][py * 16 + px][(ky * 14 + kx) * 3 + c]
    patches = x.reshape(B, G, P, G, P, 3).permute(0, 1, 3, 2, 4, 5).reshape(B, G * G, P * P * 3)
    wp = W("vision_model.embeddings.patch_embedding.weight").permute(0, 2, 3, 1).reshape(C, P * P * 3)   # OIHW -> [O][(ky, kx, c)]
    e = patches @ wp.t()
    cls = W("vision_model.embeddings.class_embedding").reshape(1, 1, C).expand(B, 1, C)
    e = torch.cat([cls, e], dim=1) + W("vision_model.embeddings.position_embedding.weight")[None]
    x = _ln(e, W("vision_model.pre_layrnorm.weight"), W("vision_model.pre_layrnorm.bias"))
    H = wtab.VIT_HEADS
    d = C // H
    prev = x
    for i in range(int(layers)):
        ln = f"vision_model.encoder.layers.{i}."
        lin = lambda t, n: t @ W(ln + n + ".weight").t() + W(ln + n + ".bias")  # noqa: E731
        prev = x
        h = _ln(x, W(ln + "layer_norm1.weight"), W(ln + "layer_norm1.bias"))
        q, k, v = (lin(h, "self_attn." + n).reshape(B, T, H, d).permute(0, 2, 1, 3) for n in ("q_proj", "k_proj", "v_proj"))
        a = torch.softmax((q @ k.transpose(-1, -2)) * (float(d) ** -0.5), dim=-1) @ v
        x = x + lin(a.permute(0, 2, 1, 3).reshape(B, T, C), "self_attn.out_proj")
        h = _ln(x, W(ln + "layer_norm2.weight"), W(ln + "layer_norm2.bias"))
        f = lin(h, "mlp.fc1")
        f = 0.5 * f * (1.0 + torch.erf(f * (0.5 ** 0.5)))
        x = x + lin(f, "mlp.fc2")
    pooled = _ln(x[:, 0], W("vision_model.post_layernorm.weight"), W("vision_model.post_layernorm.bias"))
    emb = pooled @ W("visual_projection.weight").t()
    return {"image_embeds": emb.numpy(), "last_hidden_state": x.numpy(), "penultimate": prev.numpy()}
