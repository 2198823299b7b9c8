"""T2I-Adapter structural control (Mou et al. 2023; the TencentARC ``t2iadapter_*_sd15v2`` checkpoints, diffusers'
``StableDiffusionAdapterPipeline`` / ``T2IAdapter`` / ``MultiAdapter``, the ``t2ia_*`` models of the A1111 ControlNet extension):
``generate_image(..., t2i_adapter=...)``.

An adapter is a small conv net that runs ONCE per job, on the conditioning picture alone - no timestep, no text:

    x  = PixelUnshuffle(8)(picture)            # (B, H/8, W/8, 64 cin); channel c * 64 + dy * 8 + dx (torch's order)
    x  = conv_in(x)                            # 3x3, pad 1, 64 cin -> 320, bias
    for l in 0 .. 3 with ch = (320, 640, 1280, 1280):
        if l > 0:            x = AvgPool2d(2, 2)(x)
        if ch[l] != ch[l-1]: x = in_conv_l(x)  # 1x1, bias (levels 1 and 2 only)
        for j in 0, 1:       x = block2_lj(relu(block1_lj(x))) + x    # block1: 3x3 pad 1; block2: 1x1; C -> C with bias
        feature[l] = x                         # (B, H/8/2^l, W/8/2^l, ch[l])

(the "full adapter": diffusers' FullAdapter, the original's Adapter(channels=[320, 640, 1280, 1280], nums_rb=2, ksize=1, sk=True,
use_conv=False); picture values in [0, 1], cin 3 or 1).  Every UNet pass then adds the four features, in place, at four points of
the down path - feature[l] to the output of down_blocks.{l}.attentions.1 for l = 0, 1, 2 and feature[3] to the output of
down_blocks.3.resnets.1, before that output is pushed as a skip and before the downsampler reads it (diffusers'
down_intrablock_additional_residuals) - the same feature to every row, scaled by

    s(i, u, l) = weight_u[l] * keep(i, num_steps, start_u, end_u)            (control.keep: diffusers' rule)

for step row i, unit u and site l; the terms of several adapters (MultiAdapter) add.

This module is the host side and needs no GPU: the description (``T2IAdapterSpec`` / ``parse``), the per-call upload (``table``),
the checkpoint map (``read_state``), what such a job refuses (``REFUSED`` / ``refuse``) and the float64 statements of the network
(``forward_host``) and of the add (``add_reference``).  The device side is libminsdtf_hip_t2i.so (include/minsdtf_hip_t2i.h),
engine.emit_t2i_adapter and UNetVariant.t2i_site; the weights live in ``models.T2IAdapter``.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, fields
from typing import Dict, List, Optional, Tuple

import numpy as np

from .control import keep

MAX_UNITS = 3                        # MSDA_MAX_UNITS
SITES = 4                            # MSDA_SITES
CHANNELS = (320, 640, 1280, 1280)    # the full adapter of SD 1.5: the UNet's four levels
BLOCKS = 2                           # nums_rb
# the calls whose output takes feature[l], in engine._emit_encoder's names
SITE_NAMES = ("down_blocks.0.attentions.1", "down_blocks.1.attentions.1", "down_blocks.2.attentions.1", "down_blocks.3.resnets.1")
LAUNCHES = 31                        # engine.emit_t2i_adapter: 1 + 1 + 3 pools + 2 in_convs + 8 blocks of 3

# what a job with a T2I-Adapter cannot be combined with, in the order a refusal names them: generate_image's arguments, then states
REFUSED = (("control_net_image", "regions", "pag", "sag", "reference_only", "hypertile", "tiled", "hires"), ("denoise_streams = 2",))


@dataclass
class T2IAdapterSpec:
    """``image``: the conditioning picture, an array (0 .. 255, like `control_net_image`) or a file - (H, W, 3) for a 3-channel
    adapter, (H, W) or (H, W, 1) for a 1-channel one; it is resized to the job's size.  One of ``path`` (a T2I-Adapter checkpoint)
    and ``model`` (a models.T2IAdapter).  ``weight``: a finite float >= 0, or four of them, one per site.  ``start`` / ``end``: the
    share of the steps the adapter acts on, 0 <= start <= end <= 1."""
    image: object = None
    path: Optional[str] = None
    model: object = None
    weight: object = 1.0
    start: float = 0.0
    end: float = 1.0


_FIELDS = tuple(f.name for f in fields(T2IAdapterSpec))


def _number(what, value, ok, rule) -> float:
    try:
        v = float(value)
    except (TypeError, ValueError) as e:
        raise ValueError(f"t2i_adapter: {what} = {value!r} must be {rule}") from e
    if isinstance(value, bool) or not math.isfinite(v) or not ok(v):
        raise ValueError(f"t2i_adapter: {what} = {value!r} must be {rule}")
    return v


def _one(s, n: int) -> T2IAdapterSpec:
    where = f"unit {n}: "
    if isinstance(s, dict):
        unknown = set(s) - set(_FIELDS)
        if unknown:
            raise ValueError(f"t2i_adapter: {where}unknown field(s) {sorted(unknown)}")
        s = T2IAdapterSpec(**s)
    if not isinstance(s, T2IAdapterSpec):
        raise ValueError(f"t2i_adapter: {where}{type(s).__name__}, expected a t2iadapter.T2IAdapterSpec or a dict of its fields")
    if s.image is None:
        raise ValueError(f"t2i_adapter: {where}`image` (the conditioning picture) is missing")
    if s.path is not None and s.model is not None:
        raise ValueError(f"t2i_adapter: {where}`path` and `model` should not both be given")
    if s.path is None and s.model is None:
        raise ValueError(f"t2i_adapter: {where}one of `path` (a T2I-Adapter checkpoint) and `model` (a models.T2IAdapter) is needed")
    if s.path is not None and not isinstance(s.path, (str, os.PathLike)):
        raise ValueError(f"t2i_adapter: {where}path = {s.path!r} must be a checkpoint file name")
    rule = "a finite float >= 0, or four of them (one per site)"
    if isinstance(s.weight, (list, tuple, np.ndarray)):
        if len(s.weight) != SITES:
            raise ValueError(f"t2i_adapter: {where}weight = {s.weight!r} must be {rule}")
        weight = tuple(_number(f"{where}weight[{l}]", v, lambda x: x >= 0.0, "a finite float >= 0") for l, v in enumerate(s.weight))
    else:
        weight = (_number(f"{where}weight", s.weight, lambda x: x >= 0.0, rule),) * SITES
    start = _number(f"{where}start", s.start, lambda x: 0.0 <= x <= 1.0, "a float in [0, 1]")
    end = _number(f"{where}end", s.end, lambda x: 0.0 <= x <= 1.0, "a float in [0, 1]")
    if start > end:
        raise ValueError(f"t2i_adapter: {where}start = {start!r} > end = {end!r} (0 <= start <= end <= 1)")
    return T2IAdapterSpec(s.image, s.path, s.model, weight, start, end)


def parse(t2i_adapter) -> Optional[List[T2IAdapterSpec]]:
    """None -> None; one T2IAdapterSpec / dict of its fields, or a list of 1 .. MAX_UNITS of them -> the list of checked specs
    (``weight`` as a tuple of four floats).  ValueError naming the unit and the field for anything else."""
    if t2i_adapter is None:
        return None
    units = list(t2i_adapter) if isinstance(t2i_adapter, (list, tuple)) else [t2i_adapter]
    if not 1 <= len(units) <= MAX_UNITS:
        raise ValueError(f"t2i_adapter: {len(units)} units (1 .. {MAX_UNITS})")
    return [_one(s, n) for n, s in enumerate(units)]


def table(units, num_steps: int) -> np.ndarray:
    """The per-call upload: fp32 [num_steps][U][4], built in float64 and rounded once.  Row i is the row of the job's coefficient
    table (the device step counter), whatever step the job enters at; the last axis is the site."""
    units = parse(units)
    num_steps = int(num_steps)
    if num_steps < 1:
        raise ValueError(f"t2i_adapter: num_steps = {num_steps} (>= 1)")
    t = np.zeros((num_steps, len(units), SITES), dtype=np.float64)
    for n, u in enumerate(units):
        w = np.asarray(u.weight, dtype=np.float64)
        for i in range(num_steps):
            t[i, n] = w * keep(i, num_steps, u.start, u.end)
    return t.astype(np.float32)


def picture(image, in_channels: int, height: int, width: int, resize=None) -> np.ndarray:
    """An adapter's conditioning picture -> float32 (1, height, width, in_channels) in [0, 1], by the route of a ControlNet hint
    (StableDiffusionBase._hint_batch): an array (0 .. 255) is checked for its channel count and goes through `resize`, the
    pipeline's bilinear resize; a file - a name, an os.PathLike or an open binary file - is decoded by PIL, converted to RGB or L as
    the adapter needs and resized by PIL, so a file of any mode fits.  ValueError naming both channel counts when an array does
    not fit the adapter."""
    if isinstance(image, (str, os.PathLike)) or hasattr(image, "read"):
        from PIL import Image

        with Image.open(image) as im:
            px = np.array(im.convert("RGB" if in_channels == 3 else "L").resize((int(width), int(height))))
    else:
        px = np.asarray(image)
    if px.ndim == 2:
        px = px[..., None]
    if px.ndim != 3 or px.shape[-1] != in_channels:
        got = px.shape[-1] if px.ndim == 3 else None
        raise ValueError(f"t2i_adapter: a picture of shape {px.shape} ({got} channel(s)) for an adapter of {in_channels} input channel(s): "
                         + ("(H, W, 3)" if in_channels == 3 else "(H, W) or (H, W, 1)"))
    px = np.asarray(px, dtype=np.float32)
    if px.shape[:2] != (int(height), int(width)):
        if resize is None:
            raise ValueError(f"t2i_adapter: a picture of {px.shape[0]} x {px.shape[1]}, the job is {height} x {width}")
        px = resize(px, int(height), int(width))
    px = np.asarray(px, dtype=np.float32) / np.float32(255.0)
    if not np.isfinite(px).all():
        raise ValueError("t2i_adapter: the picture has non-finite values")
    return np.ascontiguousarray(px[None])


def check_size(height: int, width: int) -> None:
    """ValueError unless the four levels are whole: the picture is unshuffled by 8 and pooled three times."""
    if height < 64 or width < 64 or height % 64 or width % 64:
        raise ValueError(f"t2i_adapter: a {height} x {width} job - the adapter's four levels need a height and a width that are "
                         "multiples of 64")


# ---- the public T2I-Adapter file layouts ------------------------------------------------------------------------------------------
def layer_names(in_channels: int = 3) -> List[Tuple[str, Tuple[int, ...]]]:
    """(layer, torch weight shape) of every conv of a full adapter, in forward order, under diffusers' names without the leading
    `adapter.`: conv_in, body.{l}.in_conv, body.{l}.resnets.{j}.block{1,2}."""
    out = [("conv_in", (CHANNELS[0], 64 * int(in_channels), 3, 3))]
    for l, ch in enumerate(CHANNELS):
        if l > 0 and ch != CHANNELS[l - 1]:
            out.append((f"body.{l}.in_conv", (ch, CHANNELS[l - 1], 1, 1)))
        for j in range(BLOCKS):
            out.append((f"body.{l}.resnets.{j}.block1", (ch, ch, 3, 3)))
            out.append((f"body.{l}.resnets.{j}.block2", (ch, ch, 1, 1)))
    return out


def _original_key(layer: str) -> str:
    """diffusers' layer name -> the original (TencentARC) one: body.{2 l + j}.block{1,2}, body.{2 l}.in_conv."""
    p = layer.split(".")
    if p[0] == "conv_in":
        return layer
    l = int(p[1])
    if p[2] == "in_conv":
        return f"body.{BLOCKS * l}.in_conv"
    return f"body.{BLOCKS * l + int(p[3])}.{p[4]}"


def read_state(state) -> Dict[str, np.ndarray]:
    """A loaded T2I-Adapter checkpoint in either public layout - diffusers' (`adapter.conv_in.weight`, `adapter.body.{l}.in_conv.*`,
    `adapter.body.{l}.resnets.{j}.block{1,2}.*`) or the original (`conv_in.*`, `body.{2 l + j}.block{1,2}.*`, `body.{2 l}.in_conv.*`) -
    as {"<layer>.weight", "<layer>.bias"} float32 arrays in torch's shapes under layer_names()' names; fp16 files load.  Every
    shape is verified.  ValueError naming what was found for a `skep` checkpoint (sk=False), a light adapter, SDXL widths, a
    missing key or a wrong shape."""
    flat = dict(state)

    def arr(key):
        v = flat[key]
        v = v.detach().to("cpu").float().numpy() if hasattr(v, "detach") else np.asarray(v)
        return np.ascontiguousarray(v, dtype=np.float32)

    skep = sorted(k for k in flat if ".skep." in k)
    if skep:
        raise ValueError(f"t2i_adapter: the checkpoint has `skep` keys ({skep[0]}, ...): an adapter built with sk=False is not supported")
    diffusers = any(k.startswith("adapter.") for k in flat)
    prefix = "adapter." if diffusers else ""
    if f"{prefix}conv_in.weight" not in flat:
        raise ValueError(f"t2i_adapter: the checkpoint has no {prefix + 'conv_in.weight'!r}")
    cw = arr(f"{prefix}conv_in.weight")
    if cw.ndim != 4 or cw.shape[0] != CHANNELS[0] or cw.shape[2:] != (3, 3) or cw.shape[1] not in (64, 192):
        raise ValueError(f"t2i_adapter: {prefix}conv_in.weight has shape {cw.shape}, expected ({CHANNELS[0]}, 64 or 192, 3, 3): the full "
                         "adapter of SD 1.5 (an SDXL adapter unshuffles by 16 and starts at 256 * cin inputs; a light adapter has other widths)")
    cin = cw.shape[1] // 64
    out: Dict[str, np.ndarray] = {}
    known = set()
    for layer, shape in layer_names(cin):
        src = prefix + (layer if diffusers else _original_key(layer))
        for suffix, want in (("weight", shape), ("bias", shape[:1])):
            key = f"{src}.{suffix}"
            known.add(key)
            if key not in flat:
                raise ValueError(f"t2i_adapter: the checkpoint has no {key!r}")
            a = arr(key)
            if a.shape != want:
                raise ValueError(f"t2i_adapter: {key} has shape {a.shape}, expected {want} (channels {CHANNELS}: a light adapter or "
                                 "SDXL widths are not supported)")
            out[f"{layer}.{suffix}"] = a
    extra = sorted(k for k in flat if k not in known and (k.startswith(prefix + "body.") or k.startswith(prefix + "conv_in.")))
    if extra:
        raise ValueError(f"t2i_adapter: unexpected checkpoint keys {extra[:4]} (a full adapter has two blocks per level and in_conv at "
                         "levels 1 and 2 only)")
    return out


def in_channels_of(named) -> int:
    return int(np.asarray(named["conv_in.weight"]).shape[1]) // 64


def synthetic_state(seed: int = 0, in_channels: int = 3, scale: float = 1.0, layout: str = "diffusers") -> Dict[str, np.ndarray]:
    """The flat state dict of a seeded synthetic adapter in a public file layout ("diffusers" or "original"), float32: Glorot-uniform
    convs (times `scale`) and small biases."""
    if int(in_channels) not in (1, 3) or layout not in ("diffusers", "original"):
        raise ValueError(f"t2i_adapter: synthetic_state(in_channels={in_channels!r}, layout={layout!r})")
    rng = np.random.default_rng([int(seed), 0x721A])
    state = {}
    for layer, shape in layer_names(in_channels):
        fan_in, fan_out = shape[1] * shape[2] * shape[3], shape[0] * shape[2] * shape[3]
        lim = float(np.sqrt(6.0 / (fan_in + fan_out))) * scale
        key = "adapter." + layer if layout == "diffusers" else _original_key(layer)
        state[key + ".weight"] = rng.uniform(-lim, lim, size=shape).astype(np.float32)
        state[key + ".bias"] = rng.uniform(-0.05, 0.05, size=shape[:1]).astype(np.float32)
    return state


# ---- what does not go together --------------------------------------------------------------------------------------------------
def refuse(given: dict, streams=None) -> None:
    """ValueError naming every argument of `given` (generate_image's, by name) that is set and every state that holds which a job
    with a T2I-Adapter cannot take."""
    arguments, states = REFUSED
    holds = {"denoise_streams = 2": streams == 2}
    refused = [n for n in arguments if given.get(n) is not None] + [s for s in states if holds[s]]
    if refused:
        raise ValueError("t2i_adapter: the adapter's features enter the plain UNet rows of one stream, one picture per job: it cannot be "
                         f"combined with {', '.join(refused)}")


# ---- the float64 statements -----------------------------------------------------------------------------------------------------
def unshuffle_host(x: np.ndarray, r: int = 8) -> np.ndarray:
    """PixelUnshuffle(r) on NHWC: (B, H, W, C) -> (B, H / r, W / r, C r r), channel c * r * r + dy * r + dx."""
    B, H, W, C = x.shape
    x = x.reshape(B, H // r, r, W // r, r, C)           # b, y, dy, x, dx, c
    return x.transpose(0, 1, 3, 5, 2, 4).reshape(B, H // r, W // r, C * r * r)


def _conv_host(x: np.ndarray, w: np.ndarray, b: np.ndarray) -> np.ndarray:
    """NHWC float64 convolution with torch's weight (out, in, k, k), k = 1 or 3 with padding k // 2, and bias."""
    k = w.shape[2]
    B, H, W, _C = x.shape
    if k == 1:
        return x @ w[:, :, 0, 0].T + b
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((B, H, W, w.shape[0]), dtype=np.float64) + b
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + H, kx:kx + W, :] @ w[:, :, ky, kx].T
    return out


def forward_host(state, picture01) -> List[np.ndarray]:
    """The adapter network in float64: `state` as read_state returns it (or a checkpoint in a public layout), picture01 (B, H, W,
    cin) or (H, W, cin) in [0, 1], H and W multiples of 64 -> the four features, float64 NHWC."""
    named = state if "body.0.resnets.0.block1.weight" in state else read_state(state)   # (read_state's own keys, or a file's)
    W = {k: np.asarray(v, dtype=np.float64) for k, v in named.items()}
    x = np.asarray(picture01, dtype=np.float64)
    x = x[None] if x.ndim == 3 else x
    cin = in_channels_of(named)
    if x.ndim != 4 or x.shape[-1] != cin:
        raise ValueError(f"t2i_adapter: a picture of shape {x.shape} for an adapter of {cin} input channel(s)")
    check_size(x.shape[1], x.shape[2])
    x = _conv_host(unshuffle_host(x), W["conv_in.weight"], W["conv_in.bias"])
    feats = []
    for l, ch in enumerate(CHANNELS):
        if l > 0:
            B, H, Wd, C = x.shape
            x = x.reshape(B, H // 2, 2, Wd // 2, 2, C).mean(axis=(2, 4))
            if ch != CHANNELS[l - 1]:
                x = _conv_host(x, W[f"body.{l}.in_conv.weight"], W[f"body.{l}.in_conv.bias"])
        for j in range(BLOCKS):
            n = f"body.{l}.resnets.{j}"
            h = np.maximum(_conv_host(x, W[n + ".block1.weight"], W[n + ".block1.bias"]), 0.0)
            x = _conv_host(h, W[n + ".block2.weight"], W[n + ".block2.bias"]) + x
        feats.append(x)
    return feats


def add_reference(x, feats, scales) -> np.ndarray:
    """msda_feature_add in float64: x (rows, n), feats a list of U arrays (n,), scales the U table entries of the step and site;
    returns (rows, n).  A unit at scale 0 drops out whatever its feature holds; with every scale 0 x comes back as it is."""
    out = np.array(x, dtype=np.float64)
    for f, s in zip(feats, scales):
        if float(s) != 0.0:
            out = out + float(s) * np.asarray(f, dtype=np.float64).reshape(1, -1)
    return out
