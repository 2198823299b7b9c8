"""HyperTile (tfernd/HyperTile; the option of that name in the A1111 web UI, Forge and ComfyUI): windowed self-attention for large
pictures, ``generate_image(..., hypertile=...)``.

At 1024x1024 the level-0 self-attention is 16,384 queries against 16,384 keys, 16x the work of the 512x512 job the model was
trained at, where the convolutions are only 4x.  HyperTile computes each selected ``attn1`` independently inside non-overlapping
rectangular windows of the feature map: with nh x nw windows the attention FLOPs fall by nh * nw, and every window has the token
count of the training size, which also reduces the duplicated-subject artefacts of large SD 1.5 pictures.  q, k and v are
per-token projections, so only the attention product changes: softmax(q k^T) v is taken per window (``msd_attention_windowed``,
csrc/window_attn.hip: one launch on the operands where the q|k|v GEMM wrote them, nothing gathered).

The tile is given in picture pixels and is FIXED: the original draws a random tile divisor per call, this one is deterministic,
so a sample stays bit-identical whatever batch it runs in.  The same number of windows applies at every
selected level (levels 0 .. depth; level 0 is the first, d = 40), as the original does; deeper levels and the mid block stay plain.

This module is the host side and needs no GPU: the job description (``HypertileSpec`` / ``parse``), its geometry on a picture
(``Resolved.windows``, ``level_geometry``) and a float64 statement of the kernel (``attention_windowed_reference``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, List, Optional, Tuple

import numpy as np

MAX_DEPTH = 2   # levels 0 .. 2 carry the head sizes 40 / 80 / 160 of msd_attention_windowed; level 3 has no attention blocks


@dataclass
class HypertileSpec:
    """``tile``: the window in picture pixels, an int or (height, width); ``depth``: the UNet levels 0 .. depth are windowed
    (0: the d = 40 blocks only)."""
    tile: Any = 512
    depth: int = 0


@dataclass(frozen=True)
class Resolved:
    """A HypertileSpec checked: tile (height, width) positive ints, each a multiple of 64 * 2**depth; depth in 0 .. 2."""
    tile: Tuple[int, int]
    depth: int

    def windows(self, height_px: int, width_px: int) -> Tuple[int, int]:
        """(nh, nw) on a picture of this size; ValueError naming the nearest valid tiles when the tile does not divide it."""
        out = []
        for axis, size, t in (("height", int(height_px), self.tile[0]), ("width", int(width_px), self.tile[1])):
            if size % t:
                near = nearest_tiles(size, t, self.depth)
                raise ValueError(f"hypertile: tile {axis} {t} does not divide the picture's {axis} {size} px; the nearest valid "
                                 f"tiles at depth {self.depth} are {', '.join(str(v) for v in near) if near else 'none'}")
            out.append(size // t)
        return out[0], out[1]

    def key(self, height_px: int, width_px: int) -> Tuple[int, int, int]:
        """(nh, nw, depth): what an engine of this picture size is keyed by."""
        nh, nw = self.windows(height_px, width_px)
        return nh, nw, self.depth


def valid_tiles(size_px: int, depth: int) -> List[int]:
    """The tile sizes a picture side of `size_px` takes at `depth`: its divisors that are multiples of 64 * 2**depth."""
    unit = 64 << int(depth)
    return [t for t in range(unit, int(size_px) + 1, unit) if size_px % t == 0]


def nearest_tiles(size_px: int, tile: int, depth: int) -> List[int]:
    """The valid tiles next to `tile`: the largest one below it and the smallest one at or above it (one or both may be missing)."""
    v = valid_tiles(size_px, depth)
    below = [t for t in v if t < tile]
    above = [t for t in v if t >= tile]
    return below[-1:] + above[:1]


def parse(hypertile) -> Optional[Resolved]:
    """None -> None; a HypertileSpec or a dict of its fields -> the checked description.  ValueError for an unknown field, a depth
    outside 0 .. 2, or a tile that is not a positive multiple of 64 * 2**depth (so that a window row is a multiple of 8 tokens at
    the deepest selected level)."""
    if hypertile is None:
        return None
    if isinstance(hypertile, Resolved):
        return hypertile
    if isinstance(hypertile, dict):
        unknown = set(hypertile) - {"tile", "depth"}
        if unknown:
            raise ValueError(f"hypertile: unknown field(s) {sorted(unknown)}")
        hypertile = HypertileSpec(**hypertile)
    if not isinstance(hypertile, HypertileSpec):
        raise ValueError(f"hypertile must be a HypertileSpec, a dict or None, not {type(hypertile).__name__}")
    depth = hypertile.depth
    if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or not 0 <= int(depth) <= MAX_DEPTH:
        raise ValueError(f"hypertile: depth = {depth!r} must be an int in 0 .. {MAX_DEPTH}")
    depth = int(depth)
    tile = hypertile.tile
    pair = (tile, tile) if isinstance(tile, (int, np.integer)) and not isinstance(tile, bool) else tile
    try:
        th, tw = pair
    except (TypeError, ValueError) as e:
        raise ValueError(f"hypertile: tile = {tile!r} must be an int or (height, width) in pixels") from e
    unit = 64 << depth
    for t in (th, tw):
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or t < 1:
            raise ValueError(f"hypertile: tile = {tile!r} must be an int or (height, width) of positive ints, in pixels")
        if t % unit:
            lo, hi = (int(t) // unit) * unit, (int(t) // unit + 1) * unit
            raise ValueError(f"hypertile: tile {int(t)} is not a multiple of {unit} px (64 * 2**depth, depth = {depth}: a window row is "
                             f"whole 16-byte chunks at every selected level); the nearest valid tiles are "
                             f"{', '.join(str(v) for v in (lo, hi) if v > 0)}")
    return Resolved((int(th), int(tw)), depth)


def level_geometry(h: int, w: int, nh: int, nw: int, depth: int) -> List[Tuple[int, int, int, int]]:
    """(H_l, W_l, wh_l, ww_l) of the levels 0 .. depth of a latent of h x w: the feature map and the window of
    msd_attention_windowed there.  ValueError when a level does not split into nh x nw whole windows of a multiple of 8 tokens."""
    h, w, nh, nw, depth = int(h), int(w), int(nh), int(nw), int(depth)
    if not 0 <= depth <= MAX_DEPTH or nh < 1 or nw < 1:
        raise ValueError(f"hypertile: {nh} x {nw} windows at depth {depth} (windows >= 1, depth in 0 .. {MAX_DEPTH})")
    out = []
    for lvl in range(depth + 1):
        if h % (1 << lvl) or w % (1 << lvl):
            raise ValueError(f"hypertile: a {h} x {w} latent has no whole level {lvl}")
        H, W = h >> lvl, w >> lvl
        if H % nh or W % nw or (W // nw) % 8:
            raise ValueError(f"hypertile: level {lvl} ({H} x {W} tokens) does not split into {nh} x {nw} windows whose width is a "
                             "multiple of 8 tokens")
        out.append((H, W, H // nh, W // nw))
    return out


def window_tokens(h: int, w: int, wh: int, ww: int) -> np.ndarray:
    """int64 (nh * nw, wh * ww): the image tokens (y * w + x) of every window, windows row-major, tokens in window-linear order."""
    h, w, wh, ww = int(h), int(w), int(wh), int(ww)
    if h % wh or w % ww:
        raise ValueError(f"window_tokens: {wh} x {ww} windows do not tile {h} x {w}")
    tok = np.arange(h * w, dtype=np.int64).reshape(h // wh, wh, w // ww, ww)
    return tok.transpose(0, 2, 1, 3).reshape((h // wh) * (w // ww), wh * ww)


def attention_windowed_reference(q, k, v, heads: int, h: int, w: int, wh: int, ww: int) -> np.ndarray:
    """float64 statement of msd_attention_windowed.  q (B, S, C) carrying scale * log2(e), k / v (B, S, C), S = h * w, C = heads * d.
    Returns (B, S, C): per sample, head and window, softmax2(q k^T) v over the window's keys, softmax2 the base-2 softmax."""
    q, k, v = (np.asarray(x, dtype=np.float64) for x in (q, k, v))
    B, S, C = q.shape
    if S != int(h) * int(w):
        raise ValueError(f"attention_windowed_reference: {S} tokens for a {h} x {w} map")
    d = C // heads
    out = np.empty((B, S, C), dtype=np.float64)
    for idx in window_tokens(h, w, wh, ww):
        n = idx.size
        qh = q[:, idx].reshape(B, n, heads, d)
        kh = k[:, idx].reshape(B, n, heads, d)
        vh = v[:, idx].reshape(B, n, heads, d)
        s = np.einsum("bshd,bthd->bhst", qh, kh)
        p = np.exp2(s - s.max(-1, keepdims=True))
        o = np.einsum("bhst,bthd->bshd", p / p.sum(-1, keepdims=True), vh)
        out[:, idx] = o.reshape(B, n, C)
    return out
