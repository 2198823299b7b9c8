"""Tiled diffusion (MultiDiffusion / Mixture-of-Diffusers): a canvas larger than the UNet's own size is denoised as overlapping
views of one latent (``generate_image(..., tiled=...)``).

Every step the UNet runs at the pipeline's own size on every view (the views are batch rows of the one denoise engine), each view
takes its own sampler step, and one launch (``msd_tile_consensus``) replaces every canvas pixel - and every view's entry for that
pixel - by the weighted mean of the stepped views that cover it.  This module is the host side of it and needs no GPU: the job
description (``TiledSpec`` / ``parse``), the view offsets and blend weight rows (``Geometry``), the view slicing of canvas-shaped
host draws (``slice_views``) and a float64 statement of the kernel (``consensus_reference``).

Offsets per axis, in latent units, for a canvas of length L, a tile of length t and a stride s:
n = ceil((L - t) / s) + 1 views at off[i] = min(i * s, L - t) - the last view is snapped to the edge, and there is one view when
L == t.  Views are ordered row-major, v = r * cols + c, and the tile buffer is sample-major: row b * V + v.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np

BLENDS = ("uniform", "gaussian")
MAX_AXIS_VIEWS = 64       # MSD_TILE_MAX_VIEWS: offsets travel by value in the kernel arguments
GAUSSIAN_VAR = 0.01       # Mixture-of-Diffusers' variance of the tile weight, in units of the tile length
# the largest view batch (images * views) generate_image accepts: the largest one the GPU tests ran at the 512-px tile
MAX_VIEW_BATCH = 6
MODE_CONSENSUS, MODE_GATHER = 0, 1


@dataclass(frozen=True)
class TiledSpec:
    """A tiled job: the canvas ``size = (height, width)`` in pixels (multiples of 64, at least the pipeline's own size, which
    is the tile), the view ``stride`` in pixels (an int or (sy, sx); multiples of 8, at most the tile side; default: half the
    tile per axis) and the ``blend`` of overlapping views (one of BLENDS)."""
    size: Tuple[int, int] = None
    stride: Union[None, int, Tuple[int, int]] = None
    blend: str = "uniform"


def axis_offsets(length: int, tile: int, stride: int) -> Tuple[int, ...]:
    """View offsets of one axis (any unit): n = ceil((L - t) / s) + 1, off[i] = min(i * s, L - t)."""
    length, tile, stride = int(length), int(tile), int(stride)
    if tile < 1 or length < tile or stride < 1:
        raise ValueError(f"tiled: axis of length {length}, tile {tile}, stride {stride}")
    n = -(-(length - tile) // stride) + 1
    return tuple(min(i * stride, length - tile) for i in range(n))


def weight_row(tile: int, blend: str) -> np.ndarray:
    """The blend weights along one axis of a tile, computed in float64 and stored as fp32 [tile]."""
    if blend not in BLENDS:
        raise ValueError(f"tiled: unknown blend {blend!r}: choose one of {', '.join(BLENDS)}")
    t = int(tile)
    if blend == "uniform":
        return np.ones(t, dtype=np.float32)
    i = np.arange(t, dtype=np.float64)
    return np.exp(-(((i - (t - 1) / 2.0) / t) ** 2) / (2.0 * GAUSSIAN_VAR)).astype(np.float32)


@dataclass(frozen=True)
class Geometry:
    """A TiledSpec resolved against a pipeline size.  height / width: the canvas in pixels; th, tw, H, W: tile and canvas in
    latent units; ys / xs: the view offsets per axis in latent units."""
    height: int
    width: int
    th: int
    tw: int
    H: int
    W: int
    ys: Tuple[int, ...]
    xs: Tuple[int, ...]
    blend: str

    @property
    def rows(self) -> int:
        return len(self.ys)

    @property
    def cols(self) -> int:
        return len(self.xs)

    @property
    def views(self) -> int:
        return len(self.ys) * len(self.xs)

    @property
    def key(self) -> tuple:
        """What an engine built for this geometry is keyed by."""
        return ("tiled", self.th, self.tw, self.H, self.W, self.ys, self.xs, self.blend)

    @property
    def wy(self) -> np.ndarray:
        return weight_row(self.th, self.blend)

    @property
    def wx(self) -> np.ndarray:
        return weight_row(self.tw, self.blend)

    def offsets(self):
        """(y, x) of every view, row-major."""
        return [(y, x) for y in self.ys for x in self.xs]


def geometry(th: int, tw: int, H: int, W: int, ys, xs, blend: str = "uniform") -> Geometry:
    """A Geometry from latent-unit sizes and explicit offsets, checked the way msd_tile_consensus checks them."""
    ys, xs = tuple(int(v) for v in ys), tuple(int(v) for v in xs)
    if blend not in BLENDS:
        raise ValueError(f"tiled: unknown blend {blend!r}: choose one of {', '.join(BLENDS)}")
    for name, off, t, L in (("ys", ys, int(th), int(H)), ("xs", xs, int(tw), int(W))):
        if t < 1 or L < t:
            raise ValueError(f"tiled: {name}: canvas length {L} with tile length {t}")
        if not 1 <= len(off) <= MAX_AXIS_VIEWS:
            raise ValueError(f"tiled: {name}: {len(off)} views on one axis (1 .. {MAX_AXIS_VIEWS})")
        if off[0] != 0 or off[-1] != L - t:
            raise ValueError(f"tiled: {name} = {off} must start at 0 and end at {L - t}")
        if any(b <= a or b - a > t for a, b in zip(off, off[1:])):
            raise ValueError(f"tiled: {name} = {off} must ascend strictly in steps of at most the tile length {t}")
    return Geometry(int(H) * 8, int(W) * 8, int(th), int(tw), int(H), int(W), ys, xs, blend)


def _pair(value, what):
    if isinstance(value, (int, np.integer)) and not isinstance(value, bool):
        return int(value), int(value)
    try:
        a, b = value
        if isinstance(a, bool) or isinstance(b, bool) or int(a) != a or int(b) != b:
            raise TypeError
        return int(a), int(b)
    except (TypeError, ValueError) as e:
        raise ValueError(f"tiled: {what} must be whole pixels, (y, x) or one int, got {value!r}") from e


def parse(tiled, img_height: int, img_width: int) -> Optional[Geometry]:
    """None -> None; a TiledSpec or a dict of its fields -> the resolved Geometry.  ValueError for an unknown field or blend,
    a canvas that is not a multiple of 64 or is smaller than the tile, a stride that is not a positive multiple of 8 or exceeds
    the tile, more than MAX_AXIS_VIEWS views on an axis."""
    if tiled is None:
        return None
    if isinstance(tiled, Geometry):
        if (tiled.th * 8, tiled.tw * 8) != (img_height, img_width):
            raise ValueError(f"tiled: the geometry's tile is {tiled.th * 8}x{tiled.tw * 8}, the pipeline's size {img_height}x{img_width}")
        return tiled
    if isinstance(tiled, dict):
        unknown = set(tiled) - {"size", "stride", "blend"}
        if unknown:
            raise ValueError(f"tiled: unknown field(s) {sorted(unknown)}")
        tiled = TiledSpec(**tiled)
    if not isinstance(tiled, TiledSpec):
        raise ValueError(f"tiled must be a TiledSpec, a dict or None, not {type(tiled).__name__}")
    if tiled.blend not in BLENDS:
        raise ValueError(f"tiled: unknown blend {tiled.blend!r}: choose one of {', '.join(BLENDS)}")
    if tiled.size is None:
        raise ValueError("tiled: give the canvas as `size` = (height, width)")
    if isinstance(tiled.size, (int, np.integer)):
        raise ValueError(f"tiled: size must be (height, width), got {tiled.size!r}")
    ch, cw = _pair(tiled.size, "size")
    if img_height % 8 or img_width % 8:
        raise ValueError(f"tiled: the tile {img_height}x{img_width} must be a multiple of 8 in both dimensions")
    if ch % 64 or cw % 64:
        raise ValueError(f"tiled: the canvas {ch}x{cw} must be a multiple of 64 in both dimensions")
    if ch < img_height or cw < img_width:
        raise ValueError(f"tiled: the canvas {ch}x{cw} is smaller than the tile {img_height}x{img_width}")
    if tiled.stride is None:
        sy, sx = img_height // 2, img_width // 2
    else:
        sy, sx = _pair(tiled.stride, "stride")
    for s, t in ((sy, img_height), (sx, img_width)):
        if s < 8 or s % 8:
            raise ValueError(f"tiled: the stride {sy}x{sx} must be a positive multiple of 8 in both dimensions")
        if s > t:
            raise ValueError(f"tiled: the stride {sy}x{sx} exceeds the tile {img_height}x{img_width}: pixels would be left uncovered")
    th, tw, H, W = img_height // 8, img_width // 8, ch // 8, cw // 8
    ys, xs = axis_offsets(H, th, sy // 8), axis_offsets(W, tw, sx // 8)
    if len(ys) > MAX_AXIS_VIEWS or len(xs) > MAX_AXIS_VIEWS:
        raise ValueError(f"tiled: {len(ys)} x {len(xs)} views: at most {MAX_AXIS_VIEWS} per axis")
    return geometry(th, tw, H, W, ys, xs, tiled.blend)


def slice_views(x, geo: Geometry):
    """Canvas-shaped data (batch, ..., H, W, C), a host array or a tensor -> its views (batch * V, ..., th, tw, C), sample-major
    and row-major over the views: what the gather launch does to the start noise, done here for per-step draws, so that
    overlapping pixels of two views share a draw."""
    if tuple(x.shape[-3:-1]) != (geo.H, geo.W):
        raise ValueError(f"tiled: data of shape {tuple(x.shape)} is not at the canvas shape (.., {geo.H}, {geo.W}, C)")
    parts = [x[b, ..., y:y + geo.th, xo:xo + geo.tw, :] for b in range(x.shape[0]) for (y, xo) in geo.offsets()]
    if isinstance(x, np.ndarray):
        return np.stack(parts, axis=0)
    import torch

    return torch.stack(parts, dim=0)


def consensus_reference(tiles, geo: Geometry):
    """float64 statement of msd_tile_consensus, mode 0: (canvas (batch, H, W, C), tiles after the launch (batch * V, th, tw, C)).
    canvas[b, Y, X] = sum_v w_v x_v / sum_v w_v over the views that cover (Y, X), w_v = wy[Y - ys[r]] * wx[X - xs[c]] of the fp32
    weight rows, x_v the view's entry; a pixel covered by one view is that entry itself.  Every covering entry then holds the
    canvas value."""
    tiles = np.asarray(tiles, dtype=np.float64)
    V = geo.views
    if tiles.ndim != 4 or tiles.shape[0] % V or tuple(tiles.shape[1:3]) != (geo.th, geo.tw):
        raise ValueError(f"tiled: tiles of shape {tiles.shape} for {V} views of {geo.th} x {geo.tw}")
    B, C = tiles.shape[0] // V, tiles.shape[3]
    w2 = np.outer(geo.wy.astype(np.float64), geo.wx.astype(np.float64))[None, :, :, None]
    acc = np.zeros((B, geo.H, geo.W, C), dtype=np.float64)
    wsum = np.zeros((1, geo.H, geo.W, 1), dtype=np.float64)
    count = np.zeros((geo.H, geo.W), dtype=np.int64)
    single = np.zeros((B, geo.H, geo.W, C), dtype=np.float64)
    t5 = tiles.reshape(B, V, geo.th, geo.tw, C)
    for v, (y, x) in enumerate(geo.offsets()):
        sl = (slice(None), slice(y, y + geo.th), slice(x, x + geo.tw))
        acc[sl] += w2 * t5[:, v]
        wsum[sl] += w2
        count[sl[1:]] += 1
        single[sl] = t5[:, v]
    if count.min() < 1:
        raise ValueError("tiled: the views do not cover the canvas")
    canvas = np.where((count == 1)[None, :, :, None], single, acc / wsum)
    out = np.stack([canvas[b, y:y + geo.th, x:x + geo.tw] for b in range(B) for (y, x) in geo.offsets()], axis=0)
    return canvas, out
