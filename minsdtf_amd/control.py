"""ControlNet units (the A1111 ControlNet extension's units, ComfyUI's "Apply ControlNet (Advanced)", diffusers'
``controlnet_conditioning_scale`` / ``control_guidance_start`` / ``control_guidance_end`` / ``guess_mode`` / ``MultiControlNetModel``):
``generate_image(..., control_net_image=img, control=...)``.

A ControlNet hands the UNet 13 residuals r_k, one per skip connection and one for the mid block's output.  A unit scales them:

    s(i, n, k, half) = weight_k * keep(i) * (0.825 ** (12 - k) if mode != "balanced" else 1)
    s(i, n, k, u)    = 0 if mode == "control"
    keep(i)          = 0.0 if (i / num_steps < start or (i + 1) / num_steps > end) else 1.0      (diffusers' rule)

for step row i, unit n, tap k and the two halves of the guidance pair (u: unconditional rows, c: conditional rows), and the skips
of a pass become skip_k + sum_n s_n r_n,k - several units add up.  "prompt" ("my prompt is more important") is the soft
injection, weaker towards the shallow taps; "control" ("ControlNet is more important") is that on the conditional half alone.

This module is the host side and needs no GPU: the unit description (``ControlUnit`` / ``parse``), the per-call upload (``table``)
and the host statement of the scaling the host loop uses (``scale_host``).  The device side is msdc_control_combine
(include/minsdtf_hip_control.h).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, fields
from typing import Optional, Tuple

import numpy as np

MODES = ("balanced", "prompt", "control")
MAX_UNITS = 3        # MSDC_MAX_UNITS
TAPS = 13            # MSDC_TAPS
SOFT = 0.825         # the soft-injection base: tap k is scaled by SOFT ** (12 - k)


@dataclass
class ControlUnit:
    """``weight``: a finite float >= 0, or 13 of them, one per tap; ``start`` / ``end``: the share of the steps the unit acts on,
    0 <= start <= end <= 1; ``mode``: one of MODES.  A unit behind the first also carries its own ``image`` (the conditioning
    picture, as `control_net_image` takes it) and at most one of ``path`` (another ControlNet checkpoint; None: the pipeline's own
    ``controlnet_path``, on this picture) and ``models`` = (ControlNet, HintNet), objects that already hold weights."""
    weight: object = 1.0
    start: float = 0.0
    end: float = 1.0
    mode: str = "balanced"
    image: object = None
    path: Optional[str] = None
    models: Optional[tuple] = None


@dataclass(frozen=True)
class Resolved:
    """A ControlUnit checked: `weight` as 13 floats."""
    weight: Tuple[float, ...]
    start: float
    end: float
    mode: str
    image: object = None
    path: Optional[str] = None
    models: Optional[tuple] = None


_FIELDS = tuple(f.name for f in fields(ControlUnit))


def _number(what, value, ok, rule) -> float:
    try:
        v = float(value)
    except (TypeError, ValueError) as e:
        raise ValueError(f"control: {what} = {value!r} must be {rule}") from e
    if isinstance(value, bool) or not math.isfinite(v) or not ok(v):
        raise ValueError(f"control: {what} = {value!r} must be {rule}")
    return v


def _unit(i: int, u) -> Resolved:
    if isinstance(u, Resolved):
        return u
    if isinstance(u, dict):
        unknown = set(u) - set(_FIELDS)
        if unknown:
            raise ValueError(f"control: unit {i}: unknown field(s) {sorted(unknown)}")
        u = ControlUnit(**u)
    if not isinstance(u, ControlUnit):
        raise ValueError(f"control: unit {i} is {type(u).__name__}, expected a control.ControlUnit or a dict of its fields")
    w = u.weight
    if isinstance(w, (list, tuple, np.ndarray)):
        if len(w) != TAPS:
            raise ValueError(f"control: unit {i}: weight has {len(w)} entries, expected one float or {TAPS} (one per tap)")
        weight = tuple(_number(f"unit {i}: weight[{k}]", v, lambda x: x >= 0.0, "a finite float >= 0") for k, v in enumerate(w))
    else:
        weight = (_number(f"unit {i}: weight", w, lambda x: x >= 0.0, "a finite float >= 0"),) * TAPS
    start = _number(f"unit {i}: start", u.start, lambda x: 0.0 <= x <= 1.0, "a float in [0, 1]")
    end = _number(f"unit {i}: end", u.end, lambda x: 0.0 <= x <= 1.0, "a float in [0, 1]")
    if start > end:
        raise ValueError(f"control: unit {i}: start = {start!r} > end = {end!r} (0 <= start <= end <= 1)")
    if not isinstance(u.mode, str) or u.mode not in MODES:
        raise ValueError(f"control: unit {i}: mode = {u.mode!r} must be one of {MODES}")
    if i == 0:
        if u.image is not None or u.path is not None or u.models is not None:
            raise ValueError("control: unit 0 is the pipeline's own ControlNet on `control_net_image`: it takes no image, path or models")
    else:
        if u.image is None:
            raise ValueError(f"control: unit {i} needs its own `image`")
        if u.path is not None and u.models is not None:
            raise ValueError(f"control: unit {i}: `path` and `models` should not both be given")
        if u.models is not None and (not isinstance(u.models, (tuple, list)) or len(u.models) != 2):
            raise ValueError(f"control: unit {i}: models = {u.models!r} must be (ControlNet, HintNet)")
    return Resolved(weight, start, end, u.mode, u.image, u.path, None if u.models is None else tuple(u.models))


def parse(control) -> Optional[Tuple[Resolved, ...]]:
    """None -> None; one unit (a ControlUnit or a dict of its fields) or a list of 1 .. MAX_UNITS of them -> the checked units.
    ValueError naming the unit and the field for anything else."""
    if control is None:
        return None
    units = list(control) if isinstance(control, (list, tuple)) else [control]
    if not 1 <= len(units) <= MAX_UNITS:
        raise ValueError(f"control: {len(units)} units (1 .. {MAX_UNITS})")
    return tuple(_unit(i, u) for i, u in enumerate(units))


def keep(i: int, num_steps: int, start: float, end: float) -> float:
    """diffusers' rule, in Python floats: 1.0 where step row i of num_steps lies inside [start, end], else 0.0."""
    return 0.0 if (i / num_steps < start or (i + 1) / num_steps > end) else 1.0


def table(units, num_steps: int) -> np.ndarray:
    """The per-call upload: fp32 [num_steps][N][13][2], the last axis (unconditional rows, conditional rows), built in float64 and
    rounded once.  Row i is the row of the job's coefficient table (the device step counter), whatever step the job enters at."""
    units = parse(units)
    num_steps = int(num_steps)
    if num_steps < 1:
        raise ValueError(f"control: num_steps = {num_steps} (>= 1)")
    t = np.zeros((num_steps, len(units), TAPS, 2), dtype=np.float64)
    for n, u in enumerate(units):
        soft = np.asarray([1.0 if u.mode == "balanced" else SOFT ** (TAPS - 1 - k) for k in range(TAPS)], dtype=np.float64)
        s = np.asarray(u.weight, dtype=np.float64) * soft
        for i in range(num_steps):
            t[i, n, :, 1] = s * keep(i, num_steps, u.start, u.end)
            t[i, n, :, 0] = 0.0 if u.mode == "control" else t[i, n, :, 1]
    return t.astype(np.float32)


def scale_host(residuals, row: np.ndarray) -> list:
    """The host loop's form of the combine: the 13 arrays sum_n s_n r_n,k (fp32, units in order) that predict_on_batch then adds
    to the skips.  residuals: per unit the 13 arrays of its ControlNet; row: table[i][:, :, half], fp32 [N][13].  A scale of
    exactly 0 is not accumulated, as on the device."""
    out = []
    for k in range(TAPS):
        acc = np.zeros_like(np.asarray(residuals[0][k], dtype=np.float32))
        for n, r in enumerate(residuals):
            if row[n, k] != 0.0:
                acc = acc + np.float32(row[n, k]) * np.asarray(r[k], dtype=np.float32)
        out.append(acc)
    return out
