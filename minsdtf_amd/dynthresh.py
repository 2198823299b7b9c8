"""Dynamic thresholding (the "CFG scale fix" / "mimic scale": the A1111 extension sd-dynamic-thresholding, the DynamicThresholding
node of ComfyUI and SwarmUI): ``generate_image(..., dynamic_threshold=...)``.

At a high guidance scale g the combined prediction burns out.  Every step, with rows u (unconditional) and c (conditional), the
prediction at the cfg scale g_i keeps its direction and each (sample, channel) plane of it is forced back to the spread the
prediction at a low "mimic" scale m_i has (the extension's ``dynthresh()`` with ``sep_feat_channels = True``); one plane is the
P = h * w values of one sample and channel:

    d = c - u;  cfg = u + g_i d;  mim = u + m_i d
    cc = cfg - mean(cfg);  mc = mim - mean(mim)
    measure "ad":  mim_ref = max |mc|,  cfg_ref = quantile(|cc|, percentile)   (torch.quantile's "linear" rule)
    measure "std": mim_ref = std(mc),   cfg_ref = std(cc)                      (unbiased: divide by P - 1)
    startpoint "mean", "ad":   mx = max(mim_ref, cfg_ref);  r = clamp(cc, -mx, mx) / mx * mim_ref + mean(cfg)
    startpoint "mean", "std":  r = cc / cfg_ref * mim_ref + mean(cfg)
    startpoint "zero":         r = cfg * (mim_ref / cfg_ref)
    out = phi r + (1 - phi) cfg

A plane whose divisor (mx, or cfg_ref) is exactly 0 is degenerate: the extension yields NaN there, here out = cfg for that plane.
The sampler step then takes `out` as it is, so ``guidance_rescale`` is not applied to such a job.

This module is the host side and needs no GPU: the job description (``DynThreshSpec`` / ``parse``), the per-step scale table
(``scales``), the rank of the order statistic (``rank``), the per-call upload (``params``) and the float64 statement of the device
launch for the host loop and the tests (``dynthresh_host``).  The device side is msdt_dynamic_threshold
(include/minsdtf_hip_dynthresh.h).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, fields
from typing import Optional, Tuple

import numpy as np

MODES = ("constant", "linear_down", "linear_up", "cosine_down", "cosine_up", "half_cosine_down", "half_cosine_up", "power_up",
         "power_down")
MEASURES = ("ad", "std")          # the upload carries the index
STARTPOINTS = ("mean", "zero")    # the upload carries the index
HALF_PI = 1.5707                  # the extension's own constant, kept: cos(1.5707) = 9.6e-5, not 0
PARAM_BYTES = 32


@dataclass
class DynThreshSpec:
    """``mimic_scale``: the scale whose spread is kept, > 0; ``percentile`` in [0, 1]: the quantile of |cc| that stands for the
    spread of the cfg prediction (1.0 = its maximum); ``mimic_mode`` / ``cfg_mode``: how the two scales move over the steps (MODES),
    from the scale itself towards ``mimic_scale_min`` / ``cfg_scale_min``; ``sched_val``: the exponent of the power modes;
    ``measure``: "ad" (absolute deviation: maximum and quantile) or "std"; ``startpoint``: "mean" or "zero"; ``phi`` in [0, 1]: the
    share of the thresholded prediction in the result."""
    mimic_scale: float = 7.0
    percentile: float = 1.0
    mimic_mode: str = "constant"
    cfg_mode: str = "constant"
    mimic_scale_min: float = 0.0
    cfg_scale_min: float = 0.0
    sched_val: float = 1.0
    measure: str = "ad"
    startpoint: str = "mean"
    phi: float = 1.0


@dataclass(frozen=True)
class Resolved:
    """A DynThreshSpec checked: finite floats in their ranges, names of MODES / MEASURES / STARTPOINTS."""
    mimic_scale: float
    percentile: float
    mimic_mode: str
    cfg_mode: str
    mimic_scale_min: float
    cfg_scale_min: float
    sched_val: float
    measure: str
    startpoint: str
    phi: float


_FIELDS = tuple(f.name for f in fields(DynThreshSpec))


def _number(name, value, ok, rule) -> float:
    try:
        v = float(value)
    except (TypeError, ValueError) as e:
        raise ValueError(f"dynamic_threshold: {name} = {value!r} must be {rule}") from e
    if isinstance(value, bool) or not math.isfinite(v) or not ok(v):
        raise ValueError(f"dynamic_threshold: {name} = {value!r} must be {rule}")
    return v


def _choice(name, value, among) -> str:
    if not isinstance(value, str) or value not in among:
        raise ValueError(f"dynamic_threshold: {name} = {value!r} must be one of {among}")
    return value


def parse(dynamic_threshold) -> Optional[Resolved]:
    """None -> None; True -> the defaults; a DynThreshSpec or a dict of its fields -> the checked description.  ValueError naming
    the field for an unknown field, a number outside its range or a name that is none of the known ones."""
    dt = dynamic_threshold
    if dt is None:
        return None
    if isinstance(dt, Resolved):
        return dt
    if dt is True:
        dt = DynThreshSpec()
    if isinstance(dt, dict):
        unknown = set(dt) - set(_FIELDS)
        if unknown:
            raise ValueError(f"dynamic_threshold: unknown field(s) {sorted(unknown)}")
        dt = DynThreshSpec(**dt)
    if not isinstance(dt, DynThreshSpec):
        raise ValueError(f"dynamic_threshold must be a DynThreshSpec, a dict, True or None, not {type(dt).__name__}")
    unit = (lambda v: 0.0 <= v <= 1.0, "a finite float in [0, 1]")
    return Resolved(_number("mimic_scale", dt.mimic_scale, lambda v: v > 0.0, "a finite float > 0"),
                    _number("percentile", dt.percentile, *unit),
                    _choice("mimic_mode", dt.mimic_mode, MODES), _choice("cfg_mode", dt.cfg_mode, MODES),
                    _number("mimic_scale_min", dt.mimic_scale_min, lambda v: v >= 0.0, "a finite float >= 0"),
                    _number("cfg_scale_min", dt.cfg_scale_min, lambda v: v >= 0.0, "a finite float >= 0"),
                    _number("sched_val", dt.sched_val, lambda v: v > 0.0, "a finite float > 0"),
                    _choice("measure", dt.measure, MEASURES), _choice("startpoint", dt.startpoint, STARTPOINTS),
                    _number("phi", dt.phi, *unit))


def _shape(mode: str, frac: float, sched_val: float) -> float:
    """f(frac) of the table in the module's documentation; frac in [0, 1]."""
    if mode == "constant":
        return 1.0
    if mode == "linear_down":
        return 1.0 - frac
    if mode == "linear_up":
        return frac
    if mode == "cosine_down":
        return math.cos(HALF_PI * frac)
    if mode == "cosine_up":
        return 1.0 - math.cos(HALF_PI * frac)
    if mode == "half_cosine_down":
        return math.cos(frac)
    if mode == "half_cosine_up":
        return 1.0 - math.cos(frac)
    if mode == "power_up":
        return frac ** sched_val
    if mode == "power_down":
        return 1.0 - frac ** sched_val
    raise ValueError(f"dynamic_threshold: mode {mode!r} is none of {MODES}")


def scales(spec, guidance: float, num_steps: int) -> np.ndarray:
    """float64 [N][2]: (g_i, m_i) of the N executed steps.  frac_i = i / (N - 1) (0 for N = 1) and
    scale_i = min + (scale - min) * f(frac_i), f by the mode; the cfg scale is the job's guidance scale."""
    spec = parse(spec)
    N = int(num_steps)
    if N < 1:
        raise ValueError(f"dynamic_threshold: {num_steps} steps")
    out = np.zeros((N, 2), dtype=np.float64)
    for i in range(N):
        frac = i / (N - 1) if N > 1 else 0.0
        out[i, 0] = spec.cfg_scale_min + (float(guidance) - spec.cfg_scale_min) * _shape(spec.cfg_mode, frac, spec.sched_val)
        out[i, 1] = spec.mimic_scale_min + (spec.mimic_scale - spec.mimic_scale_min) * _shape(spec.mimic_mode, frac, spec.sched_val)
    return out


def _rank64(percentile: float, P: int) -> Tuple[int, float]:
    if int(P) < 1 or not 0.0 <= float(percentile) <= 1.0:
        raise ValueError(f"dynamic_threshold: the rank of percentile {percentile!r} among {P} values")
    pos = float(percentile) * (int(P) - 1)
    lo = min(int(math.floor(pos)), int(P) - 1)
    return lo, pos - lo


def rank(percentile: float, P: int) -> Tuple[int, np.float32]:
    """(lo, fp32 frac) of torch.quantile's "linear" rule among P values: pos = q (P - 1) in float64, lo = floor(pos); the order
    statistic is s[lo] + frac (s[min(lo + 1, P - 1)] - s[lo]).  Computed once, here: the kernel never multiplies q by P."""
    lo, frac = _rank64(percentile, P)
    return lo, np.float32(frac)


def params(spec, P: int) -> np.ndarray:
    """The per-call upload, PARAM_BYTES bytes as int32 [8]: lo, the measure's and the startpoint's index, the bits of fp32 frac
    and fp32 phi, three zeros (MsdtDynamicThreshold.params)."""
    spec = parse(spec)
    lo, frac = rank(spec.percentile, P)
    out = np.zeros(PARAM_BYTES // 4, dtype=np.int32)
    out[0], out[1], out[2] = lo, MEASURES.index(spec.measure), STARTPOINTS.index(spec.startpoint)
    out[3:5] = np.asarray([frac, spec.phi], dtype=np.float32).view(np.int32)
    return out


def dynthresh_host(u, c, g: float, m: float, spec) -> np.ndarray:
    """The combined prediction of one step in float64: u, c (B, h, w, 4), the step's cfg and mimic scales -> (B, h, w, 4).  The
    statement of the module's documentation; a degenerate plane returns cfg."""
    spec = parse(spec)
    u, c = np.asarray(u, dtype=np.float64), np.asarray(c, dtype=np.float64)
    if u.shape != c.shape or u.ndim != 4:
        raise ValueError(f"dynamic_threshold: u {u.shape} and c {c.shape} must be one (B, h, w, C) shape")
    B, h, w, C = u.shape
    P = h * w
    d = c - u
    cfg = (u + float(g) * d).reshape(B, P, C)
    mim = (u + float(m) * d).reshape(B, P, C)
    mean_cfg = cfg.mean(axis=1, keepdims=True)
    cc, mc = cfg - mean_cfg, mim - mim.mean(axis=1, keepdims=True)
    if spec.measure == "ad":
        mim_ref = np.abs(mc).max(axis=1, keepdims=True)
        s = np.sort(np.abs(cc), axis=1)
        lo, frac = _rank64(spec.percentile, P)
        hi = min(lo + 1, P - 1)
        cfg_ref = s[:, lo:lo + 1] + frac * (s[:, hi:hi + 1] - s[:, lo:lo + 1])
    else:
        if P < 2:
            raise ValueError("dynamic_threshold: measure 'std' of a one-pixel plane")
        mim_ref = np.sqrt((mc * mc).sum(axis=1, keepdims=True) / (P - 1))
        cfg_ref = np.sqrt((cc * cc).sum(axis=1, keepdims=True) / (P - 1))
    if spec.startpoint == "mean" and spec.measure == "ad":
        div = np.maximum(mim_ref, cfg_ref)
    else:
        div = cfg_ref
    ok = div != 0.0
    safe = np.where(ok, div, 1.0)
    if spec.startpoint == "zero":
        r = cfg * (mim_ref / safe)
    elif spec.measure == "ad":
        r = np.clip(cc, -safe, safe) / safe * mim_ref + mean_cfg
    else:
        r = cc / safe * mim_ref + mean_cfg
    out = np.where(ok, spec.phi * r + (1.0 - spec.phi) * cfg, cfg)
    return out.reshape(B, h, w, C)
