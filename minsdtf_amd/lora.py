"""LoRA switch at run time: rank-r factors merged into the packed device weights in place (DESIGN.md "LoRA switch").

``StableDiffusion(lora_switch=True)`` keeps, beside the packed image, an fp32 device *master* of every LoRA-targetable layer in
its logical ``[N][K]`` pack order (``k = (ky*kw + kx)*C_in + c`` for a conv, ``[out][in]`` for a Dense) plus the fp32 vectors
the load path derived (``.lncs``, ``.lnb``, ``ffproj.b``) and the ``ffproj`` top block (fp32 of the float64 product).  A switch
writes every packed tensor a changed layer feeds, in its stored layout (rows or chunk-major, and the cached fragment-major copy),
with ONE msd_lora_merge launch (csrc/lora.hip): the addresses do not change, so launch plans and captured graphs stay valid.

This module has three parts:

* :func:`read_factors` - a kohya ``.safetensors`` / ``.pt`` file or state dict -> per target layer ``(up [N][r], down [r][K])``
  with ``alpha / r`` folded into ``up`` and ``down`` in the target's pack order; file results are cached on the device.
* :class:`Plan` - the merge plan of a packed model: the entries of its layout table (``layout.layout``, the description
  ``packing.pack`` built the image from) that a targetable layer feeds.  Nothing here matches a layer name.
* :class:`MergeBase` - the masters of one model (kept by the packing pass) and :meth:`MergeBase.apply` (validate, then prepare,
  then one launch).
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import weights as wtab
from .layout import VEC, Packed
from .packing import geglu_row_order

# --------------------------------------------------------------------------------------------------------------------------------
# factors
# --------------------------------------------------------------------------------------------------------------------------------
Factors = Dict[str, Tuple[torch.Tensor, torch.Tensor]]   # target layer name -> (up [N][r], down [r][K]), fp32
_cache: Dict[tuple, Factors] = {}


def _f32(x) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x.detach().to(torch.float32)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))


def target_name(kohya_name: str) -> Optional[str]:
    """kohya module name -> this package's layer name (the spec name: no ``.weight``), through the same maps the load-time merge
    uses (weights._lora_unet_name_map, weights._lora_te_name); None for a name the reference does not restore."""
    if kohya_name.startswith("lora_te_text_model"):
        k = wtab._lora_te_name(kohya_name)
    elif kohya_name.startswith("lora_unet_"):
        k = wtab._lora_unet_name_map().get(kohya_name)
    else:
        k = None
    return None if k is None else k[: -len(".weight")]


def factors_from_state_dict(sd, device=None) -> Factors:
    """Entries with ``.alpha`` only (as the reference): up (N, r[, 1, 1]) * alpha / r -> [N][r]; down (r, K) / (r, C, kh, kw) ->
    [r][kh*kw*C] in pack order.  Shapes are checked against a model later (MergeBase.validate)."""
    out: Factors = {}
    for key in list(sd.keys()):
        key = str(key)
        if not key.endswith(".alpha"):
            continue
        name = key[: -len(".alpha")]
        tgt = target_name(name)
        if tgt is None:
            continue
        up, down = _f32(sd[name + ".lora_up.weight"]), _f32(sd[name + ".lora_down.weight"])
        alpha = float(np.asarray(_f32(sd[key]).cpu()))
        r = up.shape[1]
        up = up.reshape(up.shape[0], r) * np.float32(alpha / float(r))
        if down.dim() == 4:
            down = down.permute(0, 2, 3, 1).reshape(down.shape[0], -1)
        out[tgt] = (up.contiguous().to(device) if device is not None else up.contiguous(),
                    down.contiguous().to(device) if device is not None else down.contiguous())
    return out


def read_factors(source, device) -> Factors:
    """`source`: a path (cached by absolute path, mtime and size: switching back reads no file) or a loaded state dict."""
    if isinstance(source, (str, os.PathLike)):
        path = os.path.abspath(os.fspath(source))
        if not os.path.exists(path):
            raise FileNotFoundError(f"LoRA file not found: {source}")
        st = os.stat(path)
        key = (path, st.st_mtime_ns, st.st_size, str(device))
        f = _cache.get(key)
        if f is None:
            f = _cache[key] = factors_from_state_dict(wtab.read_state_dict(path), device)
        return f
    if isinstance(source, dict):
        return factors_from_state_dict(source, device)
    raise TypeError(f"a LoRA source is a file path or a state dict, not {type(source).__name__}")


# --------------------------------------------------------------------------------------------------------------------------------
# merge plan
# --------------------------------------------------------------------------------------------------------------------------------
def targetable(specs) -> Dict[str, Tuple[int, int, int]]:
    """Layers a LoRA may change (the names the reference restores) -> (N, K, kernel size)."""
    unet = {v[: -len(".weight")] for v in wtab._lora_unet_name_map().values()}
    out = {}
    for s in specs:
        if s.kind not in ("conv_w", "dense_w"):
            continue
        te = s.name.startswith("text_model.encoder.layers.") and s.name.endswith(wtab._LORA_TE_SUFFIXES)
        if s.name in unet or te:
            if s.kind == "conv_w":
                kh, kw, cin, cout = s.shape
                out[s.name] = (cout, kh * kw * cin, kh)
            else:
                out[s.name] = (s.shape[1], s.shape[0], 1)
    return out


class Plan:
    """The part of a packed image a LoRA can change: the matrices of the layout table (layout.layout) that targetable layers
    feed, in table order (the order of the merge jobs); the parts of each stay in the order they are stacked."""

    def __init__(self, specs, table: List[Packed]):
        self.layers = targetable(specs)           # target layer -> (N, K, kernel size)
        fed = lambda e: not e.sources.isdisjoint(self.layers)  # noqa: E731
        self.targets = [e for e in table if e.store != VEC and fed(e)]
        assert all(e.sources <= set(self.layers) for e in self.targets), "a packed matrix is switched as a whole"
        # ffproj.b key -> (ff.net.2 layer, proj_out layer)
        self.ffproj_b = {e.key: tuple(p.layer for p in e.parts) for e in table if e.how == "ffproj_b" and fed(e)}

    def keys(self):
        ks = set(self.ffproj_b)
        for t in self.targets:
            ks |= {t.key} | ({t.colsum, t.lnb[0]} if t.norm else set())
        return ks


# --------------------------------------------------------------------------------------------------------------------------------
# masters and the merge
# --------------------------------------------------------------------------------------------------------------------------------
class MergeBase:
    """The fp32 masters of one packed model (packing.Masters, kept by the packing pass for lora.targetable's layers) and its
    merge plan, read from the layout table the image was packed by (built by HipModel.set_weights when lora_switch is on)."""

    def __init__(self, device, specs, table: List[Packed], masters):
        self.device = device
        self.plan = Plan(specs, table)
        self.master, self.top, self.vec = masters
        self.rowmaps: Dict[int, torch.Tensor] = {}
        self.active: set = set()   # layers whose factors are merged now
        self.version = 0

    # ---- checks (before any device write)
    def validate(self, factor_sets: List[Tuple[Factors, float]], model_name: str) -> None:
        for f, _scale in factor_sets:
            for n, (up, down) in f.items():
                if n not in self.plan.layers:
                    continue
                N, K, ks = self.plan.layers[n]
                if up.dim() != 2 or down.dim() != 2 or up.shape[0] != N or down.shape[1] != K or up.shape[1] != down.shape[0]:
                    raise ValueError(f"{model_name}: LoRA factors for {n}: up {tuple(up.shape)}, down {tuple(down.shape)} do not "
                                     f"fit a {N} x {K} weight")

    def _factors(self, factor_sets) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
        """Concatenate the active LoRAs per layer: U = [s_1 U_1 | s_2 U_2 ...], D = [D_1; D_2; ...]."""
        us: Dict[str, list] = {}
        ds: Dict[str, list] = {}
        for f, scale in factor_sets:
            for n, (up, down) in f.items():
                if n in self.plan.layers:
                    us.setdefault(n, []).append(up.to(self.device) * np.float32(scale))
                    ds.setdefault(n, []).append(down.to(self.device))
        return {n: (torch.cat(us[n], 1).contiguous(), torch.cat(ds[n], 0).contiguous()) for n in us}

    def _rowmap(self, n_rows: int) -> torch.Tensor:
        m = self.rowmaps.get(n_rows)
        if m is None:
            order = geglu_row_order(n_rows // 2)
            m = self.rowmaps[n_rows] = torch.from_numpy(np.argsort(order).astype(np.int32)).to(self.device)
        return m

    def apply(self, W, factor_sets: List[Tuple[Factors, float]], stream=None) -> set:
        """Merge `factor_sets` (already validated) into the packed tensors of W; returns the set of packed keys written."""
        from . import ops

        fac = self._factors(factor_sets)
        dirty = self.active | set(fac)
        jobs, keep, written = [], [], set()
        vec_updates = []
        for t in self.plan.targets:
            if not (t.sources & dirty):
                continue
            dst = W[t.key]
            frag = W._fragment.get(t.key) if hasattr(W, "_fragment") else None
            touched = bool(t.sources & set(fac))
            if dst.dtype == torch.float32:   # the fp32 time-embedding form: (1, 1, K, N_total)
                layout, out_rows, out_cols, dt = ops.LORA_LAYOUT_T, dst.shape[3], dst.shape[2], ops.OUT_F32
            elif t.key in W.chunk_major_keys:
                layout, out_rows, out_cols, dt = ops.LORA_LAYOUT_CHUNK, dst.shape[1], dst.shape[0] * 64, ops.OUT_BF16
            else:
                layout, out_rows, out_cols, dt = ops.LORA_LAYOUT_ROWS, dst.shape[0], dst.shape[1], ops.OUT_BF16
            colsum = W[t.colsum] if (t.colsum and touched) else None
            for p in t.parts:
                if p.ffproj_top:   # (the part after it is proj_out's)
                    master = self.top[p.layer]
                    U, D = self._ffproj_factors(p.layer, t.parts[1].layer, fac)
                else:
                    master = self.master[p.layer]
                    U, D = fac.get(p.layer, (None, None))
                N, K = master.shape
                rowscale = None
                if p.qscale is not None:
                    rowscale = torch.full((N,), float(p.qscale), dtype=torch.float32, device=self.device)
                    keep.append(rowscale)
                jobs.append(ops.lora_job(
                    master=master, out=dst, n=N, k=K, out_rows=out_rows, out_cols=out_cols, up=U, down=D,
                    rank=0 if U is None else U.shape[1], rowscale=rowscale, colscale=W[p.colscale] if p.colscale else None,
                    rowmap=self._rowmap(N) if p.rowmap else None, out_frag=frag, colsum=colsum, layout=layout, out_dtype=dt,
                    row_off=p.row_off, col_off=p.col_off))
                keep += [U, D]
            written.add(t.key)
            if t.colsum:
                written.add(t.colsum)
                if not touched:
                    vec_updates.append((t.colsum, self.vec[t.colsum]))
            if t.lnb:
                written.add(t.lnb[0])
                vec_updates.append((t.lnb[0], self._lnb(t, fac, W) if touched else self.vec[t.lnb[0]]))
        for bk, (l2, lp) in self.plan.ffproj_b.items():
            if {l2, lp} & dirty:
                written.add(bk)
                if lp in fac:   # b' = b + Up (Dp b2)
                    Up, Dp = fac[lp]
                    b2 = W[l2 + ".b"].double()
                    vec_updates.append((bk, (self.vec[bk].double() + Up.double() @ (Dp.double() @ b2)).float()))
                else:
                    vec_updates.append((bk, self.vec[bk]))
        if jobs:
            call = ops.lora_merge(jobs, self.device)
            call(torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream)
        for k, v in vec_updates:
            W[k].copy_(v)
        self.active = set(fac)
        return written

    def _ffproj_factors(self, l2, lp, fac):
        """Top block of ffproj in [N][K] = [C][4C]: Ap' A2' = Ap A2 + [Ap' U2 | Up] [D2 ; Dp A2] (DESIGN.md "LoRA switch")."""
        f2, fp = fac.get(l2), fac.get(lp)
        if f2 is None and fp is None:
            return None, None
        Ap, A2 = self.master[lp], self.master[l2]
        us, ds = [], []
        if f2 is not None:
            U2, D2 = f2
            ApU2 = Ap @ U2
            if fp is not None:
                ApU2 = ApU2 + fp[0] @ (fp[1] @ U2)
            us.append(ApU2)
            ds.append(D2)
        if fp is not None:
            Up, Dp = fp
            us.append(Up)
            ds.append(Dp @ A2)
        return torch.cat(us, 1).contiguous(), torch.cat(ds, 0).contiguous()

    def _lnb(self, t: Packed, fac, W) -> torch.Tensor:
        """lnb' = lnb + rowscale * U (D beta), placed at the parts' destination rows (float64)."""
        out = self.vec[t.lnb[0]].double().clone()
        beta = W[t.lnb[1]].double()
        for p in t.parts:
            f = fac.get(p.layer)
            if f is None:
                continue
            U, D = f
            c = U.double() @ (D.double() @ beta)
            if p.qscale is not None:
                c = c * float(p.qscale)
            if p.rowmap:
                idx = self._rowmap(U.shape[0]).long()
                out[idx + p.row_off] += c
            else:
                out[p.row_off: p.row_off + c.shape[0]] += c
        return out.float()
