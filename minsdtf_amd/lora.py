"""LoRA switch at run time: rank-r factors merged into the packed device weights in place (DESIGN.md "LoRA switch").

``StableDiffusion(lora_switch=True)`` keeps, beside the packed image, an fp32 device *master* of every LoRA-targetable layer in
its logical ``[N][K]`` pack order (``k = (ky*kw + kx)*C_in + c`` for a conv, ``[out][in]`` for a Dense) plus the fp32 vectors
the load path derived (``.lncs``, ``.lnb``, ``ffproj.b``) and the ``ffproj`` top block (fp32 of the float64 product).  A switch
writes every packed tensor a changed layer feeds, in its stored layout (rows or chunk-major, and the cached fragment-major copy),
with ONE msd_lora_merge launch (csrc/lora.hip): the addresses do not change, so launch plans and captured graphs stay valid.

This module has three parts:

* :func:`read_factors` - a kohya ``.safetensors`` / ``.pt`` file or state dict -> per target layer ``(up [N][r], down [r][K])``
  with ``alpha / r`` folded into ``up`` and ``down`` in the target's pack order; file results are cached on the device.
* :func:`build_plan` - the merge plan of a packed model, derived from its weight table and the keys ``HipModel._pack`` made.
* :class:`MergeBase` - the masters of one model and :meth:`MergeBase.apply` (validate, then prepare, then one launch).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import weights as wtab

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
@dataclass
class Part:
    """One source layer's block of a packed matrix: logical rows [0, N) -> destination rows row_off + (rowmap or identity),
    columns [0, K) -> col_off + k, values (master + U D) * rowscale[n] * colscale[k]."""
    layer: str
    row_off: int = 0
    col_off: int = 0
    qscale: Optional[float] = None        # uniform row scale (the query prescale)
    colscale: Optional[str] = None        # packed key of the fp32 column scale (a LayerNorm gamma)
    rowmap: bool = False                  # GEGLU row order
    ffproj_top: bool = False              # the fused ff.net.2 . proj_out block (master and factors of its own)


@dataclass
class Target:
    key: str
    parts: List[Part]
    colsum: Optional[str] = None          # .lncs key written from this matrix's rounded rows
    lnb: Optional[Tuple[str, str]] = None  # (.lnb key, packed key of the LayerNorm beta)

    @property
    def sources(self):
        s = set()
        for p in self.parts:
            s.add(p.layer)
            if p.ffproj_top:
                s.add(p.layer.replace(".transformer_blocks.0.ff.net.2", ".proj_out"))
        return s


@dataclass
class Plan:
    targets: List[Target]
    layers: Dict[str, Tuple[int, int, int]]   # target layer -> (N, K, kernel size)
    ffproj_b: Dict[str, Tuple[str, str]] = field(default_factory=dict)   # ffproj.b key -> (ff.net.2 layer, proj_out layer)

    def keys(self):
        ks = set()
        for t in self.targets:
            ks.add(t.key)
            if t.colsum:
                ks.add(t.colsum)
            if t.lnb:
                ks.add(t.lnb[0])
        return ks | set(self.ffproj_b)


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


def build_plan(specs, W) -> Plan:
    """Every packed tensor each targetable layer feeds, following the decisions HipModel._pack made (read off the keys it
    produced): stacked q|k|v / k|v, prescaled queries, the LayerNorm folds, the GEGLU row order, ffproj, conv2sc, the
    concatenated time-embedding projections."""
    from .models import _q_prescale

    layers = targetable(specs)
    targets: Dict[str, Target] = {}

    def add(key, part, colsum=None, lnb=None):
        if key not in W:
            return
        t = targets.get(key)
        if t is None:
            t = targets[key] = Target(key, [], colsum if colsum in W else None, lnb if lnb and lnb[0] in W else None)
        t.parts.append(part)

    tproj_off = 0
    ffproj_b = {}
    for s in specs:   # table order (the order _pack concatenates the time-embedding projections in)
        n = s.name
        if s.kind not in ("conv_w", "dense_w"):
            continue
        if n.endswith(".time_emb_proj"):
            if n in layers:
                add("time_emb_proj_cat.w", Part(n, row_off=tproj_off))
            tproj_off += s.shape[1]
            continue
        if n not in layers:
            continue
        N = layers[n][0]
        for trio, stacked in ((("attn1.to_q", "attn1.to_k", "attn1.to_v"), "attn1.qkv"),
                              (("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), "self_attn.qkv")):
            hit = [i for i, x in enumerate(trio) if n.endswith("." + x)]
            if hit:
                i = hit[0]
                base = n[: -len(trio[i])] + stacked
                q = _q_prescale(N) if (i == 0 and stacked == "attn1.qkv") else None
                add(base + ".w", Part(n, row_off=i * N, qscale=q))
                if stacked == "attn1.qkv":
                    tb = n[: -len(".attn1." + trio[i].split(".")[1])]
                    add(base + ".lnw", Part(n, row_off=i * N, qscale=q, colscale=tb + ".norm1.g"), base + ".lncs",
                        (base + ".lnb", tb + ".norm1.b"))
                break
        else:
            if n.endswith(".attn2.to_q"):
                tb = n[: -len(".attn2.to_q")]
                q = _q_prescale(N)
                add(n + ".w", Part(n, qscale=q))
                add(n + ".lnw", Part(n, qscale=q, colscale=tb + ".norm2.g"), n + ".lncs", (n + ".lnb", tb + ".norm2.b"))
            elif n.endswith((".attn2.to_k", ".attn2.to_v")):
                add(n[: -len(".to_k")] + ".kv.w", Part(n, row_off=0 if n.endswith(".to_k") else N))
            elif n.endswith(".ff.net.0.proj"):
                tb = n[: -len(".ff.net.0.proj")]
                add(n + ".w", Part(n, rowmap=True))
                add(n + ".lnw", Part(n, rowmap=True, colscale=tb + ".norm3.g"), n + ".lncs", (n + ".lnb", tb + ".norm3.b"))
            else:
                add(n + ".w", Part(n))
                if n.endswith(".transformer_blocks.0.ff.net.2"):
                    att = n[: -len(".transformer_blocks.0.ff.net.2")]
                    add(att + ".ffproj.w", Part(n, ffproj_top=True))
                    if att + ".ffproj.b" in W:
                        ffproj_b[att + ".ffproj.b"] = (n, att + ".proj_out")
                elif n.endswith(".proj_out"):
                    att = n[: -len(".proj_out")]
                    tb2 = att + ".transformer_blocks.0.ff.net.2"
                    if tb2 in layers:
                        add(att + ".ffproj.w", Part(n, col_off=layers[tb2][1]))
                elif n.endswith(".conv2"):
                    add(n[: -len(".conv2")] + ".conv2sc.w", Part(n))
                elif n.endswith(".conv_shortcut"):
                    rb = n[: -len(".conv_shortcut")]
                    if rb + ".conv2" in layers:
                        add(rb + ".conv2sc.w", Part(n, col_off=layers[rb + ".conv2"][1]))
    return Plan(list(targets.values()), layers, ffproj_b)


# --------------------------------------------------------------------------------------------------------------------------------
# masters and the merge
# --------------------------------------------------------------------------------------------------------------------------------
def logical(spec_kind: str, a: np.ndarray) -> torch.Tensor:
    """Keras layout -> fp32 [N][K] in pack order."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    if spec_kind == "conv_w":
        return t.permute(3, 0, 1, 2).reshape(t.shape[3], -1)
    return t.t()


class MergeBase:
    """The fp32 masters of one packed model and its merge plan (built by HipModel.set_weights when lora_switch is on)."""

    def __init__(self, model, named, W, ffproj_top: Dict[str, np.ndarray]):
        d = model.device
        self.device = d
        self.plan = build_plan(model._specs, W)
        kinds = {s.name: s.kind for s in model._specs if s.kind in ("conv_w", "dense_w")}
        self.master: Dict[str, torch.Tensor] = {}
        for n in self.plan.layers:
            self.master[n] = logical(kinds[n], named[(n, kinds[n])]).contiguous().to(d)
        self.top = {att: torch.from_numpy(np.ascontiguousarray(v.T, dtype=np.float32)).to(d) for att, v in ffproj_top.items()}
        self.vec = {k: W[k].clone() for t in self.plan.targets for k in (t.colsum, t.lnb[0] if t.lnb else None) if k}
        self.vec.update({k: W[k].clone() for k in self.plan.ffproj_b})
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
            from .packing import geglu_row_order

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
                if p.ffproj_top:
                    att = p.layer[: -len(".transformer_blocks.0.ff.net.2")]
                    master = self.top[att]
                    U, D = self._ffproj_factors(p.layer, att + ".proj_out", fac)
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

    def _lnb(self, t: Target, fac, W) -> torch.Tensor:
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
