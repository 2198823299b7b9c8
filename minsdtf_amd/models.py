"""Drop-in model objects: the duck type ``StableDiffusion`` uses for its Keras models.

The reference pipeline only touches its models through ``ctor(...)``, ``.compile(jit_compile=True)``,
``.predict_on_batch(x)`` and — from the checkpoint loader — ``.name``, ``.weights`` (ordered, Keras
layout, with ``.shape`` / ``.name``) and ``.set_weights(list)`` (reference
``stable_diffusion.py:650-725``, ``ckpt_loader.py:2136-2193``).  The classes below provide exactly
that surface over the HIP library:

=================  =============================================  ==========================
class              replaces (reference)                           predict_on_batch
=================  =============================================  ==========================
DiffusionModel     diffusion_model.py:163-296                     [latent, t_emb, context(, 13 controls)] -> (B,h,w,4)
ImageDecoder       image_decoder.py:22-66                         latent -> (B,8h,8w,3)
ControlNet         control_net.py:45-118                          [latent, t_emb, context, hint] -> 13 arrays
HintNet            control_net.py:10-42                           (B,H,W,3) -> (B,H/8,W/8,320)
ClipVisionEncoder  (transformers CLIPVisionModelWithProjection)    (B,224,224,3) 0..255 -> (B,1024) image_embeds
IPResampler        (IP-Adapter resampler.py Resampler)             (B,257,1280) hidden states -> (B,16,768) image tokens
=================  =============================================  ==========================

Inputs / outputs at this boundary are host numpy arrays like the reference's; the fused,
device-resident loop (``minsdtf_amd/pipeline.py``) bypasses the boundary and keeps everything in
HBM.  There is no CPU fallback: constructing a model without a GPU + built library raises.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, engine, layout, ops, packing
from . import reference as reference_mod
from . import weights as wtab


class WeightVar:
    """What ``model.weights[i]`` needs to be for the positional loader: a name and a Keras shape."""
    __slots__ = ("name", "shape")

    def __init__(self, name, shape):
        self.name, self.shape = name, tuple(shape)

    def __repr__(self):
        return f"<WeightVar {self.name} {self.shape}>"


def default_device() -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.HipExtensionError("no HIP device visible: the MI355X path has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


class HipModel:
    kind = ""  # weight-table kind

    def __init__(self, name=None, device=None):
        self.name = name or type(self).__name__.lower()
        self.device = device if device is not None else default_device()
        lib = _lib.load()
        _lib.check(lib.msd_init(), "msd_init")
        self._specs = wtab.table(self.kind, **self._table_kw())
        self.weights: List[WeightVar] = [
            WeightVar(s.name + (".kernel" if s.kind.endswith("_w") else "." + s.kind), s.shape) for s in self._specs]
        self._W: Optional[Dict[str, torch.Tensor]] = None
        self._plans: Dict[tuple, "_BoundPlan"] = {}
        self._use_graph = False
        # bumped by every set_weights(): launch plans hold raw device addresses of the packed weights, so whatever caches
        # a plan built on this model (its own _plans, StableDiffusion._engines) keys on it
        self.weights_version = 0
        # LoRA switch (lora.py): off unless the owner asks for it before the weights are set; then set_weights also keeps the fp32
        # masters the merge starts from
        self.lora_switch = False
        self._lora = None

    def _table_kw(self) -> dict:
        return {}

    # ---- Keras-like surface
    def compile(self, jit_compile=True, **_):
        """The reference calls ``compile(jit_compile=True)``; here it switches predict_on_batch to
        hipGraph replay (captured on first use per input shape)."""
        self._use_graph = bool(jit_compile)
        self._plans.clear()

    def count_params(self) -> int:
        return wtab.param_count(self.kind)

    def set_weights(self, arrays: Sequence[np.ndarray]) -> None:
        if len(arrays) != len(self._specs):
            raise ValueError(f"{self.name}: expected {len(self._specs)} weight arrays, got {len(arrays)}")
        named = {}
        for s, a in zip(self._specs, arrays):
            a = np.asarray(a)
            if tuple(a.shape) != tuple(s.shape):
                raise ValueError(f"{self.name}: {s.name} has shape {a.shape}, expected {s.shape}")
            named[(s.name, s.kind)] = a
        # the packed image is what the layout table says (layout.py); W records which matrices are stored chunk-major, and the
        # emitters pass that per-key layout to the op (Emitter.conv)
        table = layout.layout(self._specs, layout.Flags(engine.W_CHUNK_MAJOR, engine.MFMA_TEMB_PROJ))
        self._lora = None
        if getattr(self, "lora_switch", False):   # also keep the fp32 masters the merge starts from
            from . import lora

            W, masters = packing.pack(table, named, self.device, keep=lora.targetable(self._specs))
            self._lora = lora.MergeBase(self.device, self._specs, table, masters)
        else:
            W, _ = packing.pack(table, named, self.device)
        self._W = W
        self.weights_version += 1
        self._plans.clear()

    @property
    def lora_version(self) -> int:
        """Bumped by every LoRA switch of these packed weights (shared with the models that share_weights them); the addresses do
        not change, so weights_version does not."""
        base = getattr(self, "_lora", None)
        return 0 if base is None else base.version

    def validate_loras(self, factor_sets) -> None:
        """Raise (RuntimeError without the switch, ValueError for a factor that does not fit) before any device write."""
        if getattr(self, "_lora", None) is None:
            raise RuntimeError(f"{self.name}: LoRA switching needs weights set with lora_switch=True "
                               "(StableDiffusion(lora_switch=True)); weights adopted through load_packed cannot be switched")
        self._lora.validate(factor_sets, self.name)

    def set_loras(self, factor_sets) -> bool:
        """Merge [(lora.Factors, scale), ...] into the packed weights in place (replacing the active set; [] = the base), stream-
        ordered on the current stream, then synchronise.  Returns whether any packed tensor was rewritten."""
        self.validate_loras(factor_sets)
        written = self._lora.apply(self._W, factor_sets)
        if written:
            self._lora.version += 1
        torch.cuda.synchronize(self.device)
        return bool(written)

    def share_weights(self, other: "HipModel") -> None:
        """Use `other`'s packed device weights (same network kind, e.g. one checkpoint served at two image sizes):
        no second copy in HBM, no second packing pass."""
        if type(other) is not type(self) or other._W is None:
            raise ValueError(f"{self.name}: share_weights needs a loaded model of the same kind")
        if other.device != self.device:   # the plans hold raw device addresses
            raise ValueError(f"{self.name}: share_weights across devices ({other.device} -> {self.device})")
        self._W = other._W
        self._lora = getattr(other, "_lora", None)   # (one packed image, one master: the sharing models switch together)
        self.weights_version += 1
        self._plans.clear()

    def load_synthetic(self, seed=0, bias_scale=0.0) -> List[np.ndarray]:
        """Fill with the seeded synthetic checkpoint; returns the Keras-layout list."""
        arrays = wtab.synth_keras_weights(self.kind, seed=seed, bias_scale=bias_scale, **self._table_kw())
        self.set_weights(arrays)
        return arrays

    def save_packed(self, path: str, **meta) -> None:
        """The packed device weights of this model -> `path` (packing.save_packed; `meta`: whatever identifies the
        checkpoint, compared by load_packed)."""
        self._require_weights()
        base = getattr(self, "_lora", None)
        if base is not None and base.active:   # merged weights are not the checkpoint's: never adopted as the base
            meta = dict(meta, lora_version=base.version)
        packing.save_packed(self._W, path, dict(meta, kind=self.kind, table_kw=self._table_kw()))

    def load_packed(self, path: str, **meta) -> None:
        """Adopt weights another process packed (save_packed): no generation, no packing pass, one upload."""
        self._W = packing.load_packed(path, self.device, dict(meta, kind=self.kind, table_kw=self._table_kw()))
        self._lora = None
        self.weights_version += 1
        self._plans.clear()

    def _maybe_load(self, ckpt_path, lora_dict=None):
        """Reference constructors load a local checkpoint if given one; no network download here."""
        if ckpt_path is not None and os.path.exists(ckpt_path):
            wtab.load_weights_from_file(self, ckpt_path, self.kind, lora_dict=lora_dict, specs=self._specs)

    def _require_weights(self):
        if self._W is None:
            raise RuntimeError(f"{self.name}: no weights set (pass ckpt_path=, call set_weights() or load_synthetic())")

    # ---- plan cache
    def _bound(self, key, builder) -> "_BoundPlan":
        key = (key, engine.GN_EPOCH)   # (a reported cluster-GroupNorm give-up retires every recorded plan: engine.check_gn_sync)
        engine.retire_stale(self._plans)   # ... and frees their arenas / graphs before the replacement is built
        bp = self._plans.get(key)
        if bp is None:
            self._require_weights()
            bp = builder()
            self._plans[key] = bp
        return bp


class _BoundPlan:
    """A finalised plan + its boundary tensors, optionally captured into a hipGraph."""

    def __init__(self, plan: engine.Plan, use_graph: bool):
        self.plan = plan
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.use_graph = use_graph
        self.io: Dict[str, torch.Tensor] = {}
        _lib.track_graph_owner(self)

    def release_graphs(self) -> None:
        self.graph = None

    def run(self):
        if not self.use_graph:
            self.plan.run(torch.cuda.current_stream().cuda_stream)
            return
        if self.graph is None:
            # warm-up run outside capture (first-touch of code objects), then capture
            self.plan.run(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s):
                    self.plan.run(torch.cuda.current_stream().cuda_stream)
            torch.cuda.current_stream().wait_stream(s)
            self.graph = g
        self.graph.replay()

    def host(self, name):
        """Boundary tensor `name` (or a list of names) as host array(s) — the duck type's D2H — followed by this plan's
        cluster-GroupNorm give-up word (engine.check_gn_sync: 4 more bytes on a stream the copy has just drained); raises
        instead of returning a result computed from abandoned moments."""
        names = [name] if isinstance(name, str) else list(name)
        out = [self.io[n].cpu().numpy() for n in names]
        buf = self.plan._gn_sync_buf
        if buf is not None and self.io[names[0]].device.type == "cuda":
            word = buf.tensor(torch.int32, (engine.GN_GIVE_UP_WORD + 1,))[engine.GN_GIVE_UP_WORD:]
            engine.check_gn_sync(word.cpu())
        return out[0] if isinstance(name, str) else out


def _np32(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=np.float32)


def _stage_inputs(plan: engine.Plan, shapes: Dict[str, tuple]) -> Dict[str, engine.Buf]:
    return {k: plan.alloc(int(np.prod(s)) * 4) for k, s in shapes.items()}


class DiffusionModel(HipModel):
    """SD1.5 UNet (reference diffusion_model.py:163-296) on the HIP path."""
    kind = "civitai_model"

    def __init__(self, img_height=512, img_width=512, apply_control_net=False, name=None, ckpt_path=None, lora_dict=None,
                 device=None, lora_switch=False):
        super().__init__(name or "diffusion_model", device)
        self.lora_switch = lora_switch
        if img_height % 64 or img_width % 64:
            raise ValueError("img_height / img_width must be multiples of 64 (three stride-2 levels after the /8 VAE)")
        self.h, self.w = img_height // 8, img_width // 8
        self.apply_control_net = apply_control_net
        self._maybe_load(ckpt_path, lora_dict)

    def _build(self, B: int, T: int, with_controls: bool, pag_layers=None, regions: int = 0, reference=None, window=None,
               adain=None, sag: bool = False, ip=None, t2i: int = 0) -> _BoundPlan:
        """pag_layers: the attention blocks whose self-attention is the identity map for ALL B rows (predict_perturbed).
        regions = R: all B rows are conditional rows over R region contexts (predict_regional): the context input is
        (R * B, T, 768), region-major, and `region_w` the four levels' weight planes (regions.pack_levels).
        reference = the attention blocks of a reference-only forward (predict_reference): the plan runs B + 1 rows, the last one the
        reference row read from `ref_latent`; `t_emb` and `context` carry its row last, `ref_mix` is fp32 [B]; eps keeps B rows.
        adain = the reference AdaIN sites of such a forward (reference.ADAIN_SITES); `reference` may then be an empty set.
        window = (nh, nw, depth) of a HyperTile forward (predict_windowed): engine.UNetVariant's window / window_depth.
        sag: the mid block's self-attention also writes the attention map of all B rows (predict_sag_map): io["sag_A"], fp32
        [B][mh * mw].
        ip = a models.IPAdapter (predict_ip): every attn2 is ONE msdi_attention_decoupled launch over the text context and the
        adapter's K / V^T of `ip_tokens` (B, N, 768), scaled by row 0 of `ip_scales`, fp32 (1, 16).
        t2i = U (predict_t2i): the four sites of the down path take U T2I-Adapters' features, io["t2i_feat.{u}.{l}"] (bf16, flat), scaled
        by row 0 of `t2i_scales`, fp32 (1, U, 4)."""
        h, w = self.h, self.w
        reference = frozenset(reference or ()) if (reference or adain) else None   # (an empty layer set next to AdaIN sites)
        NB = B + 1 if reference is not None else B
        plan = engine.Plan(self.device)
        e = engine.Emitter(plan, self._W)
        CB = (regions or 1) * B + (1 if reference is not None else 0)   # context rows
        shapes = dict(latent=(B, h, w, 4), t_emb=(NB, 320), context=(CB, T, 768))
        if reference is not None:
            shapes.update(ref_latent=(1, h, w, 4), ref_mix=(B,))
        region_attn = None
        if regions:
            from . import regions as regions_mod

            levels = engine.unet_levels(h, w)
            offs = regions_mod.level_offsets(regions, levels)
            shapes["region_w"] = (offs[-1],)
        if ip is not None:
            shapes.update(ip_tokens=(B, ip.tokens, 768), ip_scales=(1, 16))
        if t2i:
            shapes["t2i_scales"] = (1, t2i, 4)
        ins = _stage_inputs(plan, shapes)
        t2i_feats = [[plan.alloc(hl * wl * ch * 2) for (hl, wl), ch in zip(engine.unet_levels(h, w), wtab.UNET_CH)] for _u in range(t2i)]
        if regions:
            region_attn = (regions, B, {lv: ins["region_w"].at(o * 4) for lv, o in zip(levels, offs)})
        ctx16 = engine.Act(plan.alloc(CB * T * 768 * 2), CB, T, 1, 768)
        plan.rec(ops.cast_f32_to_bf16, x=ins["context"], out=ctx16.buf, n=CB * T * 768, name="context.bf16")
        ctx_kv = engine.emit_context_kv(e, ctx16, engine.UNET_ATTN_LAYERS, plan)
        ip_variant = None
        if ip is not None:
            tok16 = engine.Act(plan.alloc(B * ip.tokens * 768 * 2), B, ip.tokens, 1, 768)
            plan.rec(ops.cast_f32_to_bf16, x=ins["ip_tokens"], out=tok16.buf, n=B * ip.tokens * 768, name="ip_tokens.bf16")
            ip_variant = (engine.emit_ip_kv(engine.Emitter(plan, ip._W), tok16, engine.UNET_ATTN_LAYERS, plan), ip.tokens, ins["ip_scales"], 1)
        cols = engine.temb_columns(False)
        total = sum(c for _, c in engine.resblock_names(False))
        table = plan.alloc(NB * total * 4)
        engine.emit_time_embedding(e, ins["t_emb"], NB, table, encoder_only=False)
        controls, cstage = None, []
        if with_controls:   # fp32 staging buffers; emit_unet adds them to the skips in fp32 (one add-and-round launch each)
            controls = []
            for i, ch in enumerate(wtab.UNET_SKIP_CH + (1280,)):
                hh, ww = _skip_hw(i, h, w)
                st = plan.alloc(B * hh * ww * ch * 4)
                cstage.append((st, (B, hh, ww, ch)))
                controls.append(st)
        eps = plan.alloc(NB * h * w * 4 * 4)
        sag_A = sag_ws = None
        if sag:
            mh, mw = engine.unet_levels(h, w)[3]
            sag_A = plan.alloc(B * mh * mw * 4)
            sag_ws = plan.alloc(ops.colsum_workspace_floats(B, 8, mh * mw) * 4)
        # (every predict_* entry passes its own option alone; what does not go together is emit_unet's to refuse, not dropped here)
        variant = engine.UNetVariant(
            pag_layers=pag_layers, perturbed=B if pag_layers else 0, region_attn=region_attn,
            reference=(reference, ins["ref_latent"], ins["ref_mix"]) if reference is not None else None,
            adain=frozenset(adain) if adain else None,
            window=window[:2] if window is not None else None, window_depth=window[2] if window is not None else 0,
            sag=(sag_A, sag_ws, 0, B) if sag else None, ip=ip_variant, t2i=(t2i_feats, ins["t2i_scales"], 1) if t2i else None)
        engine.emit_unet(e, ins["latent"], B, NB, h, w, (table, 0, total, cols), ctx_kv, T, eps, controls, variant=variant)
        plan.finalize()
        bp = _BoundPlan(plan, self._use_graph)
        bp.io = {k: b.tensor(torch.float32, shapes[k]) for k, b in ins.items()}
        bp.io["eps"] = eps.tensor(torch.float32, (NB, h, w, 4))
        for u, fs in enumerate(t2i_feats):
            for l, ((hl, wl), ch) in enumerate(zip(engine.unet_levels(h, w), wtab.UNET_CH)):
                bp.io[f"t2i_feat.{u}.{l}"] = fs[l].tensor(torch.bfloat16, (hl * wl * ch,))
        if sag_A is not None:
            bp.io["sag_A"] = sag_A.tensor(torch.float32, (B, mh * mw))
        for i, (st, shp) in enumerate(cstage):
            bp.io[f"control.{i}"] = st.tensor(torch.float32, shp)
        return bp

    def predict_on_batch(self, x):
        return self._predict(x, None)

    def predict_perturbed(self, x, layers):
        """predict_on_batch([latent, t_emb, context]) with the self-attention map of the attention blocks `layers` (names of
        engine.PAG_LAYERS) replaced by the identity: those layers' output is V (msd_attention_identity).  The perturbed forward of
        perturbed-attention guidance (minsdtf_amd/pag.py); a bound plan of its own per layer set."""
        layers = frozenset([layers] if isinstance(layers, str) else layers)
        unknown = layers - set(engine.PAG_LAYERS)
        if not layers or unknown:
            raise ValueError(f"predict_perturbed: layers {sorted(layers)} (a non-empty subset of engine.PAG_LAYERS)")
        if len(x) != 3:
            raise ValueError("predict_perturbed takes [latent, t_emb, context] (no control tensors)")
        return self._predict(x, layers)

    def predict_windowed(self, x, windows, depth=0):
        """predict_on_batch([latent, t_emb, context]) with the self-attention of the attention blocks of levels 0 .. `depth` taken
        inside `windows` = (nh, nw) non-overlapping windows of the feature map (msd_attention_windowed; minsdtf_amd/hypertile.py).
        The forward of a HyperTile job's host loop; a bound plan of its own per (B, T, nh, nw, depth)."""
        from . import hypertile as hypertile_mod

        if len(x) != 3:
            raise ValueError("predict_windowed takes [latent, t_emb, context] (no control tensors)")
        nh, nw = (int(v) for v in windows)
        depth = int(depth)
        hypertile_mod.level_geometry(self.h, self.w, nh, nw, depth)   # (ValueError for windows the levels cannot take)
        return self._predict(x, None, window=(nh, nw, depth))

    def predict_sag_map(self, x):
        """predict_on_batch([latent, t_emb, context]) plus the self-attention map of mid_block.attentions.0 for all its rows:
        (eps, A), A fp32 (B, mh * mw) with A[b][j] = the head-mean attention key j receives summed over the queries
        (msdx_attention_colsum; (mh, mw) = engine.unet_levels(h, w)[3]).  The first pass of a self-attention-guidance step on the
        host loop (minsdtf_amd/sag.py); eps is predict_on_batch's, bit for bit.  A bound plan of its own per (B, T)."""
        if len(x) != 3:
            raise ValueError("predict_sag_map takes [latent, t_emb, context] (no control tensors)")
        return self._predict(x, None, sag=True)

    def predict_regional(self, x, contexts, level_weights):
        """predict_on_batch([latent, t_emb]) with every attn2 mixing the R region `contexts` (each (B, T, 768), T <= 96) per query by
        `level_weights` (Resolved.level_weights(engine.unet_levels(h, w)): one fp32 (R, h_l, w_l) per level) - one
        msd_region_attention launch per layer (regions.py, mode "attention"); a bound plan of its own per (B, T, R)."""
        from . import regions as regions_mod

        if len(x) != 2:
            raise ValueError("predict_regional takes [latent, t_emb] (the contexts are its second argument; no control tensors)")
        latent, t_emb = _np32(x[0]), _np32(x[1])
        ctx = [_np32(c) for c in contexts]
        R, B = len(ctx), latent.shape[0]
        planes = [np.asarray(p, dtype=np.float32) for p in level_weights]
        levels = engine.unet_levels(self.h, self.w)
        if not 1 <= R <= regions_mod.MAX_REGIONS or any(c.shape != ctx[0].shape for c in ctx) or ctx[0].shape[0] != B or ctx[0].shape[1] > 96:
            raise ValueError(f"predict_regional: {R} contexts of shapes {[c.shape for c in ctx]} for a batch of {B} (1 .. "
                             f"{regions_mod.MAX_REGIONS} contexts of (B, T <= 96, 768))")
        if [p.shape for p in planes] != [(R,) + lv for lv in levels]:
            raise ValueError(f"predict_regional: level weights of shapes {[p.shape for p in planes]}, expected {[(R,) + lv for lv in levels]}")
        if latent.shape[1:] != (self.h, self.w, 4):
            raise ValueError(f"latent shape {latent.shape} does not match the model ({self.h},{self.w},4)")
        T = ctx[0].shape[1]
        bp = self._bound((B, T, False, ("regions", R)), lambda: self._build(B, T, False, regions=R))
        bp.io["latent"].copy_(torch.from_numpy(latent))
        bp.io["t_emb"].copy_(torch.from_numpy(t_emb))
        bp.io["context"].copy_(torch.from_numpy(np.concatenate(ctx, axis=0)))
        bp.io["region_w"].copy_(torch.from_numpy(regions_mod.pack_levels(planes)))
        bp.run()
        return bp.host("eps")

    def predict_reference(self, x, ref_latent_t, layers, mix, ref_context=None, adain=None):
        """predict_on_batch([latent, t_emb, context]) with one more row, the reference latent `ref_latent_t` (1, h, w, 4) ALREADY
        noised to this step's level, whose keys the self-attention of the attention blocks `layers` (names of engine.PAG_LAYERS)
        also attends to (msd_attention_joint; minsdtf_amd/reference.py).  `mix`: the share of the plain self-attention in each
        row's result, a float or (B,) values in [0, 1].  The reference row takes t_emb[0] and `ref_context` (T, 768) or (1, T, 768)
        (default: context[0]).  `adain`: None, or reference AdaIN site names (reference.ADAIN_SITES): behind those block outputs the
        rows are renormalised to the reference row's channel statistics (msd_reference_adain), blended by the same `mix`;
        `layers` may then be empty.  Returns the B rows' prediction; a bound plan of its own per (rows, T, layer set, site set)."""
        layers = frozenset([layers] if isinstance(layers, str) else (layers or ()))
        sites = frozenset([adain] if isinstance(adain, str) else (adain or ()))
        if (not layers and not sites) or layers - set(engine.PAG_LAYERS):
            raise ValueError(f"predict_reference: layers {sorted(layers)} (a non-empty subset of engine.PAG_LAYERS, or empty next to adain sites)")
        if sites - {n for n, _gw in reference_mod.ADAIN_SITES}:
            raise ValueError(f"predict_reference: unknown adain site(s) {sorted(sites - {n for n, _gw in reference_mod.ADAIN_SITES})}")
        if len(x) != 3:
            raise ValueError("predict_reference takes [latent, t_emb, context] (no control tensors)")
        latent, t_emb, context = _np32(x[0]), _np32(x[1]), _np32(x[2])
        ref = _np32(ref_latent_t)
        B, T = latent.shape[0], context.shape[1]
        if latent.shape[1:] != (self.h, self.w, 4) or ref.shape != (1, self.h, self.w, 4):
            raise ValueError(f"latent shape {latent.shape} / reference latent shape {ref.shape} do not match the model ({self.h},{self.w},4)")
        rc = context[:1] if ref_context is None else _np32(ref_context).reshape(1, -1, 768)
        if rc.shape[1] != T:
            raise ValueError(f"predict_reference: the reference row's context has {rc.shape[1]} tokens, the rows' {T}")
        m = np.broadcast_to(np.asarray(mix, dtype=np.float32), (B,))
        if not ((m >= 0.0) & (m <= 1.0)).all():
            raise ValueError("predict_reference: mix in [0, 1]")
        key = (B + 1, T, False, ("reference", tuple(sorted(layers))) + ((("adain",) + tuple(sorted(sites)),) if sites else ()))
        bp = self._bound(key, lambda: self._build(B, T, False, reference=layers, adain=sites or None))
        bp.io["latent"].copy_(torch.from_numpy(latent))
        bp.io["t_emb"].copy_(torch.from_numpy(np.concatenate([t_emb, t_emb[:1]], axis=0)))
        bp.io["context"].copy_(torch.from_numpy(np.concatenate([context, rc], axis=0)))
        bp.io["ref_latent"].copy_(torch.from_numpy(ref))
        bp.io["ref_mix"].copy_(torch.from_numpy(np.ascontiguousarray(m)))
        bp.run()
        return bp.host("eps")[:B]

    def predict_ip(self, x, adapter, tokens, scales):
        """predict_on_batch([latent, t_emb, context(, 13 controls)]) with an IP-Adapter image prompt: every attn2 also attends to the
        image `tokens` - (N, 768) for every row, or (B, N, 768) - through `adapter` (a models.IPAdapter), its share scaled per
        attention block by `scales`, fp32 (16,) in engine.PAG_LAYERS order (one row of ipadapter.table).  The forward of an image-prompt
        job's host loop (minsdtf_amd/ipadapter.py); a bound plan of its own per (B, T, adapter)."""
        from . import ipadapter as ipadapter_mod

        if len(x) not in (3, 16):
            raise ValueError("predict_ip takes [latent, t_emb, context] and, with a ControlNet, its 13 control tensors")
        latent, t_emb, context = _np32(x[0]), _np32(x[1]), _np32(x[2])
        controls = [_np32(c) for c in x[3:]]
        B, T = latent.shape[0], context.shape[1]
        if latent.shape[1:] != (self.h, self.w, 4):
            raise ValueError(f"latent shape {latent.shape} does not match the model ({self.h},{self.w},4)")
        adapter._require_weights()
        tok = _np32(tokens)
        tok = np.array(np.broadcast_to(tok, (B,) + tok.shape)) if tok.ndim == 2 else tok   # (a copy: every row its own)
        sc = _np32(scales).reshape(-1)
        if tok.shape != (B, adapter.tokens, 768) or sc.shape != (16,):
            raise ValueError(f"predict_ip: tokens of shape {tok.shape} and {sc.shape[0]} scales, expected {(B, adapter.tokens, 768)} "
                             f"(or {(adapter.tokens, 768)}) and 16")
        ipadapter_mod.check_context(T, adapter.tokens)
        key = (B, T, bool(controls), ("ip", adapter.tokens, id(adapter), adapter.weights_version))
        bp = self._bound(key, lambda: self._build(B, T, bool(controls), ip=adapter))
        bp.keep_alive = adapter   # (the plan holds raw addresses of its packed weights)
        bp.io["latent"].copy_(torch.from_numpy(latent))
        bp.io["t_emb"].copy_(torch.from_numpy(t_emb))
        bp.io["context"].copy_(torch.from_numpy(context))
        bp.io["ip_tokens"].copy_(torch.from_numpy(tok))
        bp.io["ip_scales"].copy_(torch.from_numpy(sc.reshape(1, 16)))
        for i, c in enumerate(controls):
            bp.io[f"control.{i}"].copy_(torch.from_numpy(c))
        bp.run()
        return bp.host("eps")

    def predict_t2i(self, x, features, scales, ip=None):
        """predict_on_batch([latent, t_emb, context]) with T2I-Adapter features: `features` is a list of U units, each the four bf16
        features of models.T2IAdapter.features (device tensors, or arrays) - the same for every row - and `scales` fp32 (U, 4), one row
        of t2iadapter.table: site l takes sum_u scales[u][l] * features[u][l] (msda_feature_add).  ip = (adapter, tokens, scales16):
        the forward also carries predict_ip's image prompt.  The forward of a T2I-Adapter job's host loop (minsdtf_amd/t2iadapter.py); a
        bound plan of its own per (B, T, U) and image-prompt adapter."""
        if len(x) != 3:
            raise ValueError("predict_t2i takes [latent, t_emb, context] (no control tensors)")
        latent, t_emb, context = _np32(x[0]), _np32(x[1]), _np32(x[2])
        B, T = latent.shape[0], context.shape[1]
        if latent.shape[1:] != (self.h, self.w, 4):
            raise ValueError(f"latent shape {latent.shape} does not match the model ({self.h},{self.w},4)")
        U = len(features)
        sc = _np32(scales).reshape(-1)
        sizes = [hl * wl * ch for (hl, wl), ch in zip(engine.unet_levels(self.h, self.w), wtab.UNET_CH)]
        if not 1 <= U <= 3 or sc.shape != (U * 4,) or any(len(f) != 4 or [int(np.prod(a.shape)) for a in f] != sizes for f in features):
            raise ValueError(f"predict_t2i: {U} unit(s) (1 .. 3) of features {[[tuple(a.shape) for a in f] for f in features]} and "
                             f"{sc.shape[0]} scales, expected four features of {sizes} elements per unit and {U * 4} scales")
        key = (B, T, False, ("t2i", U))
        adapter = None
        if ip is not None:
            from . import ipadapter as ipadapter_mod

            adapter, tokens, ip_scales = ip
            adapter._require_weights()
            tok = _np32(tokens)
            tok = np.array(np.broadcast_to(tok, (B,) + tok.shape)) if tok.ndim == 2 else tok
            ipadapter_mod.check_context(T, adapter.tokens)
            key += (("ip", adapter.tokens, id(adapter), adapter.weights_version),)
        bp = self._bound(key, lambda: self._build(B, T, False, ip=adapter, t2i=U))
        bp.io["latent"].copy_(torch.from_numpy(latent))
        bp.io["t_emb"].copy_(torch.from_numpy(t_emb))
        bp.io["context"].copy_(torch.from_numpy(context))
        bp.io["t2i_scales"].copy_(torch.from_numpy(sc.reshape(1, U, 4)))
        for u, fs in enumerate(features):
            for l, f in enumerate(fs):
                f = f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32))
                bp.io[f"t2i_feat.{u}.{l}"].copy_(f.reshape(-1))   # (bf16 -> bf16 as it is; fp32 arrays are rounded once)
        if adapter is not None:
            bp.keep_alive = adapter
            bp.io["ip_tokens"].copy_(torch.from_numpy(tok))
            bp.io["ip_scales"].copy_(torch.from_numpy(_np32(ip_scales).reshape(1, 16)))
        bp.run()
        return bp.host("eps")

    def _predict(self, x, pag_layers, window=None, sag=False):
        latent, t_emb, context = _np32(x[0]), _np32(x[1]), _np32(x[2])
        controls = [_np32(c) for c in x[3:]]
        if controls and len(controls) != 13:
            raise ValueError("expected 13 control tensors")
        B, T = latent.shape[0], context.shape[1]
        if latent.shape[1:] != (self.h, self.w, 4):
            raise ValueError(f"latent shape {latent.shape} does not match the model ({self.h},{self.w},4)")
        key = (B, T, bool(controls)) if pag_layers is None else (B, T, False, ("pag", tuple(sorted(pag_layers))))
        if window is not None:
            key = (B, T, False, ("hypertile",) + tuple(window))
        if sag:
            key = (B, T, False, ("sag",))
        bp = self._bound(key, lambda: self._build(B, T, bool(controls), pag_layers, window=window, sag=sag))
        bp.io["latent"].copy_(torch.from_numpy(latent))
        bp.io["t_emb"].copy_(torch.from_numpy(t_emb))
        bp.io["context"].copy_(torch.from_numpy(context))
        for i, c in enumerate(controls):
            bp.io[f"control.{i}"].copy_(torch.from_numpy(c))
        bp.run()
        if sag:
            eps, A = bp.host(["eps", "sag_A"])
            return eps, A
        return bp.host("eps")

    __call__ = predict_on_batch


class IPAdapter:
    """The weights of an IP-Adapter (minsdtf_amd/ipadapter.py): a small model object of its own beside the UNet - 32 bias-free
    matrices, to_k_ip / to_v_ip of the 16 cross-attentions, packed per attention as ONE bf16 [2 C][768] matrix
    `<attn2 name>.kv_ip.w` (k rows, then v rows) the way layout.py describes a bias-free dense (ROWS, chunk-major as the UNet's) -
    and, on the host in float64, the image projection Linear(1024 -> N * 768) + LayerNorm(768).  They do not enter the UNet's
    packed image, and a LoRA switch does not touch them."""

    def __init__(self, tokens: int = 4, name=None, device=None, path=None):
        from . import ipadapter as ipadapter_mod

        if not 1 <= int(tokens) <= ipadapter_mod.MAX_TOKENS:
            raise ValueError(f"ip_adapter: {tokens} image tokens (1 .. {ipadapter_mod.MAX_TOKENS})")
        self.name = name or "ip_adapter"
        self.device = device if device is not None else default_device()
        self.tokens = int(tokens)
        self._W = None
        self.projection: Optional[Dict[str, np.ndarray]] = None
        # a models.IPResampler when the adapter came from a "plus" checkpoint (or synthetic_plus); settable.  Then the image tokens are
        # its output on the vision tower's penultimate hidden states, there is no projection, and `tokens` is its query count
        self.resampler = None
        self.weights_version = 0
        if path is not None:
            self.load(path)

    def _require_weights(self):
        if self._W is None:
            raise RuntimeError(f"{self.name}: no weights set (pass path=, call set_state() or IPAdapter.synthetic())")

    @staticmethod
    def packed_layout() -> List["layout.Packed"]:
        """The packed image: per cross-attention one ROWS entry over its two source layers, in engine.UNET_ATTN_LAYERS order."""
        out = []
        for name, C in engine.UNET_ATTN_LAYERS:
            parts = [layout.Part(name + ".to_k_ip"), layout.Part(name + ".to_v_ip", row_off=C)]
            out.append(layout.Packed(name + ".kv_ip.w", layout.ROWS, (2 * C, 768), parts, chunk_major=engine.W_CHUNK_MAJOR))
        return out

    def set_state(self, state) -> None:
        """Adopt a loaded checkpoint (ipadapter.read_state's input: the nested dict of a .bin or flat prefixed keys); raises on any
        key or shape that does not fit."""
        from . import ipadapter as ipadapter_mod

        named = ipadapter_mod.read_state(state)
        plus = {k[len("resampler."):]: v for k, v in named.items() if k.startswith("resampler.")}
        n = plus["latents"].shape[1] if plus else named["proj.weight"].shape[0] // 768
        named_keras = {}
        for name, _C in engine.UNET_ATTN_LAYERS:
            blk = name[:-len(".transformer_blocks.0.attn2")]
            for m in ("to_k_ip", "to_v_ip"):   # torch Linear [out][in] -> the Keras Dense (in, out) the packer starts from
                named_keras[(f"{name}.{m}", "dense_w")] = np.ascontiguousarray(named[f"{blk}.{m}"].T)
        W, _ = packing.pack(self.packed_layout(), named_keras, self.device)
        self._W, self.tokens = W, n
        if plus:
            rs = IPResampler(name=self.name + ".resampler", device=self.device)
            rs.set_state(plus)
            self.projection, self.resampler = None, rs
        else:
            self.projection = {k: np.asarray(named[k], dtype=np.float64) for k in ("proj.weight", "proj.bias", "norm.weight", "norm.bias")}
            self.resampler = None
        self.weights_version += 1

    def load(self, path: str) -> None:
        if not os.path.exists(str(path)):
            raise ValueError(f"ip_adapter: checkpoint {path!r} not found")
        self.set_state(wtab.read_state_dict(path))

    @classmethod
    def synthetic(cls, seed: int = 0, tokens: int = 4, device=None, scale: float = 1.0) -> "IPAdapter":
        """A seeded synthetic adapter, for tests and fixtures like the synthetic UNet: Glorot-uniform matrices (times `scale`)."""
        m = cls(tokens, device=device)
        m.set_state(cls.synthetic_state(seed, tokens, scale))
        return m

    @classmethod
    def synthetic_plus(cls, seed: int = 0, depth: int = wtab.RS_DEPTH, device=None, scale: float = 1.0) -> "IPAdapter":
        """A seeded synthetic "plus" adapter: synthetic()'s 32 to_k_ip / to_v_ip matrices at 16 tokens and, in place of the projection,
        a `depth`-layer synthetic Resampler (resampler.synthetic_state) as `resampler`."""
        from . import resampler as resampler_mod

        state = {k: v for k, v in cls.synthetic_state(seed, wtab.RS_TOKENS, scale).items() if not k.startswith("image_proj.")}
        state.update(resampler_mod.synthetic_state(seed, depth, wtab.RS_TOKENS))
        m = cls(wtab.RS_TOKENS, device=device)
        m.set_state(state)
        return m

    @staticmethod
    def synthetic_state(seed: int = 0, tokens: int = 4, scale: float = 1.0) -> Dict[str, np.ndarray]:
        """The flat state dict of synthetic(): the public file layout, float32 arrays."""
        from . import ipadapter as ipadapter_mod

        rng = np.random.default_rng([int(seed), 0x1BAD])

        def glorot(out_f, in_f):
            lim = float(np.sqrt(6.0 / (in_f + out_f))) * scale
            return rng.uniform(-lim, lim, size=(out_f, in_f)).astype(np.float32)

        state = {"image_proj.proj.weight": glorot(tokens * 768, 1024),
                 "image_proj.proj.bias": rng.uniform(-0.05, 0.05, size=(tokens * 768,)).astype(np.float32),
                 "image_proj.norm.weight": rng.uniform(0.8, 1.2, size=(768,)).astype(np.float32),
                 "image_proj.norm.bias": rng.uniform(-0.1, 0.1, size=(768,)).astype(np.float32)}
        for j, width in enumerate(ipadapter_mod.CHECKPOINT_WIDTHS):
            state[f"ip_adapter.{2 * j + 1}.to_k_ip.weight"] = glorot(width, 768)
            state[f"ip_adapter.{2 * j + 1}.to_v_ip.weight"] = glorot(width, 768)
        return state

    def project(self, embeds) -> np.ndarray:
        """(1024,) CLIP image embedding -> the (N, 768) fp32 image tokens (ipadapter.project)."""
        from . import ipadapter as ipadapter_mod

        self._require_weights()
        if self.resampler is not None:
            raise ValueError("ip_adapter: a \"plus\" adapter has no projection of the pooled embedding - its Resampler reads the vision "
                             "tower's hidden states: pass `image` (with StableDiffusion(clip_vision_path=...)) or the image `tokens`")
        p = self.projection
        return ipadapter_mod.project(embeds, p["proj.weight"], p["proj.bias"], p["norm.weight"], p["norm.bias"], self.tokens)


def _skip_hw(i: int, h: int, w: int):
    """Spatial size of skip / control tensor i (index 12 = mid block output)."""
    lvl = (0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3)[i]
    return h >> lvl, w >> lvl


class ImageDecoder(HipModel):
    """VAE decoder (reference image_decoder.py:22-66) on the HIP path."""
    kind = "decoder"

    def __init__(self, name=None, ckpt_path=None, device=None):
        super().__init__(name or "image_decoder", device)
        self._maybe_load(ckpt_path)

    def _build(self, B, h, w, out_u8: bool) -> _BoundPlan:
        plan = engine.Plan(self.device)
        e = engine.Emitter(plan, self._W)
        lat = plan.alloc(B * h * w * 4 * 4)
        out = plan.alloc(B * 8 * h * 8 * w * 3 * (1 if out_u8 else 4))
        engine.emit_decoder(e, lat, B, h, w, out, ops.OUT_U8 if out_u8 else ops.OUT_F32)
        plan.finalize()
        bp = _BoundPlan(plan, self._use_graph)
        bp.io["latent"] = lat.tensor(torch.float32, (B, h, w, 4))
        bp.io["image"] = out.tensor(torch.uint8 if out_u8 else torch.float32, (B, 8 * h, 8 * w, 3))
        return bp

    def predict_on_batch(self, x):
        latent = _np32(x)
        B, h, w, _ = latent.shape
        bp = self._bound((B, h, w, False), lambda: self._build(B, h, w, False))
        bp.io["latent"].copy_(torch.from_numpy(latent))
        bp.run()
        return bp.host("image")

    def decode_to_uint8(self, latent_dev: torch.Tensor) -> torch.Tensor:
        """Device-resident variant used by the fused pipeline: fp32 latent tensor on the GPU ->
        uint8 image tensor on the GPU with the reference's truncating conversion fused in."""
        B, h, w, _ = latent_dev.shape
        bp = self._bound((B, h, w, True), lambda: self._build(B, h, w, True))
        bp.io["latent"].copy_(latent_dev)
        bp.run()
        return bp.io["image"]

    __call__ = predict_on_batch


class ControlNet(HipModel):
    """ControlNet (reference control_net.py:45-118) on the HIP path."""
    kind = "controlnet"

    def __init__(self, img_height=512, img_width=512, name=None, controlnet_path=None, device=None):
        super().__init__(name or "control_net", device)
        self.h, self.w = img_height // 8, img_width // 8
        self._maybe_load(controlnet_path)

    def _build(self, B: int, T: int) -> _BoundPlan:
        h, w = self.h, self.w
        plan = engine.Plan(self.device)
        e = engine.Emitter(plan, self._W)
        ins = _stage_inputs(plan, dict(latent=(B, h, w, 4), t_emb=(B, 320), context=(B, T, 768), hint=(B, h, w, 320)))
        ctx16 = engine.Act(plan.alloc(B * T * 768 * 2), B, T, 1, 768)
        plan.rec(ops.cast_f32_to_bf16, x=ins["context"], out=ctx16.buf, n=B * T * 768, name="context.bf16")
        hint16 = plan.act(B, h, w, 320)
        plan.rec(ops.cast_f32_to_bf16, x=ins["hint"], out=hint16.buf, n=B * h * w * 320, name="hint.bf16")
        ctx_kv = engine.emit_context_kv(e, ctx16, engine.ENCODER_ATTN_LAYERS, plan)
        cols = engine.temb_columns(True)
        total = sum(c for _, c in engine.resblock_names(True))
        table = plan.alloc(B * total * 4)
        engine.emit_time_embedding(e, ins["t_emb"], B, table, encoder_only=True)
        outs, outs32 = [], []
        for i, ch in enumerate(wtab.UNET_SKIP_CH + (1280,)):
            hh, ww = _skip_hw(i, h, w)
            outs.append(plan.act(B, hh, ww, ch))
        engine.emit_controlnet(e, ins["latent"], B, B, h, w, (table, 0, total, cols), ctx_kv, T, hint16, outs)
        for i, a in enumerate(outs):
            o32 = plan.alloc(a.M * a.C * 4)
            plan.rec(ops.cast_bf16_to_f32, x=a.buf, out=o32, n=a.M * a.C, name=f"control.{i}.f32")
            outs32.append((o32, (a.B, a.H, a.W, a.C)))
        plan.finalize()
        bp = _BoundPlan(plan, self._use_graph)
        shapes = dict(latent=(B, h, w, 4), t_emb=(B, 320), context=(B, T, 768), hint=(B, h, w, 320))
        bp.io = {k: ins[k].tensor(torch.float32, s) for k, s in shapes.items()}
        for i, (o32, shp) in enumerate(outs32):
            bp.io[f"out.{i}"] = o32.tensor(torch.float32, shp)
        return bp

    def predict_on_batch(self, x):
        latent, t_emb, context, hint = (_np32(v) for v in x)
        B, T = latent.shape[0], context.shape[1]
        bp = self._bound((B, T), lambda: self._build(B, T))
        for k, v in (("latent", latent), ("t_emb", t_emb), ("context", context), ("hint", hint)):
            bp.io[k].copy_(torch.from_numpy(v))
        bp.run()
        return bp.host([f"out.{i}" for i in range(13)])

    __call__ = predict_on_batch


class HintNet(HipModel):
    """HintNet (reference control_net.py:10-42) on the HIP path."""
    kind = "hintnet"

    def __init__(self, img_height=512, img_width=512, name=None, controlnet_path=None, device=None):
        super().__init__(name or "hint_net", device)
        self.H, self.W = img_height, img_width
        self._maybe_load(controlnet_path)

    def _build(self, B: int) -> _BoundPlan:
        plan = engine.Plan(self.device)
        e = engine.Emitter(plan, self._W)
        img = plan.alloc(B * self.H * self.W * 3 * 4)
        out = plan.act(B, self.H // 8, self.W // 8, 320)
        engine.emit_hintnet(e, img, B, self.H, self.W, out)
        o32 = plan.alloc(out.M * 320 * 4)
        plan.rec(ops.cast_bf16_to_f32, x=out.buf, out=o32, n=out.M * 320, name="hint.f32")
        plan.finalize()
        bp = _BoundPlan(plan, self._use_graph)
        bp.io["image"] = img.tensor(torch.float32, (B, self.H, self.W, 3))
        bp.io["hint"] = o32.tensor(torch.float32, (B, self.H // 8, self.W // 8, 320))
        return bp

    def predict_on_batch(self, x):
        img = _np32(x)
        B = img.shape[0]
        bp = self._bound((B,), lambda: self._build(B))
        bp.io["image"].copy_(torch.from_numpy(img))
        bp.run()
        return bp.host("hint")

    __call__ = predict_on_batch


class ImageEncoder(HipModel):
    """VAE encoder (reference image_encoder.py:21-59) on the HIP path: image in [-1, 1] ->
    mean latent * 0.18215 (no sampling, like the reference's ``split(x, 2)[0] * 0.18215``)."""
    kind = "encoder"

    def __init__(self, ckpt_path=None, name=None, device=None):
        super().__init__(name or "image_encoder", device)
        self._maybe_load(ckpt_path)

    def _build(self, B, H, Wd) -> _BoundPlan:
        plan = engine.Plan(self.device)
        e = engine.Emitter(plan, self._W)
        img = plan.alloc(B * H * Wd * 3 * 4)
        lat = plan.alloc(B * (H // 8) * (Wd // 8) * 4 * 4)
        engine.emit_encoder(e, img, B, H, Wd, lat)
        plan.finalize()
        bp = _BoundPlan(plan, self._use_graph)
        bp.io["image"] = img.tensor(torch.float32, (B, H, Wd, 3))
        bp.io["latent"] = lat.tensor(torch.float32, (B, H // 8, Wd // 8, 4))
        return bp

    def predict_on_batch(self, x):
        img = _np32(x)
        B, H, Wd, _ = img.shape
        if H % 8 or Wd % 8 or ((H // 8) * (Wd // 8)) % 64:
            # the reference documents multiples of 128 only (stable_diffusion.py:589-593); the mid-block
            # attention GEMMs here need a token count that is a multiple of 64
            raise ValueError("image height / width must be multiples of 8 with (H/8)*(W/8) a multiple of 64")
        bp = self._bound((B, H, Wd), lambda: self._build(B, H, Wd))
        bp.io["image"].copy_(torch.from_numpy(img))
        bp.run()
        return bp.host("latent")

    __call__ = predict_on_batch


class TextClipEmbedding(HipModel):
    """CLIP token + position embedding (reference text_encoder.py:104-121): [tokens, positions] int32
    (B, 77) -> (B, 77, 768)."""
    kind = "text_clip_embedding"

    def __init__(self, max_length=77, embed_dim=768, vocab_size=49408, name=None, ckpt_path=None, device=None):
        if (max_length, embed_dim, vocab_size) != (wtab.CLIP_MAX_LEN, wtab.CLIP_DIM, wtab.CLIP_VOCAB):
            raise ValueError("only the SD1.5 CLIP ViT-L/14 text model geometry is built (77, 768, 49408)")
        super().__init__(name or "text_clip_embedding", device)
        self._maybe_load(ckpt_path)

    def emit(self, plan: engine.Plan, tokens, positions, out: engine.Act, status) -> None:
        plan.rec(ops.embedding_sum, tokens=tokens, positions=positions,
                 tok_table=self._W["text_model.embeddings.token_embedding"],
                 pos_table=self._W["text_model.embeddings.position_embedding"], out=out.buf, rows=out.M, dim=wtab.CLIP_DIM,
                 vocab=wtab.CLIP_VOCAB, max_len=wtab.CLIP_MAX_LEN, status=status, name="text_model.embeddings")

    def _build(self, B, T) -> _BoundPlan:
        plan = engine.Plan(self.device)
        tok, pos = plan.alloc(B * T * 4), plan.alloc(B * T * 4)
        x = plan.act(B, T, 1, wtab.CLIP_DIM)
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.emit(plan, tok, pos, x, status)
        o32 = plan.alloc(x.M * wtab.CLIP_DIM * 4)
        plan.rec(ops.cast_bf16_to_f32, x=x.buf, out=o32, n=x.M * wtab.CLIP_DIM, name="clip_emb.f32")
        plan.finalize()
        bp = _BoundPlan(plan, self._use_graph)
        bp.io["tokens"], bp.io["positions"] = tok.tensor(torch.int32, (B, T)), pos.tensor(torch.int32, (B, T))
        bp.io["emb"], bp.io["status"] = o32.tensor(torch.float32, (B, T, wtab.CLIP_DIM)), status
        return bp

    def predict_on_batch(self, x):
        tokens, positions = (np.ascontiguousarray(np.asarray(a), dtype=np.int32) for a in x)
        positions = np.array(np.broadcast_to(positions, tokens.shape), dtype=np.int32)
        B, T = tokens.shape
        bp = self._bound((B, T), lambda: self._build(B, T))
        bp.io["tokens"].copy_(torch.from_numpy(tokens))
        bp.io["positions"].copy_(torch.from_numpy(positions))
        bp.run()
        if int(bp.io["status"].item()):
            bp.io["status"].zero_()
            raise ValueError("token / position id outside the embedding table")
        return bp.host("emb")

    __call__ = predict_on_batch


class TextEncoder(HipModel):
    """CLIP text transformer (reference text_encoder.py:123-169): clip_emb (B, 77, 768) -> final
    LayerNorm of the output of layer `clip_skip` (B, 77, 768)."""
    kind = "text_encoder"

    def __init__(self, max_length=77, embed_dim=768, num_heads=12, num_layers=12, clip_skip=-2, name=None, ckpt_path=None,
                 lora_dict=None, device=None, lora_switch=False):
        if (embed_dim, num_heads, num_layers) != (wtab.CLIP_DIM, wtab.CLIP_HEADS, wtab.CLIP_LAYERS):
            raise ValueError("only the SD1.5 CLIP ViT-L/14 text model geometry is built (768, 12 heads, 12 layers)")
        if not -num_layers <= clip_skip <= -1:
            raise ValueError("clip_skip must be in [-num_layers, -1]")
        self.clip_skip, self.max_length = clip_skip, max_length
        super().__init__(name or "text_encoder", device)
        self.lora_switch = lora_switch
        self._maybe_load(ckpt_path, lora_dict)

    def _table_kw(self):
        return {"clip_skip": self.clip_skip}

    def count_params(self) -> int:
        return int(sum(int(np.prod(s.shape)) for s in self._specs))

    @property
    def n_layers(self) -> int:
        return wtab.CLIP_LAYERS + self.clip_skip + 1

    def _build(self, B, T) -> _BoundPlan:
        plan = engine.Plan(self.device)
        e = engine.Emitter(plan, self._W)
        C = wtab.CLIP_DIM
        x32 = plan.alloc(B * T * C * 4)
        x = plan.act(B, T, 1, C)
        plan.rec(ops.cast_f32_to_bf16, x=x32, out=x.buf, n=B * T * C, name="clip_emb.bf16")
        y = engine.emit_text_encoder(e, x, self.n_layers)
        o32 = plan.alloc(B * T * C * 4)
        plan.rec(ops.cast_bf16_to_f32, x=y.buf, out=o32, n=B * T * C, name="context.f32")
        plan.finalize()
        bp = _BoundPlan(plan, self._use_graph)
        bp.io["emb"], bp.io["context"] = x32.tensor(torch.float32, (B, T, C)), o32.tensor(torch.float32, (B, T, C))
        return bp

    def predict_on_batch(self, x):
        emb = _np32(x)
        B, T, _ = emb.shape
        bp = self._bound((B, T), lambda: self._build(B, T))
        bp.io["emb"].copy_(torch.from_numpy(emb))
        bp.run()
        return bp.host("context")

    __call__ = predict_on_batch


class ClipVisionEncoder(HipModel):
    """CLIP ViT-H/14 vision tower with its projection (transformers' CLIPVisionModelWithProjection; the `image_encoder` that ships with
    the SD 1.5 IP-Adapters): pixels (B, 224, 224, 3) on the 0 .. 255 scale (vision.preprocess) -> the (B, 1024) float32 image
    embedding an IP-Adapter projects.  `layers`: how many of the 32 encoder layers are built (tests build 2-layer towers)."""
    kind = "clip_vision"
    OUTPUTS = ("image_embeds", "penultimate", "last_hidden_state")

    def __init__(self, layers=wtab.VIT_LAYERS, name=None, path=None, device=None):
        self.layers = int(layers)
        super().__init__(name or "clip_vision", device)
        if path is not None:
            self.load(path)

    def _table_kw(self):
        return {"layers": self.layers}

    def count_params(self) -> int:
        return int(sum(int(np.prod(s.shape)) for s in self._specs))

    def set_state(self, state) -> None:
        """Adopt a loaded checkpoint (key -> tensor / array under CLIPVisionModelWithProjection's key names; fp16 files load); raises on
        a missing key or a wrong shape, naming it."""
        self.set_weights(wtab.clip_vision_arrays(state, self.layers))

    def load(self, path: str) -> None:
        if not os.path.exists(str(path)):
            raise ValueError(f"clip_vision: checkpoint {path!r} not found")
        self.set_state(wtab.read_state_dict(path))

    def load_synthetic(self, seed=0, bias_scale=0.0):
        """Fill with the seeded synthetic tower (wtab.clip_vision_synthetic_state; `bias_scale` is not used: its biases are always
        drawn); returns that state - what vision.forward_host takes."""
        state = wtab.clip_vision_synthetic_state(seed, self.layers)
        self.set_state(state)
        return state

    def _build(self, B: int, output: str) -> _BoundPlan:
        plan = engine.Plan(self.device)
        e = engine.Emitter(plan, self._W)
        T, C = wtab.VIT_TOKENS, wtab.VIT_DIM
        px = plan.alloc(B * wtab.VIT_IMAGE * wtab.VIT_IMAGE * 3 * 4)
        emb = plan.alloc(B * wtab.VIT_PROJ * 4) if output == "image_embeds" else None
        x = engine.emit_clip_vision(e, px, self.layers, penultimate=output == "penultimate", B=B, embeds=emb)
        h32 = None
        if output != "image_embeds":   # the hidden state leaves as fp32 (the slot of the pooled head: the launch count stays 2 + 8 L)
            h32 = plan.alloc(B * T * C * 4)
            plan.rec(ops.cast_bf16_to_f32, x=x.buf, out=h32, n=B * T * C, name=output + ".f32")
        plan.finalize()
        bp = _BoundPlan(plan, self._use_graph)
        bp.io["pixels"] = px.tensor(torch.float32, (B, wtab.VIT_IMAGE, wtab.VIT_IMAGE, 3))
        bp.io["out"] = emb.tensor(torch.float32, (B, wtab.VIT_PROJ)) if h32 is None else h32.tensor(torch.float32, (B, T, C))
        return bp

    def predict_on_batch(self, pixels, output="image_embeds"):
        """pixels (B, 224, 224, 3) or (224, 224, 3), 0 .. 255 -> `image_embeds` (B, 1024) float32; output="penultimate": the
        (B, 257, 1280) float32 input of the last layer (diffusers' hidden_states[-2], what a "plus" resampler consumes);
        output="last_hidden_state": the output of the last layer, before the post-LayerNorm."""
        px = _np32(pixels)
        px = px[None] if px.ndim == 3 else px
        if output not in self.OUTPUTS:
            raise ValueError(f"clip_vision: output {output!r} (one of {self.OUTPUTS})")
        if px.ndim != 4 or px.shape[1:] != (wtab.VIT_IMAGE, wtab.VIT_IMAGE, 3) or not 1 <= px.shape[0] <= 8:
            raise ValueError(f"clip_vision: pixels of shape {px.shape} ((B, 224, 224, 3), B = 1 .. 8; vision.preprocess makes them)")
        if output == "penultimate" and self.layers < 2:
            raise ValueError("clip_vision: output='penultimate' needs at least 2 layers")
        B = px.shape[0]
        bp = self._bound((B, output), lambda: self._build(B, output))
        bp.io["pixels"].copy_(torch.from_numpy(px))
        bp.run()
        return bp.host("out")

    __call__ = predict_on_batch


class IPResampler(HipModel):
    """The Resampler of an IP-Adapter "plus" checkpoint (minsdtf_amd/resampler.py; diffusers' IPAdapterPlusImageProjection): the CLIP
    ViT-H/14 tower's penultimate hidden states (B, 257, 1280) -> the (B, N, 768) float32 image tokens of the decoupled
    cross-attention.  `depth`: the number of layers (4 in the SD 1.5 plus adapters; tests build 1- and 2-layer resamplers);
    `tokens`: the learned queries N (16).  set_state adopts both from the checkpoint.  engine.emit_ip_resampler is the launch plan:
    6 + 10 * depth launches (+ 1 when B > 1) with the two boundary casts; the attention scale sits on the scores."""
    kind = "ip_resampler"

    def __init__(self, depth=wtab.RS_DEPTH, tokens=wtab.RS_TOKENS, name=None, device=None):
        self.depth, self.tokens = int(depth), int(tokens)
        if device is not None and torch.device(device).type != "cuda":
            # a host-side object (a reader's result, the tests' stand-in devices): it holds and packs weights, it cannot run
            self.name, self.device = name or "ip_resampler", torch.device(device)
            self._retable()
            self._W, self._plans, self._use_graph = None, {}, False
            self.weights_version, self.lora_switch, self._lora = 0, False, None
        else:
            super().__init__(name or "ip_resampler", device)
        self.state: Optional[Dict[str, np.ndarray]] = None   # resampler.read_state's result: what resampler.forward_host takes

    def _table_kw(self):
        return {"depth": self.depth, "tokens": self.tokens}

    def _retable(self) -> None:
        """The weight table and the Keras-like `weights` list of the current depth and token count."""
        self._specs = wtab.table(self.kind, **self._table_kw())
        self.weights = [WeightVar(s.name + (".kernel" if s.kind.endswith("_w") else "." + s.kind), s.shape) for s in self._specs]

    def count_params(self) -> int:
        return int(sum(int(np.prod(s.shape)) for s in self._specs))

    def set_state(self, state) -> None:
        """Adopt a loaded plus checkpoint (resampler.read_state's input: nested or flat `image_proj.` keys, fp16 files load) or
        read_state's own result; `depth` and `tokens` follow the state.  Raises on a missing key or a wrong shape, naming it."""
        from . import resampler as resampler_mod

        state = dict(state)
        named = state if "latents" in state and "proj_in.weight" in state else resampler_mod.read_state(state)
        depth, tokens = resampler_mod.depth_of(named), int(np.asarray(named["latents"]).shape[-2])
        if (depth, tokens) != (self.depth, self.tokens):
            self.depth, self.tokens = depth, tokens
            self._retable()
        self.set_weights(wtab.ip_resampler_arrays(named, depth, tokens))
        self.state = {k: np.asarray(v, dtype=np.float32) for k, v in named.items()}

    def load_synthetic(self, seed=0, bias_scale=0.0):
        """Fill with the seeded synthetic resampler (resampler.synthetic_state at this depth and token count; `bias_scale` is not
        used: its biases are always drawn); returns that state, under the checkpoint's flat keys."""
        from . import resampler as resampler_mod

        state = resampler_mod.synthetic_state(seed, self.depth, self.tokens)
        self.set_state(state)
        return state

    def _build(self, B: int) -> _BoundPlan:
        plan = engine.Plan(self.device)
        e = engine.Emitter(plan, self._W)
        T, C = wtab.VIT_TOKENS, wtab.VIT_DIM
        h32 = plan.alloc(B * T * C * 4)
        h16 = engine.Act(plan.alloc(B * T * C * 2), B, T, 1, C)
        plan.rec(ops.cast_f32_to_bf16, x=h32, out=h16.buf, n=B * T * C, name="hidden.bf16")
        y = engine.emit_ip_resampler(e, h16, self.depth, self.tokens)
        o32 = plan.alloc(B * self.tokens * wtab.RS_DIM * 4)
        plan.rec(ops.cast_bf16_to_f32, x=y.buf, out=o32, n=B * self.tokens * wtab.RS_DIM, name="tokens.f32")
        plan.finalize()
        bp = _BoundPlan(plan, self._use_graph)
        bp.io["hidden"] = h32.tensor(torch.float32, (B, T, C))
        bp.io["out"] = o32.tensor(torch.float32, (B, self.tokens, wtab.RS_DIM))
        return bp

    def predict_on_batch(self, hidden):
        """hidden (B, 257, 1280) or (257, 1280) float32, B = 1 .. 8: ClipVisionEncoder.predict_on_batch(..., output="penultimate")
        -> the (B, N, 768) float32 image tokens."""
        h = _np32(hidden)
        h = h[None] if h.ndim == 2 else h
        if h.ndim != 3 or h.shape[1:] != (wtab.VIT_TOKENS, wtab.VIT_DIM) or not 1 <= h.shape[0] <= 8:
            raise ValueError(f"ip_resampler: hidden states of shape {h.shape} ((B, {wtab.VIT_TOKENS}, {wtab.VIT_DIM}), B = 1 .. 8: "
                             "the tower's output='penultimate')")
        B = h.shape[0]
        bp = self._bound((B,), lambda: self._build(B))
        bp.io["hidden"].copy_(torch.from_numpy(h))
        bp.run()
        return bp.host("out")

    __call__ = predict_on_batch


class T2IAdapter:
    """A T2I-Adapter (minsdtf_amd/t2iadapter.py; diffusers' T2IAdapter "full adapter"): a small model object of its own beside the
    UNet - 19 convs with bias, packed through layout.py under `adapter.<layer>` the way every other MFMA conv is - that turns one
    conditioning picture into the four feature maps the UNet's down path takes.  engine.emit_t2i_adapter is the launch plan: 31
    launches, once per job.  `in_channels`: 3 (depth, pose, seg, ...) or 1 (sketch, canny); set_state adopts it from the checkpoint.
    The last picture's features are kept (keyed by a digest of the preprocessed pixels, the size and `weights_version`): a repeated
    job does not run the adapter."""
    kind = "t2i_adapter"

    def __init__(self, in_channels: int = 3, name=None, device=None, path=None):
        if int(in_channels) not in (1, 3):
            raise ValueError(f"t2i_adapter: in_channels = {in_channels!r} (1 or 3)")
        self.name = name or "t2i_adapter"
        self.device = device if device is not None else default_device()
        self.in_channels = int(in_channels)
        self._W = None
        self.state: Optional[Dict[str, np.ndarray]] = None   # t2iadapter.read_state's result: what t2iadapter.forward_host takes
        self.weights_version = 0
        self._plans: Dict[tuple, _BoundPlan] = {}
        self._use_graph = False
        self._last = None   # (key, the four bf16 device tensors) of the last picture
        self.runs = 0       # how often the network ran (the cache's tests count it)
        if path is not None:
            self.load(path)

    def _require_weights(self):
        if self._W is None:
            raise RuntimeError(f"{self.name}: no weights set (pass path=, call set_state() or T2IAdapter.synthetic())")

    def compile(self, jit_compile=True, **_):
        """As HipModel.compile: the plan of a picture size is replayed from a hipGraph captured on its first use.  Off by default: the
        31 launches run once per job, and only for a new picture."""
        self._use_graph = bool(jit_compile)
        self._plans.clear()

    @staticmethod
    def specs(in_channels: int) -> List["wtab.WeightSpec"]:
        """The weight table: per conv a Keras-layout kernel and a bias, under `adapter.<layer>` (t2iadapter.layer_names)."""
        from . import t2iadapter as t2i_mod

        out = []
        for layer, (co, ci, k, _k) in t2i_mod.layer_names(in_channels):
            out.append(wtab.WeightSpec("adapter." + layer + ".weight", None, "adapter." + layer, "conv_w", wtab.CONV_PERM, (k, k, ci, co)))
            out.append(wtab.WeightSpec("adapter." + layer + ".bias", None, "adapter." + layer, "bias", None, (co,)))
        return out

    def set_state(self, state) -> None:
        """Adopt a loaded checkpoint in either public layout (t2iadapter.read_state's input; fp16 files load) or read_state's own
        result; `in_channels` follows the state.  Raises on a missing key or a wrong shape, naming it."""
        from . import t2iadapter as t2i_mod

        state = dict(state)
        named = state if "body.0.resnets.0.block1.weight" in state else t2i_mod.read_state(state)
        cin = t2i_mod.in_channels_of(named)
        specs = self.specs(cin)
        arrays = {}
        for s in specs:   # torch (out, in, k, k) -> the Keras (k, k, in, out) the packer starts from
            a = named[s.key[len("adapter."):]]
            arrays[(s.name, s.kind)] = np.ascontiguousarray(np.transpose(a, s.perm)) if s.perm is not None else a
        W, _ = packing.pack(layout.layout(specs, layout.Flags(engine.W_CHUNK_MAJOR, engine.MFMA_TEMB_PROJ)), arrays, self.device)
        self._W, self.in_channels = W, cin
        self.state = {k: np.asarray(v, dtype=np.float32) for k, v in named.items()}
        self.weights_version += 1
        self._plans.clear()
        self._last = None

    def load(self, path: str) -> None:
        path = os.fspath(path)
        if not os.path.exists(path):
            raise ValueError(f"t2i_adapter: checkpoint {path!r} not found")
        self.set_state(wtab.read_state_dict(path))

    @staticmethod
    def synthetic_state(seed: int = 0, in_channels: int = 3, scale: float = 1.0) -> Dict[str, np.ndarray]:
        """The flat state dict of synthetic(): diffusers' file layout, float32 arrays (t2iadapter.synthetic_state)."""
        from . import t2iadapter as t2i_mod

        return t2i_mod.synthetic_state(seed, in_channels, scale)

    @classmethod
    def synthetic(cls, seed: int = 0, in_channels: int = 3, device=None, scale: float = 1.0) -> "T2IAdapter":
        """A seeded synthetic adapter, for tests and fixtures like the synthetic UNet."""
        m = cls(in_channels, device=device)
        m.set_state(cls.synthetic_state(seed, in_channels, scale))
        return m

    def _build(self, H: int, W: int) -> _BoundPlan:
        plan = engine.Plan(self.device)
        e = engine.Emitter(plan, self._W)
        cin = self.in_channels
        px = plan.alloc(H * W * cin * 4)
        feats = engine.emit_t2i_adapter(e, px, 1, H, W, cin)
        plan.finalize()
        bp = _BoundPlan(plan, self._use_graph)
        bp.io["picture"] = px.tensor(torch.float32, (1, H, W, cin))
        for l, f in enumerate(feats):
            bp.io[f"feature.{l}"] = f.buf.tensor(torch.bfloat16, (1, f.H, f.W, f.C))
        return bp

    def _picture(self, picture) -> np.ndarray:
        from . import t2iadapter as t2i_mod

        px = _np32(picture)
        px = px[None] if px.ndim == 3 else px
        if px.ndim != 4 or px.shape[0] != 1 or px.shape[3] != self.in_channels:
            raise ValueError(f"t2i_adapter: a picture of shape {px.shape} for an adapter of {self.in_channels} input channel(s): "
                             f"(1, H, W, {self.in_channels}) in [0, 1], one picture per job")
        t2i_mod.check_size(px.shape[1], px.shape[2])
        return px

    def features(self, picture) -> List[torch.Tensor]:
        """picture (1, H, W, cin) or (H, W, cin) float32 in [0, 1] (t2iadapter.picture's result) -> the four bf16 feature tensors
        (1, H / 8 / 2^l, W / 8 / 2^l, ch_l) on the device, copies the caller owns.  The last picture's are kept."""
        import hashlib

        self._require_weights()
        px = self._picture(picture)
        key = (hashlib.sha256(px.tobytes()).hexdigest(), px.shape, self.weights_version, engine.GN_EPOCH)
        if self._last is None or self._last[0] != key:
            H, W = px.shape[1], px.shape[2]
            bp = self._plans.get((H, W))
            if bp is None:
                bp = self._plans[(H, W)] = self._build(H, W)
            bp.io["picture"].copy_(torch.from_numpy(px))
            bp.run()
            self.runs += 1
            self._last = (key, [bp.io[f"feature.{l}"].clone() for l in range(4)])
        return [f.clone() for f in self._last[1]]   # (small, once per job: a caller that writes into them cannot reach the kept ones)

    def predict_on_batch(self, picture) -> List[np.ndarray]:
        """picture (1, H, W, cin) or (H, W, cin) in [0, 1], H and W multiples of 64 -> the four features as float32 NHWC arrays, the
        plan's bf16 values widened."""
        return [f.to(torch.float32).cpu().numpy() for f in self.features(picture)]

    __call__ = predict_on_batch
