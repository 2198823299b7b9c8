"""``StableDiffusion`` — the reference's public pipeline API over the MI355X path.

Mirrors reference ``stable_diffusion/stable_diffusion.py`` (class ``StableDiffusionBase`` :47-568 and
``StableDiffusion`` :575-725): same constructor arguments, same ``text_to_image`` /
``image_to_image`` / ``generate_image`` signatures and defaults, same lazily-built model
properties, same return value (``uint8 (B, H, W, 3)``).  What differs is where the loop runs:

* ``generate_image`` keeps the whole denoise loop on the GPU (:class:`DenoiseEngine`): the
  cond + uncond UNet passes of one step run as ONE batch-2B forward (no op couples samples, so
  this is the same arithmetic as the reference's two ``predict_on_batch`` calls, uncond rows
  first), CFG + rescale + the sampler step are one kernel, and the step (or the whole loop when no
  per-step callback is installed) is replayed from a hipGraph.  The latent never leaves HBM.
* ``host_loop=True`` runs the reference's own control flow instead — numpy CFG / rescale /
  ``Scheduler.step`` around ``predict_on_batch`` calls (stable_diffusion.py:442-479) — which is
  what a maintainer gets by only swapping the model classes; tests use it to check that both
  routes agree.

* With ``model.shard_batch = True`` (default False = the reference's semantics: every process runs the batch it was given),
  under a ``torch.distributed`` process group ``generate_image`` treats ``batch_size`` as the GLOBAL batch and shards it over
  the ranks: one packed broadcast of rank 0's inputs, no traffic inside a step, one all-gather of the result.

Also on this path: ``image_to_image`` (VAE encoder + shortened schedule), ``inpaint`` (latent blend
inside the sampler kernel, pixel blend before the uint8 cast), the TCD sampler, and the CLIP text models behind
``encode_text`` (token ids or, with a local BPE merge list, strings).  Not here: the reference's download helpers and
its Gradio / Streamlit shells.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib, engine, ops
from . import control as control_mod
from . import ipadapter as ipadapter_mod
from . import t2iadapter as t2i_mod
from . import hires as hires_mod
from . import dynthresh as dynthresh_mod
from . import hypertile as hypertile_mod
from . import pag as pag_mod
from . import sag as sag_mod
from . import reference as reference_mod
from . import regions as regions_mod
from . import samplers as smp
from . import tiled as tiled_mod
from . import weights as wtab
from .jobopts import REFUSED, EngineOptions, job_options
from .models import (ControlNet, DiffusionModel, HintNet, ImageDecoder, ImageEncoder, TextClipEmbedding, TextEncoder, _BoundPlan,
                     _skip_hw, default_device)
from .scheduler import Scheduler

MAX_PROMPT_LENGTH = 77
# the ControlNet encoder on a side stream beside the UNet's down path (DenoiseEngine); "0": in line, in front of the UNet
CONTROLNET_OVERLAP = os.environ.get("MSD_CONTROLNET_OVERLAP", "1") != "0"


def get_timestep_embedding(timestep, batch_size, dim=320, max_period=10000):
    """Sinusoidal embedding, [cos | sin] (reference stable_diffusion.py:543-553)."""
    half = dim // 2
    freqs = np.exp(-np.log(max_period) * np.asarray(range(0, half), dtype=np.float32) / half)
    args = np.asarray([timestep], dtype=np.float32) * freqs
    embedding = np.concatenate([np.cos(args), np.sin(args)], axis=0)
    embedding = np.reshape(embedding, [1, -1])
    return np.repeat(embedding, batch_size, axis=0)


def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale=0.0, epsilon=1e-05):
    """Host version of the guidance rescale (reference stable_diffusion.py:304-315)."""
    axes = tuple(range(1, len(noise_pred_text.shape)))
    std_text = np.std(noise_pred_text, axis=axes, keepdims=True)
    std_cfg = np.std(noise_cfg, axis=axes, keepdims=True) + epsilon
    noise_pred_rescaled = noise_cfg * (std_text / std_cfg)
    return guidance_rescale * noise_pred_rescaled + (1.0 - guidance_rescale) * noise_cfg


class DenoiseEngine:
    """Device-resident denoise loop for a fixed (batch, context lengths, steps, guidance) shape."""

    def __init__(self, unet: DiffusionModel, B: int, t_cond: int, t_uncond: int, num_steps: int, guidance: float,
                 guidance_rescale: float, control_net: Optional[ControlNet] = None, hint_net: Optional[HintNet] = None,
                 use_graph: bool = True, streams: Optional[int] = None, inpaint: bool = False, tcd: bool = False,
                 control_nets=(), ip_adapter=None, **options):
        """`options`: the fields of jobopts.EngineOptions as a caller gives them; kept as `options` and each as its own attribute.
        `ip_adapter`: the models.IPAdapter of an engine built with ip_tokens = N - a model object, not an option.
        `control_nets`: the (ControlNet, HintNet) pairs of the units behind the first of an engine built with control_units = N -
        model objects, not options: N - 1 of them (unit 0 is `control_net` / `hint_net`)."""
        unet._require_weights()
        self.unet, self.B, self.num_steps = unet, B, num_steps
        self.h, self.w = unet.h, unet.w
        self.options = EngineOptions.of(**options)
        self.options.check(self.h, self.w, B, guidance, control_net is not None, inpaint, tcd, streams)   # (before anything is allocated)
        # self.sampler, .tiled, .regions, .region_mode, .pag, .reference, .adain, .hypertile, .sag, .dynthresh, .control_units: the
        # fields, as they are
        vars(self).update(vars(self.options))
        self.control_nets = [(control_net, hint_net)] + [tuple(pair) for pair in control_nets] if control_net is not None else []
        if len(self.control_nets) != max(self.control_units, 1 if control_net is not None else 0):
            raise ValueError(f"control: an engine of {self.control_units} unit(s) takes {max(self.control_units - 1, 0)} further "
                             f"(ControlNet, HintNet) pair(s) as control_nets, got {len(tuple(control_nets))}")
        self.ip_model = ip_adapter
        if (ip_adapter is None) != (self.ip_tokens == 0) or (ip_adapter is not None and ip_adapter.tokens != self.ip_tokens):
            raise ValueError(f"ip_adapter: an engine of ip_tokens = {self.ip_tokens} takes a models.IPAdapter of that many image tokens as "
                             f"ip_adapter, got {None if ip_adapter is None else ip_adapter.tokens}")
        if self.ip_tokens:
            for t in (t_cond, t_uncond) if guidance > 0.0 else (t_cond,):
                ipadapter_mod.check_context(t, self.ip_tokens)
        self.region_attn = self.region_mode == "attention"   # ("latent" without regions)
        if self.reference is not None and guidance > 0.0 and t_cond != t_uncond:
            raise ValueError("reference_only: the negative prompt must have the conditional context's token length "
                             f"({t_uncond} != {t_cond} tokens): the reference row rides in the one fused pass")
        self.use_graph = use_graph
        self.guidance = float(guidance)
        # ---- the rows of a step, computed here once: `passes`, the number of `eps` rows, the pass whose mid block writes SAG's map
        self.cfg = cfg = self.guidance > 0.0
        # Two ways to run the cond and uncond halves of a step (no op couples samples, so both are the
        # reference's two predict_on_batch calls, :442-460):
        #  * fused: ONE batch-2B forward;
        #  * dual (streams=2): two batch-B forwards on two HIP streams that fork after the previous
        #    sampler step and join before the next one.
        # The two forms measure the same within noise on MI355X at 512x512 because the small-batch
        # kernels are bounded by per-workgroup latency with idle CUs either way.  Fused is the default (one arena,
        # one kernel chain); dual stays selectable.
        self.dual = bool(cfg and streams == 2)
        fuse = cfg and (t_cond == t_uncond) and not self.dual
        # regions (R, the number of evaluated region prompts, or 0): the conditional half is R * B rows, region-major (row
        # r * B + b) behind the unconditional rows; one msd_region_combine launch in front of the guidance / sampler step sums them
        # per pixel with the weights of `region_w` into the first B of those rows, in place (minsdtf_amd/regions.py)
        # region_mode "attention": the UNet keeps the plain job's rows (only the CONTEXT rows grow); every attn2 gives the
        # conditional rows ONE msd_region_attention launch over the R region contexts with the level's weight plane (`region_w`: the
        # four levels' planes, regions.pack_levels), and there is no combine in the tail
        # pag (the set of attention blocks of a perturbed-attention-guidance job, or None): the conditional half is 2 * B rows, the
        # c rows and behind them the p rows (the same context; the selected blocks' attn1 is the identity for them); one
        # msd_region_combine launch in front of the guidance / sampler step writes c' = (1 + k) c - k p over the c rows with the two
        # constant planes of `pag_w` (minsdtf_amd/pag.py)
        RC = 1 if self.region_attn else (self.regions or (2 if self.pag else 1))   # conditional copies of the batch
        if not cfg:
            passes = [(0, RC * B, t_cond, "cond")]
        elif fuse:
            passes = [(0, (1 + RC) * B, t_cond, "both")]   # uncond rows, then cond rows
        else:
            passes = [(0, B, t_uncond, "uncond"), (B, RC * B, t_cond, "cond")]
        # reference (the set of attention blocks of a reference-only job, or None): the one fused pass carries one more row behind
        # the u and c rows, the reference latent noised to the step's level (msd_reference_latent at the head of the step plan);
        # in the selected blocks the rows in front of it attend to its keys too (msd_attention_joint, `ref_mix` per row).  The step
        # kernels still read eps as [2B][n]: the reference row's prediction is written and never read (minsdtf_amd/reference.py)
        # adain (the set of reference AdaIN sites of such a job, reference.ADAIN_SITES, or None): behind those block outputs the rows
        # in front of the reference row are renormalised to its channel statistics (msd_reference_adain, the same `ref_mix`); the
        # layer set may then be empty (AdaIN without the attention part)
        if self.reference is not None:
            (row0, nb, t, tag), = passes
            passes = [(row0, nb + 1, t, tag)]
        # sag (self-attention guidance, minsdtf_amd/sag.py): the step records the UNet TWICE - behind the pass that holds the u rows
        # (the c rows without guidance) in its first B rows, whose mid block also writes the attention map `sag_A`
        # (msdx_attention_colsum), ONE msdx_sag_degrade launch builds the degraded latent and a second forward of B rows over the same
        # context K/V writes the d rows; the tail combines (u, c, d) in front of the unchanged step kernel (engine.emit_sag_pass /
        # emit_sag_combine).  eps row groups of B rows: (u, c, d, copy of u, c') with guidance, (c, d) without
        self._sag_tag = passes[0][3] if self.sag else None
        self._eps_rows = (5 if cfg else 2) * B if self.sag else passes[-1][0] + passes[-1][1]   # (else: the rows the passes write)
        self.passes = passes
        self.has_control = control_net is not None
        prep = self._build_prep(control_net, hint_net)
        step = self._build_steps(control_net, prep)
        tail = self._build_tail(step, guidance, guidance_rescale, inpaint, tcd)
        if self.cn_plan is not None:
            self.cn_plan.finalize()   # (first: the main plan's zero convs record addresses of its feature maps)
            self._join = step.marks["controls"]
        for pl in self.branches:
            pl.finalize()
        self.tail = tail if self.dual else None
        if self.dual:
            tail.finalize()
        if self.dual or self.cn_plan is not None:
            self._side = torch.cuda.Stream(device=unet.device)
        self._step_graph: Optional[torch.cuda.CUDAGraph] = None
        self._loop_graph: Optional[torch.cuda.CUDAGraph] = None
        self._loop_graph_steps = 0
        self._warmed = False
        _lib.track_graph_owner(self)

    def _build_prep(self, control_net, hint_net) -> dict:
        """The preparation plans: per SCHEDULE the time-embedding tables (timestep -> MLP -> every ResBlock's projection: they do
        not depend on the prompt, so they run when the schedule changes, not per call); per CALL contexts -> K/V^T, hint.
        Returns what the step plans read of them: the tables, the K/V^T of every pass and the hint's activation."""
        unet, B, num_steps, h, w, passes = self.unet, self.B, self.num_steps, self.h, self.w, self.passes
        dev = unet.device
        prep_t = engine.Plan(dev)
        prep = engine.Plan(dev)
        e_t = engine.Emitter(prep_t, unet._W)
        e_u = engine.Emitter(prep, unet._W)
        self.step_ptr = torch.zeros(2, dtype=torch.int32, device=dev)   # {step index, ticket of msd_cfg_step's in-kernel advance}
        self._sched_key = None       # schedule whose coefficient / time-embedding tables are on the device
        self._step_init: Dict[int, torch.Tensor] = {}
        self.latent = torch.zeros(B, h, w, 4, dtype=torch.float32, device=dev)
        self.coef = torch.zeros(num_steps, smp.ROW if self.sampler is not None else 4, dtype=torch.float32, device=dev)
        self.temb_in = torch.zeros(num_steps, 320, dtype=torch.float32, device=dev)
        total_u = sum(c for _, c in engine.resblock_names(False))
        table_u = prep_t.alloc(num_steps * total_u * 4)
        engine.emit_time_embedding(e_t, self.temb_in, num_steps, table_u, encoder_only=False)
        self.ctx_in: Dict[str, torch.Tensor] = {}
        ctx_kv_u, ctx_kv_c = {}, {}
        # ip_tokens (N, or 0): the image tokens of an IP-Adapter job, fp32 [nb][N][768] per pass (a per-call upload: the unconditional
        # rows carry the tokens of the zero embedding, the conditional rows the picture's), their K / V^T for the 16 attn2 layers
        # recorded here once (engine.emit_ip_kv, the adapter's weights) - constant over the steps, nothing of it runs per step
        self.ip_in: Dict[str, torch.Tensor] = {}
        self._ip_kv: dict = {}
        e_ip = None
        if self.ip_tokens:
            self.ip_model._require_weights()
            e_ip = engine.Emitter(prep, self.ip_model._W)
        e_c = None
        table_c = total_c = None
        # control units (minsdtf_amd/control.py): every unit behind the first has its own time-embedding table, context K/V and hint,
        # recorded behind unit 0's; a unit on the ControlNet of a unit in front of it (another picture, the same weights) shares
        # that unit's table and K/V
        further = self.control_nets[1:]
        e_cn, tables_cn, kv_cn = [], [], [{} for _ in further]
        if self.has_control:
            control_net._require_weights()
            hint_net._require_weights()
            e_c = engine.Emitter(prep, control_net._W)
            total_c = sum(c for _, c in engine.resblock_names(True))
            table_c = prep_t.alloc(num_steps * total_c * 4)
            engine.emit_time_embedding(engine.Emitter(prep_t, control_net._W), self.temb_in, num_steps, table_c, encoder_only=True)
            for n, (cn, hn) in enumerate(further):
                cn._require_weights()
                hn._require_weights()
                same = [m for m in range(n + 1) if self.control_nets[m][0] is cn]   # (unit m, in front of unit n + 1)
                if same:
                    e_cn.append(None)
                    tables_cn.append(table_c if same[0] == 0 else tables_cn[same[0] - 1])
                    kv_cn[n] = ctx_kv_c if same[0] == 0 else kv_cn[same[0] - 1]
                    continue
                e_cn.append(engine.Emitter(prep, cn._W))
                tables_cn.append(prep_t.alloc(num_steps * total_c * 4))
                engine.emit_time_embedding(engine.Emitter(prep_t, cn._W), self.temb_in, num_steps, tables_cn[-1], encoder_only=True)
        for (_row0, nb, t, tag) in passes:
            if self.region_attn and tag != "uncond":   # context rows, not UNet rows: the B conditional rows read R * B contexts
                nb = nb + (self.regions - 1) * B
            st = torch.zeros(nb, t, 768, dtype=torch.float32, device=dev)
            self.ctx_in[tag] = st
            c16 = engine.Act(prep.alloc(nb * t * 768 * 2), nb, t, 1, 768)
            prep.rec(ops.cast_f32_to_bf16, x=st, out=c16.buf, n=nb * t * 768, name=f"context.{tag}.bf16")
            ctx_kv_u[tag] = engine.emit_context_kv(e_u, c16, engine.UNET_ATTN_LAYERS, prep)
            if e_ip is not None:
                N = self.ip_tokens
                self.ip_in[tag] = torch.zeros(nb, N, 768, dtype=torch.float32, device=dev)
                tok16 = engine.Act(prep.alloc(nb * N * 768 * 2), nb, N, 1, 768)
                prep.rec(ops.cast_f32_to_bf16, x=self.ip_in[tag], out=tok16.buf, n=nb * N * 768, name=f"ip_tokens.{tag}.bf16")
                self._ip_kv[tag] = engine.emit_ip_kv(e_ip, tok16, engine.UNET_ATTN_LAYERS, prep)
            if self.has_control:
                ctx_kv_c[tag] = engine.emit_context_kv(e_c, c16, engine.ENCODER_ATTN_LAYERS, prep)
                for n, e_n in enumerate(e_cn):
                    if e_n is not None:
                        kv_cn[n][tag] = engine.emit_context_kv(e_n, c16, engine.ENCODER_ATTN_LAYERS, prep)
        self.hint_img = None
        self.hint_imgs_further: List[torch.Tensor] = []
        hint_act = None
        hints_cn = []
        if self.has_control:
            # hint computed once per image batch (stable_diffusion.py:427-441), tiled to both halves
            nb_max = max(nb for (_r, nb, _t, _g) in passes)
            self.hint_img = torch.zeros(B, 8 * h, 8 * w, 3, dtype=torch.float32, device=dev)
            e_h = engine.Emitter(prep, hint_net._W)
            hint_act = prep.act(nb_max, h, w, 320)
            engine.emit_hintnet(e_h, self.hint_img, B, 8 * h, 8 * w, hint_act, copies=nb_max // B)
            for _cn, hn in further:   # every further unit: its HintNet on its own hint buffer
                img = torch.zeros(B, 8 * h, 8 * w, 3, dtype=torch.float32, device=dev)
                self.hint_imgs_further.append(img)
                hints_cn.append(prep.act(nb_max, h, w, 320))
                engine.emit_hintnet(engine.Emitter(prep, hn._W), img, B, 8 * h, 8 * w, hints_cn[-1], copies=nb_max // B)
        cols_c = engine.temb_columns(True)
        self._units_prep = [dict(table=(t, total_c, 0, cols_c), kv=kv, hint=hi) for t, kv, hi in zip(tables_cn, kv_cn, hints_cn)]
        prep_t.finalize()
        prep.finalize()
        self.prep, self.prep_t = prep, prep_t
        return dict(table_u=(table_u, total_u, 0, engine.temb_columns(False)), table_c=(table_c, total_c, 0, engine.temb_columns(True)),
                    kv_u=ctx_kv_u, kv_c=ctx_kv_c, hint=hint_act)

    def _build_steps(self, control_net, prep: dict) -> "engine.Plan":
        """The per-step UNet plans, one per stream (`branches`; `cn_plan`: the ControlNet encoder beside the UNet's down path).
        Returns the last of them, which takes the tail unless the engine is dual."""
        unet, B, h, w, R, passes = self.unet, self.B, self.h, self.w, self.regions, self.passes
        dev = unet.device
        n = h * w * 4
        self.eps = torch.zeros(self._eps_rows, n, dtype=torch.float32, device=dev)
        self.sag_A = self.sag_latent = self.sag_params = self.sag_w = None
        if self.sag:
            mh, mw = engine.unet_levels(h, w)[3]
            self.sag_A = torch.zeros(B, mh * mw, dtype=torch.float32, device=dev)
            self.sag_latent = torch.zeros(B, h, w, 4, dtype=torch.float32, device=dev)
            self.sag_params = torch.zeros(10, dtype=torch.float32, device=dev)
            self.sag_w = torch.zeros(3 if self.cfg else 2, h, w, dtype=torch.float32, device=dev)
        self.ref_z = self.ref_noise = self.ref_latent = self.ref_coef = self.ref_mix = None
        if self.reference is not None:
            self.ref_z, self.ref_noise, self.ref_latent = (torch.zeros(1, h, w, 4, dtype=torch.float32, device=dev) for _ in range(3))
            self.ref_coef = torch.zeros(self.num_steps, 2, dtype=torch.float32, device=dev)
            self.ref_mix = torch.zeros((2 if self.cfg else 1) * B, dtype=torch.float32, device=dev)
        self.region_w = torch.zeros(R, h, w, dtype=torch.float32, device=dev) if R else None
        region_planes = None
        if self.region_attn:   # one buffer for the four levels' planes [R][h_l * w_l] (regions.pack_levels)
            levels = engine.unet_levels(h, w)
            offs = regions_mod.level_offsets(R, levels)
            self.region_w = torch.zeros(offs[-1], dtype=torch.float32, device=dev)
            region_planes = {lv: _Ptr(self.region_w.data_ptr() + o * 4) for lv, o in zip(levels, offs)}
        self.pag_w = torch.zeros(2, h, w, dtype=torch.float32, device=dev) if self.pag else None
        # control_units (N, or 0): the per-step scale table of the N units, fp32 [num_steps][N][13][2] (control.table), a per-call upload
        self.cn_scales = torch.zeros(self.num_steps, self.control_units, 13, 2, dtype=torch.float32, device=dev) if self.control_units else None
        # ip_tokens: the per-step scale table of the image prompt, fp32 [num_steps][16] (ipadapter.table), a per-call upload
        self.ip_scales = torch.zeros(self.num_steps, 16, dtype=torch.float32, device=dev) if self.ip_tokens else None
        # t2i_units (U, or 0): the adapters' features, bf16 [h_l * w_l * ch_l] per unit and site, and their per-step scale table, fp32
        # [num_steps][U][4] (t2iadapter.table): buffers the engine owns, per-call uploads - one engine serves every picture
        self.t2i_scales = self.t2i_feat = None
        if self.t2i_units:
            self.t2i_scales = torch.zeros(self.num_steps, self.t2i_units, 4, dtype=torch.float32, device=dev)
            self.t2i_feat = [[torch.zeros(hl * wl * ch, dtype=torch.bfloat16, device=dev) for (hl, wl), ch in zip(engine.unet_levels(h, w), wtab.UNET_CH)]
                             for _u in range(self.t2i_units)]
        self.branches = []
        step = None
        # ControlNet beside the UNet's down path: its encoder reads the same latent and is independent of the UNet until the
        # 13 residuals are added after the down path (diffusion_model.py:230-234), so with one fused pass it runs as its own
        # plan (own arena, GroupNorm / split-K scratch) on a side stream: ONE fork after the sampler step, ONE join in front
        # of the zero convs.  (Two passes — a negative prompt of another length — and the two-stream mode keep it in line.)
        self.cn_plan = None
        overlap = self.has_control and CONTROLNET_OVERLAP and len(passes) == 1 and not self.dual
        for (row0, nb, t, tag) in passes:
            if step is None or self.dual:
                step = engine.Plan(dev)   # dual: each half owns its arena, the halves are live at the same time
                self.branches.append(step)
                s_u = engine.Emitter(step, unet._W, step_ptr=self.step_ptr)
                s_c = engine.Emitter(step, control_net._W, step_ptr=self.step_ptr) if self.has_control else None
                s_cn = [engine.Emitter(step, cn._W, step_ptr=self.step_ptr) for cn, _hn in self.control_nets[1:]]
            taps = None
            units = None
            if self.has_control:
                # ControlNet encoder first; its 13 zero convs run inside the UNet plan, fused with the residual adds
                hint_nb = engine.Act(prep["hint"].buf, nb, h, w, 320)  # first nb rows of the tiled hint
                s_cf = s_c
                if overlap:
                    self.cn_plan = engine.Plan(dev)
                    s_cf = engine.Emitter(self.cn_plan, control_net._W, step_ptr=self.step_ptr)
                feats = engine.emit_controlnet_features(s_cf, self.latent, B, nb, h, w, prep["table_c"], prep["kv_c"][tag], t, hint_nb)
                taps = (s_c, feats)
            if self.control_units:
                # one encoder per unit, where unit 0's runs (beside the UNet's down path, or in line); their zero convs and the ONE
                # msdc_control_combine run inside the UNet plan, the scales read from row *step_ptr of `cn_scales`
                unit_taps = [taps]
                for (cn, _hn), s_n, up in zip(self.control_nets[1:], s_cn, self._units_prep):
                    s_nf = engine.Emitter(self.cn_plan, cn._W, step_ptr=self.step_ptr) if overlap else s_n
                    feats = engine.emit_controlnet_features(s_nf, self.latent, B, nb, h, w, up["table"], up["kv"][tag], t,
                                                            engine.Act(up["hint"].buf, nb, h, w, 320))
                    unit_taps.append((s_n, feats))
                rows_u = {"both": B, "uncond": nb, "cond": 0}[tag]
                taps, units = None, (self.cn_scales, self.num_steps, rows_u, unit_taps)
            eps_view = _Ptr(self.eps.data_ptr() + row0 * n * 4)
            if self.reference is not None:   # x_r of this step first, then the forward whose last row reads it
                step.rec(ops.reference_latent, z=self.ref_z, noise=self.ref_noise, coef=self.ref_coef, step_ptr=self.step_ptr,
                         out=self.ref_latent, n=n, num_steps=self.num_steps)
            sag_here, sag_ws = tag == self._sag_tag, None
            if sag_here:
                sag_ws = step.alloc(ops.colsum_workspace_floats(B, 8, mh * mw) * 4)
            engine.emit_unet(s_u, self.latent, B, nb, h, w, prep["table_u"], prep["kv_u"][tag], t, eps_view, control_taps=taps,
                             variant=self._unet_variant(tag, region_planes, sag_ws), **({} if units is None else dict(control_units=units)))
            if sag_here:
                step.free(sag_ws)
                d_rows = _Ptr(self.eps.data_ptr() + (2 if self.cfg else 1) * B * n * 4)
                engine.emit_sag_pass(s_u, self.latent, eps_view, self.coef, int(self.coef.shape[1]), self.num_steps, self.sag_A,
                                     self.sag_params, self.sag_latent, B, h, w, prep["table_u"], prep["kv_u"][tag], t, d_rows)
        return step

    def _unet_variant(self, tag: str, region_planes, sag_ws) -> "engine.UNetVariant":
        """How the pass `tag` differs from the plain forward, every option adding its own fields.  The refusals (jobopts.REFUSED) are
        what makes the contributions disjoint: pag, regions in attention mode, reference, hypertile and sag exclude each other."""
        kw, B = {}, self.B
        if self.pag and tag != "uncond":   # the p rows are the last B rows of the pass that holds the conditional rows
            kw.update(pag_layers=self.pag, perturbed=B)
        if self.region_attn and tag != "uncond":   # the conditional rows are the last B rows of their pass
            kw.update(region_attn=(self.regions, B, region_planes))
        if self.reference is not None:
            kw.update(reference=(self.reference, self.ref_latent, self.ref_mix), adain=self.adain)
        # hypertile ((nh, nw, depth) of a HyperTile job, or None): the self-attention of the attention blocks of levels 0 .. depth
        # is taken inside nh x nw windows (msd_attention_windowed in place of msd_attention, every row of every pass); nothing else
        # in the step changes and nothing is uploaded per call (minsdtf_amd/hypertile.py)
        if self.hypertile is not None:
            kw.update(window=self.hypertile[:2], window_depth=self.hypertile[2])
        if sag_ws is not None:   # this pass holds the u rows (the c rows without guidance) in its first B rows
            kw.update(sag=(self.sag_A, sag_ws, 0, B))
        # ip_tokens: every attn2 of the UNet (not of a ControlNet's encoder) is ONE msdi_attention_decoupled launch over the text
        # keys and this pass's image-token K / V^T, its scale read from row *step_ptr of `ip_scales` (minsdtf_amd/ipadapter.py)
        if self.ip_tokens:
            kw.update(ip=(self._ip_kv[tag], self.ip_tokens, self.ip_scales, self.num_steps))
        # t2i_units: behind each of the four sites of the down path ONE msda_feature_add launch adds the units' features to every row
        # of the pass, its scales read from row *step_ptr of `t2i_scales` (minsdtf_amd/t2iadapter.py)
        if self.t2i_units:
            kw.update(t2i=(self.t2i_feat, self.t2i_scales, self.num_steps))
        return engine.UNetVariant(**kw)

    def _build_tail(self, step, guidance, guidance_rescale, inpaint, tcd) -> "engine.Plan":
        """What follows the UNet in a step: the region combine, the guidance / sampler step, the tile consensus - recorded behind
        the UNet in `step`, or (dual) in a plan of their own, which is returned."""
        B, num_steps, h, w, R, tiled = self.B, self.num_steps, self.h, self.w, self.regions, self.tiled
        dev = self.unet.device
        n = h * w * 4
        tail = engine.Plan(dev) if self.dual else step
        # inpainting (reference :469-475): the blend with the re-noised encoded image is part of the sampler kernel
        self.inpaint = None
        if inpaint:
            self.inpaint = {"init": torch.zeros(n, dtype=torch.float32, device=dev),
                            "noise": torch.zeros(B, n, dtype=torch.float32, device=dev),
                            "mask": torch.ones(n, dtype=torch.float32, device=dev)}
        ip = self.inpaint or {}
        # TCD sampler: one N(0,1) draw per step and sample, made on the host in the reference's order (prepare())
        stochastic = tcd or (self.sampler is not None and self.sampler.stochastic)
        self.step_noise = torch.zeros(num_steps, B, n, dtype=torch.float32, device=dev) if stochastic else None
        self.noise_coef = torch.zeros(num_steps, dtype=torch.float32, device=dev) if tcd else None
        self.denoised_prev = None
        if R and not self.region_attn:
            # (R == 1 too: a weight of all ones copies the row bit for bit)  Behind it the step kernels read [2B][n] (or [B][n])
            cond = _Ptr(self.eps.data_ptr() + (B if self.cfg else 0) * n * 4)
            tail.rec(ops.region_combine, eps=cond, w=self.region_w, out=cond, regions=R, batch=B, n=n)
        if self.pag:
            # c' = (1 + k) c - k p over the c rows; behind it the step kernels read [2B][n] (or [B][n]) as always
            cond = _Ptr(self.eps.data_ptr() + (B if self.cfg else 0) * n * 4)
            tail.rec(ops.region_combine, eps=cond, w=self.pag_w, out=cond, regions=2, batch=B, n=n, name="pag_combine")
        eps_in = self.eps
        if self.sag:   # (u, c, d) -> (u, c') where the step kernels read them; behind it they read [2B][n] (or [B][n]) as always
            group = engine.emit_sag_combine(tail, lambda g_: _Ptr(self.eps.data_ptr() + g_ * B * n * 4),
                                            lambda i: _Ptr(self.sag_w.data_ptr() + i * h * w * 4), B, n, self.cfg)
            eps_in = _Ptr(self.eps.data_ptr() + group * B * n * 4)
        # dynthresh (dynamic thresholding, minsdtf_amd/dynthresh.py): behind the regions / PAG / SAG combines ONE msdt_dynamic_threshold
        # launch writes the combined prediction of the rows (u, c) over the u rows, its scales read from row *step_ptr of
        # `dt_scales`; the step kernel then takes those rows as they are (guidance 0, no rescale: engine.emit_dynamic_threshold)
        self.dt_scales = self.dt_params = None
        if self.dynthresh:   # (u, c) -> the combined prediction over the u rows; the step kernels then read [B][n] and combine nothing
            self.dt_scales = torch.zeros(num_steps, 2, dtype=torch.float32, device=dev)
            self.dt_params = torch.zeros(dynthresh_mod.PARAM_BYTES // 4, dtype=torch.int32, device=dev)
            eps_in = engine.emit_dynamic_threshold(tail, eps_in, self.dt_scales, self.dt_params, self.step_ptr, B, h, w, num_steps)
            guidance = guidance_rescale = 0.0
        # sampler (a name of minsdtf_amd/samplers.py, or None): a multistep / ancestral sampler through msd_sampler_step, with
        # the 8-wide coefficient rows, the previous denoised estimate and (stochastic samplers) per-step draws on the device
        if self.sampler is None:
            tail.rec(ops.cfg_step, eps=eps_in, latent=self.latent, coef=self.coef, step_ptr=self.step_ptr, batch=B, n=n,
                     num_steps=num_steps, guidance=guidance, guidance_rescale=guidance_rescale, advance=2,
                     inpaint_init=ip.get("init"), inpaint_noise=ip.get("noise"), inpaint_mask=ip.get("mask"),
                     step_noise=self.step_noise, noise_coef=self.noise_coef)
        else:
            # (P needs no initial value: the first executed row has c_P = 0 and the kernel does not read it there)
            self.denoised_prev = torch.zeros(B, n, dtype=torch.float32, device=dev)
            tail.rec(ops.sampler_step, eps=eps_in, latent=self.latent, coef=self.coef, step_ptr=self.step_ptr,
                     denoised_prev=self.denoised_prev, batch=B, n=n, num_steps=num_steps, guidance=guidance,
                     guidance_rescale=guidance_rescale, advance=2, inpaint_init=ip.get("init"), inpaint_noise=ip.get("noise"),
                     inpaint_mask=ip.get("mask"), step_noise=self.step_noise)
        # tiled (a tiled.Geometry, or None): the B rows are the views of B / V canvases, sample-major (row b * V + v); the step
        # plan ends with one msd_tile_consensus launch that averages the stepped views into `canvas` and back into `latent`
        self.canvas = self._tile_args = None
        if tiled is not None:
            images = B // tiled.views
            self.canvas = torch.zeros(images, tiled.H, tiled.W, 4, dtype=torch.float32, device=dev)
            self._tile_w = (torch.from_numpy(tiled.wy).to(dev), torch.from_numpy(tiled.wx).to(dev))
            self._tile_args = dict(tiles=self.latent, canvas=self.canvas, wy=self._tile_w[0], wx=self._tile_w[1], ys=tiled.ys, xs=tiled.xs,
                                   th=tiled.th, tw=tiled.tw, H=tiled.H, W=tiled.W, batch=images)
            # after the sampler step, so inside the per-step graph and the whole-loop graph
            tail.rec(ops.tile_consensus, mode=tiled_mod.MODE_CONSENSUS, **self._tile_args)
        return tail

    def release_graphs(self) -> None:
        """Destroy the captured step / loop graphs (re-captured on the next run_steps)."""
        self._step_graph = self._loop_graph = None
        self._loop_graph_steps = 0

    def load_canvas(self, canvas_noise) -> None:
        """Tiled engines: upload the canvas-shaped start latent and cut it into the views with ONE gather launch
        (msd_tile_consensus, mode 1), stream-ordered in front of prepare(noise=None, ...)."""
        if self.tiled is None:
            raise ValueError("load_canvas: not a tiled engine")
        self.canvas.copy_(_f32_tensor(canvas_noise))
        ops.tile_consensus(mode=tiled_mod.MODE_GATHER, **self._tile_args)(torch.cuda.current_stream().cuda_stream)

    @property
    def calls(self):
        """Every launch of one sampler step, in issue order (profiling / bench helpers)."""
        out = [c for pl in self.branches for c in pl.calls]
        if self.cn_plan is not None:   # (listed in front of the UNet's calls, which is where they ran before the overlap)
            out = self.cn_plan.calls + out
        return out + (self.tail.calls if self.tail is not None else [])

    def contexts(self, unconditional_context, context) -> dict:
        """The `prepare` input for this engine's pass layout (host arrays or device tensors).  A regional engine takes `context`
        as the list of its R region contexts, each (B, T, 768): laid out uncond, region 0, region 1, ..., each B rows.  A PAG engine
        repeats `context` for its p rows: uncond, cond, cond."""
        if isinstance(context, (list, tuple)):
            if len(context) != self.regions:
                raise ValueError(f"this engine evaluates {self.regions} region prompt(s): pass that many contexts as a list")
            if any(isinstance(c, torch.Tensor) for c in context):
                dev = next(c.device for c in context if isinstance(c, torch.Tensor))
                context = torch.cat([_f32_tensor(c).to(dev) for c in context], dim=0)
            else:
                context = np.concatenate([np.asarray(c, dtype=np.float32) for c in context], axis=0)
        if self.pag:   # the p rows read the conditional context again
            context = torch.cat([context, context], dim=0) if isinstance(context, torch.Tensor) else np.concatenate([context, context], axis=0)
        if self.reference is not None:   # the reference row reads the conditional context of sample 0
            context = torch.cat([context, context[:1]], dim=0) if isinstance(context, torch.Tensor) else np.concatenate([context, context[:1]], axis=0)
        if not self.cfg:
            return {"cond": context}
        if len(self.passes) == 1:
            if isinstance(context, torch.Tensor) or isinstance(unconditional_context, torch.Tensor):
                u, c = _f32_tensor(unconditional_context), _f32_tensor(context)
                dev = c.device if isinstance(context, torch.Tensor) else u.device   # ONE target: the tensor argument's device
                return {"both": torch.cat([u.to(dev), c.to(dev)], dim=0)}
            return {"both": np.concatenate([unconditional_context, context], axis=0)}
        return {"uncond": unconditional_context, "cond": context}

    def _one_step(self, main: "torch.cuda.Stream") -> None:
        """Issue one sampler step on `main` (dual: the cond half forks to the side stream and joins
        before the CFG / sampler kernel).  Works eagerly and under stream capture."""
        if self.cn_plan is not None:
            side = self._side
            side.wait_stream(main)
            self.cn_plan.run(side.cuda_stream)                          # ControlNet encoder ...
            self.branches[0].run_range(main.cuda_stream, 0, self._join)   # ... beside conv_in + the UNet's down path + mid block
            main.wait_stream(side)
            self.branches[0].run_range(main.cuda_stream, self._join)      # zero convs (+ residual adds), up path, sampler step
            return
        if not self.dual:
            self.branches[0].run(main.cuda_stream)
            return
        side = self._side
        side.wait_stream(main)
        self.branches[0].run(main.cuda_stream)
        self.branches[1].run(side.cuda_stream)
        main.wait_stream(side)
        self.tail.run(main.cuda_stream)

    # ---- graphs
    def _capture(self, fn) -> torch.cuda.CUDAGraph:
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                fn(torch.cuda.current_stream())
        torch.cuda.current_stream().wait_stream(s)
        return g

    def _warm(self) -> None:
        """One eager step before the first capture (code objects load on first launch, which must
        not happen inside a stream capture); the latent and step counter are restored."""
        if self._warmed:
            return
        saved = (self.latent.clone(), self.step_ptr.clone())
        self._one_step(torch.cuda.current_stream())
        torch.cuda.synchronize()
        self.latent.copy_(saved[0])
        self.step_ptr.copy_(saved[1])
        self._warmed = True

    def run_steps(self, count: int, callback: Optional[Callable[[int], None]] = None) -> None:
        """Advance the latent by `count` sampler steps from the current device step counter."""
        if not self.use_graph:
            st = torch.cuda.current_stream()
            for i in range(count):
                self._one_step(st)
                if callback is not None:
                    st.synchronize()   # callback(iteration) fires after the step has finished, like the reference's
                    callback(i + 1)
            return
        if callback is None:
            if self._loop_graph is None or self._loop_graph_steps != count:
                def whole(stream):
                    for _ in range(count):
                        self._one_step(stream)
                self._warm()
                self._loop_graph = self._capture(whole)  # capture records, it does not execute
                self._loop_graph_steps = count
            self._loop_graph.replay()
            return
        if self._step_graph is None:
            self._warm()
            self._step_graph = self._capture(self._one_step)
        # the reference calls callback(iteration) after the step has FINISHED (stable_diffusion.py:476-479): progress
        # bars and cancellation rely on that, so wait for each replay before reporting it
        done = torch.cuda.Event()
        for i in range(count):
            self._step_graph.replay()
            done.record()
            done.synchronize()
            callback(i + 1)

    def prepare(self, contexts: Dict[str, np.ndarray], noise: np.ndarray, scheduler: Scheduler, timesteps,
                start_index: int = 0, hint_image: Optional[np.ndarray] = None, inpaint=None, step_noise=None, sampler=None,
                regions=None, pag_scale=None, reference=None, sag=None, dynamic_threshold=None, control=None, ip_adapter=None,
                t2i_adapter=None) -> None:
        """Upload the per-call inputs and run the preparation plan.  Every array may be a host array or a (device) tensor.
        noise = None: the start latent is already in `self.latent` (written there by stream-ordered device work queued before
        this call: the hand-off of a hires job), nothing is uploaded for it.
        inpaint = (init_latent (1,h,w,4), noise (B,h,w,4), latent mask (h,w) or (h,w,1)) for an engine built with
        inpaint=True; step_noise = (B, num_steps, h*w*4) TCD draws made by the caller (sharded runs: the slice of the
        draws for the global batch) instead of the draws made here.  An engine built with a sampler takes its
        samplers.Schedule as `sampler` (the coefficient rows are built here for `start_index`) and, for the stochastic samplers,
        its draws as `step_noise` (B, num_steps, ...) (drawn here from numpy's global stream when None).
        regions = the normalised weights (R, h, w) of a regional engine (regions.weights): a per-call upload, like the inpaint mask;
        an attention-mode engine takes the four levels' planes as one flat array (regions.pack_levels of Resolved.level_weights).
        pag_scale = the scale s of a PAG engine: the two planes fp32(1 + k), fp32(-k) (pag.weights, k from s and the engine's
        guidance in float64) are a per-call upload too, so another scale needs no other engine.
        reference = (z_ref (1, h, w, 4), n_ref (1, h, w, 4), fidelity) of an engine built with reference=<layers>: the two latents,
        the rate table of this schedule and start index (reference.rates) and mix = [fidelity] * B + [0] * B are per-call uploads.
        sag = the sag.Resolved (or SagSpec / dict) of an engine built with sag=True: the 9 taps and the threshold (sag.params) and the
        planes of the combine (sag.weights, k from the scale and the engine's guidance in float64) are per-call uploads too.
        dynamic_threshold = the dynthresh.Resolved (or DynThreshSpec / dict) of an engine built with dynthresh=True: the scale table
        of the executed steps (dynthresh.scales over num_steps - start_index steps from the engine's guidance, rounded once to fp32,
        in rows start_index ..) and the 32 bytes of dynthresh.params are per-call uploads too.
        control = (table, hints) of an engine built with control_units = N: the scale table fp32 [num_steps][N][13][2] (control.table
        over this engine's num_steps: its rows are the step counter's, whatever `start_index` is) and the N - 1 conditioning
        pictures of the further units, each like `hint_image`, are per-call uploads too: weights, ranges and modes re-record nothing.
        ip_adapter = (tokens_u, tokens_c, table) of an engine built with ip_tokens = N: the image tokens (N, 768) of the unconditional
        and of the conditional rows and the scale table fp32 [num_steps][16] (ipadapter.table over this engine's num_steps) are
        per-call uploads too: another picture, weight, range or weight type re-records nothing.
        t2i_adapter = (features, table) of an engine built with t2i_units = U: per unit the four bf16 features of
        models.T2IAdapter.features and the scale table fp32 [num_steps][U][4] (t2iadapter.table over this engine's num_steps) are
        per-call uploads too: another picture, weight or range re-records nothing."""
        if (t2i_adapter is None) != (self.t2i_scales is None):
            raise ValueError("prepare: `t2i_adapter` goes with an engine built with t2i_units=U, and only with one")
        if self.t2i_scales is not None:
            feats, tab = t2i_adapter
            tab = _f32_tensor(tab)
            got = [[int(f.numel()) for f in fs] for fs in feats]
            want = [[int(f.numel()) for f in fs] for fs in self.t2i_feat]
            if tuple(tab.shape) != tuple(self.t2i_scales.shape) or got != want:
                raise ValueError(f"prepare: adapter features of {got} elements and a table of shape {tuple(tab.shape)}, this engine's are "
                                 f"{want} and {tuple(self.t2i_scales.shape)}")
            self.t2i_scales.copy_(tab)
            for dst_u, src_u in zip(self.t2i_feat, feats):
                for dst, src in zip(dst_u, src_u):
                    dst.copy_(src.reshape(-1))
        if (ip_adapter is None) != (self.ip_scales is None):
            raise ValueError("prepare: `ip_adapter` goes with an engine built with ip_tokens=N, and only with one")
        if self.ip_scales is not None:
            tok_u, tok_c, tab = (_f32_tensor(a) for a in ip_adapter)
            want = (self.ip_tokens, 768)
            if tuple(tab.shape) != tuple(self.ip_scales.shape) or tuple(tok_u.shape) != want or tuple(tok_c.shape) != want:
                raise ValueError(f"prepare: image tokens of shapes {tuple(tok_u.shape)}, {tuple(tok_c.shape)} and a table of shape "
                                 f"{tuple(tab.shape)}, this engine's are {want} and {tuple(self.ip_scales.shape)}")
            self.ip_scales.copy_(tab)
            for tag, dst in self.ip_in.items():
                if tag == "both":   # the unconditional rows first
                    dst[:self.B].copy_(tok_u.to(dst.device).expand(self.B, -1, -1))
                    dst[self.B:].copy_(tok_c.to(dst.device).expand(dst.shape[0] - self.B, -1, -1))
                else:
                    dst.copy_((tok_u if tag == "uncond" else tok_c).to(dst.device).expand(dst.shape[0], -1, -1))
        if (control is None) != (self.cn_scales is None):
            raise ValueError("prepare: `control` goes with an engine built with control_units=N, and only with one")
        if self.cn_scales is not None:
            tab, hints = control
            tab = _f32_tensor(tab)
            if tuple(tab.shape) != tuple(self.cn_scales.shape) or len(hints) != len(self.hint_imgs_further):
                raise ValueError(f"prepare: control table of shape {tuple(tab.shape)} with {len(hints)} further hint(s), this engine's "
                                 f"are {tuple(self.cn_scales.shape)} and {len(self.hint_imgs_further)}")
            self.cn_scales.copy_(tab)
            for dst, hi in zip(self.hint_imgs_further, hints):
                hi = _f32_tensor(hi)
                if hi.shape[0] != self.B:
                    hi = hi.repeat(self.B // hi.shape[0], 1, 1, 1)
                dst.copy_(hi)
        if (dynamic_threshold is None) != (self.dt_params is None):
            raise ValueError("prepare: `dynamic_threshold` goes with an engine built with dynthresh=True, and only with one")
        if self.dt_params is not None:
            spec = dynthresh_mod.parse(dynamic_threshold)
            first = int(start_index)
            tab = dynthresh_mod.scales(spec, self.guidance, self.num_steps - first).astype(np.float32)
            tab = np.concatenate([np.repeat(tab[:1], first, axis=0), tab], axis=0)   # (rows in front of the first step: never read)
            self.dt_scales.copy_(torch.from_numpy(np.ascontiguousarray(tab)))
            self.dt_params.copy_(torch.from_numpy(dynthresh_mod.params(spec, self.h * self.w)))
        if (sag is None) != (self.sag_w is None):
            raise ValueError("prepare: `sag` goes with an engine built with sag=True, and only with one")
        if self.sag_w is not None:   # taps, threshold and the combine's planes: per-call uploads, another scale needs no other engine
            spec = sag_mod.parse(sag)
            self.sag_params.copy_(torch.from_numpy(sag_mod.params(spec)))
            self.sag_w.copy_(torch.from_numpy(sag_mod.weights(spec.scale, self.guidance, self.h, self.w)))
        if (reference is None) != (self.ref_mix is None):
            raise ValueError("prepare: `reference` goes with an engine built with reference=<layers>, and only with one")
        if self.ref_mix is not None:
            z_ref, n_ref, fidelity = reference
            self.ref_z.copy_(_f32_tensor(z_ref).reshape(self.ref_z.shape))
            self.ref_noise.copy_(_f32_tensor(n_ref).reshape(self.ref_noise.shape))
            rates = reference_mod.rates(sampler if self.sampler is not None else scheduler, int(start_index))
            self.ref_coef.copy_(torch.from_numpy(rates.astype(np.float32)))
            mix = [float(fidelity)] * self.B + [0.0] * self.B if self.cfg else [0.0] * self.B
            self.ref_mix.copy_(torch.tensor(mix, dtype=torch.float32))
        if (pag_scale is None) != (self.pag_w is None):
            raise ValueError("prepare: `pag_scale` goes with an engine built with pag=<layers>, and only with one")
        if self.pag_w is not None:
            self.pag_w.copy_(torch.from_numpy(pag_mod.weights(pag_scale, self.guidance, self.h, self.w)))
        if (regions is None) != (self.region_w is None):
            raise ValueError("prepare: `regions` (the weights) goes with an engine built with regions=R, and only with one")
        if self.region_w is not None:
            rw = _f32_tensor(regions)
            if tuple(rw.shape) != tuple(self.region_w.shape):
                raise ValueError(f"prepare: region weights of shape {tuple(rw.shape)}, this engine's are {tuple(self.region_w.shape)}")
            self.region_w.copy_(rw)
        if self.inpaint is not None:
            init, ip_noise, mask = inpaint
            self.inpaint["init"].copy_(_f32_tensor(init).reshape(-1))
            self.inpaint["noise"].copy_(_f32_tensor(ip_noise).reshape(self.B, -1))
            m = mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else mask
            m = np.asarray(m, dtype=np.float32)
            # preprocessed_mask keeps the reference's (width//8, height//8) resize (:301), which is only the latent's
            # (h, w) for square images; the reference's blend then fails to broadcast — fail the same way, loudly
            if m.shape[:2] != (self.h, self.w):
                raise ValueError(f"latent mask has shape {m.shape[:2]}, the latent is {(self.h, self.w)} "
                                 "(the reference's mask resize swaps width and height: non-square inpainting is unsupported)")
            m = m.reshape(self.h, self.w, 1)
            self.inpaint["mask"].copy_(torch.from_numpy(np.ascontiguousarray(np.broadcast_to(m, (self.h, self.w, 4))).reshape(-1)))
        for tag, arr in contexts.items():
            self.ctx_in[tag].copy_(_f32_tensor(arr))
        if noise is not None:
            self.latent.copy_(_f32_tensor(noise))
        # the schedule's tables: uploaded when the schedule changes, not per call (pageable host -> device copies make the
        # host wait for the stream, which keeps it from queueing this job behind the previous one's last kernels)
        # (keyed by the table's VALUES: a scheduler with other betas / final alpha / eta on the same timesteps is another schedule)
        if self.sampler is not None:
            if sampler is None or sampler.spec.name != self.sampler.name or sampler.num_steps != self.num_steps:
                raise ValueError(f"this engine runs the {self.sampler.name} sampler over {self.num_steps} steps: pass its Schedule")
            # (the rows depend on the start index: the first executed row never reads P)
            coef = smp.coefficient_table(sampler, int(start_index))
            taus = [float(t) for t in sampler.timesteps]   # fractional for Karras: the time embedding is taken at the float t
            sched_key = ("sampler", sampler.spec.name, sampler.timesteps.tobytes(), int(start_index), coef.tobytes())
        else:
            coef = scheduler.coefficient_table()
            taus = [int(t) for t in scheduler.timesteps]
            sched_key = (tuple(int(t) for t in scheduler.timesteps), bool(getattr(scheduler, "active_tcd", False)), coef.tobytes())
        # (and by the UNet's LoRA version: the table is the time_emb_proj layers' output, which a LoRA switch changes in place)
        sched_key = sched_key + (getattr(self.unet, "lora_version", 0),)
        if self._sched_key != sched_key:
            self.coef.copy_(torch.from_numpy(coef))
            temb = np.concatenate([get_timestep_embedding(t, 1) for t in taus], axis=0)
            self.temb_in.copy_(torch.from_numpy(np.ascontiguousarray(temb, dtype=np.float32)))
            self.prep_t.run(torch.cuda.current_stream().cuda_stream)
            self._sched_key = sched_key
        init = self._step_init.get(int(start_index))
        if init is None:
            init = self._step_init[int(start_index)] = torch.tensor([int(start_index), 0], dtype=torch.int32, device=self.step_ptr.device)
        self.step_ptr.copy_(init)   # {first step, ticket 0}: device -> device
        if self.step_noise is not None:
            if self.sampler is None:
                self.noise_coef.copy_(torch.from_numpy(scheduler.noise_coefficients()))
            if step_noise is None:
                step_noise = (tcd_step_noise(self.B, self.num_steps, self.h, self.w, start_index) if self.sampler is None
                              else smp.draw_step_noise(self.B, self.num_steps, self.h, self.w))
            self.step_noise.copy_(_f32_tensor(step_noise).reshape(self.B, self.num_steps, -1).transpose(0, 1))
        if self.has_control:
            hi = _f32_tensor(hint_image)
            if hi.shape[0] != self.B:   # (one hint for the whole batch: the reference tiles it, :435)
                hi = hi.repeat(self.B // hi.shape[0], 1, 1, 1)
            self.hint_img.copy_(hi)   # the cond / uncond replicas are made on the device (emit_hintnet)
        self.prep.run(torch.cuda.current_stream().cuda_stream)


def tcd_step_noise(B, num_steps, h, w, start_index) -> np.ndarray:
    """The TCD sampler's draws (B, num_steps, h*w*4), sample-major, from numpy's global stream in the reference's order:
    scheduler.py:301 draws np.random.randn(*latent.shape) once per executed step except the last."""
    z = np.zeros((B, num_steps, h * w * 4), dtype=np.float32)
    for i in range(int(start_index), num_steps - 1):
        z[:, i] = np.random.randn(B, h, w, 4).astype(np.float32).reshape(B, -1)
    return z


def _f32_tensor(x) -> torch.Tensor:
    """Host array or (device) tensor -> fp32 tensor for a copy_ into an engine buffer (no host round trip for tensors)."""
    if isinstance(x, torch.Tensor):
        return x.to(torch.float32)
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))


class _Ptr:
    def __init__(self, ptr):
        self.ptr = ptr


class StableDiffusionBase:
    """Base class for the stable diffusion 1.5 pipeline (reference stable_diffusion.py:47-568)."""

    def __init__(self, img_height=512, img_width=512, jit_compile=False, active_tcd=False):
        self.img_height = img_height
        self.img_width = img_width
        self._image_encoder = None
        self._text_encoder = None
        self._hint_net = None
        self._control_net = None
        self._text_clip_embedding = None
        self._diffusion_model = None
        self._image_decoder = None
        self._tokenizer = None
        self.jit_compile = jit_compile
        self.active_tcd = active_tcd
        self.scheduler = Scheduler(active_tcd=active_tcd)
        self._engines: Dict[tuple, DenoiseEngine] = {}
        self.denoise_streams = None  # None / 1: cond+uncond as one fused batch; 2: two concurrent HIP streams
        self.text_frontend = None
        # any callable picture -> (1024,) CLIP image embedding (ViT-H/14): what ip_adapter={"image": ...} goes through when it is
        # set, as text_frontend is for string prompts; without one the package's own tower encodes the picture (clip_vision below)
        self.image_prompt_encoder = None
        # the CLIP ViT-H/14 vision tower (models.ClipVisionEncoder): set one, or give the path of the `image_encoder/model.safetensors`
        # that ships with the SD 1.5 IP-Adapters and it is built on first use
        self.clip_vision_path = None
        self._clip_vision = None
        self._image_prompt_cache = None   # ((pixel digest, tower, its weights_version), embedding) of the last picture encoded
        # a "plus" adapter's image tokens (image_prompt_tokens): ((pixel digest, tower / adapter / resampler ids and versions), tokens_c)
        # of the last picture, and ((the same ids and versions), tokens_u) of the zero-normalised picture
        self._image_tokens_cache = None
        self._image_tokens_negative = None
        self.bpe_path = None  # local copy of CLIP's bpe_simple_vocab_16e6.txt.gz (or $MSD_BPE_PATH) for string prompts
        self.unconditional_context = None  # (77, 768) embedding of the empty prompt, supplied by the caller
        # False (default, the reference's meaning of batch_size: stable_diffusion.py:384-397 tiles one prompt to the batch THIS
        # process runs): every rank of a process group runs the whole batch on its own (independent replicas).
        # True (opt in; bench.py's jobs call dist.generate_sharded directly): under an initialised torch.distributed process
        # group generate_image() treats batch_size as the GLOBAL batch and shards it over the ranks.
        self.shard_batch = False

    # ---- public entry points (reference :84-139)
    def text_to_image(self, prompt, negative_prompt=None, batch_size=1, num_steps=50, unconditional_guidance_scale=7.5,
                      embedding=None, negative_embedding=None, seed=None, control_net_image=None, guidance_rescale=0.7,
                      callback=None, hires=None, tiled=None, regions=None, pag=None, reference_only=None, hypertile=None, sag=None,
                      dynamic_threshold=None, **kw):
        """``hires``: None, or a hires.HiresSpec / dict for the two-pass hires fix; ``tiled``: None, or a tiled.TiledSpec / dict
        for tiled diffusion on a canvas larger than the pipeline's size; ``regions``: None, or a regions.Regions / dict for
        regional prompting, `prompt` being the base prompt; ``pag``: None, or a pag.PagSpec / dict for perturbed-attention
        guidance; ``reference_only``: None, or a reference.ReferenceSpec / dict for reference-only control; ``hypertile``: None, or a
        hypertile.HypertileSpec / dict for windowed self-attention; ``sag``: None, or a sag.SagSpec / dict for self-attention guidance;
        ``dynamic_threshold``: None, or a dynthresh.DynThreshSpec / dict for dynamic thresholding; ``control`` (through **kw, with
        ``control_net_image``): None, or one control.ControlUnit / dict or a list of them - weight, start / end, mode and further
        ControlNets (see generate_image); ``ip_adapter`` (through **kw): None, or an ipadapter.IPAdapterSpec / dict for an IP-Adapter
        image prompt (see generate_image); ``t2i_adapter`` (through **kw): None, or one t2iadapter.T2IAdapterSpec / dict or a list of
        them for T2I-Adapter structural control (see generate_image)."""
        encoded_text = self.encode_text(prompt, embedding)
        return self.generate_image(encoded_text, negative_prompt=negative_prompt, batch_size=batch_size, num_steps=num_steps,
                                   unconditional_guidance_scale=unconditional_guidance_scale, seed=seed,
                                   negative_embedding=negative_embedding, control_net_image=control_net_image,
                                   guidance_rescale=guidance_rescale, callback=callback, hires=hires, tiled=tiled, regions=regions,
                                   pag=pag, reference_only=reference_only, hypertile=hypertile, sag=sag,
                                   dynamic_threshold=dynamic_threshold, **kw)

    def image_to_image(self, prompt, negative_prompt=None, batch_size=1, num_steps=50, unconditional_guidance_scale=7.5,
                       embedding=None, negative_embedding=None, seed=None, control_net_image=None, reference_image=None,
                       reference_image_strength=0.8, guidance_rescale=0.7, callback=None, **kw):
        """Reference :111-139.  ``control`` (through **kw, with ``control_net_image``): the ControlNet units of generate_image;
        ``ip_adapter`` (through **kw): its IP-Adapter image prompt; ``t2i_adapter`` (through **kw): its T2I-Adapter(s)."""
        encoded_text = self.encode_text(prompt, embedding)
        return self.generate_image(encoded_text, negative_prompt=negative_prompt, batch_size=batch_size, num_steps=num_steps,
                                   unconditional_guidance_scale=unconditional_guidance_scale, seed=seed,
                                   negative_embedding=negative_embedding, control_net_image=control_net_image,
                                   reference_image=reference_image, reference_image_strength=reference_image_strength,
                                   guidance_rescale=guidance_rescale, callback=callback, **kw)

    def inpaint(self, prompt, negative_prompt=None, batch_size=1, num_steps=50, unconditional_guidance_scale=7.5,
                embedding=None, negative_embedding=None, seed=None, control_net_image=None, reference_image=None,
                reference_image_strength=0.8, inpaint_mask=None, mask_blur_strength=None, guidance_rescale=0.7,
                callback=None, **kw):
        """Reference :141-175.  ``control`` (through **kw, with ``control_net_image``): the ControlNet units of generate_image;
        ``ip_adapter`` (through **kw): its IP-Adapter image prompt; ``t2i_adapter`` (through **kw): its T2I-Adapter(s)."""
        encoded_text = self.encode_text(prompt, embedding)
        return self.generate_image(encoded_text, negative_prompt=negative_prompt, batch_size=batch_size, num_steps=num_steps,
                                   unconditional_guidance_scale=unconditional_guidance_scale, seed=seed,
                                   negative_embedding=negative_embedding, control_net_image=control_net_image,
                                   reference_image=reference_image, reference_image_strength=reference_image_strength,
                                   inpaint_mask=inpaint_mask, mask_blur_strength=mask_blur_strength,
                                   guidance_rescale=guidance_rescale, callback=callback, **kw)

    def encode_text(self, prompt, embedding_data=None):
        """Prompt -> context (77k, 768).  Accepted forms:
        * a float array: an already encoded context, returned as is;
        * an integer array of CLIP token ids, (77,) or (k, 77) (start / end / padding tokens included):
          run through the CLIP embedding + text transformer on the device;
          k chunks are concatenated along the token axis like the reference's long prompts;
        * a string: tokenizer + prompt weighting (minsdtf_amd/text.py, reference :176-215) in front of the text
          models; needs a local copy of CLIP's BPE merge list (``bpe_path`` / ``$MSD_BPE_PATH``), or a
          ``text_frontend`` (any object with ``encode(prompt, embedding_data) -> ndarray``)."""
        if isinstance(prompt, torch.Tensor):
            prompt = prompt.detach().cpu().numpy()
        if isinstance(prompt, np.ndarray):
            if np.issubdtype(prompt.dtype, np.integer):
                return self.encode_tokens(prompt)
            return np.asarray(prompt, dtype=np.float32)
        if self.text_frontend is not None:
            return np.asarray(self.text_frontend.encode(prompt, embedding_data), dtype=np.float32)
        # reference :176-215: optional textual-inversion vectors, then tokenizer + prompt weighting + the text models
        from .text import get_weighted_text_embeddings

        embedding, count = None, 0
        if embedding_data is not None and isinstance(embedding_data, str):
            embedding = self.load_embedding(embedding_data)
            if embedding is None:
                raise ValueError(f"failed to load embedding file: {embedding_data}.")
            count = embedding.shape[0]
            embedding = np.expand_dims(embedding, axis=0)
        return get_weighted_text_embeddings(self.tokenizer, self.text_clip_embedding, self.text_encoder, prompt,
                                            model_max_length=MAX_PROMPT_LENGTH, embedding=embedding,
                                            embedding_tokens_count=count, pad_token_id=49407)

    def load_embedding(self, embedding_path):
        """Textual-inversion file -> (n_vectors, 768) array or None (reference :71-82)."""
        if not os.path.exists(str(embedding_path)):
            return None
        state = torch.load(embedding_path, map_location="cpu")
        embedding = None
        for value in (state.get("string_to_param", {}) if isinstance(state, dict) else {}).values():
            if value.dtype in (torch.float32, torch.float16):
                embedding = value.detach().numpy()
        return embedding

    @property
    def tokenizer(self):
        """CLIP BPE tokenizer (reference :533-541).  The merge list is a download in the reference; here it is a
        local file: StableDiffusion.bpe_path or $MSD_BPE_PATH."""
        if self._tokenizer is None:
            path = getattr(self, "bpe_path", None) or os.environ.get("MSD_BPE_PATH")
            if not path or not os.path.exists(path):
                raise NotImplementedError(
                    "string prompts need CLIP's BPE merge list (bpe_simple_vocab_16e6.txt.gz), which cannot be downloaded here: "
                    "set StableDiffusion.bpe_path / $MSD_BPE_PATH, or pass CLIP token ids (int array (77,)), the (77k,768) "
                    "text embedding, or set StableDiffusion.text_frontend")
            from .text import SimpleTokenizer

            self._tokenizer = SimpleTokenizer(path)
        return self._tokenizer

    @tokenizer.setter
    def tokenizer(self, value):
        self._tokenizer = value

    def encode_tokens(self, tokens) -> np.ndarray:
        """CLIP token ids (k, 77) -> context (77k, 768): embedding lookup + text transformer on the device
        (reference stable_diffusion.py:488-493 for the unconditional tokens; long_prompt_weighting.py feeds
        the same two models chunk by chunk)."""
        tokens = np.asarray(tokens, dtype=np.int32).reshape(-1, MAX_PROMPT_LENGTH)
        emb = self.text_clip_embedding.predict_on_batch([tokens, self._get_pos_ids()])
        ctx = self.text_encoder.predict_on_batch(emb)
        return np.asarray(ctx, dtype=np.float32).reshape(-1, ctx.shape[-1])

    @staticmethod
    def _get_pos_ids():
        return np.asarray([list(range(MAX_PROMPT_LENGTH))], dtype=np.int32)

    def _text_models_ready(self) -> bool:
        return False

    def _get_unconditional_context(self):
        if self.unconditional_context is None:
            if self.text_frontend is not None:
                self.unconditional_context = np.asarray(self.text_frontend.encode("", None), dtype=np.float32)
            elif self._text_models_ready():
                # reference :488-493: start token + 76 end tokens through the embedding and the text encoder
                ids = np.asarray([[49406] + [49407] * (MAX_PROMPT_LENGTH - 1)], dtype=np.int32)
                self.unconditional_context = self.encode_tokens(ids)
                self._computed_uncond = self.unconditional_context   # (a text-encoder LoRA switch recomputes it: set_loras)
            else:
                raise NotImplementedError(
                    "the unconditional context is CLIP's embedding of the empty prompt; pass text_encoder_ckpt=, or set "
                    "StableDiffusion.unconditional_context to a (77,768) array, or install text_frontend")
        u = np.asarray(self.unconditional_context, dtype=np.float32)
        return u[None] if u.ndim == 2 else u

    def _expand_tensor(self, text_embedding, batch_size):
        """Reference :495-503: one (T, 768) context -> (B, T, 768); a batch of contexts passes through."""
        return self._batch_of(text_embedding, batch_size, 2)

    _get_timestep_embedding = staticmethod(lambda timestep, batch_size, dim=320, max_period=10000:
                                           get_timestep_embedding(timestep, batch_size, dim, max_period))
    rescale_noise_cfg = staticmethod(rescale_noise_cfg)

    def _get_initial_diffusion_noise(self, batch_size, seed, height=None, width=None):
        """The reference draws keras.random.normal(seed) (backend RNG, :555-557); here the noise is
        numpy's PCG64 standard normal for the GLOBAL batch, so a sharded run slices the same draw.
        height / width: another image size than the pipeline's own (a tiled job's canvas)."""
        rng = np.random.default_rng(seed)
        height, width = self.img_height if height is None else height, self.img_width if width is None else width
        return rng.standard_normal((batch_size, height // 8, width // 8, 4)).astype(np.float32)

    @staticmethod
    def resize(image_array, new_h=None, new_w=None):
        """Bilinear resize with align-corners sampling (reference :242-275)."""
        h, w, _c = image_array.shape
        if new_h == h and new_w == w:
            return image_array
        y = np.expand_dims(np.linspace(0, h - 1, new_h), axis=-1)
        x = np.expand_dims(np.linspace(0, w - 1, new_w), axis=0)
        x0, x1 = np.clip(np.floor(x).astype(int), 0, w - 1), np.clip(np.ceil(x).astype(int), 0, w - 1)
        y0, y1 = np.clip(np.floor(y).astype(int), 0, h - 1), np.clip(np.ceil(y).astype(int), 0, h - 1)
        dx, dy = np.expand_dims(x - x0, -1), np.expand_dims(y - y0, -1)
        top = image_array[y0, x0, :] * (1.0 - dx) + image_array[y0, x1, :] * dx
        bot = image_array[y1, x0, :] * (1.0 - dx) + image_array[y1, x1, :] * dx
        return top * (1.0 - dy) + bot * dy

    @staticmethod
    def gaussian_blur(image, radius=3, h_axis=1, v_axis=2):
        """Separable binomial blur, reflected borders (reference :217-240): the 1-D filter is row
        `radius - 1` of Pascal's triangle, normalised."""
        from math import comb

        from scipy.ndimage import correlate1d

        weights = np.asarray([comb(radius - 1, k) for k in range(radius)], dtype=np.float64)
        weights = weights / np.sum(weights)
        out = correlate1d(image, weights, axis=h_axis, output=None, mode="reflect", cval=0.0, origin=0)
        return correlate1d(out, weights, axis=v_axis, output=None, mode="reflect", cval=0.0, origin=0)

    @staticmethod
    def _pixels(source, pil_mode):
        """A file path (decoded with PIL in `pil_mode`) or anything array-like -> ndarray."""
        if type(source) is str:
            from PIL import Image

            with Image.open(source) as im:
                return np.array(im.convert(pil_mode))
        return np.array(source)

    def preprocessed_mask(self, x, blur_radius=5):
        """Mask (path or HxW[xC] array, 0..255) -> (image-resolution mask (1,H,W,1) in [0,1], latent-resolution mask
        (1,·,·,1)); behaviour of reference :288-302, pinned by goldens G2e / G7: channels are averaged AFTER the bilinear
        resize, the optional binomial blur runs at image resolution, and the latent mask is a second bilinear resize of the
        blurred one to (img_width//8, img_height//8) — rows from the width, as the reference has it (equal for squares)."""
        m = self._pixels(x, "L")
        m = m[..., None] if m.ndim == 2 else m
        m = self.resize(m, self.img_height, self.img_width)
        if m.shape[-1] > 1:
            m = m.mean(axis=-1, keepdims=True)
        unit = np.asarray(m, dtype=np.float32) / 255.0
        if blur_radius is not None:
            unit = self.gaussian_blur(unit, radius=blur_radius, h_axis=0, v_axis=1)
        small = self.resize(unit, self.img_width // 8, self.img_height // 8)
        return unit[None], small[None]

    def preprocessed_image(self, x):
        """Picture (path or HxWx3 array, 0..255) -> ((1,H,W,3) in [0,1] for the pixel blend, the same in [-1,1] for the VAE
        encoder); reference :277-286."""
        px = self.resize(self._pixels(x, "RGB"), self.img_height, self.img_width)
        unit = (np.asarray(px, dtype=np.float32) / 255.0)[None, :, :, :3]
        return unit, unit * 2.0 - 1.0

    # ---- the loop (reference :317-486)
    def _batch_of(self, value, batch_size, sample_ndim):
        """One sample (rank `sample_ndim`, after dropping size-1 axes like the reference's np.squeeze, :395,:498) is
        repeated `batch_size` times; a full batch passes through."""
        value = np.squeeze(value)
        if value.ndim == sample_ndim:
            value = np.repeat(value[None], batch_size, axis=0)
        return value

    def _negative_context(self, negative_prompt, negative_embedding, batch_size):
        """(B, 77k, 768) unconditional half of the guidance pair (reference :384-392)."""
        if negative_prompt is None and negative_embedding is None:
            return np.repeat(self._get_unconditional_context(), batch_size, axis=0)
        if isinstance(negative_prompt, (np.ndarray, torch.Tensor)):
            enc = np.asarray(negative_prompt, dtype=np.float32)
        else:
            enc = self.encode_text(negative_prompt or "", negative_embedding)
        return self._batch_of(enc, batch_size, 2)

    def _hint_batch(self, control_net_image, batch_size):
        """ControlNet conditioning picture -> (B, H, W, 3) in [0,1] (reference :427-437: arrays go through the bilinear
        resize, files through PIL's)."""
        if control_net_image is None:
            return None
        if isinstance(control_net_image, np.ndarray):
            px = self.resize(control_net_image, self.img_height, self.img_width)
        else:
            from PIL import Image

            px = Image.open(control_net_image).convert("RGB").resize((self.img_width, self.img_height))
        unit = np.array(px, dtype=np.float32) / 255.0
        return np.tile(unit[None], (batch_size, 1, 1, 1))

    def generate_image(self, encoded_text, negative_prompt=None, batch_size=1, num_steps=50, unconditional_guidance_scale=7.5,
                       diffusion_noise=None, seed=None, negative_embedding=None, control_net_image=None, inpaint_mask=None,
                       mask_blur_strength=None, reference_image=None, reference_image_strength=0.8, guidance_rescale=0.0,
                       callback=None, host_loop=False, return_latent=False, sampler=None, hires=None, hires_noise=None,
                       tiled=None, regions=None, pag=None, reference_only=None, hypertile=None, sag=None, dynamic_threshold=None,
                       control=None, ip_adapter=None, t2i_adapter=None):
        """Reference :317-486.  ``sampler``: None (the reference's DDIM-style step, or TCD on an active_tcd pipeline) or one of
        "dpmpp_2m", "dpmpp_2m_sde", "euler_a", each optionally with "_karras" (minsdtf_amd/samplers.py; not with active_tcd).
        With ``self.shard_batch = True`` under an initialised torch.distributed process group `batch_size` is the GLOBAL batch: every rank calls this with the same arguments, rank 0's inputs are broadcast, each
        rank denoises + decodes its contiguous slice and every rank returns the whole gathered batch (minsdtf_amd/dist.py).
        Default (False): the reference's meaning, this process runs all `batch_size` samples.
        ``hires`` (a hires.HiresSpec or a dict of its fields; txt2img only): the two-pass hires fix - `num_steps` steps at the
        pipeline's own size, then the latent is resampled to the target size and re-noised on the device (msd_latent_resample)
        and the last int(steps * strength + 0.5) steps of a `steps`-step schedule run at the target size; the result has the
        target size.  ``hires_noise``: the re-noise draw (B, H2/8, W2/8, 4) (default: default_rng([seed, 2]), or numpy's global
        stream without a seed).  `callback` counts through both passes.
        ``tiled`` (a tiled.TiledSpec or a dict of its fields: size = (height, width) of the canvas, stride, blend; txt2img only):
        tiled diffusion (MultiDiffusion) - every step the UNet runs at the pipeline's own size on overlapping views of one canvas
        latent, the views being batch rows of the one engine, and one msd_tile_consensus launch averages the stepped views where
        they overlap.  The result has the canvas size; `seed` draws the start noise - and a stochastic sampler's per-step draws -
        at canvas shape, `diffusion_noise` is taken at canvas shape.  At most tiled.MAX_VIEW_BATCH views (batch_size * views).
        ``regions`` (a regions.Regions or a dict {"regions": [{"prompt", "mask", "weight"}, ...], "base_weight": 0.0}; txt2img only):
        regional prompting - every step the UNet's conditional half runs once per region prompt (further batch rows of the one
        engine) and one msd_region_combine launch sums the predictions per latent pixel with the normalised mask weights in front
        of the guidance / sampler step.  With base_weight > 0 `encoded_text` joins as region 0 with that constant mask; with 0 it is
        not evaluated.  The region contexts share one token length.  At most 2 * tiled.MAX_VIEW_BATCH UNet rows
        ((1 + R) * batch_size).  Works with host_loop=True too.  With the further key "mode": "attention" the masks act inside every
        attn2 instead (one msd_region_attention launch per layer over the R region contexts, the masks reduced to each level by
        regions.Resolved.level_weights): the UNet runs the plain job's rows, so the cap is 2 * batch_size rows against the same
        constant whatever R is; contexts of at most 96 tokens (ValueError naming mode="latent" otherwise).
        ``pag`` (a pag.PagSpec or a dict {"scale": 3.0, "layers": "mid"}; txt2img only): perturbed-attention guidance - every step the
        UNet evaluates the conditional context once more with the self-attention of the selected blocks replaced by the identity map
        (further batch rows of the one engine, msd_attention_identity in those blocks) and eps = u + g (c - u) + s (c - p); one
        msd_region_combine launch writes c' = (1 + k) c - k p over the conditional rows (k = s / g, or s without guidance) in front of
        the guidance / sampler step, so `guidance_rescale` takes its reference std from c'.  ``layers``: "mid" or names of
        engine.PAG_LAYERS.  scale = 0 is the plain job.  Works with every sampler, on a TCD pipeline, with shard_batch and with
        host_loop=True; at most 2 * tiled.MAX_VIEW_BATCH UNet rows (3 * batch_size with guidance, 2 * batch_size without).
        ``reference_only`` (a reference.ReferenceSpec or a dict {"image" or "latent", "fidelity": 0.5, "layers": "all", "noise"}; txt2img
        only): reference-only control - the picture follows the subject / style of a reference image with no extra network.  Every
        step the UNet runs one more row, the reference latent noised to the step's level, and in the selected attention blocks the
        generated rows' self-attention also attends to that row's keys (one msd_attention_joint launch per block); ``fidelity`` is
        the share of the plain self-attention in the unconditional rows (diffusers' style_fidelity).  (`reference_image` is
        image_to_image's start picture, another thing.)  Works with every sampler, with shard_batch and with host_loop=True; at most
        2 * tiled.MAX_VIEW_BATCH UNet rows (2 * batch_size + 1); the negative prompt has the prompt's token length.
        Its field ``adain`` (None, "auto" = weight 1.0, "all", a weight in (0, 2] or site names of reference.ADAIN_SITES) adds reference
        AdaIN (the extension's reference_adain / reference_adain+attn): behind the selected block outputs every generated row's
        feature map is renormalised, channel by channel, to the mean and standard deviation the reference row has there (one
        msd_reference_adain launch per site, in place, the unconditional rows blended by ``fidelity``); with ``adain`` given
        ``layers`` may be [] (AdaIN alone).  Same refusals, row cap and token-length rule; the engine is keyed by both sets.
        ``hypertile`` (a hypertile.HypertileSpec or a dict {"tile": 512, "depth": 0}; txt2img only): HyperTile - the self-attention of
        the attention blocks of the UNet levels 0 .. depth is taken inside non-overlapping windows of `tile` picture pixels (an int
        or (height, width), a multiple of 64 * 2**depth that divides the picture), one msd_attention_windowed launch per block in
        place of msd_attention: with nh x nw windows the attention FLOPs fall by nh * nw.  The tile is fixed, never drawn.  With
        ``hires`` the spec applies to the second pass only, its geometry taken from the target size - the use it is for; one window
        is the plain job.  Works with every sampler, on a TCD pipeline, with shard_batch and with host_loop=True.
        ``sag`` (a sag.SagSpec or a dict {"scale": 0.75, "blur_sigma": 1.0, "threshold": 1.0}, diffusers' defaults; txt2img only):
        self-attention guidance - every step the mid block's self-attention of the unconditional rows also yields the attention
        each key receives (msdx_attention_colsum), the latent is blurred where that map exceeds ``threshold`` (msdx_sag_degrade) and
        the UNet runs a second time on it with the unconditional context; eps = u + g (c - u) + s (u - d).  The second pass
        depends on the first, so the step records the UNet twice, with the two launches in between, inside the one captured loop
        graph; msd_region_combine writes c' = k u + c - k d (k = s / g) in front of the unchanged guidance / sampler step, so
        `guidance_rescale` takes its reference std from c', as with ``pag``.  Without guidance the map comes from the c rows and
        eps = (1 + s) c - s d.  Works with every sampler, on a TCD pipeline, with shard_batch and with host_loop=True; at most
        2 * tiled.MAX_VIEW_BATCH UNet rows (3 * batch_size with guidance, 2 * batch_size without).
        ``dynamic_threshold`` (a dynthresh.DynThreshSpec or a dict {"mimic_scale": 7.0, "percentile": 1.0, "mimic_mode": "constant",
        "cfg_mode": "constant", "mimic_scale_min": 0.0, "cfg_scale_min": 0.0, "sched_val": 1.0, "measure": "ad", "startpoint": "mean",
        "phi": 1.0}; needs guidance > 0): dynamic thresholding, the "CFG scale fix" of the sd-dynamic-thresholding extension - the
        prediction at the (high) guidance scale keeps its direction while each (sample, channel) plane of it is forced back to the
        spread the prediction at ``mimic_scale`` has: one msdt_dynamic_threshold launch behind the regions / PAG / SAG combines
        writes the combined prediction (an exact quantile of every plane, on the device), and the guidance / sampler step takes it
        as it is - so `guidance_rescale` is NOT applied to such a job.  The two scales may move over the steps (``cfg_mode``,
        ``mimic_mode``: dynthresh.MODES); a plane without spread keeps its plain prediction.  Works with every sampler, with
        ``hires`` (both passes, each schedule over its own executed steps), ``regions``, ``pag``, ``sag``, ``hypertile``,
        ``reference_only``, shard_batch and host_loop=True; the engine is keyed by the fact only.
        ``control`` (with ``control_net_image``; one control.ControlUnit or dict {"weight": 1.0, "start": 0.0, "end": 1.0, "mode":
        "balanced"}, or a list of 1 .. control.MAX_UNITS of them): ControlNet units.  Unit 0 is the pipeline's own ControlNet on
        ``control_net_image``; every further unit carries its own ``image`` and ``path`` (another ControlNet checkpoint, loaded once
        and kept on the pipeline; None: the pipeline's own, on this picture) or ``models`` = (ControlNet, HintNet).  ``weight`` (one
        float >= 0 or 13, one per residual) scales the unit's residuals, ``start`` / ``end`` bound the share of the steps it acts on
        (diffusers' rule), ``mode`` is "balanced", "prompt" (soft injection: residual k times 0.825 ** (12 - k)) or "control" (that,
        on the conditional half only).  Every unit's 13 zero convs write fp32 and ONE msdc_control_combine launch per UNet pass adds
        them to the skips, the scales read from a per-step device table - so weights, ranges and modes are per-call uploads and the
        engine is keyed by the number of units alone.  Works with whatever a ControlNet job works with: every sampler, a TCD pipeline,
        image_to_image, inpainting, denoise_streams = 2, a negative prompt of another length, shard_batch and host_loop=True.
        ``control`` = None is the job as it was, bit for bit.
        ``ip_adapter`` (an ipadapter.IPAdapterSpec or a dict {"embeds": (1024,) CLIP image embedding | "tokens": (N, 768) image tokens |
        "image": a picture, "weight": 1.0, "start": 0.0, "end": 1.0, "weight_type": "linear" | "style" | "composition" | {attention
        block: factor}, "path": an IP-Adapter checkpoint | "model": a models.IPAdapter}): an IP-Adapter image prompt.  Every
        cross-attention of the UNet also attends to the N image tokens through the adapter's own to_k_ip / to_v_ip, decoupled from the
        text attention: out = softmax(q K_text^T) V_text + s softmax(q K_ip^T) V_ip as ONE msdi_attention_decoupled launch per block,
        s read from a per-step device table (``weight`` inside [``start``, ``end``) by diffusers' rule, times the block factors of
        ``weight_type``: "style" is up_blocks.1 only, "composition" down_blocks.2.attentions.1 only).  The tokens are the adapter's
        projection of the embedding, made on the host once per call; the unconditional rows take the zero embedding's tokens.
        ``image`` goes through ``self.image_prompt_encoder`` (any callable picture -> (1024,) embedding) when one is set, else through
        the package's CLIP ViT-H/14 tower (``self.clip_vision`` / ``clip_vision_path=``); ``tokens`` bypasses the projection
        (the entry for "plus" adapters without a picture).  A "plus" checkpoint (``ip-adapter-plus_sd15``, 16 tokens: its
        ``image_proj`` is a Resampler, recognised by ``image_proj.latents``) takes ``image`` too: the tokens are the adapter's
        ``resampler`` (models.IPResampler) on the tower's penultimate hidden states, the unconditional rows take the resampler's tokens
        of the zero-normalised picture (``self.image_prompt_tokens``; both are kept, a repeated job runs neither network); it needs
        the package's own tower - a callable returns the pooled embedding, which it cannot use - and refuses ``embeds``.
        Tokens and table are per-call uploads, so the engine is keyed by N and the adapter alone and one engine serves every picture, weight and schedule.  Works with every sampler, a TCD pipeline, ``control_net_image`` with or
        without ``control`` (the ControlNet's own encoder stays plain), image_to_image, inpainting, ``dynamic_threshold``,
        shard_batch and host_loop=True; not with regions, pag, sag, reference_only, hypertile, tiled, hires or denoise_streams = 2,
        nor with prompts of more than 77 tokens.  One adapter and one picture per job.  A spec whose table is all 0 (weight 0) is the
        plain job on the plain engine; ``ip_adapter`` = None is the job as it was, bit for bit.
        ``t2i_adapter`` (a t2iadapter.T2IAdapterSpec or a dict {"image": the conditioning picture, "path": a T2I-Adapter checkpoint |
        "model": a models.T2IAdapter, "weight": 1.0 or four per-site weights, "start": 0.0, "end": 1.0}, or a list of 1 ..
        t2iadapter.MAX_UNITS of them): T2I-Adapter structural control (depth, sketch, pose, ...).  The adapter's conv net runs once per
        job on the picture alone (31 launches; the last picture's features are kept, a repeated job runs nothing) and every UNet pass
        adds its four feature maps, in place, behind down_blocks.{0,1,2}.attentions.1 and down_blocks.3.resnets.1 - before the skip
        and the downsampler read them - the same feature to every row: ONE msda_feature_add launch per site, its scale ``weight[site]``
        inside [``start``, ``end``) by diffusers' rule, read from a per-step device table; several adapters add.  Features and table
        are per-call uploads, so the engine is keyed by the number of units alone.  The picture (an array 0 .. 255 or a file; (H, W, 3),
        or (H, W) / (H, W, 1) for a 1-channel adapter) is resized to the job's size, whose height and width are multiples of 64.
        Works with every sampler, a TCD pipeline, image_to_image, inpainting, ``ip_adapter``, ``dynamic_threshold``, shard_batch and
        host_loop=True; not with control_net_image, regions, pag, sag, reference_only, hypertile, tiled, hires or denoise_streams = 2.
        A description whose table is all 0 (weight 0) is the plain job on the plain engine; ``t2i_adapter`` = None is the job as it
        was, bit for bit."""
        t2i = t2i_mod.parse(t2i_adapter)   # (ValueError for a bad description)
        t2i_tab = None
        if t2i is not None:
            t2i_mod.refuse(dict(control_net_image=control_net_image, regions=regions, pag=pag, sag=sag, reference_only=reference_only,
                                hypertile=hypertile, tiled=tiled, hires=hires), self.denoise_streams)
            t2i_mod.check_size(self.img_height, self.img_width)
            t2i_tab = t2i_mod.table(t2i, num_steps)
            if not t2i_tab.any():
                t2i = t2i_tab = None   # (every scale 0: the plain job, on the plain engine)
        ipa = ipadapter_mod.parse(ip_adapter)   # (ValueError for a bad description)
        ipa_tab = None
        if ipa is not None:
            ipadapter_mod.refuse(dict(regions=regions, pag=pag, sag=sag, reference_only=reference_only, hypertile=hypertile, tiled=tiled,
                                      hires=hires), self.denoise_streams)
            ipa_tab = ipadapter_mod.table(ipa, num_steps)
            if not ipa_tab.any():
                ipa = ipa_tab = None   # (every scale 0: the plain job, on the plain engine)
        cu = control_mod.parse(control)   # (ValueError for a bad description)
        if cu is not None and control_net_image is None:
            raise ValueError("control: the units scale the ControlNet of `control_net_image`, which is missing")
        given = dict(tiled=tiled, hires=hires, control_net_image=control_net_image, reference_image=reference_image,
                     inpaint_mask=inpaint_mask, regions=regions, pag=pag, reference_only=reference_only, hypertile=hypertile)
        dt = dynthresh_mod.parse(dynamic_threshold)   # (ValueError for a bad description)
        if dt is not None:
            self._refuse_combinations("dynamic_threshold", given, host_loop)
            if not float(unconditional_guidance_scale) > 0.0:
                raise ValueError(f"dynamic_threshold: unconditional_guidance_scale = {unconditional_guidance_scale!r} - without guidance "
                                 "there is nothing to threshold")
        sg = sag_mod.parse(sag)   # (ValueError for a bad description)
        if sg is not None:
            self._refuse_combinations("sag", given, host_loop)
            self._cap_rows("sag", batch_size, (3 if float(unconditional_guidance_scale) > 0.0 else 2) * int(batch_size))
        ht = hypertile_mod.parse(hypertile)   # (ValueError for a bad description)
        if ht is not None:
            self._refuse_combinations("hypertile", given, host_loop)
        ref = reference_mod.parse(reference_only)   # (ValueError for a bad description)
        if ref is not None:
            self._refuse_combinations("reference_only", given, host_loop)
            self._cap_rows("reference_only", batch_size, 2 * int(batch_size) + 1)
        pg = pag_mod.parse(pag)   # (ValueError for a bad description)
        if pg is not None and pg.scale == 0.0:
            pg = None   # (c' = c: the plain job, on the plain engine)
        if pg is not None:
            self._refuse_combinations("pag", given, host_loop)
            self._cap_rows("pag", batch_size, (3 if float(unconditional_guidance_scale) > 0.0 else 2) * int(batch_size))
        reg = regions_mod.parse(regions, self.img_height, self.img_width)   # (ValueError for a bad description)
        if reg is not None:
            self._refuse_combinations("regions", given, host_loop)
            if reg.mode == "attention":   # the UNet runs the plain job's rows whatever the number of regions
                self._cap_rows("regions", batch_size, 2 * int(batch_size), ' in mode="attention"')
            else:
                self._cap_rows("regions", batch_size, (1 + reg.count) * int(batch_size), f" of 1 + {reg.count} prompts",
                               "use fewer regions or a smaller batch")
        geo = tiled_mod.parse(tiled, self.img_height, self.img_width)   # (ValueError for a bad description)
        if geo is not None:
            self._refuse_combinations("tiled", given, host_loop)
            if int(batch_size) * geo.views > tiled_mod.MAX_VIEW_BATCH:
                raise ValueError(f"tiled: {batch_size} image(s) of {geo.rows} x {geo.cols} views are {int(batch_size) * geo.views} UNet rows "
                                 f"per step, more than tiled.MAX_VIEW_BATCH = {tiled_mod.MAX_VIEW_BATCH}: use a larger stride, a smaller "
                                 "canvas or a smaller batch")
        job = hires_mod.parse(hires, self.img_height, self.img_width, num_steps)   # (ValueError for a bad description)
        if job is None and hires_noise is not None:
            raise ValueError("`hires_noise` without `hires`")
        if job is not None:
            self._refuse_combinations("hires", given, host_loop)
        ht_key = None
        if ht is not None:   # (nh, nw, depth) on the picture the windowed pass produces; one window: the plain job, on the plain engine
            size = (job.height, job.width) if job is not None else (self.img_height, self.img_width)
            ht_key = ht.key(*size)   # (ValueError naming the nearest valid tiles)
            hypertile_mod.level_geometry(size[0] // 8, size[1] // 8, *ht_key)
            if ht_key[:2] == (1, 1):
                ht_key = None
        if diffusion_noise is not None and seed is not None:
            raise ValueError("`diffusion_noise` and `seed` should not both be passed to `generate_image`. `seed` is only "
                             "used to generate diffusion noise when it's not already user-specified.")
        spec = smp.parse(sampler)   # (ValueError for an unknown name)
        if spec is not None and self.active_tcd:
            raise ValueError(f"sampler={sampler!r} on a TCD pipeline (active_tcd=True): the TCD sampler is the only one it runs")
        # what the job's engines are built with, built here once.  A tiled or hires job takes all of it too: every option but the sampler,
        # dynthresh and (hires, second pass only) the windows is refused with those two - its REFUSED row names `tiled` / `hires`
        engine_opts = job_options(sampler=spec, regions=reg, pag=pg, reference=ref, hypertile=ht_key, sag=sg, dynthresh=dt, control=cu)
        B = batch_size
        context = self._batch_of(encoded_text, B, 2)
        unconditional_context = self._negative_context(negative_prompt, negative_embedding, B)
        ipa_model = ipa_tok = None
        if ipa is not None:   # the adapter, its tokens of the picture and of the zero embedding: (N, 768) each
            ipa_model, ipa_tok = self._ip_inputs(ipa)
            for t in (context.shape[1], unconditional_context.shape[1]) if float(unconditional_guidance_scale) > 0.0 else (context.shape[1],):
                ipadapter_mod.check_context(t, ipa_model.tokens)
            engine_opts = dict(engine_opts, ip_tokens=ipa_model.tokens, ip_adapter=ipa_model)   # (a model object beside the options)
        t2i_feats = None
        if t2i is not None:   # per unit the four bf16 features of its picture, on the device (every rank of a sharded job makes its own)
            t2i_feats = self._t2i_inputs(t2i)
            engine_opts = dict(engine_opts, t2i_units=len(t2i))
        if geo is not None:
            noise = (self._get_initial_diffusion_noise(B, seed, geo.height, geo.width) if diffusion_noise is None
                     else self._batch_of(diffusion_noise, B, 3))
            if tuple(noise.shape) != (B, geo.H, geo.W, 4):
                raise ValueError(f"tiled: diffusion_noise has shape {tuple(noise.shape)}, the {geo.height}x{geo.width} canvas latent of "
                                 f"batch {B} is {(B, geo.H, geo.W, 4)}")
            return self._generate_tiled(geo, spec, context, unconditional_context, noise, num_steps, float(unconditional_guidance_scale),
                                        float(guidance_rescale), seed, callback, return_latent, engine_opts)
        noise = self._get_initial_diffusion_noise(B, seed) if diffusion_noise is None else self._batch_of(diffusion_noise, B, 3)
        if job is not None:
            return self._generate_hires(job, spec, context, unconditional_context, noise, hires_noise, num_steps,
                                        float(unconditional_guidance_scale), float(guidance_rescale), seed, callback, return_latent,
                                        ({k: v for k, v in engine_opts.items() if k != "hypertile"}, engine_opts), dt)
        self.scheduler.set_timesteps(num_steps)

        # image_to_image (reference :410-418,559-568): encode the picture, run only the last int(n*strength+0.5) steps,
        # starting from signal[t]*z0 + noise[t]*eps; a strength outside (0,1) silently means txt2img, like the reference.
        # inpainting (:406-409,469-475,484-485) needs both mask and picture: every step the latent outside the mask is
        # replaced by the encoded picture re-noised for that step, and the decoded pixels are blended once more.
        ascending = self.scheduler.timesteps[::-1]
        run_steps = num_steps
        pixel_mask = latent_mask = picture01 = encoded = None
        start_latent = noise
        if inpaint_mask is not None:
            pixel_mask, latent_mask = self.preprocessed_mask(inpaint_mask, mask_blur_strength)
        if reference_image is not None and 0.0 < reference_image_strength < 1.0:
            picture01, picture11 = self.preprocessed_image(reference_image)
            run_steps = int(num_steps * reference_image_strength + 0.5)
            t_entry = ascending[run_steps]
            ascending = ascending[:run_steps]
            encoded = self.image_encoder.predict_on_batch(picture11)
            start_latent = (self.scheduler.signal_rates[t_entry] * np.repeat(encoded, B, axis=0)
                            + self.scheduler.noise_rates[t_entry] * noise)
        inpainting = latent_mask is not None and encoded is not None
        blend_pixels = pixel_mask is not None and picture01 is not None
        start_index = num_steps - run_steps  # position of the first executed timestep in the descending schedule
        sched, sampler_z = self._sampler_inputs(spec, B, num_steps, noise.shape[1], noise.shape[2], seed)
        if sched is not None and encoded is not None:   # (k-diffusion's entry point: the first executed evaluation's own alpha / sigma)
            start_latent = sched.entry_latent(start_index, encoded, noise)
        hint = self._hint_batch(control_net_image, B)
        g, phi = float(unconditional_guidance_scale), float(guidance_rescale)
        cu_tab = cu_nets = cu_hints = None
        if cu is not None:   # the table over the whole schedule (its rows are the step counter's), the further units' models and hints
            cu_tab = control_mod.table(cu, num_steps)
            cu_nets = [self._control_models(u) for u in cu[1:]]
            cu_hints = [self._hint_batch(u.image, B) for u in cu[1:]]
            if cu_nets:   # (model objects, not options: in front of the options on the way to the engine)
                engine_opts = dict(engine_opts, control_nets=tuple(cu_nets))
        ref_in = None
        if ref is not None:
            if g > 0.0 and unconditional_context.shape[1] != context.shape[1]:
                raise ValueError("reference_only: the negative prompt must have the conditional context's token length "
                                 f"({unconditional_context.shape[1]} != {context.shape[1]} tokens)")
            ref_in = self._reference_inputs(ref, noise.shape[1], noise.shape[2], seed)   # (z_ref, n_ref), each (1, h, w, 4)
        region_ctx = region_w = None
        if reg is not None:
            region_ctx, region_w = self._region_inputs(reg, context)   # (R', T, 768) without the base prompt, (R, h, w)
            if reg.mode == "attention":
                if region_ctx.shape[1] > 96:
                    raise ValueError(f'regions: mode="attention" takes contexts of at most 96 tokens, got {region_ctx.shape[1]}: use '
                                     'mode="latent"')
                region_w = reg.level_weights(engine.unet_levels(noise.shape[1], noise.shape[2]))
                region_w = region_w if host_loop else regions_mod.pack_levels(region_w)
            if host_loop:   # the conditional context becomes the list of region contexts, each (B, T, 768)
                context = ([context] if reg.base_weight > 0.0 else []) + [np.repeat(rc[None], B, axis=0) for rc in region_ctx]

        def finish(decoded, picture=picture01, mask=pixel_mask):
            """Decoder output in [-1,1] -> uint8, truncating (reference :482-486), through the pixel-space inpaint blend."""
            decoded = np.array(((decoded + 1.0) * 0.5), dtype=np.float32)
            if blend_pixels:
                decoded = picture * (1.0 - mask) + decoded * mask
            return np.clip(decoded * 255.0, 0, 255).astype("uint8")

        if host_loop:
            ip = (encoded, noise, latent_mask[0]) if inpainting else None
            if spec is not None:
                latent = self._host_loop_sampler(context, unconditional_context, start_latent, g, phi, hint, callback, sched, start_index,
                                                 sampler_z, ip, region_w=region_w, pag=pg, hypertile=ht_key, sag=sg, dynthresh=dt,
                                                 control=None if cu is None else (cu_tab, cu_nets, cu_hints),
                                                 ip=None if ipa is None else (ipa_model, ipa_tok, ipa_tab),
                                                 t2i=None if t2i is None else (t2i_feats, t2i_tab),
                                                 reference=None if ref is None else (ref, ref_in, reference_mod.rates(sched, start_index)))
            else:
                latent = self._host_loop(context, unconditional_context, start_latent, g, phi, hint, callback, ascending, ip,
                                         region_w=region_w, pag=pg, hypertile=ht_key, sag=sg, dynthresh=dt,
                                         control=None if cu is None else (cu_tab, cu_nets, cu_hints, start_index),
                                         ip=None if ipa is None else (ipa_model, ipa_tok, ipa_tab, start_index),
                                         t2i=None if t2i is None else (t2i_feats, t2i_tab, start_index),
                                         reference=None if ref is None else (ref, ref_in, reference_mod.rates(self.scheduler, start_index)))
            if return_latent:
                return np.asarray(latent, dtype=np.float32)
            return finish(self.image_decoder.predict_on_batch(latent))

        # ---- device loop, sharded over the process group when there is one --------------------------------
        world = self._world()
        per_sample, shared = {}, {}   # name -> array; insertion order = order in the packed broadcast
        if hint is not None:
            per_sample["hint"] = hint
        if inpainting:
            per_sample["noise"] = noise
            shared["encoded"], shared["mask"] = encoded, latent_mask[0]
        if blend_pixels and world > 1:   # rank 0's picture and mask are the ones every slice is blended with
            shared["picture"], shared["pixel_mask"] = picture01, pixel_mask
        if self.active_tcd and world > 1:
            # the TCD draws, made here for the GLOBAL batch so that a sample's draws do not depend on the number of ranks
            per_sample["tcd"] = tcd_step_noise(B, num_steps, noise.shape[1], noise.shape[2], start_index)
        if sampler_z is not None:
            per_sample["sampler_z"] = sampler_z.reshape(B, num_steps, -1)
        if reg is not None:   # one context per region and the weights: whole on every rank
            shared["region_ctx"], shared["region_w"] = region_ctx, region_w
        if ref is not None:   # the reference latent and its draw: whole on every rank, every rank runs its own reference row
            shared["ref_z"], shared["ref_noise"] = ref_in
        if cu is not None:   # the further units' hints per sample, the table whole on every rank (like region_w)
            for n, hi in enumerate(cu_hints):
                per_sample[f"control_hint{n + 1}"] = hi
            shared["control_table"] = cu_tab
        if ipa is not None:   # the two token sets and the table: whole on every rank
            shared["ip_tokens"], shared["ip_table"] = np.stack(ipa_tok, axis=0), ipa_tab
        if t2i is not None:   # the table: whole on every rank (the features are this rank's own, of the same picture)
            shared["t2i_table"] = t2i_tab

        def local(c, u, z, a):
            """This rank's slice of the batch: one denoise pass -> decode; returns a device tensor."""
            b = int(z.shape[0])
            if reg is not None:   # the region contexts, each repeated over this rank's samples; the base prompt's rows first
                rc = a["region_ctx"]
                rep = (lambda x: x.unsqueeze(0).expand(b, -1, -1)) if isinstance(rc, torch.Tensor) else (lambda x: np.repeat(x[None], b, axis=0))
                c = ([c] if reg.base_weight > 0.0 else []) + [rep(rc[i]) for i in range(rc.shape[0])]
            eng = self._denoise_pass(u, c, z, num_steps, g, phi, start_index, run_steps, callback, engine_opts,
                                     dict(hint_image=a.get("hint"), inpaint=(a["encoded"], a["noise"], a["mask"]) if inpainting else None,
                                          step_noise=a.get("tcd") if spec is None else a.get("sampler_z"), sampler=sched,
                                          regions=a.get("region_w"), pag_scale=None if pg is None else pg.scale,
                                          reference=None if ref is None else (a["ref_z"], a["ref_noise"], ref.fidelity), sag=sg,
                                          dynamic_threshold=dt,
                                          control=None if cu is None else (a["control_table"], [a[f"control_hint{n + 1}"] for n in range(len(cu) - 1)]),
                                          ip_adapter=None if ipa is None else (a["ip_tokens"][0], a["ip_tokens"][1], a["ip_table"]),
                                          t2i_adapter=None if t2i is None else (t2i_feats, a["t2i_table"])))
            if return_latent:
                return eng.latent
            if blend_pixels:   # pixel blend in fp32 before the uint8 cast
                host = [np.asarray(a[k].cpu()) for k in ("picture", "pixel_mask")] if "picture" in a else []
                return torch.from_numpy(finish(self.image_decoder.predict_on_batch(eng.latent), *host)).to(eng.latent.device)
            return self.image_decoder.decode_to_uint8(eng.latent)

        return self._run_sharded(local, context, unconditional_context, start_latent, per_sample, shared)

    _REFUSED = REFUSED   # (jobopts.py: the one table generate_image and the engines refuse from)

    def _refuse_combinations(self, kind, given: dict, host_loop) -> None:
        """ValueError naming every argument of `given` that is set and every state that holds which job `kind` cannot take."""
        what, arguments, states = self._REFUSED[kind]
        holds = {"host_loop=True": host_loop, "a TCD pipeline (active_tcd=True)": self.active_tcd,
                 "denoise_streams = 2": self.denoise_streams == 2}
        refused = [n for n in arguments if given[n] is not None] + [s for s in states if holds[s]]
        if refused:
            raise ValueError(f"{kind} is {what}: it cannot be combined with {', '.join(refused)}")

    @staticmethod
    def _cap_rows(kind, batch_size, rows, how="", advice="use a smaller batch") -> None:
        """ValueError when a job of `kind` would run more UNet rows per step than 2 * tiled.MAX_VIEW_BATCH."""
        if rows > 2 * tiled_mod.MAX_VIEW_BATCH:
            raise ValueError(f"{kind}: {batch_size} image(s){how} are {rows} UNet rows per step, more than 2 * tiled.MAX_VIEW_BATCH = "
                             f"{2 * tiled_mod.MAX_VIEW_BATCH}: {advice}")

    def _control_models(self, unit):
        """The (ControlNet, HintNet) of a control unit behind the first: its own `models`, the pipeline's own ControlNet (path None),
        or the models of the checkpoint `path`, loaded once and kept on the pipeline by path."""
        if unit.models is not None:
            return tuple(unit.models)
        if unit.path is None or unit.path == getattr(self, "controlnet_path", None):
            return (self.control_net, self.hint_net)
        cache = self.__dict__.setdefault("_control_models_by_path", {})
        if unit.path not in cache:
            dev = getattr(self, "device", None)
            cache[unit.path] = (ControlNet(self.img_height, self.img_width, controlnet_path=unit.path, device=dev),
                                HintNet(self.img_height, self.img_width, controlnet_path=unit.path, device=dev))
            if self.jit_compile:
                for m in cache[unit.path]:
                    m.compile(jit_compile=True)
        return cache[unit.path]

    @property
    def clip_vision(self):
        """The CLIP ViT-H/14 vision tower of image prompts (models.ClipVisionEncoder), or None: the one that was set, or the checkpoint
        `clip_vision_path` loaded on first use."""
        if self._clip_vision is None and self.clip_vision_path is not None:
            from .models import ClipVisionEncoder

            tower = ClipVisionEncoder(path=self.clip_vision_path, device=getattr(self, "device", None))
            if self.jit_compile:
                tower.compile(jit_compile=True)
            self._clip_vision = tower
        return self._clip_vision

    @clip_vision.setter
    def clip_vision(self, tower):
        self._clip_vision = tower

    def encode_image_prompt(self, picture) -> np.ndarray:
        """A picture (anything vision.preprocess takes: uint8 / float HxWx3 on the 0 .. 255 scale, or a path) -> its (1024,) float64 CLIP
        image embedding through `clip_vision`: what ip_adapter={"embeds": ...} takes.  The last picture's embedding is kept, keyed
        by a digest of the preprocessed pixels and the tower's weights_version: encoding it again does not run the tower."""
        from . import vision

        tower = self.clip_vision
        if tower is None:
            raise ValueError("encode_image_prompt: no vision tower: set StableDiffusion.clip_vision (a models.ClipVisionEncoder) or pass "
                             "clip_vision_path= (the IP-Adapter's image_encoder/model.safetensors)")
        px = vision.preprocess(picture)
        key = (vision.digest(px), id(tower), tower.weights_version)
        if self._image_prompt_cache is None or self._image_prompt_cache[0] != key:
            embeds = np.asarray(tower.predict_on_batch(px[None]), dtype=np.float64).reshape(-1)
            if embeds.shape != (ipadapter_mod.EMBED_DIM,) or not np.isfinite(embeds).all():
                raise ValueError(f"clip_vision returned shape {embeds.shape}, expected a finite ({ipadapter_mod.EMBED_DIM},)")
            self._image_prompt_cache = (key, embeds)
        return self._image_prompt_cache[1].copy()

    def image_prompt_tokens(self, picture, adapter):
        """A picture (anything vision.preprocess takes) -> (tokens_u, tokens_c), each (N, 768) float32: the image tokens of a "plus"
        `adapter` (a models.IPAdapter with a `resampler`).  tokens_c = the resampler on the tower's `penultimate` hidden states of
        preprocess(picture); tokens_u = the same route on the picture whose NORMALISED pixels are zero (IP-Adapter's
        IPAdapterPlus.get_image_embeds; built from vision.pixel_affine, zero to fp32 rounding) - not the zero embedding's projection.
        tokens_c is kept for the last picture, keyed by the pixel digest, the tower's id and weights_version and the adapter's and
        resampler's weights_version; tokens_u per (tower, adapter, resampler) versions: a repeated job runs neither network, a new
        picture runs each once."""
        from . import vision

        rs = getattr(adapter, "resampler", None)
        if rs is None:
            raise ValueError("image_prompt_tokens: the adapter has no resampler (a base adapter projects the pooled embedding: "
                             "encode_image_prompt and IPAdapter.project)")
        tower = self.clip_vision
        if tower is None:
            raise ValueError("ip_adapter: `image` with a \"plus\" adapter needs the pipeline's own vision tower, whose hidden states its "
                             "resampler reads: set StableDiffusion.clip_vision (a models.ClipVisionEncoder) or pass clip_vision_path= (an "
                             "image_prompt_encoder callable returns the pooled embedding, which a plus adapter cannot use), or pass `tokens`")

        def run(px):
            hidden = np.asarray(tower.predict_on_batch(px[None], output="penultimate"), dtype=np.float32)
            tok = np.asarray(rs.predict_on_batch(hidden), dtype=np.float32)
            if tok.shape != (1, adapter.tokens, ipadapter_mod.CONTEXT_DIM) or not np.isfinite(tok).all():
                raise ValueError(f"ip_resampler returned shape {tok.shape}, expected a finite {(1, adapter.tokens, ipadapter_mod.CONTEXT_DIM)}")
            return np.ascontiguousarray(tok[0])

        versions = (id(tower), tower.weights_version, id(adapter), adapter.weights_version, id(rs), rs.weights_version)
        px = vision.preprocess(picture)
        key = (vision.digest(px),) + versions
        if self._image_tokens_cache is None or self._image_tokens_cache[0] != key:
            self._image_tokens_cache = (key, run(px))
        if self._image_tokens_negative is None or self._image_tokens_negative[0] != versions:
            self._image_tokens_negative = (versions, run(vision.zero_normalised_pixels()))
        return self._image_tokens_negative[1].copy(), self._image_tokens_cache[1].copy()

    def _ip_inputs(self, ipa):
        """(the models.IPAdapter of an image-prompt job, (tokens_u, tokens_c)): its own `model`, or the checkpoint `path` loaded once
        and kept on the pipeline by path; the (N, 768) fp32 tokens of the unconditional rows (the zero embedding's, or
        `negative_tokens` / zeros beside `tokens`) and of the conditional rows (the picture's).  A "plus" adapter (one with a
        `resampler`) takes `image` through image_prompt_tokens, or `tokens`."""
        model = ipa.model
        if model is None:
            if ipa.path is None:
                raise ValueError("ip_adapter: one of `path` (an IP-Adapter checkpoint) and `model` (a models.IPAdapter) is needed")
            from .models import IPAdapter

            cache = self.__dict__.setdefault("_ip_adapters_by_path", {})
            if ipa.path not in cache:
                cache[ipa.path] = IPAdapter(path=ipa.path, device=getattr(self, "device", None))
                if self.jit_compile and cache[ipa.path].resampler is not None:
                    cache[ipa.path].resampler.compile(jit_compile=True)
            model = cache[ipa.path]
        model._require_weights()
        if ipa.tokens is not None:
            if ipa.tokens.shape[0] != model.tokens:
                raise ValueError(f"ip_adapter: {ipa.tokens.shape[0]} `tokens`, the adapter takes {model.tokens}")
            neg = np.zeros_like(ipa.tokens) if ipa.negative_tokens is None else ipa.negative_tokens
            return model, (np.asarray(neg, dtype=np.float32), np.asarray(ipa.tokens, dtype=np.float32))
        if getattr(model, "resampler", None) is not None:   # a "plus" adapter: the resampler over the tower's hidden states
            if ipa.embeds is not None:
                raise ValueError("ip_adapter: `embeds` with a \"plus\" adapter: its resampler reads the vision tower's hidden states, not the "
                                 "pooled embedding: pass `image` (the picture) or `tokens` (the resampler's output) instead")
            return model, self.image_prompt_tokens(ipa.image, model)
        embeds = ipa.embeds
        if embeds is None and self.image_prompt_encoder is not None:   # (a callable that was set wins over the package's tower)
            embeds = np.asarray(self.image_prompt_encoder(ipa.image), dtype=np.float64).reshape(-1)
            if embeds.shape != (ipadapter_mod.EMBED_DIM,) or not np.isfinite(embeds).all():
                raise ValueError(f"ip_adapter: image_prompt_encoder returned shape {embeds.shape}, expected a finite ({ipadapter_mod.EMBED_DIM},)")
        elif embeds is None:
            if self.clip_vision is None:
                raise ValueError("ip_adapter: `image` needs StableDiffusion.image_prompt_encoder (a callable picture -> (1024,) CLIP image "
                                 "embedding), which is not set: pass `embeds` (the embedding) or `tokens` (the image tokens) instead, or give "
                                 "the pipeline its own tower (StableDiffusion.clip_vision / clip_vision_path=)")
            if model.tokens > 4:
                raise ValueError(f"ip_adapter: `image` with a \"plus\" adapter ({model.tokens} image tokens): its resampler over the tower's hidden "
                                 "states is not part of the package: pass tokens= (the resampler's output) instead")
            embeds = self.encode_image_prompt(ipa.image)
        return model, (model.project(np.zeros(ipadapter_mod.EMBED_DIM)), model.project(embeds))

    def _reference_inputs(self, ref, h, w, seed):
        """(z_ref, n_ref) of a reference-only job, each (1, h, w, 4) float32: the given latent, or the picture through the VAE
        encoder; the given draw, or reference.draw_noise (default_rng([seed, 3]), numpy's global stream without a seed)."""
        if ref.latent is not None:
            z = ref.latent
        else:
            _p01, picture11 = self.preprocessed_image(ref.image)
            z = np.asarray(self.image_encoder.predict_on_batch(picture11), dtype=np.float32)
        if tuple(z.shape) != (1, h, w, 4):
            raise ValueError(f"reference_only: the reference latent has shape {tuple(z.shape)}, this job's is {(1, h, w, 4)}")
        n = ref.noise if ref.noise is not None else reference_mod.draw_noise(h, w, seed)
        if tuple(n.shape) != (1, h, w, 4):
            raise ValueError(f"reference_only: noise has shape {tuple(n.shape)}, this job's reference latent is {(1, h, w, 4)}")
        return np.ascontiguousarray(z, dtype=np.float32), np.ascontiguousarray(n, dtype=np.float32)

    def _sampler_inputs(self, spec, B, steps, h, w, seed, stream_key=1):
        """(the sampler's Schedule over `steps`, a stochastic sampler's per-step draws of the GLOBAL batch (B, steps, h, w, 4),
        sample-major, else None); (None, None) without a sampler."""
        if spec is None:
            return None, None
        sched = smp.schedule(spec, self.scheduler, steps)
        return sched, smp.draw_step_noise(B, steps, h, w, seed, stream_key=stream_key) if spec.stochastic else None

    def _world(self) -> int:
        """Ranks this job's batch is sharded over."""
        from . import dist as mdist

        return mdist.world_size() if getattr(self, "shard_batch", False) else 1

    def _run_sharded(self, local, context, unconditional_context, noise, per_sample: dict, shared: dict):
        """The tail of every device-loop job: `local(context, unconditional_context, noise, extras)` runs on this rank's slice of
        the batch - `extras` holding the slices of `per_sample` (name -> array of the GLOBAL batch) and `shared` (name -> array
        every rank needs whole) by name - and returns a device tensor; the gathered result comes back as a host array."""
        from . import dist as mdist

        dev = getattr(self, "device", None) or self.diffusion_model.device
        names = list(per_sample) + list(shared)
        # (a one-rank group with FORCE_COLLECTIVES still takes the real exchanges: tests/test_rccl_gpu.py)
        sharded = self._world() > 1 or (getattr(self, "shard_batch", False) and mdist.collectives_on())
        out = mdist.generate_sharded(lambda c, u, z, *rest: local(c, u, z, dict(zip(names, rest))), context, unconditional_context,
                                     noise, dev, per_sample=list(per_sample.values()), shared=list(shared.values()), shard=sharded)
        return self._to_host(out, dev, sharded)

    def _denoise_pass(self, u, c, start, steps, g, phi, first, count, callback, engine_opts: dict, extras: dict) -> DenoiseEngine:
        """Engine for these rows -> contexts -> prepare -> `count` steps from step `first` of the `steps`-step schedule; returns the
        engine.  `start`: the start latent, or a function of the engine whose device work leaves it in `engine.latent`.
        `engine_opts`: _engine's keywords.  `extras` (prepare's) are passed on without their None entries, so a job hands prepare
        only what is its own."""
        extras = {k: v for k, v in extras.items() if v is not None}
        tc = c[0].shape[1] if isinstance(c, list) else c.shape[1]
        eng = self._engine(int(u.shape[0]), tc, u.shape[1], steps, g, phi, "hint_image" in extras, "inpaint" in extras, **engine_opts)
        if callable(start):
            start = start(eng)
        eng.prepare(eng.contexts(u, c), start, self.scheduler, self.scheduler.timesteps, first, **extras)
        eng.run_steps(count, callback)
        return eng

    def _to_host(self, out, dev, sharded):
        """The job's device result -> host array, behind the cluster-GroupNorm give-up check."""
        flags = engine.gn_sync_flags(dev)   # (None without a cluster-GroupNorm plan on `dev`) queued behind the job, read with its D2H
        host = out.cpu().numpy()
        if flags is not None:   # a cluster GroupNorm that gave up - on ANY rank of a sharded job: raise, never return that image
            # group-wide ONLY for a job the group ran together: an independent replica (shard_batch False under a process
            # group that exists for other reasons) must not issue a collective its peers never match
            engine.check_gn_sync(flags.cpu(), device=dev, group_wide=sharded)
        return host

    # ---- hires fix: two passes with an on-device hand-off (minsdtf_amd/hires.py)
    def _unet_for(self, height, width) -> DiffusionModel:
        """The UNet at another image size: a view that shares the base model's packed weights (HipModel.share_weights: no
        second copy, one LoRA master, so set_loras reaches every size).  Kept per size; shared again when the base's weights
        were replaced."""
        base = self.diffusion_model
        if (height, width) == (self.img_height, self.img_width):
            return base
        base._require_weights()
        views = self.__dict__.setdefault("_unet_views", {})
        view, seen = views.get((height, width), (None, None))
        if view is None:
            view = DiffusionModel(height, width, device=base.device, name=f"{base.name}.{height}x{width}")
        if seen != base.weights_version:
            view.share_weights(base)
            views[(height, width)] = (view, base.weights_version)
        return view

    def _hires_taps(self, h1, w1, h2, w2, mode, dev):
        """Device copies of the two tap tables of a hand-off (uploaded once per shape and upscaler)."""
        cache = self.__dict__.setdefault("_hires_tap_cache", {})
        key = (h1, w1, h2, w2, mode, str(dev))
        if key not in cache:
            cache[key] = tuple(torch.from_numpy(hires_mod.pack_rows(*hires_mod.taps(n_in, n_out, mode))).to(dev)
                               for n_in, n_out in ((w1, w2), (h1, h2)))
        return cache[key]

    def _generate_hires(self, job, spec, context, unconditional_context, noise, hires_noise, num_steps, g, phi, seed, callback,
                        return_latent, pass_opts, dynthresh=None):
        """Pass 1 (the txt2img job at the pipeline's own size, no decode) -> one msd_latent_resample launch from the pass-1 engine's
        latent into the pass-2 engine's, scaled and re-noised with the pass-2 entry rates -> pass 2 at the target size -> decode.
        Both engines stay resident, so a repeated job constructs nothing and captures nothing.  pass_opts = _engine's option keywords
        for the two passes (pass 2 gets the UNet of the target size here).  dynthresh = the dynthresh.Resolved of a job with dynamic
        thresholding: both passes, each with the scale schedule over its own executed steps."""
        B = noise.shape[0]
        h1, w1, h2, w2 = self.img_height // 8, self.img_width // 8, job.height // 8, job.width // 8
        a2, s2, start2, run2 = hires_mod.entry(self.scheduler, spec, job.steps, job.strength)
        zh = hires_mod.draw_noise(B, h2, w2, seed) if hires_noise is None else self._batch_of(hires_noise, B, 3)
        if tuple(zh.shape) != (B, h2, w2, 4):
            raise ValueError(f"hires_noise has shape {tuple(zh.shape)}, the {job.height}x{job.width} latent of batch {B} is {(B, h2, w2, 4)}")
        per_sample = {"hires_noise": zh}
        # (a stochastic sampler's draws: pass 1 [seed, 1], pass 2 [seed, 3])
        sched1, z1 = self._sampler_inputs(spec, B, num_steps, h1, w1, seed)
        sched2, z2 = self._sampler_inputs(spec, B, job.steps, h2, w2, seed, stream_key=3)
        if z1 is not None:
            per_sample["z1"], per_sample["z2"] = z1.reshape(B, num_steps, -1), z2.reshape(B, job.steps, -1)
        callback2 = None if callback is None else (lambda i: callback(num_steps + i))

        def local(c, u, z, a):
            """This rank's slice: pass 1 -> hand-off into the pass-2 engine -> pass 2 -> decode; returns a device tensor."""
            b = int(z.shape[0])
            opts = [pass_opts[0], dict(pass_opts[1], unet=self._unet_for(job.height, job.width))]
            # (both keys in front of the first build: whatever neither pass needs goes before either arena is allocated)
            keys = [self._engine_key(b, c.shape[1], u.shape[1], n, g, phi, False, **o) for n, o in zip((num_steps, job.steps), opts)]
            self.scheduler.set_timesteps(num_steps)
            eng1 = self._denoise_pass(u, c, z, num_steps, g, phi, 0, num_steps, callback, dict(opts[0], job_keys=keys),
                                      dict(step_noise=a.get("z1"), sampler=sched1, dynamic_threshold=dynthresh))

            def hand_off(eng2):
                wx, wy = self._hires_taps(h1, w1, h2, w2, job.upscaler, eng1.latent.device)
                zh_dev = _f32_tensor(a["hires_noise"]).to(eng1.latent.device).contiguous()
                if zh_dev.data_ptr() % 16:   # (a slice of a packed broadcast buffer: the kernel reads 16-byte vectors)
                    zh_dev = zh_dev.clone()
                ops.latent_resample(x=eng1.latent, out=eng2.latent, wx=wx, wy=wy, batch=b, h_in=h1, w_in=w1, h_out=h2, w_out=w2,
                                    a=a2, s=s2, noise=zh_dev)(torch.cuda.current_stream().cuda_stream)

            self.scheduler.set_timesteps(job.steps)
            eng2 = self._denoise_pass(u, c, hand_off, job.steps, g, phi, start2, run2, callback2, dict(opts[1], job_keys=keys),
                                      dict(step_noise=a.get("z2"), sampler=sched2, dynamic_threshold=dynthresh))
            if return_latent:
                return eng2.latent
            return self.image_decoder.decode_to_uint8(eng2.latent)

        return self._run_sharded(local, context, unconditional_context, noise, per_sample, {})

    # ---- tiled diffusion: the views of a canvas as batch rows of one engine (minsdtf_amd/tiled.py)
    def _generate_tiled(self, geo, spec, context, unconditional_context, noise, num_steps, g, phi, seed, callback, return_latent,
                        engine_opts):
        """One engine of batch images * V keyed by the geometry: the canvas noise is uploaded and gathered into the views by one
        launch, the loop (UNet on every view, sampler step per view, consensus) is the engine's replayed graph, the canvas latent
        is decoded.  The engine stays resident, so a repeated job constructs nothing and captures nothing."""
        B, V = noise.shape[0], geo.views
        self.scheduler.set_timesteps(num_steps)
        # (a stochastic sampler's draws at CANVAS shape, cut per view (tiled.slice_views): overlapping pixels share a draw)
        sched, sampler_z = self._sampler_inputs(spec, B, num_steps, geo.H, geo.W, seed)
        per_sample = {} if sampler_z is None else {"sampler_z": sampler_z.reshape(B, num_steps, -1)}

        def per_view(x):
            """(b, ...) -> (b * V, ...): a sample's rows repeated for its V views (sample-major)."""
            return x.repeat_interleave(V, dim=0) if isinstance(x, torch.Tensor) else np.repeat(x, V, axis=0)

        def local(c, u, z, a):
            """This rank's slice of the images: engine for b * V views -> gather -> prepare -> loop -> decode the canvas."""
            zs = a.get("sampler_z")
            if zs is not None:
                zs = tiled_mod.slice_views(zs.reshape(int(z.shape[0]), num_steps, geo.H, geo.W, 4), geo)
            eng = self._denoise_pass(per_view(u), per_view(c), lambda eng: eng.load_canvas(z), num_steps, g, phi, 0, num_steps, callback,
                                     dict(engine_opts, tiled=geo), dict(step_noise=zs, sampler=sched))
            if return_latent:
                return eng.canvas
            return self.image_decoder.decode_to_uint8(eng.canvas)

        return self._run_sharded(local, context, unconditional_context, noise, per_sample, {})

    # ---- regional prompting: one prompt per masked region (minsdtf_amd/regions.py)
    def _region_inputs(self, reg, context):
        """The region prompts encoded -> (R', T, 768) fp32 (the base prompt, which `context` (B, T, 768) holds per sample, is not
        among them), and the normalised weights (R, h, w) with the base prompt's first when it takes part.  ValueError when the
        evaluated contexts do not share one token length."""
        encoded = []
        for i, prompt in enumerate(reg.prompts):
            e = np.asarray(self.encode_text(prompt), dtype=np.float32)
            e = e[0] if e.ndim == 3 and e.shape[0] == 1 else e
            if e.ndim != 2 or e.shape[1] != 768:
                raise ValueError(f"regions: the prompt of region {i} encodes to shape {tuple(e.shape)}, expected (T, 768)")
            encoded.append(e)
        lengths = ([("the base prompt", context.shape[1])] if reg.base_weight > 0.0 else []) + \
            [(f"region {i}", e.shape[0]) for i, e in enumerate(encoded)]
        if len({n for _w, n in lengths}) != 1:
            raise ValueError("regions: the region contexts must share one token length, got "
                             + ", ".join(f"{w}: {n}" for w, n in lengths))
        return np.stack(encoded, axis=0), reg.weights()

    def _t2i_model(self, unit):
        """The models.T2IAdapter of a unit: its `model`, or the checkpoint at its `path`, loaded once and kept on the pipeline."""
        from .models import T2IAdapter

        if unit.model is not None:
            if not isinstance(unit.model, T2IAdapter):
                raise ValueError(f"t2i_adapter: model is {type(unit.model).__name__}, expected a models.T2IAdapter")
            return unit.model
        cache = self.__dict__.setdefault("_t2i_adapters_by_path", {})
        if unit.path not in cache:
            cache[unit.path] = T2IAdapter(path=unit.path, device=self.diffusion_model.device)
        return cache[unit.path]

    def _t2i_inputs(self, units) -> list:
        """Per unit the four bf16 feature tensors of its picture at the job's size (models.T2IAdapter.features: the last picture's
        are kept, a repeated job does not run the adapter)."""
        out = []
        for u in units:
            model = self._t2i_model(u)
            px = t2i_mod.picture(u.image, model.in_channels, self.img_height, self.img_width, self.resize)
            out.append(model.features(px))
        return out

    def _engine_key(self, B, tc, tu, steps, g, phi, control, inpaint=False, job_keys=None, control_nets=(), ip_adapter=None, **opts) -> tuple:
        """`opts` as _engine takes them: one at its default (None) adds nothing to the key, an unknown name is a TypeError.
        `control_nets`: the further units' (ControlNet, HintNet) pairs - which objects they are and their weights' versions.
        `ip_adapter`: the models.IPAdapter of an image-prompt job - which object it is and its weights' version."""
        # the engine's plans (and captured hipGraphs) hold raw addresses of the packed weights: a set_weights() /
        # load_synthetic() / LoRA reload on any of the models it was built from must retire it
        base = self.diffusion_model
        unet = opts.pop("unet", None) or base
        wver = (unet.weights_version,) + ((self.control_net.weights_version, self.hint_net.weights_version) if control else ())
        key = (B, tc, tu, steps, g, phi, control, self.denoise_streams, inpaint, self.active_tcd, wver, engine.GN_EPOCH, opts.get("sampler"))
        key = key if unet is base else key + ((unet.h, unet.w),)   # (a hires job's second size: a view of the same weights)
        key += tuple(("control_net", id(cn), cn.weights_version, id(hn), hn.weights_version) for cn, hn in control_nets)
        key += (("ip_adapter", id(ip_adapter), ip_adapter.weights_version),) if ip_adapter is not None else ()
        return key + EngineOptions.of(**opts).key()

    def _engine(self, B, tc, tu, steps, g, phi, control, inpaint=False, job_keys=None, control_nets=(), ip_adapter=None, **opts) -> DenoiseEngine:
        """The resident engine of this shape, built if need be.  `opts`: `unet` (the UNet of another size: a hires job's second pass) and
        DenoiseEngine's options (jobopts.EngineOptions).  `job_keys`: the keys of every engine the current job uses (default: this one
        alone).  The engines' arenas are the big allocations, so whatever the current job does not need goes BEFORE anything is built: a
        re-recording (another shape, new weights, a cluster-GroupNorm give-up: GN_EPOCH) never needs room for more than the job's own engines."""
        key = self._engine_key(B, tc, tu, steps, g, phi, control, inpaint, control_nets=control_nets, ip_adapter=ip_adapter, **opts)
        keep = {key} | set(job_keys or ())
        if any(k not in keep for k in self._engines):
            import gc

            for k, old in self._engines.items():
                if k not in keep:
                    old.release_graphs()
            old = None
            self._engines = {k: e for k, e in self._engines.items() if k in keep}
            gc.collect()
        eng = self._engines.get(key)
        if eng is None:
            eng = DenoiseEngine(opts.pop("unet", None) or self.diffusion_model, B, tc, tu, steps, g, phi,
                                control_net=self.control_net if control else None,
                                hint_net=self.hint_net if control else None, use_graph=self.jit_compile,
                                # (`regions` always as an int: what the residency tests read off this call for a plain job)
                                streams=self.denoise_streams, inpaint=inpaint, tcd=self.active_tcd,
                                **(dict(control_nets=control_nets) if control_nets else {}),
                                **(dict(ip_adapter=ip_adapter) if ip_adapter is not None else {}), **dict(opts, regions=opts.get("regions") or 0))
            self._engines[key] = eng
        return eng

    def _host_loop(self, context, unconditional_context, latent, g, phi, hint_image, callback, timesteps=None, inpaint=None,
                   region_w=None, pag=None, reference=None, hypertile=None, sag=None, dynthresh=None, control=None, ip=None, t2i=None):
        """The reference's own loop over predict_on_batch (stable_diffusion.py:442-479).  t2i = (the units' features, table, the first
        executed row) of a job with T2I-Adapters.  control = (table, the further units'
        (ControlNet, HintNet) pairs, their hint pictures, the first executed row) of a job with ControlNet units.
        ip = (the models.IPAdapter, (tokens_u, tokens_c), table, the first executed row) of a job with an image prompt."""
        if timesteps is None:
            timesteps = self.scheduler.timesteps[::-1]
        batch_size = latent.shape[0]
        hint = self.hint_net.predict_on_batch(hint_image) if hint_image is not None else None
        cu_units = None if control is None else self._host_control_units(hint, control)
        iteration = 0
        n_sched = len(self.scheduler.timesteps)
        # (a job with dynamic thresholding: the scales of the executed steps as the device reads them, fp32)
        dt_tab = None if dynthresh is None else dynthresh_mod.scales(dynthresh, g, len(timesteps)).astype(np.float32)
        for _index, timestep in list(enumerate(timesteps))[::-1]:
            latent_prev = latent
            t_emb = get_timestep_embedding(timestep, batch_size)
            # (a reference-only job: the position of this evaluation in the descending schedule indexes its rate table)
            ref_step = None if reference is None else reference + (n_sched - 1 - _index,)
            # (a SAG job: its description and this timestep's rates as the device reads them, fp32 columns 0 / 1 of the coefficient row)
            sag_step = None if sag is None else (sag, float(np.float32(self.scheduler.signal_rates[timestep])),
                                                 float(np.float32(self.scheduler.noise_rates[timestep])))
            dt_step = None if dynthresh is None else (dynthresh, float(dt_tab[iteration, 0]), float(dt_tab[iteration, 1]))
            # (a job with ControlNet units: row control[3] + iteration of its table, the device step counter's row)
            cu_step = None if control is None else (cu_units, control[0][control[3] + iteration])
            # (a job with an image prompt: row ip[3] + iteration of its table, the device step counter's row)
            ip_step = None if ip is None else (ip[0], ip[1], ip[2][ip[3] + iteration])
            t2i_step = None if t2i is None else (t2i[0], t2i[1][t2i[2] + iteration])
            latent = self._guided_eps(latent, t_emb, context, unconditional_context, g, phi, hint, region_w, pag, ref_step, hypertile,
                                      sag_step, dt_step, cu_step, ip_step, t2i_step)
            latent = self.scheduler.step(latent, timestep, latent_prev)
            if inpaint is not None:   # reference :469-475
                init_latent, noise, latent_mask = inpaint
                origin = (self.scheduler.signal_rates[timestep] * np.repeat(init_latent, batch_size, axis=0)
                          + self.scheduler.noise_rates[timestep] * noise)
                latent = origin * (1.0 - latent_mask[None]) + latent * latent_mask[None]
            iteration += 1
            if callback is not None:
                callback(iteration)
        return latent

    def _host_control_units(self, hint, control):
        """[(ControlNet, its hint activation), ...] of a host-loop job with ControlNet units, unit 0 first."""
        units = [(self.control_net, hint)]
        for (cn, hn), img in zip(control[1], control[2]):
            units.append((cn, hn.predict_on_batch(img)))
        return units

    def _guided_eps(self, latent, t_emb, context, unconditional_context, g, phi, hint, region_w=None, pag=None, reference=None,
                    hypertile=None, sag=None, dynthresh=None, control=None, ip=None, t2i=None):
        """The UNet's noise prediction with classifier-free guidance and rescale over predict_on_batch (reference :442-467).
        A regional job passes `context` as the list of its region contexts and the normalised weights as `region_w`: one
        predict_on_batch per region, combined in fp32 in msd_region_combine's order (regions.combine_host); in mode "attention"
        `region_w` is the list of the four levels' planes and the conditional prediction is ONE predict_regional.  A PAG job passes
        its pag.Resolved: the conditional prediction becomes c' = (1 + k) c - k p, p from predict_perturbed (pag.combine_host).
        A SAG job passes (its sag.Resolved, alpha_t, sigma_t): predict_sag_map for the rows that yield the map, sag.degrade_host, a
        second predict_on_batch on the degraded latent, sag.combine_host - the device step's four parts in its order.
        A job with dynamic thresholding passes (its dynthresh.Resolved, the step's fp32 cfg scale, its fp32 mimic scale): behind
        whatever made u and c (the regions, PAG or SAG combine included) the result is dynthresh.dynthresh_host of the two, and no
        rescale follows - the device step's order.
        A job with ControlNet units passes ([(ControlNet, hint activation), ...], the step's table row fp32 [N][13][2]): the 13 arrays
        of every unit's predict_on_batch are scaled and summed (control.scale_host) with column 0 for the unconditional and column
        1 for the conditional prediction.
        A job with an image prompt passes (the models.IPAdapter, (tokens_u, tokens_c), the step's table row fp32 [16]): every UNet
        forward is predict_ip, with the zero embedding's tokens for the unconditional and the picture's for the conditional one.
        A job with T2I-Adapters passes (the units' features, the step's table row fp32 [U][4]): every UNet forward is predict_t2i -
        the same features for both halves - which also carries the image prompt when there is one."""
        def unet(x, half):
            """The UNet's forward of one half (0: unconditional) over [latent, t_emb, context(, 13 controls)]."""
            if t2i is not None:
                return self.diffusion_model.predict_t2i(x, t2i[0], t2i[1], ip=None if ip is None else (ip[0], ip[1][half], ip[2]))
            if ip is not None:
                return self.diffusion_model.predict_ip(x, ip[0], ip[1][half], ip[2])
            return self.diffusion_model.predict_on_batch(x)

        def guided(u, c):
            if dynthresh is not None:
                spec_dt, g_i, m_i = dynthresh
                return dynthresh_mod.dynthresh_host(u, c, g_i, m_i, spec_dt).astype(np.float32)
            e = u + g * (c - u)
            return rescale_noise_cfg(e, c, guidance_rescale=phi) if phi > 0.0 else e

        if sag is not None:
            spec, alpha, sigma = sag
            dm = self.diffusion_model
            h_, w_ = latent.shape[1], latent.shape[2]
            if g > 0.0:
                u, A = dm.predict_sag_map([latent, t_emb, unconditional_context])
                c = dm.predict_on_batch([latent, t_emb, context])
                base, base_ctx = u, unconditional_context
            else:
                c, A = dm.predict_sag_map([latent, t_emb, context])
                u, base, base_ctx = None, c, context
            degraded = sag_mod.degrade_host(latent, base, alpha, sigma, A, engine.unet_levels(h_, w_)[3], sag_mod.taps(spec.blur_sigma),
                                            spec.threshold).astype(np.float32)
            d = dm.predict_on_batch([degraded, t_emb, base_ctx])
            c = sag_mod.combine_host(u, c, d, sag_mod.weights(spec.scale, g, h_, w_))
            if u is None:
                return c
            return guided(u, c)
        if reference is not None:
            # reference-only control: (reference.Resolved, (z_ref, n_ref), rate table, evaluation index).  x_r in the device kernel's
            # arithmetic, then one predict_reference for the u rows (mix = fidelity) and one for the c rows (mix = 0)
            ref, (z_ref, n_ref), rates, i = reference
            x_r = reference_mod.reference_latent_host(z_ref, n_ref, rates[i])
            rc = np.asarray(context[:1], dtype=np.float32)
            c = self.diffusion_model.predict_reference([latent, t_emb, context], x_r, ref.layers, 0.0, ref_context=rc, adain=ref.adain)
            if g <= 0.0:
                return c
            u = self.diffusion_model.predict_reference([latent, t_emb, unconditional_context], x_r, ref.layers, ref.fidelity, ref_context=rc,
                                                        adain=ref.adain)
            return guided(u, c)

        def predict(ctx, half=1):
            """The UNet's prediction for one context, through the ControlNet if there is a hint (half: 0 for the unconditional
            prediction - the column of a control-units table); a HyperTile job's through predict_windowed ((nh, nw, depth))."""
            if hypertile is not None:
                return self.diffusion_model.predict_windowed([latent, t_emb, ctx], hypertile[:2], hypertile[2])
            if hint is None:
                return unet([latent, t_emb, ctx], half)
            if control is not None:
                units, row = control
                controls = control_mod.scale_host([cn.predict_on_batch([latent, t_emb, ctx, hi]) for cn, hi in units], row[:, :, half])
                return unet([latent, t_emb, ctx] + list(controls), half)
            controls = self.control_net.predict_on_batch([latent, t_emb, ctx, hint])
            return unet([latent, t_emb, ctx] + list(controls), half)

        regional = isinstance(context, (list, tuple))   # (its region prompts run in front of the unconditional one)
        if regional and isinstance(region_w, (list, tuple)):   # mode "attention": the level planes, one forward for all regions
            c = self.diffusion_model.predict_regional([latent, t_emb], context, region_w)
        else:
            c = regions_mod.combine_host([predict(rc) for rc in context], region_w) if regional else None
        u = predict(unconditional_context, 0) if g > 0.0 else None
        c = c if regional else predict(context)
        if pag is not None:
            p = self.diffusion_model.predict_perturbed([latent, t_emb, context], pag.layers)
            c = pag_mod.combine_host(c, p, pag_mod.weights(pag.scale, g, latent.shape[1], latent.shape[2]))
        if u is None:
            return c
        return guided(u, c)

    def _host_loop_sampler(self, context, unconditional_context, latent, g, phi, hint_image, callback, sched, start, step_noise=None,
                           inpaint=None, region_w=None, pag=None, reference=None, hypertile=None, sag=None, dynthresh=None, control=None,
                           ip=None, t2i=None):
        """A samplers.py sampler over predict_on_batch, its step in float64 (samplers.host_step), from evaluation `start`.
        t2i = (the units' features, table) of a job with T2I-Adapters.
        control = (table, the further units' (ControlNet, HintNet) pairs, their hint pictures) of a job with ControlNet units.
        ip = (the models.IPAdapter, (tokens_u, tokens_c), table) of a job with an image prompt."""
        batch_size = latent.shape[0]
        hint = self.hint_net.predict_on_batch(hint_image) if hint_image is not None else None
        cu_units = None if control is None else self._host_control_units(hint, control)
        tab = smp.rows(sched, start)
        x = np.asarray(latent, dtype=np.float64)
        prev = None
        dt_tab = None if dynthresh is None else dynthresh_mod.scales(dynthresh, g, sched.num_steps - start).astype(np.float32)
        for iteration, i in enumerate(range(start, sched.num_steps), start=1):
            t_emb = get_timestep_embedding(float(sched.timesteps[i]), batch_size)
            e = self._guided_eps(x.astype(np.float32), t_emb, context, unconditional_context, g, phi, hint, region_w, pag,
                                 None if reference is None else reference + (i,), hypertile,
                                 None if sag is None else (sag, float(np.float32(tab[i, 0])), float(np.float32(tab[i, 1]))),
                                 None if dynthresh is None else (dynthresh, float(dt_tab[i - start, 0]), float(dt_tab[i - start, 1])),
                                 None if control is None else (cu_units, control[0][i]),
                                 None if ip is None else (ip[0], ip[1], ip[2][i]),
                                 None if t2i is None else (t2i[0], t2i[1][i]))
            z = step_noise[:, i] if step_noise is not None else None
            x, prev = smp.host_step(tab[i], x, e, prev, z)
            if inpaint is not None:   # the row's own alpha / sigma, as in the device kernel
                init_latent, noise, latent_mask = inpaint
                origin = tab[i, 0] * np.repeat(init_latent, batch_size, axis=0) + tab[i, 1] * np.asarray(noise, dtype=np.float64)
                x = origin * (1.0 - latent_mask[None]) + x * latent_mask[None]
            if callback is not None:
                callback(iteration)
        return x


class StableDiffusion(StableDiffusionBase):
    """Reference ``StableDiffusion`` (stable_diffusion.py:575-725) with HIP-backed models; `batch_size` means what it means in the
    reference (the samples THIS process runs) unless ``shard_batch`` is set to True, which makes it the global batch of the
    initialised torch.distributed process group ("More than one GPU")."""

    def __init__(self, img_height=512, img_width=512, jit_compile=False, clip_skip=-1, unet_ckpt=None, text_encoder_ckpt=None,
                 vae_ckpt=None, lora_path=None, controlnet_path=None, active_tcd=False, device=None, lora_switch=False,
                 clip_vision_path=None):
        super().__init__(img_height, img_width, jit_compile, active_tcd)
        self.clip_vision_path = clip_vision_path   # the CLIP ViT-H/14 tower of image prompts, loaded on first use (clip_vision)
        # lora_switch (opt in: fp32 masters of the targetable weights stay on the device, ~3.4 GB for the UNet): LoRAs are merged
        # into the packed weights in place by set_loras() instead of at load time (minsdtf_amd/lora.py)
        self.lora_switch = bool(lora_switch)
        self._active_loras: List[Tuple[object, float]] = []
        self._computed_uncond = None
        self.clip_skip = clip_skip
        self.unet_ckpt = unet_ckpt
        self.text_encoder_ckpt = text_encoder_ckpt
        self.vae_ckpt = vae_ckpt
        self.controlnet_path = controlnet_path
        self.lora_path = None
        self.text_encoder_lora_dict = None
        self.unet_lora_dict = None
        if lora_path is not None and os.path.exists(str(lora_path)):   # reference :641-643
            self.text_encoder_lora_dict, self.unet_lora_dict = wtab.load_weights_from_lora(lora_path)
            self.lora_path = lora_path
        self.device = device if device is not None else default_device()
        if self.lora_switch and self.lora_path is not None:
            self._active_loras = [(self.lora_path, 1.0)]   # merged when each model gets its weights (_with_loras)

    # ---- LoRA switch at run time
    @property
    def active_loras(self) -> Tuple[Tuple[object, float], ...]:
        """The LoRAs merged into the weights now: ((source, scale), ...)."""
        return tuple(self._active_loras)

    def _lora_models(self):
        """The models a LoRA changes that hold weights now (the ControlNet and the VAE are not LoRA targets)."""
        out = [self.diffusion_model]
        if self._text_models_ready():
            out.append(self.text_encoder)
        return [m for m in out if m._W is not None]

    def set_loras(self, loras) -> None:
        """Replace the active LoRA set with `loras` = [(source, scale), ...] (source: a kohya .safetensors / .pt path or a loaded
        state dict; scale: any float).  Entry i adds scale_i * alpha_i / rank_i * up_i @ down_i to its layers; [] restores the base
        weights bit for bit.  The packed weights are rewritten in place (same tensors, same layouts), so launch plans and the
        captured whole-loop graph stay valid.  Stream-ordered on the model's device, then synchronised: a job started afterwards
        on any stream sees the new weights.  Not allowed from inside a generate_image callback.  Every check (the switch, the
        files, the shapes) runs before the first device write."""
        if not self.lora_switch:
            raise RuntimeError("set_loras needs StableDiffusion(lora_switch=True)")
        from . import lora

        loras = [(src, float(scale)) for src, scale in loras]
        sets = [(lora.read_factors(src, self.device), scale) for src, scale in loras]
        models = self._lora_models()
        for m in models:
            m.validate_loras(sets)
        for m in models:
            changed = m.set_loras(sets)
            if changed and m is self._text_encoder and self._computed_uncond is not None \
                    and self.unconditional_context is self._computed_uncond:
                self.unconditional_context = self._computed_uncond = None
        self._active_loras = loras

    def _with_loras(self, model):
        """A model created after set_loras (the properties build them lazily) gets the active set merged at once."""
        if self.lora_switch and self._active_loras and model._W is not None:
            from . import lora

            model.set_loras([(lora.read_factors(src, self.device), scale) for src, scale in self._active_loras])
        return model

    @property
    def diffusion_model(self):
        if self._diffusion_model is None:
            self._diffusion_model = DiffusionModel(self.img_height, self.img_width, ckpt_path=self.unet_ckpt,
                                                   apply_control_net=self.controlnet_path is not None,
                                                   lora_dict=None if self.lora_switch else self.unet_lora_dict, device=self.device,
                                                   lora_switch=self.lora_switch)
            self._with_loras(self._diffusion_model)
            if self.jit_compile:
                self._diffusion_model.compile(jit_compile=True)
        return self._diffusion_model

    @property
    def image_decoder(self):
        if self._image_decoder is None:
            self._image_decoder = ImageDecoder(ckpt_path=self.vae_ckpt, device=self.device)
            if self.jit_compile:
                self._image_decoder.compile(jit_compile=True)
        return self._image_decoder

    @property
    def text_clip_embedding(self):
        """Reference :686-691."""
        if self._text_clip_embedding is None:
            self._text_clip_embedding = TextClipEmbedding(MAX_PROMPT_LENGTH, ckpt_path=self.text_encoder_ckpt, device=self.device)
            if self.jit_compile:
                self._text_clip_embedding.compile(jit_compile=True)
        return self._text_clip_embedding

    @property
    def text_encoder(self):
        """Reference :672-683."""
        if self._text_encoder is None:
            self._text_encoder = TextEncoder(MAX_PROMPT_LENGTH, clip_skip=self.clip_skip, ckpt_path=self.text_encoder_ckpt,
                                             lora_dict=None if self.lora_switch else self.text_encoder_lora_dict, device=self.device,
                                             lora_switch=self.lora_switch)
            self._with_loras(self._text_encoder)
            if self.jit_compile:
                self._text_encoder.compile(jit_compile=True)
        return self._text_encoder

    def _text_models_ready(self) -> bool:
        if self._text_encoder is not None and self._text_clip_embedding is not None:
            return self._text_encoder._W is not None and self._text_clip_embedding._W is not None
        return self.text_encoder_ckpt is not None and os.path.exists(str(self.text_encoder_ckpt))

    @property
    def image_encoder(self):
        if self._image_encoder is None:
            self._image_encoder = ImageEncoder(ckpt_path=self.vae_ckpt, device=self.device)
            if self.jit_compile:
                self._image_encoder.compile(jit_compile=True)
        return self._image_encoder

    @property
    def control_net(self):
        if self._control_net is None:
            self._control_net = ControlNet(self.img_height, self.img_width, controlnet_path=self.controlnet_path, device=self.device)
            if self.jit_compile:
                self._control_net.compile(jit_compile=True)
        return self._control_net

    @property
    def hint_net(self):
        if self._hint_net is None:
            self._hint_net = HintNet(self.img_height, self.img_width, controlnet_path=self.controlnet_path, device=self.device)
            if self.jit_compile:
                self._hint_net.compile(jit_compile=True)
        return self._hint_net
