"""Typed launch records for the C ABI (include/minsdtf_hip.h).

Every function here only *describes* one library call: it fills the ctypes argument block from
raw device addresses + shapes and returns a :class:`Call`.  Running a Call on a stream is one
foreign call, so a whole UNet forward is a flat Python list of Calls that is recorded once and
then replayed from a hipGraph.  No arithmetic happens in this module and nothing falls back to
PyTorch: if the library is missing, :func:`_lib.load` raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from . import _lib, _lib_control, _lib_dynthresh, _lib_ext, _lib_ipadapter, _lib_resampler, _lib_t2i, _lib_vision
from ._lib import ACT_GEGLU, ACT_NONE, ACT_QUICK_GELU, ACT_SILU, OUT_BF16, OUT_F32, OUT_U8  # noqa: F401


class Call:
    """One stream-ordered library call: ``fn(*args, stream)``."""

    __slots__ = ("fn", "args", "name", "keep", "check")

    def __init__(self, fn, args, name, keep=None, check=_lib.check):
        """check: the owning library's (rc, name) -> raise (the extension library keeps its own error text)."""
        self.fn, self.args, self.name, self.keep, self.check = fn, args, name, keep, check

    def __call__(self, stream: int) -> None:
        rc = self.fn(*self.args, stream)
        if rc != 0:
            self.check(rc, self.name)


def _p(x) -> Optional[int]:
    """Device address of a torch tensor / Buf / int / None."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "ptr"):
        return x.ptr
    return x.data_ptr()


def conv_gemm(*, a0, w, out, batch, h_in, w_in, c0, N, a1=None, c1=0, ksize=1, stride=1, upsample=False, bias=None,
              rowvec=None, rv_step_stride=0, rv_batch_stride=0, step_ptr=None, residual=None, res_ld=None, act=ACT_NONE,
              out_dtype=OUT_BF16, out_ld=None, split=None, workspace=None, workspace_floats=0, splitk=1, tile_n=0,
              tile_m=0, stages=0, pad=None, pad_end=None, ln_in=None, ln_in_slots=0, ln_colsum=None, ln_out=None,
              ln_out_slots=0, ln_eps=1e-5, a2=None, c2=0, a3=None, c3=0, w_layout=0, name="conv_gemm") -> Call:
    """split = (ns0, ns1, out1, out1_ld, out2, out2_ld) selects the q|k|v^T epilogue.
    pad / pad_end: leading / trailing zero padding (default: symmetric 1 for 3x3, 0 for 1x1);
    (0, 1) is the VAE encoder's stride-2 padding ((0,1),(0,1))."""
    lib = _lib.load()
    if pad is None:
        pad = 1 if ksize == 3 else 0
    if pad_end is None:
        pad_end = pad
    hl, wl = (2 * h_in, 2 * w_in) if upsample else (h_in, w_in)
    h_out = (hl + pad + pad_end - ksize) // stride + 1
    w_out = (wl + pad + pad_end - ksize) // stride + 1
    n_out = N // 2 if act == ACT_GEGLU else N
    s = _lib.MsdConvGemm()
    s.a0, s.a1, s.w = _p(a0), _p(a1), _p(w)
    s.bias, s.rowvec, s.step_ptr, s.residual = _p(bias), _p(rowvec), _p(step_ptr), _p(residual)
    s.out = _p(out)
    s.workspace, s.workspace_floats = _p(workspace), int(workspace_floats)
    s.batch, s.h_in, s.w_in, s.c0, s.c1 = batch, h_in, w_in, c0, c1
    s.h_out, s.w_out, s.ksize, s.stride, s.pad, s.upsample = h_out, w_out, ksize, stride, pad, int(bool(upsample))
    s.N, s.act, s.out_dtype = N, act, out_dtype
    s.out_ld = n_out if out_ld is None else out_ld
    s.res_ld = (n_out if res_ld is None else res_ld) if residual is not None else 0
    s.rv_step_stride, s.rv_batch_stride = rv_step_stride, rv_batch_stride
    if split is not None:
        ns0, ns1, out1, out1_ld, out2, out2_ld = split
        s.split_mode, s.ns0, s.ns1 = 1, ns0, ns1
        s.out1, s.out1_ld, s.out2, s.out2_ld = _p(out1), out1_ld, _p(out2), out2_ld
        if out_ld is None:
            s.out_ld = max(ns0, 4)
    s.splitk, s.tile_n, s.tile_m, s.stages = splitk, tile_n, tile_m, stages
    # LayerNorm fold (include/minsdtf_hip.h): row-moment partials in / out, column sums of the folded weights
    s.ln_in, s.ln_colsum, s.ln_out = _p(ln_in), _p(ln_colsum), _p(ln_out)
    s.ln_in_slots, s.ln_out_slots, s.ln_eps = ln_in_slots, ln_out_slots, float(ln_eps)
    s.a2, s.a3, s.c2, s.c3 = _p(a2), _p(a3), c2, c3   # shortcut operand: extra K tiles read at the output pixel
    s.w_layout = int(w_layout)   # 0: [N][K]; 1: chunk-major [K/64][N][64] (packing.chunk_major); 2: fragment-major (packing.fragment_major)
    return Call(lib.msd_conv_gemm, (C.byref(s),), name, keep=s)


def conv_gemm_ln_slots(*, N, tile_n, tile_m=0, ksize=1, act=ACT_NONE) -> int:
    """Row-moment partials per row a launch with these parameters writes to ``ln_out``."""
    lib = _lib.load()
    s = _lib.MsdConvGemm()
    s.N, s.tile_n, s.tile_m, s.ksize, s.act = N, tile_n, tile_m, ksize, act
    n = lib.msd_conv_gemm_ln_slots(C.byref(s))
    if n <= 0:
        _lib.check(n, "conv_gemm_ln_slots")
    return n


def conv_direct(*, x, w, out, batch, h_in, w_in, c_in, c_out, ksize=3, stride=1, bias=None, residual=None,
                in_batch_mod=None, in_dtype=OUT_BF16, out_dtype=OUT_BF16, act=ACT_NONE, act_in=False, in_scale=1.0,
                name="conv_direct") -> Call:
    lib = _lib.load()
    pad = 1 if ksize == 3 else 0
    s = _lib.MsdConvDirect()
    s.in_, s.w, s.bias, s.residual, s.out = _p(x), _p(w), _p(bias), _p(residual), _p(out)
    s.batch, s.in_batch_mod = batch, (batch if in_batch_mod is None else in_batch_mod)
    s.h_in, s.w_in, s.c_in = h_in, w_in, c_in
    s.h_out = (h_in + 2 * pad - ksize) // stride + 1
    s.w_out = (w_in + 2 * pad - ksize) // stride + 1
    s.c_out, s.ksize, s.stride, s.pad = c_out, ksize, stride, pad
    s.in_dtype, s.out_dtype, s.act, s.act_in, s.in_scale = in_dtype, out_dtype, act, int(bool(act_in)), float(in_scale)
    return Call(lib.msd_conv_direct, (C.byref(s),), name, keep=s)


GN_MAX_CHUNKS = 1024


GN_SYNC_WORDS_PER_SAMPLE = 16384   # MSD_GN_SYNC_WORDS_PER_SAMPLE


def group_norm(*, x0, gamma, beta, stats, partials, out, batch, hw, c0, x1=None, c1=0, silu=False, eps=1e-5,
               partials_floats=None, sync=None, sync_words=None, name="group_norm") -> Call:
    """sync: zero-initialised uint32 block of >= batch * GN_SYNC_WORDS_PER_SAMPLE words owned by the calling stream (see
    include/minsdtf_hip.h): enables the single-launch cluster form for the larger tensors."""
    lib = _lib.load()
    s = _lib.MsdGroupNorm()
    s.x0, s.x1, s.gamma, s.beta, s.stats, s.out = _p(x0), _p(x1), _p(gamma), _p(beta), _p(stats), _p(out)
    s.partials = _p(partials)
    s.partials_floats = batch * GN_MAX_CHUNKS * 64 if partials_floats is None else partials_floats
    s.batch, s.hw, s.c0, s.c1, s.silu, s.eps = batch, hw, c0, c1, int(bool(silu)), float(eps)
    s.sync = _p(sync)
    s.sync_words = 0 if sync is None else (batch * GN_SYNC_WORDS_PER_SAMPLE if sync_words is None else sync_words)
    return Call(lib.msd_group_norm, (C.byref(s),), name, keep=s)


def layer_norm(*, x, gamma, beta, out, rows, c, eps=1e-5, name="layer_norm") -> Call:
    lib = _lib.load()
    return Call(lib.msd_layer_norm, (_p(x), _p(gamma), _p(beta), _p(out), rows, c, C.c_float(eps)), name)


def attention(*, q, k, vt, out, batch, heads, head_dim, s, t, q_ld, k_ld, vt_ld, o_ld, scale, causal=False,
              q_prescaled=False, workspace=None, workspace_floats=0, name="attention") -> Call:
    lib = _lib.load()
    a = _lib.MsdAttention()
    a.q, a.k, a.vt, a.out = _p(q), _p(k), _p(vt), _p(out)
    a.batch, a.heads, a.head_dim, a.s, a.t = batch, heads, head_dim, s, t
    a.q_ld, a.k_ld, a.vt_ld, a.o_ld, a.scale = q_ld, k_ld, vt_ld, o_ld, float(scale)
    a.causal = int(bool(causal))
    a.q_prescaled = int(bool(q_prescaled))
    a.workspace, a.workspace_floats = _p(workspace), int(workspace_floats)   # (head_dim 512: scratch of the 4-way key split)
    return Call(lib.msd_attention, (C.byref(a),), name, keep=a)


def cross_attention_q(*, x, ln_in, ln_in_slots, wq, ln_colsum, bias, k, vt, out, batch, heads, head_dim, s, t, k_ld, vt_ld, o_ld,
                      ln_eps=1e-5, w_layout=0, name="cross_attention_q") -> Call:
    """attn2.to_q (LayerNorm folded in) + attention over the text context in one launch (msd_cross_attention_q)."""
    lib = _lib.load()
    a = _lib.MsdCrossAttnQ()
    a.x, a.ln_in, a.wq, a.ln_colsum, a.bias, a.k, a.vt, a.out = _p(x), _p(ln_in), _p(wq), _p(ln_colsum), _p(bias), _p(k), _p(vt), _p(out)
    a.batch, a.heads, a.head_dim, a.s, a.t = batch, heads, head_dim, s, t
    a.k_ld, a.vt_ld, a.o_ld, a.ln_in_slots, a.ln_eps, a.w_layout = k_ld, vt_ld, o_ld, ln_in_slots, float(ln_eps), int(w_layout)
    return Call(lib.msd_cross_attention_q, (C.byref(a),), name, keep=a)


def softmax_rows(*, x, out, rows, cols, ld_in, ld_out, scale, name="softmax_rows") -> Call:
    lib = _lib.load()
    return Call(lib.msd_softmax_rows, (_p(x), _p(out), rows, cols, ld_in, ld_out, C.c_float(scale)), name)


def cfg_step(*, eps, latent, coef, step_ptr, batch, n, num_steps, guidance, guidance_rescale, advance=True,
             inpaint_init=None, inpaint_noise=None, inpaint_mask=None, step_noise=None, noise_coef=None,
             name="cfg_step") -> Call:
    lib = _lib.load()
    s = _lib.MsdCfgStep()
    s.eps, s.latent, s.coef, s.step_ptr = _p(eps), _p(latent), _p(coef), _p(step_ptr)
    s.inpaint_init, s.inpaint_noise, s.inpaint_mask = _p(inpaint_init), _p(inpaint_noise), _p(inpaint_mask)
    s.step_noise, s.noise_coef = _p(step_noise), _p(noise_coef)
    s.batch, s.n, s.num_steps = batch, n, num_steps
    s.guidance, s.guidance_rescale, s.advance = float(guidance), float(guidance_rescale), int(advance)   # 2: in-kernel ({step, ticket})
    return Call(lib.msd_cfg_step, (C.byref(s),), name, keep=s)


def sampler_step(*, eps, latent, coef, step_ptr, denoised_prev, batch, n, num_steps, guidance, guidance_rescale, advance=True,
                 inpaint_init=None, inpaint_noise=None, inpaint_mask=None, step_noise=None, name="sampler_step") -> Call:
    """msd_sampler_step: coef fp32 [num_steps][8] (minsdtf_amd/samplers.py), denoised_prev fp32 [batch][n] (read where the row's
    c_P != 0, written every step), step_noise fp32 [num_steps][batch][n] or None."""
    lib = _lib.load()
    s = _lib.MsdSamplerStep()
    s.eps, s.latent, s.coef, s.step_ptr = _p(eps), _p(latent), _p(coef), _p(step_ptr)
    s.inpaint_init, s.inpaint_noise, s.inpaint_mask = _p(inpaint_init), _p(inpaint_noise), _p(inpaint_mask)
    s.step_noise, s.denoised_prev = _p(step_noise), _p(denoised_prev)
    s.batch, s.n, s.num_steps = batch, n, num_steps
    s.guidance, s.guidance_rescale, s.advance = float(guidance), float(guidance_rescale), int(advance)   # 2: in-kernel ({step, ticket})
    return Call(lib.msd_sampler_step, (C.byref(s),), name, keep=s)


def latent_resample(*, x, out, wx, wy, batch, h_in, w_in, h_out, w_out, a=1.0, s=0.0, noise=None, name="latent_resample") -> Call:
    """msd_latent_resample: out = a * resample(x) + s * noise on the fp32 NHWC latent (C = 4).  wx / wy: the device copies of the
    per-axis tap rows (hires.pack_rows: int32 [w_out][8] / [h_out][8]); noise fp32 [batch][h_out][w_out][4] or None."""
    lib = _lib.load()
    r = _lib.MsdLatentResample()
    r.in_, r.out, r.noise, r.wx, r.wy = _p(x), _p(out), _p(noise), _p(wx), _p(wy)
    r.batch, r.h_in, r.w_in, r.h_out, r.w_out = int(batch), int(h_in), int(w_in), int(h_out), int(w_out)
    r.a, r.s = float(a), float(s)
    return Call(lib.msd_latent_resample, (C.byref(r),), name, keep=r)


def tile_consensus(*, tiles, canvas, wy, wx, ys, xs, th, tw, H, W, batch, mode=0, name="tile_consensus") -> Call:
    """msd_tile_consensus: mode 0 - every canvas pixel and every view's entry for it become the weighted mean of the views that
    cover it; mode 1 (gather) - the canvas is copied into the views.  tiles fp32 [batch * len(ys) * len(xs)][th][tw][4] (in
    place), canvas fp32 [batch][H][W][4], wy / wx: device fp32 weight rows [th] / [tw], ys / xs: the view offsets per axis."""
    lib = _lib.load()
    ys, xs = [int(v) for v in ys], [int(v) for v in xs]
    if not 1 <= len(ys) <= _lib.TILE_MAX_VIEWS or not 1 <= len(xs) <= _lib.TILE_MAX_VIEWS:
        raise ValueError(f"tile_consensus: {len(ys)} x {len(xs)} views (1 .. {_lib.TILE_MAX_VIEWS} per axis)")
    t = _lib.MsdTileConsensus()
    t.tiles, t.canvas, t.wy, t.wx = _p(tiles), _p(canvas), _p(wy), _p(wx)
    t.ys[:len(ys)], t.xs[:len(xs)] = ys, xs
    t.rows, t.cols, t.th, t.tw, t.H, t.W, t.batch, t.mode = len(ys), len(xs), int(th), int(tw), int(H), int(W), int(batch), int(mode)
    return Call(lib.msd_tile_consensus, (C.byref(t),), name, keep=t)


def region_combine(*, eps, w, out, regions, batch, n, name="region_combine") -> Call:
    """msd_region_combine: out[b] = sum_r w[r] * eps[r * batch + b] per pixel, r ascending, fp32 FMAs.  eps fp32 [regions * batch][n]
    (region-major), w fp32 [regions][n / 4] (normalised on the host: regions.weights), out fp32 [batch][n] (may be eps: in place)."""
    lib = _lib.load()
    s = _lib.MsdRegionCombine()
    s.eps, s.w, s.out = _p(eps), _p(w), _p(out)
    s.regions, s.batch, s.n = int(regions), int(batch), int(n)
    return Call(lib.msd_region_combine, (C.byref(s),), name, keep=s)


def region_attention(*, q, k, vt, w, out, batch, heads, head_dim, s, t, regions, q_ld, k_ld, vt_ld, w_ld, o_ld,
                     name="region_attention") -> Call:
    """msd_region_attention: out[b] = sum_r w[r] * softmax(q[b] k[r * batch + b]^T) v[r * batch + b] per query, r ascending, a
    weight of exactly 0 not accumulated.  q bf16 [batch][s][q_ld] carrying scale * log2(e), k bf16 [regions * batch][t][k_ld],
    vt bf16 [regions * batch][heads * head_dim][vt_ld], w fp32 [regions][w_ld] (regions.Resolved.level_weights), out bf16
    [batch][s][o_ld]."""
    lib = _lib.load()
    a = _lib.MsdRegionAttention()
    a.q, a.k, a.vt, a.w, a.out = _p(q), _p(k), _p(vt), _p(w), _p(out)
    a.batch, a.heads, a.head_dim, a.s, a.t, a.regions = int(batch), int(heads), int(head_dim), int(s), int(t), int(regions)
    a.q_ld, a.k_ld, a.vt_ld, a.w_ld, a.o_ld = int(q_ld), int(k_ld), int(vt_ld), int(w_ld), int(o_ld)
    return Call(lib.msd_region_attention, (C.byref(a),), name, keep=a)


def attention_identity(*, vt, out, batch, channels, s, vt_ld, o_ld, name="attention_identity") -> Call:
    """msd_attention_identity: out[b][k][c] = vt[b][c][k] - self-attention with the identity map (the perturbed rows of a PAG job).
    vt bf16 [batch][channels][vt_ld] (msd_attention's operand), out bf16 [batch][s][o_ld]."""
    lib = _lib.load()
    a = _lib.MsdAttentionIdentity()
    a.vt, a.out = _p(vt), _p(out)
    a.batch, a.channels, a.s, a.vt_ld, a.o_ld = int(batch), int(channels), int(s), int(vt_ld), int(o_ld)
    return Call(lib.msd_attention_identity, (C.byref(a),), name, keep=a)


def attention_joint(*, q, k, vt, k_ref, vt_ref, out, batch, heads, head_dim, s, t, t_ref, q_ld, k_ld, vt_ld, o_ld, mix=None,
                    name="attention_joint") -> Call:
    """msd_attention_joint: out[b] = mix[b] * softmax(q[b] k[b]^T) v[b] + (1 - mix[b]) * softmax(q[b] [k[b] ; k_ref]^T) [v[b] ; v_ref]
    - the generated rows of a reference-only job.  q bf16 [batch][s][q_ld] carrying scale * log2(e), k bf16 [batch][t][k_ld], vt bf16
    [batch][heads * head_dim][vt_ld], k_ref bf16 [t_ref][k_ld] and vt_ref bf16 [heads * head_dim][vt_ld] (ONE row, shared by the
    batch), mix fp32 [batch] or None (all 0), out bf16 [batch][s][o_ld]."""
    lib = _lib.load()
    a = _lib.MsdAttentionJoint()
    a.q, a.k, a.vt, a.k_ref, a.vt_ref, a.mix, a.out = _p(q), _p(k), _p(vt), _p(k_ref), _p(vt_ref), _p(mix), _p(out)
    a.batch, a.heads, a.head_dim, a.s, a.t, a.t_ref = int(batch), int(heads), int(head_dim), int(s), int(t), int(t_ref)
    a.q_ld, a.k_ld, a.vt_ld, a.o_ld = int(q_ld), int(k_ld), int(vt_ld), int(o_ld)
    return Call(lib.msd_attention_joint, (C.byref(a),), name, keep=a)


def attention_windowed(*, q, k, vt, out, batch, heads, head_dim, h, w, wh, ww, q_ld, k_ld, vt_ld, o_ld, name="attention_windowed") -> Call:
    """msd_attention_windowed (HyperTile): per sample, head and window of wh x ww tokens of the h x w feature map, out = softmax(q k^T) v
    over that window's keys only.  q bf16 [batch][h * w][q_ld] carrying scale * log2(e), k bf16 [batch][h * w][k_ld], vt bf16
    [batch][heads * head_dim][vt_ld], out bf16 [batch][h * w][o_ld]: msd_attention's operands in image order, nothing gathered."""
    lib = _lib.load()
    a = _lib.MsdAttentionWindowed()
    a.q, a.k, a.vt, a.out = _p(q), _p(k), _p(vt), _p(out)
    a.batch, a.heads, a.head_dim = int(batch), int(heads), int(head_dim)
    a.h, a.w, a.wh, a.ww = int(h), int(w), int(wh), int(ww)
    a.q_ld, a.k_ld, a.vt_ld, a.o_ld = int(q_ld), int(k_ld), int(vt_ld), int(o_ld)
    return Call(lib.msd_attention_windowed, (C.byref(a),), name, keep=a)


def reference_latent(*, z, noise, coef, out, n, num_steps, step_ptr=None, name="reference_latent") -> Call:
    """msd_reference_latent: out = coef[step][0] * z + coef[step][1] * noise (one fp32 FMA per element), step = *step_ptr.  z / noise /
    out fp32 [n], coef fp32 [num_steps][2] (reference.rates)."""
    lib = _lib.load()
    r = _lib.MsdReferenceLatent()
    r.z, r.noise, r.coef, r.step_ptr, r.out = _p(z), _p(noise), _p(coef), _p(step_ptr), _p(out)
    r.n, r.num_steps = int(n), int(num_steps)
    return Call(lib.msd_reference_latent, (C.byref(r),), name, keep=r)


ADAIN_RESIDENT_HW = 1024   # csrc/adain.hip AD_RESIDENT_HW: the largest hw whose row slab msd_reference_adain keeps in registers


def reference_adain(*, x, ref, rows, hw, c, mix=None, eps=1e-6, name="reference_adain") -> Call:
    """msd_reference_adain: x[b] = mix[b] * x[b] + (1 - mix[b]) * ((x[b] - mean_b) * std_r / std_b + mean_r) per channel, the statistics
    over the hw pixels, in place - reference AdaIN of a reference-only job.  x bf16 [rows][hw][c], ref bf16 [hw][c] (apart from
    those rows), mix fp32 [rows] or None (all 0)."""
    lib = _lib.load()
    a = _lib.MsdReferenceAdain()
    a.x, a.ref, a.mix = _p(x), _p(ref), _p(mix)
    a.rows, a.hw, a.c, a.eps = int(rows), int(hw), int(c), float(eps)
    return Call(lib.msd_reference_adain, (C.byref(a),), name, keep=a)


# ---- the extension library (include/minsdtf_hip_ext.h, minsdtf_amd/_lib_ext.py) ----------------------------------------------------
def attention_colsum(*, q, k, out, workspace, batch, heads, head_dim, s, q_ld, k_ld, workspace_floats=None,
                     name="attention_colsum") -> Call:
    """msdx_attention_colsum: out[b][j] = (1 / heads) * sum_h sum_i softmax_j(q_h k_h^T)[i][j] - the attention every key receives
    (self-attention guidance, minsdtf_amd/sag.py).  q bf16 [batch][s][q_ld] carrying scale * log2(e), k bf16 [batch][s][k_ld],
    out fp32 [batch][s], workspace fp32 [batch][heads][s][2] (COLSUM_WS floats per (sample, head, query))."""
    lib = _lib_ext.load()
    a = _lib_ext.MsdxAttentionColsum()
    a.q, a.k, a.out, a.workspace = _p(q), _p(k), _p(out), _p(workspace)
    a.workspace_floats = int(colsum_workspace_floats(batch, heads, s) if workspace_floats is None else workspace_floats)
    a.batch, a.heads, a.head_dim, a.s, a.q_ld, a.k_ld = int(batch), int(heads), int(head_dim), int(s), int(q_ld), int(k_ld)
    return Call(lib.msdx_attention_colsum, (C.byref(a),), name, keep=a, check=_lib_ext.check)


def colsum_workspace_floats(batch: int, heads: int, s: int) -> int:
    """Floats of msdx_attention_colsum's workspace: (row maximum, row sum) per (sample, head, query)."""
    return int(batch) * int(heads) * int(s) * 2


def sag_degrade(*, latent, eps, coef, coef_stride, colsum, params, out, batch, h, w, mh, mw, num_steps, step_ptr=None,
                name="sag.degrade") -> Call:
    """msdx_sag_degrade: the degraded latent of a self-attention-guidance step.  latent / eps / out fp32 [batch][h][w][4], coef fp32
    [num_steps][coef_stride] (columns 0, 1: alpha_t, sigma_t of row *step_ptr), colsum fp32 [batch][mh * mw], params fp32 [10]
    (sag.params: the 9 taps, the threshold)."""
    lib = _lib_ext.load()
    d = _lib_ext.MsdxSagDegrade()
    d.latent, d.eps, d.coef, d.step_ptr, d.colsum, d.params, d.out = _p(latent), _p(eps), _p(coef), _p(step_ptr), _p(colsum), _p(params), _p(out)
    d.batch, d.h, d.w, d.mh, d.mw = int(batch), int(h), int(w), int(mh), int(mw)
    d.coef_stride, d.num_steps = int(coef_stride), int(num_steps)
    return Call(lib.msdx_sag_degrade, (C.byref(d),), name, keep=d, check=_lib_ext.check)


# ---- the dynamic-thresholding library (include/minsdtf_hip_dynthresh.h, minsdtf_amd/_lib_dynthresh.py) -----------------------------
def dynamic_threshold(*, eps, out, scales, params, batch, h, w, num_steps, step_ptr=None, name="dynamic_threshold") -> Call:
    """msdt_dynamic_threshold: the combined prediction of a guidance step with dynamic thresholding (minsdtf_amd/dynthresh.py).
    eps fp32 [2 * batch][h * w * 4] (the u rows, then the c rows), out fp32 [batch][h * w * 4] (eps itself, or apart from it), scales
    fp32 [num_steps][2] (row *step_ptr: the cfg and the mimic scale), params the 32 bytes of dynthresh.params."""
    lib = _lib_dynthresh.load()
    a = _lib_dynthresh.MsdtDynamicThreshold()
    a.eps, a.out, a.scales, a.step_ptr, a.params = _p(eps), _p(out), _p(scales), _p(step_ptr), _p(params)
    a.batch, a.h, a.w, a.num_steps = int(batch), int(h), int(w), int(num_steps)
    return Call(lib.msdt_dynamic_threshold, (C.byref(a),), name, keep=a, check=_lib_dynthresh.check)


# ---- the ControlNet-units library (include/minsdtf_hip_control.h, minsdtf_amd/_lib_control.py) -------------------------------------
def control_chunk_prefix(counts) -> list:
    """MsdcControlCombine.chunk_prefix of the 13 per-row element counts: the workgroups of a row in front of every tap, then all."""
    out = [0]
    for n in counts:
        out.append(out[-1] + (int(n) + _lib_control.CHUNK - 1) // _lib_control.CHUNK)
    return out


def control_combine(*, skips, resid, counts, scales, rows, rows_u, num_steps, step_ptr=None, name="control_combine") -> Call:
    """msdc_control_combine: skip_k[b] = bf16(fp32(skip_k[b]) + sum_n s_n * resid[n][k][b]), one fmaf per unit in unit order, over the 13
    taps of one UNet pass in ONE launch (minsdtf_amd/control.py).  skips: 13 bf16 [rows][counts[k]] (in place); resid: 1 .. 3 lists of
    13 fp32 [rows][counts[k]]; scales fp32 [num_steps][len(resid)][13][2] (row *step_ptr; column 0 for the rows < rows_u, else 1)."""
    lib = _lib_control.load()
    T = _lib_control.TAPS
    if len(skips) != T or len(counts) != T or not 1 <= len(resid) <= _lib_control.MAX_UNITS or any(len(r) != T for r in resid):
        raise ValueError(f"control_combine: {len(skips)} skips, {len(counts)} counts, {[len(r) for r in resid]} residuals "
                         f"({T} of each, 1 .. {_lib_control.MAX_UNITS} units)")
    a = _lib_control.MsdcControlCombine()
    for k in range(T):
        a.skip[k], a.count[k] = _p(skips[k]), int(counts[k])
        for n, r in enumerate(resid):
            a.resid[n][k] = _p(r[k])
    a.chunk_prefix[:] = control_chunk_prefix(counts)
    a.scales, a.step_ptr = _p(scales), _p(step_ptr)
    a.rows, a.rows_u, a.units, a.num_steps = int(rows), int(rows_u), len(resid), int(num_steps)
    return Call(lib.msdc_control_combine, (C.byref(a),), name, keep=a, check=_lib_control.check)


# ---- the IP-Adapter library (include/minsdtf_hip_ipadapter.h, minsdtf_amd/_lib_ipadapter.py) ---------------------------------------
def ip_attention(*, q, k, vt, k_ip, vt_ip, out, scales, batch, heads, head_dim, s, t, n, q_ld, k_ld, vt_ld, kip_ld, vtip_ld, o_ld, layer,
                 num_steps, step_ptr=None, name="ip_attention") -> Call:
    """msdi_attention_decoupled: out[b] = softmax(q[b] k[b]^T) v[b] + sc * softmax(q[b] k_ip[b]^T) v_ip[b] per query, two independent
    softmaxes in one launch, sc = scales[*step_ptr][layer] (minsdtf_amd/ipadapter.py).  q bf16 [batch][s][q_ld] carrying scale *
    log2(e), k bf16 [batch][t][k_ld], vt bf16 [batch][heads * head_dim][vt_ld], k_ip bf16 [batch][n][kip_ld], vt_ip bf16
    [batch][heads * head_dim][vtip_ld], scales fp32 [num_steps][16], out bf16 [batch][s][o_ld]."""
    lib = _lib_ipadapter.load()
    a = _lib_ipadapter.MsdiAttentionDecoupled()
    a.q, a.k, a.vt, a.k_ip, a.vt_ip, a.out = _p(q), _p(k), _p(vt), _p(k_ip), _p(vt_ip), _p(out)
    a.scales, a.step_ptr = _p(scales), _p(step_ptr)
    a.batch, a.heads, a.head_dim, a.s, a.t, a.n = int(batch), int(heads), int(head_dim), int(s), int(t), int(n)
    a.q_ld, a.k_ld, a.vt_ld, a.kip_ld, a.vtip_ld, a.o_ld = int(q_ld), int(k_ld), int(vt_ld), int(kip_ld), int(vtip_ld), int(o_ld)
    a.layer, a.num_steps = int(layer), int(num_steps)
    return Call(lib.msdi_attention_decoupled, (C.byref(a),), name, keep=a, check=_lib_ipadapter.check)


# ---- the vision library (include/minsdtf_hip_vision.h, minsdtf_amd/_lib_vision.py) -------------------------------------------------
def patch_embed(*, pixels, w, cls, pos, gamma, beta, out, batch, scale, shift, w_ld, o_ld=_lib_vision.WIDTH, eps=1e-5,
                image=_lib_vision.IMAGE, patch=_lib_vision.PATCH, width=_lib_vision.WIDTH, name="patch_embed") -> Call:
    """msdv_patch_embed: pixels fp32 [batch][224][224][3] (0 .. 255) -> out bf16 [batch][257][o_ld], the input of layer 0 of the CLIP
    ViT-H/14 vision tower: x = bf16(fma(pixel, scale[c], shift[c])), the 14 x 14 / stride-14 patch product with w bf16 [1280][w_ld]
    (k = (ky * 14 + kx) * 3 + c, the columns >= 588 ignored), + pos fp32 [257][1280] (token 0: cls + pos[0]), LayerNorm(gamma, beta).
    scale / shift: three floats each (vision.pixel_affine)."""
    lib = _lib_vision.load()
    a = _lib_vision.MsdvPatchEmbed()
    a.pixels, a.w, a.cls, a.pos, a.gamma, a.beta, a.out = _p(pixels), _p(w), _p(cls), _p(pos), _p(gamma), _p(beta), _p(out)
    a.scale[:], a.shift[:] = [float(v) for v in scale], [float(v) for v in shift]
    a.eps = float(eps)
    a.batch, a.image, a.patch, a.width, a.w_ld, a.o_ld = int(batch), int(image), int(patch), int(width), int(w_ld), int(o_ld)
    return Call(lib.msdv_patch_embed, (C.byref(a),), name, keep=a, check=_lib_vision.check)


def gelu(*, x, out, rows, cols, ld_in=None, ld_out=None, name="gelu") -> Call:
    """msdv_gelu: out[r][:cols] = bf16(0.5 x (1 + erf(x / sqrt 2))), x fp32 [rows][ld_in], out bf16 [rows][ld_out]."""
    lib = _lib_vision.load()
    return Call(lib.msdv_gelu, (_p(x), _p(out), int(rows), int(cols), int(cols if ld_in is None else ld_in),
                                int(cols if ld_out is None else ld_out)), name, check=_lib_vision.check)


def pool_project(*, x, gamma, beta, w, out, batch, x_stride, w_layout=0, eps=1e-5, width=_lib_vision.WIDTH, proj=_lib_vision.PROJ,
                 name="pool_project") -> Call:
    """msdv_pool_project: out fp32 [batch][1024] = LayerNorm(x[b]) w^T, x bf16 rows of 1280 at a stride of x_stride elements (the
    class token of the last layer), w bf16 [1024][1280] rows (w_layout 0) or their chunk-major image (1); no bias."""
    lib = _lib_vision.load()
    a = _lib_vision.MsdvPoolProject()
    a.x, a.gamma, a.beta, a.w, a.out = _p(x), _p(gamma), _p(beta), _p(w), _p(out)
    a.x_stride, a.eps = int(x_stride), float(eps)
    a.batch, a.width, a.proj, a.w_layout = int(batch), int(width), int(proj), int(w_layout)
    return Call(lib.msdv_pool_project, (C.byref(a),), name, keep=a, check=_lib_vision.check)


# ---- the resampler library (include/minsdtf_hip_resampler.h, minsdtf_amd/_lib_resampler.py) ----------------------------------------
def perceiver_attention(*, q, k_x, vt_x, k_l, vt_l, out, batch, heads, n, t_x, q_ld, kx_ld, vtx_ld, kl_ld, vtl_ld, o_ld, scale,
                        head_dim=_lib_resampler.HEAD_DIM, name="perceiver_attention") -> Call:
    """msdr_perceiver_attention: out bf16 [batch][n][o_ld] = softmax2(scale * q [k_x ; k_l]^T) [v_x ; v_l] per head of 64, one softmax
    over the t_x + n keys of both segments (x keys first), the V operands transposed ([batch][heads * 64][ld], keys contiguous).
    `scale` carries log2(e): the kernel takes exp2."""
    lib = _lib_resampler.load()
    a = _lib_resampler.MsdrPerceiverAttention()
    a.q, a.k_x, a.vt_x, a.k_l, a.vt_l, a.out = _p(q), _p(k_x), _p(vt_x), _p(k_l), _p(vt_l), _p(out)
    a.scale = float(scale)
    a.batch, a.heads, a.head_dim, a.n, a.t_x = int(batch), int(heads), int(head_dim), int(n), int(t_x)
    a.q_ld, a.kx_ld, a.vtx_ld, a.kl_ld, a.vtl_ld, a.o_ld = int(q_ld), int(kx_ld), int(vtx_ld), int(kl_ld), int(vtl_ld), int(o_ld)
    return Call(lib.msdr_perceiver_attention, (C.byref(a),), name, keep=a, check=_lib_resampler.check)


# ---- the T2I-Adapter library (include/minsdtf_hip_t2i.h, minsdtf_amd/_lib_t2i.py) ---------------------------------------------------
def feature_add(*, x, feats, scales, rows, n, site, num_steps, step_ptr=None, name="feature_add") -> Call:
    """msda_feature_add: x[r] = bf16(fp32(x[r]) + sum_u s_u * feats[u]) for every row r, one fmaf per unit in unit order, a unit at
    scale 0 not read, s_u = scales[*step_ptr][u][site] (minsdtf_amd/t2iadapter.py).  x bf16 [rows][n] (in place); feats: 1 .. 3 bf16
    [n]; scales fp32 [num_steps][len(feats)][4]."""
    lib = _lib_t2i.load()
    if not 1 <= len(feats) <= _lib_t2i.MAX_UNITS:
        raise ValueError(f"feature_add: {len(feats)} features (1 .. {_lib_t2i.MAX_UNITS} units)")
    a = _lib_t2i.MsdaFeatureAdd()
    a.x, a.scales, a.step_ptr = _p(x), _p(scales), _p(step_ptr)
    for u, f in enumerate(feats):
        a.feat[u] = _p(f)
    a.rows, a.n, a.units, a.site, a.num_steps = int(rows), int(n), len(feats), int(site), int(num_steps)
    return Call(lib.msda_feature_add, (C.byref(a),), name, keep=a, check=_lib_t2i.check)


def unshuffle(*, x, out, batch, h, w, cin, name="unshuffle") -> Call:
    """msda_unshuffle: PixelUnshuffle(8), x fp32 [batch][h][w][cin] -> out bf16 [batch][h / 8][w / 8][64 cin], channel
    c * 64 + dy * 8 + dx: the one rounding of the picture."""
    lib = _lib_t2i.load()
    return Call(lib.msda_unshuffle, (_p(x), _p(out), int(batch), int(h), int(w), int(cin)), name, check=_lib_t2i.check)


def relu(*, x, n, name="relu") -> Call:
    """msda_relu: x = max(x, +0) over n bf16 elements in place (-0 becomes +0, a NaN keeps its bits)."""
    lib = _lib_t2i.load()
    return Call(lib.msda_relu, (_p(x), int(n)), name, check=_lib_t2i.check)


def avgpool2(*, x, out, batch, h, w, c, name="avgpool2") -> Call:
    """msda_avgpool2: AvgPool2d(2, 2), x bf16 [batch][h][w][c] -> out bf16 [batch][h / 2][w / 2][c], ((a00 + a01) + (a10 + a11)) *
    0.25 in fp32, one rounding."""
    lib = _lib_t2i.load()
    return Call(lib.msda_avgpool2, (_p(x), _p(out), int(batch), int(h), int(w), int(c)), name, check=_lib_t2i.check)


def add_bf16(*, a, b, out, n, name="add_bf16") -> Call:
    lib = _lib.load()
    return Call(lib.msd_add_bf16, (_p(a), _p(b), _p(out), n), name)


def add_f32_bf16(*, a, b, out, n, name="add_f32_bf16") -> Call:
    lib = _lib.load()
    return Call(lib.msd_add_f32_bf16, (_p(a), _p(b), _p(out), n), name)


def cast_f32_to_bf16(*, x, out, n, name="cast_f2b") -> Call:
    lib = _lib.load()
    return Call(lib.msd_cast_f32_to_bf16, (_p(x), _p(out), n), name)


def cast_bf16_to_f32(*, x, out, n, name="cast_b2f") -> Call:
    lib = _lib.load()
    return Call(lib.msd_cast_bf16_to_f32, (_p(x), _p(out), n), name)


def embedding_sum(*, tokens, positions, tok_table, pos_table, out, rows, dim, vocab, max_len, status=None,
                  name="embedding_sum") -> Call:
    lib = _lib.load()
    return Call(lib.msd_embedding_sum, (_p(tokens), _p(positions), _p(tok_table), _p(pos_table), _p(out), rows, dim, vocab, max_len,
                                        _p(status)), name)


def replicate(*, src, dst, nbytes, copies, name="replicate") -> Call:
    """dst = `copies` replicas of src's nbytes back to back (src may be dst: replica 0 in place)."""
    lib = _lib.load()
    return Call(lib.msd_replicate, (_p(src), _p(dst), int(nbytes), int(copies)), name)


def memset_zero(*, ptr, nbytes, name="memset") -> Call:
    lib = _lib.load()
    return Call(lib.msd_memset_zero, (_p(ptr), nbytes), name)


LORA_LAYOUT_ROWS, LORA_LAYOUT_CHUNK, LORA_LAYOUT_T = 0, 1, 2   # MsdLoraJob.layout


def lora_job(*, master, out, n, k, out_rows, out_cols, up=None, down=None, rank=0, master_ld=None, rowscale=None, colscale=None,
             rowmap=None, out_frag=None, colsum=None, layout=LORA_LAYOUT_ROWS, out_dtype=OUT_BF16, ld=None, row_off=0,
             col_off=0) -> _lib.MsdLoraJob:
    """One msd_lora_merge job descriptor (include/minsdtf_hip.h); first_block is filled by lora_merge."""
    j = _lib.MsdLoraJob()
    j.master, j.up, j.down = _p(master), _p(up), _p(down)
    j.rowscale, j.colscale, j.rowmap = _p(rowscale), _p(colscale), _p(rowmap)
    j.out, j.out_frag, j.colsum = _p(out), _p(out_frag), _p(colsum)
    j.n, j.k, j.rank = int(n), int(k), int(rank)
    j.master_ld = int(k if master_ld is None else master_ld)
    j.layout, j.out_dtype = int(layout), int(out_dtype)
    j.ld = int(out_cols if ld is None else ld)
    j.out_rows, j.out_cols, j.row_off, j.col_off = int(out_rows), int(out_cols), int(row_off), int(col_off)
    return j


def lora_merge(jobs, device, name="lora_merge") -> Call:
    """One grouped msd_lora_merge launch over `jobs` (lora_job records): the host array is validated by the library, a device
    copy (kept alive by the returned Call) is what the kernel reads."""
    import torch

    lib = _lib.load()
    arr = (_lib.MsdLoraJob * len(jobs))()
    first = 0
    for i, j in enumerate(jobs):
        arr[i] = j
        arr[i].first_block = first
        first += (j.n + _lib.LORA_ROWS_PER_BLOCK - 1) // _lib.LORA_ROWS_PER_BLOCK
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8) if jobs else torch.zeros(0, dtype=torch.uint8)
    dev = host.to(device) if jobs else None
    s = _lib.MsdLoraMerge()
    s.jobs, s.jobs_dev, s.num_jobs = C.addressof(arr), _p(dev), len(jobs)
    return Call(lib.msd_lora_merge, (C.byref(s),), name, keep=(arr, dev, s))
