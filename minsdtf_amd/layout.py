"""The packed weight image, described once: ``layout(specs, flags)`` lists every packed key and what it is made of.

Every launch plan reads the packed image ``model._W`` by key (engine.py), the host packer builds it at ``set_weights``
(``packing.pack``) and the LoRA switch rewrites it in place (``lora.MergeBase``).  Both execute this table, so a layer feeds
exactly the keys the table says.  This is the only place that matches layer names.

An entry (:class:`Packed`) is one packed key.  Its storage class is

* ``KERAS``: fp32, the Keras layout unchanged (a Dense as a 1x1 conv), for the convs / denses of the vector-FMA path;
* ``ROWS``:  bf16 ``[N][K]`` rows, K contiguous, ``k = (ky*kw + kx)*C_in + c``; stored chunk-major (``packing.chunk_major``) when
  ``chunk_major`` is set;
* ``VEC``:   fp32 vectors, derived as ``how`` says (the embedding tables, passed through, are of this class too).

The matrices are made of :class:`Part` blocks, one per source layer, in the order they are concatenated.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from .weights import UNET_HEADS   # CrossAttention(num_heads=8) everywhere in the UNet / ControlNet (diffusion_model.py:60-65)

KERAS, ROWS, VEC = "keras", "rows", "vec"


class Flags(NamedTuple):
    """The switches that change the image (engine.W_CHUNK_MAJOR, engine.MFMA_TEMB_PROJ)."""
    chunk_major: bool = True
    mfma_temb_proj: bool = True


# names whose convs / denses run on the fp32 vector-FMA path (channel counts below an MFMA tile)
DIRECT = {
    "conv_in", "conv_out", "time_embedding.linear_1", "time_embedding.linear_2",
    "post_quant_conv", "decoder.conv_in", "decoder.conv_out", "encoder.conv_in", "quant_conv",
} | {f"input_hint_block.{i}" for i in range(7)}

# first member of a group of projections stacked along the output axis -> (the members, the stacked name); the members have no
# packed matrix of their own
STACKS = {
    ".attn1.to_q": (("to_q", "to_k", "to_v"), "qkv"),              # diffusion_model.py:102-104: one GEMM feeds the attention kernel
    ".attn2.to_k": (("to_k", "to_v"), "kv"),
    ".query": (("query", "key", "value"), "qkv"),                  # VAE attention
    ".self_attn.q_proj": (("q_proj", "k_proj", "v_proj"), "qkv"),  # CLIP
}
_STACKED = tuple(first[: first.rindex(".") + 1] + m for first, (members, _) in STACKS.items() for m in members)

LATENT_SCALE = 0.18215   # image_encoder.py: split(x, 2)[0] * 0.18215


def q_prescale(c_out: int) -> np.float32:
    """Factor folded into the UNet's query projections (attn1.to_q, attn2.to_q) at pack time: the attention scale
    head_size**-0.5 (diffusion_model.py:105,123) times log2(e), so the attention kernel takes exp2 of q k^T directly
    (MsdAttention.q_prescaled).  Exact up to the bf16 rounding of the weights, which happens once either way."""
    return np.float32((c_out // UNET_HEADS) ** -0.5 * 1.4426950408889634)


@dataclass
class Part:
    """One source layer's block of a packed matrix: logical rows [0, N) -> destination rows row_off + (rowmap or identity),
    columns [0, K) -> col_off + k, values (W[n][k] * qscale) * colscale[k].  In a vector: that layer's bias, treated alike."""
    layer: str
    row_off: int = 0
    col_off: int = 0
    qscale: Optional[float] = None        # uniform row scale (the query prescale)
    colscale: Optional[str] = None        # packed key of the fp32 column scale (a LayerNorm gamma)
    rowmap: bool = False                  # GEGLU row order (packing.geglu_row_order)
    ffproj_top: bool = False              # the block is the float64 product of this layer (ff.net.2) and the next part's (proj_out)
    rows: Optional[int] = None            # only the first `rows` outputs of the layer


@dataclass
class Packed:
    key: str
    store: str                            # KERAS | ROWS | VEC
    shape: Tuple[int, ...]                # as packed; a chunk-major matrix's logical [N][K] (see stored_shape)
    parts: List[Part] = field(default_factory=list)
    # VEC: "bias" / "gamma" / "beta" / "embedding": the parts' arrays of that kind, concatenated; "bias_sum": their sum;
    # "ffproj_b": b2 Wp + bp in float64 (parts: ff.net.2, proj_out); "lncs" / "lnb": made with the .lnw matrix that names them
    # (lnb = W beta + the parts' bias)
    how: str = "w"
    chunk_major: bool = False
    norm: Optional[str] = None            # (.lnw) the LayerNorm folded in: its gamma is the parts' colscale
    colsum: Optional[str] = None          # (.lnw) the .lncs key: float64 row sums of this matrix's ROUNDED rows
    lnb: Optional[Tuple[str, str]] = None  # (.lnw) (the .lnb key, packed key of the LayerNorm beta)
    pad_k: Optional[int] = None           # (ROWS) stored row length when K is no multiple of 8: the columns K .. pad_k - 1 are zeros

    @property
    def dtype(self) -> str:
        return "bfloat16" if self.store == ROWS else "float32"

    @property
    def stored_shape(self) -> Tuple[int, ...]:
        if self.pad_k is not None:
            return (self.shape[0], self.pad_k)
        return (self.shape[1] // 64, self.shape[0], 64) if self.chunk_major else self.shape

    @property
    def sources(self) -> set:
        return {p.layer for p in self.parts}


def layout(specs, flags: Flags = Flags()) -> List[Packed]:
    """The packed image of the weight table `specs`, in table order (an entry stands where its first source layer does)."""
    shape = {(s.name, s.kind): tuple(s.shape) for s in specs}
    out: List[Packed] = []

    def nk(n):   # logical (N, K) of a conv / Dense
        s = shape.get((n, "conv_w"))
        return (s[3], s[0] * s[1] * s[2]) if s else shape[(n, "dense_w")][::-1]

    def rows(key, parts, **kw) -> Packed:
        n = max(p.row_off + nk(p.layer)[0] for p in parts)
        k = max(p.col_off + nk(p.layer)[1] for p in parts)
        # chunk-major: the bf16 matrices the MFMA kernels read (msd_conv_gemm, msd_cross_attention_q: every ROWS key is a *.w or
        # a *.lnw); a K that is no multiple of 64 stays in rows, the kernels take either layout
        out.append(Packed(key, ROWS, (n, k), parts, chunk_major=flags.chunk_major and k % 64 == 0, **kw))
        return out[-1]

    def keras(key, parts):
        conv = shape.get((parts[0].layer, "conv_w"))
        kh, kw, cin = conv[:3] if conv else (1, 1, shape[(parts[0].layer, "dense_w")][0])
        n = max(p.row_off + (p.rows or nk(p.layer)[0]) for p in parts)
        out.append(Packed(key, KERAS, (kh, kw, cin, n), parts))

    def vec(key, how, parts):
        kind = how if how in ("gamma", "beta") else "bias"
        n = sum(p.rows or shape[(p.layer, kind)][0] for p in (parts[:1] if how in ("bias_sum", "ffproj_b") else parts))
        out.append(Packed(key, VEC, (n,), parts, how=how))

    def fold(w_key, parts, norm, bias=()):
        """LayerNorm `norm` folded into the matrix that consumes it (engine.Emitter.attentions; packing.fold_layer_norm):
        <consumer>.lnw (bf16, gamma-folded), .lncs (row sums), .lnb (W beta + b)."""
        if (norm, "gamma") not in shape:
            return
        base = w_key[: -len(".w")]
        e = rows(base + ".lnw", [replace(p, colscale=norm + ".g") for p in parts], norm=norm, colsum=base + ".lncs",
                 lnb=(base + ".lnb", norm + ".b"))
        out.append(Packed(base + ".lncs", VEC, e.shape[:1], how="lncs"))
        out.append(Packed(base + ".lnb", VEC, e.shape[:1], list(bias), how="lnb"))

    tproj = [s.name for s in specs if s.kind == "dense_w" and s.name.endswith(".time_emb_proj")]
    for n in dict.fromkeys(s.name for s in specs):
        has = lambda kind, n=n: (n, kind) in shape  # noqa: E731
        if has("embedding"):   # the CLIP token / position tables: fp32, under the layer's own name
            out.append(Packed(n, VEC, shape[(n, "embedding")], [Part(n)], how="embedding"))
        elif has("gamma"):
            vec(n + ".g", "gamma", [Part(n)])
            vec(n + ".b", "beta", [Part(n)])
        elif n.endswith(".patch_embedding"):
            # the CLIP vision tower's 14 x 14 / stride-14 patch conv (no bias): K = 588 is no multiple of 8, and msdv_patch_embed
            # reads 16-byte fragments of a row: rows of 592, the four last columns zeros (the kernel ignores them anyway)
            e = rows(n + ".w", [Part(n)])
            e.pad_k = (e.shape[1] + 7) // 8 * 8
        elif n.endswith(".time_emb_proj"):
            # every ResBlock's projection of the time embedding as ONE matrix, in table order (engine.emit_time_embedding):
            # bf16 rows for the MFMA kernel, or the fp32 (1, 1, 1280, sum C_out) of the vector-FMA one
            if n == tproj[0]:
                parts, off = [], 0
                for m in tproj:
                    parts.append(Part(m, row_off=off))
                    off += nk(m)[0]
                (rows if flags.mfma_temb_proj else keras)("time_emb_proj_cat.w", parts)
                vec("time_emb_proj_cat.b", "bias", [Part(m) for m in tproj])
        elif n in DIRECT:
            keras(n + ".w", [Part(n)])
            vec(n + ".b", "bias", [Part(n)])
            if n == "conv_out" and has("conv_w") and shape[(n, "conv_w")][2] % 64 == 0:
                # 320 -> 4: K = 2880 fills MFMA tiles even though N does not; 48 -> ~15 us per step (engine.MFMA_CONV_OUT)
                rows(n + ".m.w", [Part(n)])
                vec(n + ".m.b", "bias", [Part(n)])
            if n == "quant_conv":
                # quant_conv (1x1, 8 -> 8) followed by "take the first 4 channels, times 0.18215" is one 8 -> 4 conv with
                # pre-scaled weights (exact: both steps are linear)
                keras(n + ".mean.w", [Part(n, rows=4, qscale=np.float32(LATENT_SCALE))])
                vec(n + ".mean.b", "bias", [Part(n, rows=4, qscale=np.float32(LATENT_SCALE))])
        elif n.endswith(".ff.net.0.proj"):
            # GEGLU (diffusion_model.py:142-153): the 8C projection rows interleaved in 16-wide x | gate groups
            parts = [Part(n, rowmap=True)]
            rows(n + ".w", parts)
            vec(n + ".b", "bias", parts)
            fold(n + ".w", parts, n[: -len(".ff.net.0.proj")] + ".norm3", bias=parts)
        elif n.endswith(".attn2.to_q"):
            parts = [Part(n, qscale=q_prescale(nk(n)[0]))]
            rows(n + ".w", parts)
            fold(n + ".w", parts, n[: -len(".attn2.to_q")] + ".norm2")
        elif n.endswith(tuple(STACKS)):
            first = next(f for f in STACKS if n.endswith(f))
            members, stacked = STACKS[first]
            base = n[: n.rindex(".") + 1]
            members = [base + m for m in members]
            unet = first == ".attn1.to_q"   # the UNet's self-attention: prescaled queries, norm1 folded in
            parts = [Part(m, row_off=i * nk(m)[0], qscale=q_prescale(nk(m)[0]) if unet and i == 0 else None)
                     for i, m in enumerate(members)]
            rows(base + stacked + ".w", parts)
            if (members[0], "bias") in shape:
                vec(base + stacked + ".b", "bias", [Part(m) for m in members])
            if unet:
                fold(base + stacked + ".w", parts, n[: -len(first)] + ".norm1")
        elif n.endswith(_STACKED):
            pass   # stacked above
        elif n.endswith(".attn.to_q") and (n[: -len("to_q")] + "to_kv", "dense_w") in shape:
            # the Resampler's PerceiverAttention (resampler.py): the latents' q | k | v as ONE GEMM, to_q stacked over to_kv; to_kv
            # keeps its own matrix below, which the x side reads
            kvn = n[: -len("to_q")] + "to_kv"
            rows(n[: -len("to_q")] + "qkv.w", [Part(n), Part(kvn, row_off=nk(n)[0])])
        else:
            rows(n + ".w", [Part(n)])
            if has("bias"):
                vec(n + ".b", "bias", [Part(n)])
            if n.endswith(".transformer_blocks.0.ff.net.2"):
                # ff.net.2 followed by proj_out (diffusion_model.py:146-147 and :66-67: two Dense layers with only the
                # residual add of t2 between them) as ONE GEMM over the channel concat [ff | t2]:
                #   proj_out(ff W2 + b2 + t2) = ff (W2 Wp) + t2 Wp + (b2 Wp + bp)        key <attentions>.ffproj
                att = n[: -len(".transformer_blocks.0.ff.net.2")]
                if (att + ".proj_out", "conv_w") in shape:
                    rows(att + ".ffproj.w", [Part(n, ffproj_top=True), Part(att + ".proj_out", col_off=nk(n)[1])])
                    vec(att + ".ffproj.b", "ffproj_b", [Part(n), Part(att + ".proj_out")])
            elif n.endswith(".conv2"):
                # ResBlock conv2 + conv_shortcut (diffusion_model.py:34-38,50) as one contraction:
                # W = [conv2 taps | shortcut], b = b2 + bs; for a 3x3 conv2 with a 1x1 shortcut whose C_in fills K chunks
                rb = n[: -len(".conv2")]
                sc = rb + ".conv_shortcut"
                w2, ws = shape.get((n, "conv_w")), shape.get((sc, "conv_w"))
                if w2 and ws and w2[0] == 3 and ws[0] == 1 and ws[2] % 64 == 0:
                    rows(rb + ".conv2sc.w", [Part(n), Part(sc, col_off=nk(n)[1])])
                    vec(rb + ".conv2sc.b", "bias_sum", [Part(n), Part(sc)])
    return out
