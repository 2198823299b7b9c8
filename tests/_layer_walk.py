"""The tensor-less walk of the launch plans, shared by the CPU and GPU tests (and by tools/tune_conv.py): every
msd_conv_gemm launch the emitters record for a network at a latent size, with what decides its arithmetic and code path.

The walk hooks engine.Plan.rec and leaves tuning.lookup in place, so a record holds the configuration the engine really
chose (table row, nearest measured batch, or tuning.shape_config), the epilogue it asked for and the weight layout it would
read.  Nothing is launched; ops.conv_gemm_ln_slots loads the built library (LayerNorm-fold producers ask it for their slot
count).  The same walk keeps the other launch families of a default job - msd_group_norm, msd_attention, msd_cross_attention_q,
msd_conv_direct, msd_layer_norm - for tests/test_layer_launches_gpu.py (walk_families, family_cases).  Not a conftest: plain
helpers, imported by name."""
import collections

# what one recorded ops.conv_gemm call keeps.  Presence flags are booleans; split = the q|k|v^T / k|v^T epilogue (ns0, ns1 its
# column counts); ln_in_slots / ln_out_slots = row-moment partials per row read / written (0: none)
Launch = collections.namedtuple("Launch", [
    "name", "batch", "h_in", "w_in", "c0", "c1", "N", "ksize", "stride", "upsample", "pad", "pad_end", "c2", "c3",
    "tile_m", "tile_n", "splitk", "stages", "w_layout",
    "act", "out_dtype", "bias", "residual", "rowvec", "step_ptr", "ln_in", "ln_in_slots", "ln_out", "ln_out_slots", "split", "ns0", "ns1"])

# a layer signature: the launch without its batch, its configuration and its name
SIG_FIELDS = ("h_in", "w_in", "c0", "c1", "N", "ksize", "stride", "upsample", "pad", "pad_end", "c2", "c3",
              "act", "out_dtype", "bias", "residual", "rowvec", "step_ptr", "ln_in", "ln_out", "split", "ns0", "ns1")
Sig = collections.namedtuple("Sig", SIG_FIELDS)

# (network, fused batch, latent height, latent width).  TUNED: what tools/tune_conv.py measures and BASELINE.md benchmarks, in the tuner's order
TUNED_WALKS = (("unet", 2, 64, 64), ("vae", 1, 64, 64), ("unet", 4, 64, 64), ("unet", 8, 64, 64), ("unet", 2, 96, 96), ("unet", 1, 64, 64),
               ("vae", 4, 64, 64), ("vae", 1, 96, 96), ("controlnet", 2, 64, 64), ("vae_enc", 1, 64, 64))
# ... plus the 96 x 96 UNet at fused batch 1 (nearest-batch / shape_config), fused batches 6 and 10 at 64 x 64 (nearest batch with
# its is_big / 256-row rewrites) and the 80 x 80 UNet at fused batch 2 (no table row at all: shape_config)
ALL_WALKS = TUNED_WALKS + (("unet", 1, 96, 96), ("unet", 6, 64, 64), ("unet", 10, 64, 64), ("unet", 2, 80, 80))


class _Tensor:
    """Stands in for a device tensor / buffer while walking the topology."""
    ptr = 0

    def at(self, off):
        return self


class _AnyWeights(dict):
    """Every weight "exists" (so the folded layer forms are the ones walked), none is real.  layout / fragment_major as
    packing.PackedWeights has them: the models keep every MFMA matrix chunk-major and hand the wreg form a fragment-major copy."""

    def __contains__(self, k):
        return True

    def __missing__(self, k):
        return _Tensor()

    def layout(self, key):
        from minsdtf_amd import engine

        return 1 if engine.W_CHUNK_MAJOR else 0

    def fragment_major(self, key):
        return _Tensor()


def _launch(kw):
    pad = kw.get("pad")
    pad = (1 if kw.get("ksize", 1) == 3 else 0) if pad is None else pad
    pad_end = kw.get("pad_end")
    split = kw.get("split")
    return Launch(name=kw.get("name", ""), batch=kw["batch"], h_in=kw["h_in"], w_in=kw["w_in"], c0=kw["c0"], c1=kw.get("c1", 0), N=kw["N"],
                  ksize=kw.get("ksize", 1), stride=kw.get("stride", 1), upsample=bool(kw.get("upsample", False)), pad=pad,
                  pad_end=pad if pad_end is None else pad_end, c2=kw.get("c2", 0), c3=kw.get("c3", 0),
                  tile_m=kw.get("tile_m", 0), tile_n=kw.get("tile_n", 0), splitk=kw.get("splitk", 1), stages=kw.get("stages", 0),
                  w_layout=kw.get("w_layout", 0), act=kw.get("act", 0), out_dtype=kw.get("out_dtype", 0),
                  bias=kw.get("bias") is not None, residual=kw.get("residual") is not None, rowvec=kw.get("rowvec") is not None,
                  step_ptr=kw.get("rowvec") is not None, ln_in=kw.get("ln_in") is not None, ln_in_slots=kw.get("ln_in_slots", 0),
                  ln_out=kw.get("ln_out") is not None, ln_out_slots=kw.get("ln_out_slots", 0), split=split is not None,
                  ns0=split[0] if split else 0, ns1=split[1] if split else 0)


# ---- the other launch families of a default job: what one recorded call keeps -------------------------------------------------------
# ops.group_norm.  sync: whether the caller lent its sync block (the cluster and the row-major forms run only then)
NormLaunch = collections.namedtuple("NormLaunch", ["name", "batch", "hw", "c0", "c1", "silu", "sync"])
# ops.attention.  workspace_floats: the d = 512 key-split scratch the engine lent (0: none)
AttnLaunch = collections.namedtuple("AttnLaunch", ["name", "batch", "heads", "head_dim", "s", "t", "q_ld", "k_ld", "vt_ld", "o_ld", "causal",
                                                   "q_prescaled", "workspace_floats", "scale"])
# ops.cross_attention_q.  ln_in_slots: the row-moment partials per row its producer left; w_layout: how the folded to_q weights lie
XattnLaunch = collections.namedtuple("XattnLaunch", ["name", "batch", "heads", "head_dim", "s", "t", "k_ld", "vt_ld", "o_ld", "ln_in_slots", "w_layout"])
# ops.conv_direct.  in_batch_mod: the input's rows (output row b reads input row b % in_batch_mod)
DirectLaunch = collections.namedtuple("DirectLaunch", ["name", "batch", "in_batch_mod", "h_in", "w_in", "c_in", "c_out", "ksize", "stride", "in_dtype",
                                                       "out_dtype", "act", "act_in", "in_scale", "bias", "residual"])
# ops.layer_norm as a launch of its own (the text encoder's; the UNet's LayerNorms are folded into their consumers)
LnLaunch = collections.namedtuple("LnLaunch", ["name", "batch", "rows", "c"])

FAMILIES = ("conv_gemm", "group_norm", "attention", "cross_attention_q", "conv_direct", "layer_norm")


def _norm_launch(kw):
    return NormLaunch(name=kw.get("name", ""), batch=kw["batch"], hw=kw["hw"], c0=kw["c0"], c1=kw.get("c1", 0), silu=bool(kw.get("silu", False)),
                      sync=kw.get("sync") is not None)


def _attn_launch(kw):
    return AttnLaunch(name=kw.get("name", ""), batch=kw["batch"], heads=kw["heads"], head_dim=kw["head_dim"], s=kw["s"], t=kw["t"], q_ld=kw["q_ld"],
                      k_ld=kw["k_ld"], vt_ld=kw["vt_ld"], o_ld=kw["o_ld"], causal=bool(kw.get("causal", False)),
                      q_prescaled=bool(kw.get("q_prescaled", False)),
                      workspace_floats=int(kw.get("workspace_floats", 0)) if kw.get("workspace") is not None else 0, scale=float(kw["scale"]))


def _xattn_launch(kw):
    return XattnLaunch(name=kw.get("name", ""), batch=kw["batch"], heads=kw["heads"], head_dim=kw["head_dim"], s=kw["s"], t=kw["t"], k_ld=kw["k_ld"],
                       vt_ld=kw["vt_ld"], o_ld=kw["o_ld"], ln_in_slots=kw["ln_in_slots"], w_layout=kw.get("w_layout", 0))


def _direct_launch(kw):
    from minsdtf_amd import ops

    mod = kw.get("in_batch_mod")
    return DirectLaunch(name=kw.get("name", ""), batch=kw["batch"], in_batch_mod=kw["batch"] if mod is None else mod, h_in=kw["h_in"], w_in=kw["w_in"],
                        c_in=kw["c_in"], c_out=kw["c_out"], ksize=kw.get("ksize", 3), stride=kw.get("stride", 1),
                        in_dtype=kw.get("in_dtype", ops.OUT_BF16), out_dtype=kw.get("out_dtype", ops.OUT_BF16), act=kw.get("act", ops.ACT_NONE),
                        act_in=bool(kw.get("act_in", False)), in_scale=float(kw.get("in_scale", 1.0)), bias=kw.get("bias") is not None,
                        residual=kw.get("residual") is not None)


def _ln_launch(kw, nb):
    return LnLaunch(name=kw.get("name", ""), batch=nb, rows=kw["rows"], c=kw["c"])


def walk_families(what, nb, h, w):
    """Every launch of the families above that the emitters record for `what` ("unet" | "controlnet" | "vae" | "vae_enc" | "text") at
    fused batch nb and latent size h x w (text: h tokens, w = 1), in recording order: {family: [records]}.  The decoder is walked
    with the uint8 output a default job asks of it (models.ImageDecoder.decode_to_uint8); no msd_conv_gemm record reads that."""
    from minsdtf_amd import engine, ops
    from minsdtf_amd import weights as wtab

    out = {f: [] for f in FAMILIES}
    orig = engine.Plan.rec

    def rec(self, fn, **kw):
        if fn is ops.conv_gemm:
            out["conv_gemm"].append(_launch(kw))
        elif fn is ops.group_norm:
            out["group_norm"].append(_norm_launch(kw))
        elif fn is ops.attention:
            out["attention"].append(_attn_launch(kw))
        elif fn is ops.cross_attention_q:
            out["cross_attention_q"].append(_xattn_launch(kw))
        elif fn is ops.conv_direct:
            out["conv_direct"].append(_direct_launch(kw))
        elif fn is ops.layer_norm:
            out["layer_norm"].append(_ln_launch(kw, nb))
        return orig(self, fn, **kw)

    engine.Plan.rec = rec
    try:
        p = engine.Plan("cpu")
        e = engine.Emitter(p, _AnyWeights())
        T = _Tensor
        if what in ("unet", "controlnet"):
            layers = engine.UNET_ATTN_LAYERS if what == "unet" else engine.ENCODER_ATTN_LAYERS
            ctx = engine.Act(p.alloc(nb * 77 * 768 * 2), nb, 77, 1, 768)
            kv = engine.emit_context_kv(e, ctx, layers, p)
            temb = (T(), 0, 0, engine.temb_columns(what == "controlnet"))
            if what == "unet":
                engine.emit_unet(e, T(), nb, nb, h, w, temb, kv, 77, T(), None)
            else:
                outs = [p.act(nb, h >> lv, w >> lv, ch) for lv, ch in zip((0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3), wtab.UNET_SKIP_CH + (1280,))]
                engine.emit_controlnet(e, T(), nb, nb, h, w, temb, kv, 77, p.act(nb, h, w, 320), outs)
        elif what == "vae":
            engine.emit_decoder(e, T(), nb, h, w, T(), ops.OUT_U8)
        elif what == "vae_enc":
            engine.emit_encoder(e, T(), nb, 8 * h, 8 * w, T())
        elif what == "text":
            engine.emit_text_encoder(e, p.act(nb, h, w, 768), 12)
        else:
            raise ValueError(what)
    finally:
        engine.Plan.rec = orig
    return out


def walk(what, nb, h, w):
    """Every ops.conv_gemm call the emitters record for `what` ("unet" | "controlnet" | "vae" | "vae_enc") at fused batch nb and
    latent size h x w, in recording order, as Launch records."""
    return walk_families(what, nb, h, w)["conv_gemm"]


def out_hw(l):
    hl, wl = (2 * l.h_in, 2 * l.w_in) if l.upsample else (l.h_in, l.w_in)
    return (hl + l.pad + l.pad_end - l.ksize) // l.stride + 1, (wl + l.pad + l.pad_end - l.ksize) // l.stride + 1


def lookup_args(l):
    """The arguments Emitter.conv handed tuning.lookup for this launch: (batch, h_in, w_in, cin, N, ksize, stride, upsample, M, nk,
    allow_split, cx)."""
    from minsdtf_amd import ops

    ho, wo = out_hw(l)
    cin, cx = l.c0 + l.c1, l.c2 + l.c3
    return (l.batch, l.h_in, l.w_in, cin, l.N, l.ksize, l.stride, l.upsample, l.batch * ho * wo, l.ksize * l.ksize * (cin // 64) + cx // 64,
            not (l.split or l.act == ops.ACT_GEGLU), cx)


def walk_shapes(nb, h, w, what="unet"):
    """The tuner's view of a walk: the tuning.lookup arguments of every launch that went through Emitter.conv."""
    return [lookup_args(l) for l in walk(what, nb, h, w) if l.tile_m or l.tile_n]


def shape_key(l):
    from minsdtf_amd import tuning

    a = lookup_args(l)
    return tuning.shape_key(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[10], a[11])


def signature(l):
    return Sig(*(getattr(l, f) for f in SIG_FIELDS))


def sig_id(s):
    """'64x64x640->320k3s1u0+x960 resid rowvec': the shape key without its batch, the operand boundaries where a tensor is a
    concat, then the epilogue."""
    from minsdtf_amd import ops, tuning

    key = tuning.shape_key(0, s.h_in, s.w_in, s.c0 + s.c1, s.N, s.ksize, s.stride, s.upsample, not (s.split or s.act == ops.ACT_GEGLU), s.c2 + s.c3)
    words = [key.split("x", 1)[1]]
    if s.c1:
        words.append(f"in{s.c0}|{s.c1}")
    if s.c3:
        words.append(f"sc{s.c2}|{s.c3}")
    if s.pad != (1 if s.ksize == 3 else 0) or s.pad_end != s.pad:
        words.append(f"pad{s.pad},{s.pad_end}")
    words += [n for n, on in (("bias", s.bias), ("resid", s.residual), ("rowvec", s.rowvec), ("ln_in", s.ln_in), ("ln_out", s.ln_out)) if on]
    if s.split:
        words.append(f"split{s.ns0}|{s.ns1}")
    act = {ops.ACT_NONE: None, ops.ACT_SILU: "silu", ops.ACT_GEGLU: "geglu", ops.ACT_QUICK_GELU: "quick_gelu"}[s.act]
    if act:
        words.append(act)
    if s.out_dtype == ops.OUT_F32:
        words.append("f32")
    return " ".join(words)


# Layer signatures over ALL_WALKS.  tests/test_layer_cases_cpu.py keeps this number equal to what the walk finds, tests/test_layer_shapes_gpu.py
# asserts that it ran this many cases: a signature the engine starts to record cannot stay untested unnoticed.
EXPECTED_CASES = 222

_cases = None


def cases(walks=ALL_WALKS):
    """{signature: {batch: [distinct Launch records, names dropped]}} over `walks`, in first-seen order: one GPU test case per key."""
    global _cases
    if walks is ALL_WALKS and _cases is not None:
        return _cases
    out = collections.OrderedDict()
    for (what, nb, h, w) in walks:
        for l in walk(what, nb, h, w):
            per = out.setdefault(signature(l), {}).setdefault(l.batch, [])
            l = l._replace(name="")
            if l not in per:
                per.append(l)
    if walks is ALL_WALKS:
        _cases = out
    return out


def config_is_built(cfg, shape):
    """The (tile_m, tile_n, stages) of a launch configuration names a kernel the library builds AND that takes this shape (the
    tuner's candidate filters, tools/tune_conv.py): the wreg / big / staged-halo forms fail the launch otherwise."""
    from minsdtf_amd import tuning as t

    bm, bn, sk, stg = cfg
    batch, h_in, w_in, cin, N, ks, stride, ups, M, nk, allow_split, cx = shape
    hl, wl = (2 * h_in, 2 * w_in) if ups else (h_in, w_in)
    key = (bm, bn, stg)
    form = t.form_of(bm, bn, stg)
    if t.is_halo(bm):
        return key in t.HALO_TILES and ks == 3 and stride == 1 and not ups and w_in % 16 == 0 and h_in % form.th == 0   # (round 6: with a shortcut operand too)
    if t.is_rowpanel(bm):
        return ks == 1 and stride == 1 and not ups and not cx and cin in t.ROWPANEL_ROWS and bm in t.ROWPANEL_ROWS[cin] and bn in t.ROWPANEL_COLS and N % bn == 0 and N % 32 == 0
    if t.is_wreg(bm):
        return key in t.WREG_TILES and N % 16 == 0 and not (bn > 64 and N <= 64) and (allow_split or t.wreg_nj(bm, bn, stg) % 2 == 0)
    if t.is_big(bm):
        ok = not (bn == 160 and (N % 160 or not allow_split)) and not (bn > 128 and N <= 128) and not (ks == 1 and allow_split and cin == N and not cx)
        if form.family == "bighalo":
            return ok and key in t.BIG_TILES_HALO_IMAGE and ks == 3 and stride == 1 and not (cx and ups) and hl % 16 == 0 and wl % 16 == 0 and M >= t.HALO_IMAGE_MIN_ROWS
        if form.chunk_major:
            return ok and key in t.BIG_TILES_CHUNK_MAJOR and ks == 3 and stride == 1 and not cx
        return ok and key in t.BIG_TILES
    if key not in t.TILES:
        return False
    if -(-N // bn) >= 256:   # column tiles travel in 8 bits of a packed launch argument (cg_hot_ok)
        return False
    return not (bm == 256 and M < 1024) and not (bn == 128 and N <= 64) and not (bn == 80 and (N % 80 or not allow_split)) and not (bn == 160 and (N % 160 or N < 1280))


# ---- signatures, ids and case lists of the other families (tests/test_layer_launches_gpu.py) -----------------------------------------
# A signature is the record without its batch and its name, and without what follows from the batch or from the producer's
# configuration: attention keeps the workspace PER SAMPLE (the engine lends 4 * batch * s * 514 floats), cross_attention_q leaves
# ln_in_slots and w_layout to the records (the producing GEMM's tile decides the slots, and the tile follows the batch), conv_direct
# keeps whether all output rows read the same input rows (in_batch_mod < batch) instead of the row count.
# The walks: ALL_WALKS plus the CLIP text transformer at one and two prompts (its causal d = 64 attention, its LayerNorm launches)
FAMILY_WALKS = ALL_WALKS + (("text", 1, 77, 1), ("text", 2, 77, 1))

NormSig = collections.namedtuple("NormSig", ["hw", "c0", "c1", "silu", "sync"])
AttnSig = collections.namedtuple("AttnSig", ["heads", "head_dim", "s", "t", "q_ld", "k_ld", "vt_ld", "o_ld", "causal", "q_prescaled",
                                             "workspace_per_sample", "scale"])
XattnSig = collections.namedtuple("XattnSig", ["heads", "head_dim", "s", "t", "k_ld", "vt_ld", "o_ld"])
DirectSig = collections.namedtuple("DirectSig", ["shared_input", "h_in", "w_in", "c_in", "c_out", "ksize", "stride", "in_dtype", "out_dtype", "act",
                                                 "act_in", "in_scale", "bias", "residual"])
LnSig = collections.namedtuple("LnSig", ["rows_per_sample", "c"])


def family_signature(family, l):
    if family == "conv_gemm":
        return signature(l)
    if family == "group_norm":
        return NormSig(l.hw, l.c0, l.c1, l.silu, l.sync)
    if family == "attention":
        assert l.workspace_floats % l.batch == 0
        return AttnSig(l.heads, l.head_dim, l.s, l.t, l.q_ld, l.k_ld, l.vt_ld, l.o_ld, l.causal, l.q_prescaled, l.workspace_floats // l.batch, l.scale)
    if family == "cross_attention_q":
        return XattnSig(l.heads, l.head_dim, l.s, l.t, l.k_ld, l.vt_ld, l.o_ld)
    if family == "conv_direct":
        return DirectSig(l.in_batch_mod != l.batch, l.h_in, l.w_in, l.c_in, l.c_out, l.ksize, l.stride, l.in_dtype, l.out_dtype, l.act, l.act_in,
                         l.in_scale, l.bias, l.residual)
    if family == "layer_norm":
        assert l.rows % l.batch == 0
        return LnSig(l.rows // l.batch, l.c)
    raise ValueError(family)


def family_id(family, s):
    """'gn 4096x640|320 silu', 'attn 8x40 s4096 t4096 vt4096 presc', 'xattn 8x40 s4096 t77 vt80', 'direct 64x64x4->320k3s1 f32->bf16 bias',
    'ln 77x768'."""
    from minsdtf_amd import ops

    if family == "conv_gemm":
        return sig_id(s)
    if family == "group_norm":
        words = [f"gn {s.hw}x{s.c0}" + (f"|{s.c1}" if s.c1 else "")] + [n for n, on in (("silu", s.silu), ("nosync", not s.sync)) if on]
    elif family == "attention":
        words = [f"attn {s.heads}x{s.head_dim} s{s.s} t{s.t} vt{s.vt_ld}"]
        if not (s.q_ld == s.k_ld == s.o_ld == s.heads * s.head_dim):
            words.append(f"ld{s.q_ld},{s.k_ld},{s.o_ld}")
        words += [n for n, on in (("causal", s.causal), ("presc", s.q_prescaled), ("ws", s.workspace_per_sample)) if on]
        if abs(s.scale - s.head_dim ** -0.5) > 1e-6 * s.scale:
            words.append(f"scale{s.scale:.6g}")
    elif family == "cross_attention_q":
        words = [f"xattn {s.heads}x{s.head_dim} s{s.s} t{s.t} vt{s.vt_ld}"]
        if not (s.k_ld == s.o_ld == s.heads * s.head_dim):
            words.append(f"ld{s.k_ld},{s.o_ld}")
    elif family == "conv_direct":
        dt = {ops.OUT_BF16: "bf16", ops.OUT_F32: "f32", ops.OUT_U8: "u8"}
        words = [f"direct {s.h_in}x{s.w_in}x{s.c_in}->{s.c_out}k{s.ksize}s{s.stride} {dt[s.in_dtype]}->{dt[s.out_dtype]}"]
        words += [n for n, on in (("bias", s.bias), ("resid", s.residual), ("shared_in", s.shared_input), ("act_in", s.act_in)) if on]
        if s.in_scale != 1.0:
            words.append(f"scale{s.in_scale:.6g}")
        act = {ops.ACT_NONE: None, ops.ACT_SILU: "silu", ops.ACT_QUICK_GELU: "quick_gelu"}[s.act]
        if act:
            words.append(act)
    elif family == "layer_norm":
        words = [f"ln {s.rows_per_sample}x{s.c}"]
    else:
        raise ValueError(family)
    return " ".join(words)


# Signatures per family over FAMILY_WALKS, kept like EXPECTED_CASES: tests/test_layer_cases_cpu.py holds them to what the walk finds,
# tests/test_layer_launches_gpu.py asserts that it ran this many cases of each.
EXPECTED_FAMILY_CASES = {"group_norm": 70, "attention": 21, "cross_attention_q": 6, "conv_direct": 12, "layer_norm": 1}

_family_cases = None


def family_cases(family=None, walks=FAMILY_WALKS):
    """{family: {signature: {batch: [distinct records, names dropped]}}} over `walks`, in first-seen order (or one family's dict): one
    GPU test case per signature.  "conv_gemm" is left to cases(): its list is ALL_WALKS', without the text transformer."""
    global _family_cases
    if walks is FAMILY_WALKS and _family_cases is not None:
        out = _family_cases
    else:
        out = {f: collections.OrderedDict() for f in FAMILIES if f != "conv_gemm"}
        for (what, nb, h, w) in walks:
            fam = walk_families(what, nb, h, w)
            for f in out:
                for l in fam[f]:
                    per = out[f].setdefault(family_signature(f, l), {}).setdefault(l.batch, [])
                    l = l._replace(name="")
                    if l not in per:
                        per.append(l)
        if walks is FAMILY_WALKS:
            _family_cases = out
    return out if family is None else out[family]


def cases_group_norm():
    return family_cases("group_norm")


def cases_attention():
    return family_cases("attention")


def cases_cross_attention_q():
    return family_cases("cross_attention_q")


def cases_conv_direct():
    return family_cases("conv_direct")


def cases_layer_norm():
    return family_cases("layer_norm")


# ---- the second walker: EVERY recorded launch with the state of its buffers (tests/test_plan_extents_cpu.py) -----------------------
# walk() above keeps what decides a conv launch's arithmetic; this one keeps, for every Plan.rec call of any op, the keyword
# arguments and - at the moment of the rec - where each Buf / BufView / Act operand lies and whether its Buf was already freed.
# Beyond ALL_WALKS: the CLIP text transformer (engine.emit_text_encoder), a UNet with perturbed-attention rows (msd_attention_identity
# next to msd_attention), the ControlNet's HintNet, and the UNet fed by ControlNet taps (zero convs with residual == out).
EXTENT_WALKS = ALL_WALKS + (("text", 1, 77, 1), ("text", 2, 77, 1), ("unet_pag", 3, 64, 64), ("hintnet", 2, 64, 64), ("unet_taps", 2, 64, 64))

# one operand of a recorded launch: the Buf's identity, the operand's first byte in the arena, the bytes from there to the end of its
# Buf, whether the Buf was freed when the launch was recorded; kind "buf" | "ws" | "gn_partials" | "gn_sync" | "gn_stats" (plan scratch,
# sized at finalize()) | "outside" (a _Tensor stand-in: weights and buffers handed in from outside the plan, no size known)
Operand = collections.namedtuple("Operand", ["kind", "buf", "offset", "avail", "freed"])
Rec = collections.namedtuple("Rec", ["op", "name", "kw", "operands"])


def _operand(v):
    from minsdtf_amd import engine

    if isinstance(v, engine.Act):
        v = v.buf
    if isinstance(v, engine.Buf):
        return Operand("buf", id(v), v.offset, v.nbytes, v.freed)
    if isinstance(v, engine.BufView):
        return Operand("buf", id(v.buf), v.buf.offset + v.off, v.buf.nbytes - v.off, v.buf.freed)
    if isinstance(v, engine._Lazy):
        return Operand("gn_stats", None, 0, 0, False)
    if isinstance(v, _Tensor):
        return Operand("outside", None, 0, 0, False)
    return None


def walk_all(what, nb, h, w):
    """Every Plan.rec call the emitters make for `what` at fused batch nb and latent size h x w, in recording order, as Rec records,
    and the Plan (not finalized: ws_floats, gn_batch, gn_slots are what finalize() would size the scratch by)."""
    from minsdtf_amd import engine
    from minsdtf_amd import weights as wtab

    out = []
    orig = engine.Plan.rec

    def rec(self, fn, **kw):
        ops_ = {}
        for k, v in kw.items():
            if k == "split" and v is not None:
                for part, item in (("out1", v[2]), ("out2", v[4])):
                    o = _operand(item)
                    if o is not None:
                        ops_[part] = o
                continue
            if k in ("workspace", "partials", "sync") and isinstance(v, engine._Lazy):
                ops_[k] = Operand({"workspace": "ws", "partials": "gn_partials", "sync": "gn_sync"}[k], None, 0, 0, False)
                continue
            o = _operand(v)
            if o is not None:
                ops_[k] = o
        out.append(Rec(fn.__name__, kw.get("name", ""), kw, ops_))
        return orig(self, fn, **kw)

    engine.Plan.rec = rec
    try:
        p = engine.Plan("cpu")
        e = engine.Emitter(p, _AnyWeights())
        T = _Tensor
        if what in ("unet", "controlnet", "unet_pag", "unet_taps"):
            layers = engine.ENCODER_ATTN_LAYERS if what == "controlnet" else engine.UNET_ATTN_LAYERS
            ctx = engine.Act(p.alloc(nb * 77 * 768 * 2), nb, 77, 1, 768)
            kv = engine.emit_context_kv(e, ctx, layers, p)
            temb = (T(), 0, 0, engine.temb_columns(what == "controlnet"))
            if what == "unet":
                engine.emit_unet(e, T(), nb, nb, h, w, temb, kv, 77, T(), None)
            elif what == "unet_pag":   # the last row perturbed, in a 64x64-level block, the mid block and an up block
                layers_ = (engine.PAG_LAYERS[1], "mid_block.attentions.0", engine.PAG_LAYERS[-1])
                engine.emit_unet(e, T(), 1, nb, h, w, temb, kv, 77, T(), None, variant=engine.UNetVariant(pag_layers=layers_, perturbed=1))
            elif what == "unet_taps":  # ControlNet features -> zero convs into the skips (residual == out)
                kv_c = engine.emit_context_kv(e, ctx, engine.ENCODER_ATTN_LAYERS, p)
                feats = engine.emit_controlnet_features(e, T(), nb // 2, nb, h, w, (T(), 0, 0, engine.temb_columns(True)), kv_c, 77,
                                                        p.act(nb, h, w, 320))
                engine.emit_unet(e, T(), nb // 2, nb, h, w, temb, kv, 77, T(), None, control_taps=(e, feats))
            else:
                outs = [p.act(nb, h >> lv, w >> lv, ch) for lv, ch in zip((0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3), wtab.UNET_SKIP_CH + (1280,))]
                engine.emit_controlnet(e, T(), nb, nb, h, w, temb, kv, 77, p.act(nb, h, w, 320), outs)
        elif what == "vae":
            engine.emit_decoder(e, T(), nb, h, w, T(), 0)
        elif what == "vae_enc":
            engine.emit_encoder(e, T(), nb, 8 * h, 8 * w, T())
        elif what == "text":
            engine.emit_text_encoder(e, p.act(nb, h, w, 768), 12)
        elif what == "hintnet":
            engine.emit_hintnet(e, T(), nb // 2, 8 * h, 8 * w, p.act(nb, h, w, 320), copies=2)
        else:
            raise ValueError(what)
    finally:
        engine.Plan.rec = orig
    return out, p
