"""The bytes a launch may touch, restated from the struct comments of include/minsdtf_hip.h (not from the kernels).

One function per op of minsdtf_amd/ops.py that the engines record or the kernel tests call.  It takes the op's keyword
arguments with DIMENSIONS only: where ops.* takes a tensor / buffer, pass anything that is not None (its presence is all that
is read) or leave it out.  It returns {operand name: (bytes needed from the operand's base address, role)}, role "in", "out" or
"inout", for every operand that is present.  The operand names are the keyword names of ops.*; the parts of conv_gemm's `split`
tuple are "out1" and "out2".

A [rows][ld] operand that carries `cols` columns needs (rows - 1) * ld + cols elements: the unused columns of the last row are not
the operand's.  Where the header gives an operand whole rows (vt: [batch][heads * d][vt_ld]) the padding columns belong to it.

tests/_guard.py sizes the payload of every operand of a kernel test by these figures; tests/test_plan_extents_cpu.py checks them against
the Buf every recorded launch was handed.  Not a conftest: plain helpers, imported by name."""

ACT_GEGLU = 2                              # MSD_ACT_GEGLU: writes N / 2 columns
OUT_BF16, OUT_F32, OUT_U8 = 0, 1, 2        # MSD_OUT_*
GN_SYNC_WORDS_PER_SAMPLE = 16384           # MSD_GN_SYNC_WORDS_PER_SAMPLE
GN_MAX_CHUNKS = 1024                       # MSD_GN_MAX_CHUNKS
ESZ = {OUT_BF16: 2, OUT_F32: 4, OUT_U8: 1}


def _rows(rows, ld, cols, esz):
    return ((rows - 1) * ld + cols) * esz


def _put(d, kw, name, nbytes, role="in"):
    if kw.get(name) is not None:
        d[name] = (int(nbytes), role)


def conv_out_hw(*, h_in, w_in, ksize=1, stride=1, upsample=False, pad=None, pad_end=None, **_):
    pad = (1 if ksize == 3 else 0) if pad is None else pad
    pad_end = pad if pad_end is None else pad_end
    hl, wl = (2 * h_in, 2 * w_in) if upsample else (h_in, w_in)
    return (hl + pad + pad_end - ksize) // stride + 1, (wl + pad + pad_end - ksize) // stride + 1


def conv_gemm(*, rv_steps=1, **kw):
    """MsdConvGemm.  rv_steps: rows of the per-step row-vector table (the header indexes it with *step_ptr; its length is the
    caller's)."""
    batch, N = kw["batch"], kw["N"]
    c0, c1, c2, c3 = kw["c0"], kw.get("c1", 0) or 0, kw.get("c2", 0) or 0, kw.get("c3", 0) or 0
    ks = kw.get("ksize", 1)
    ho, wo = conv_out_hw(**kw)
    M = batch * ho * wo
    K = ks * ks * (c0 + c1) + c2 + c3
    n_out = N // 2 if kw.get("act", 0) == ACT_GEGLU else N
    esz = ESZ[kw.get("out_dtype", OUT_BF16)]
    split = kw.get("split")
    d = {}
    _put(d, kw, "a0", batch * kw["h_in"] * kw["w_in"] * c0 * 2)           # bf16 [batch][h_in][w_in][c0]
    _put(d, kw, "a1", batch * kw["h_in"] * kw["w_in"] * c1 * 2)
    _put(d, kw, "a2", M * c2 * 2)                                           # bf16 [batch][h_out][w_out][c2]
    _put(d, kw, "a3", M * c3 * 2)
    _put(d, kw, "w", N * K * 2)                                             # bf16 [N][K], whatever the storage order
    _put(d, kw, "bias", N * 4)
    _put(d, kw, "rowvec", ((rv_steps - 1) * kw.get("rv_step_stride", 0) + (batch - 1) * kw.get("rv_batch_stride", 0) + N) * 4)
    _put(d, kw, "step_ptr", 4)
    if kw.get("residual") is not None:
        res_ld = kw.get("res_ld") or n_out
        d["residual"] = (_rows(M, res_ld, n_out, 2), "in")                  # bf16 [M][res_ld]
    if split is not None:
        ns0, ns1, out1, out1_ld, out2, out2_ld = split
        out_ld = kw.get("out_ld") or max(ns0, 4)
        if ns0 and kw.get("out") is not None:
            d["out"] = (_rows(M, out_ld, ns0, 2), "out")
        if ns1 and out1 is not None:
            d["out1"] = (_rows(M, out1_ld, ns1, 2), "out")                  # bf16 [M][out1_ld]
        if out2 is not None:
            d["out2"] = (batch * (N - ns0 - ns1) * out2_ld * 2, "out")      # bf16 transposed [batch][N - ns0 - ns1][out2_ld]
    else:
        _put(d, kw, "out", _rows(M, kw.get("out_ld") or n_out, n_out, esz), "out")
    splitk = kw.get("splitk", 1)
    if splitk > 1:
        _put(d, kw, "workspace", splitk * M * N * 4, "inout")               # fp32 partial slabs
    _put(d, kw, "ln_in", M * kw.get("ln_in_slots", 0) * 8)                  # float2 [M][ln_in_slots]
    _put(d, kw, "ln_colsum", N * 4)
    _put(d, kw, "ln_out", M * kw.get("ln_out_slots", 0) * 8, "out")         # float2 [M][ln_out_slots]
    return d


def conv_direct(**kw):
    """MsdConvDirect: in [in_batch_mod][h_in][w_in][c_in], w fp32 [ksize][ksize][c_in][c_out]."""
    batch, ks, stride = kw["batch"], kw.get("ksize", 3), kw.get("stride", 1)
    pad = 1 if ks == 3 else 0
    ho, wo = (kw["h_in"] + 2 * pad - ks) // stride + 1, (kw["w_in"] + 2 * pad - ks) // stride + 1
    M = batch * ho * wo
    mod = kw.get("in_batch_mod") or batch
    d = {}
    _put(d, kw, "x", mod * kw["h_in"] * kw["w_in"] * kw["c_in"] * ESZ[kw.get("in_dtype", OUT_BF16)])
    _put(d, kw, "w", ks * ks * kw["c_in"] * kw["c_out"] * 4)
    _put(d, kw, "bias", kw["c_out"] * 4)
    _put(d, kw, "residual", M * kw["c_out"] * 2)
    _put(d, kw, "out", M * kw["c_out"] * ESZ[kw.get("out_dtype", OUT_BF16)], "out")
    return d


def group_norm(**kw):
    """MsdGroupNorm: stats fp32 [batch][32][2]; partials as many floats as the caller announces (batch * MSD_GN_MAX_CHUNKS * 64
    "is always enough"); sync batch * MSD_GN_SYNC_WORDS_PER_SAMPLE words."""
    batch, hw, c0, c1 = kw["batch"], kw["hw"], kw["c0"], kw.get("c1", 0) or 0
    d = {}
    _put(d, kw, "x0", batch * hw * c0 * 2)
    _put(d, kw, "x1", batch * hw * c1 * 2)
    _put(d, kw, "gamma", (c0 + c1) * 4)
    _put(d, kw, "beta", (c0 + c1) * 4)
    _put(d, kw, "stats", batch * 64 * 4, "out")
    pf = kw.get("partials_floats")
    _put(d, kw, "partials", (batch * GN_MAX_CHUNKS * 64 if pf is None else pf) * 4, "inout")
    _put(d, kw, "out", batch * hw * (c0 + c1) * 2, "out")
    sw = kw.get("sync_words")
    _put(d, kw, "sync", (batch * GN_SYNC_WORDS_PER_SAMPLE if sw is None else sw) * 4, "inout")
    return d


def layer_norm(**kw):
    rows, c = kw["rows"], kw["c"]
    d = {}
    _put(d, kw, "x", rows * c * 2)
    _put(d, kw, "gamma", c * 4)
    _put(d, kw, "beta", c * 4)
    _put(d, kw, "out", rows * c * 2, "out")
    return d


def attention_workspace_floats(batch, heads, s):
    """MsdAttention.workspace (head_dim 512): 4 * batch * heads * s * (512 + 2) floats."""
    return 4 * batch * heads * s * (512 + 2)


def attention(**kw):
    """MsdAttention: q / k / out are rows of a wider buffer (head block only), vt whole rows of vt_ld keys."""
    batch, heads, d_, s, t = kw["batch"], kw["heads"], kw["head_dim"], kw["s"], kw["t"]
    c = heads * d_
    d = {}
    _put(d, kw, "q", _rows(batch * s, kw["q_ld"], c, 2))
    _put(d, kw, "k", _rows(batch * t, kw["k_ld"], c, 2))
    _put(d, kw, "vt", batch * c * kw["vt_ld"] * 2)
    _put(d, kw, "out", _rows(batch * s, kw["o_ld"], c, 2), "out")
    if d_ == 512:
        _put(d, kw, "workspace", attention_workspace_floats(batch, heads, s) * 4, "inout")
    return d


def cross_attention_q(**kw):
    batch, heads, d_, s, t = kw["batch"], kw["heads"], kw["head_dim"], kw["s"], kw["t"]
    c = heads * d_
    d = {}
    _put(d, kw, "x", batch * s * c * 2)                                     # bf16 [batch * s][c]
    _put(d, kw, "ln_in", batch * s * kw["ln_in_slots"] * 8)
    _put(d, kw, "wq", c * c * 2)
    _put(d, kw, "ln_colsum", c * 4)
    _put(d, kw, "bias", c * 4)
    _put(d, kw, "k", _rows(batch * t, kw["k_ld"], c, 2))
    _put(d, kw, "vt", batch * c * kw["vt_ld"] * 2)
    _put(d, kw, "out", _rows(batch * s, kw["o_ld"], c, 2), "out")
    return d


def attention_identity(**kw):
    batch, ch, s = kw["batch"], kw["channels"], kw["s"]
    d = {}
    _put(d, kw, "vt", batch * ch * kw["vt_ld"] * 2)
    _put(d, kw, "out", _rows(batch * s, kw["o_ld"], ch, 2), "out")
    return d


def softmax_rows(**kw):
    d = {}
    _put(d, kw, "x", _rows(kw["rows"], kw["ld_in"], kw["cols"], 4))
    _put(d, kw, "out", _rows(kw["rows"], kw["ld_out"], kw["cols"], 2), "out")
    return d


def embedding_sum(**kw):
    rows, dim = kw["rows"], kw["dim"]
    d = {}
    _put(d, kw, "tokens", rows * 4)
    _put(d, kw, "positions", rows * 4)
    _put(d, kw, "tok_table", kw["vocab"] * dim * 4)
    _put(d, kw, "pos_table", kw["max_len"] * dim * 4)
    _put(d, kw, "out", rows * dim * 2, "out")
    _put(d, kw, "status", 4, "inout")
    return d


def replicate(**kw):
    d = {}
    _put(d, kw, "src", kw["nbytes"])
    _put(d, kw, "dst", kw["nbytes"] * kw["copies"], "out")
    return d


def memset_zero(**kw):
    return {"ptr": (int(kw["nbytes"]), "out")}


def add_bf16(**kw):
    n = kw["n"]
    return {"a": (n * 2, "in"), "b": (n * 2, "in"), "out": (n * 2, "out")}


def add_f32_bf16(**kw):
    n = kw["n"]
    return {"a": (n * 2, "in"), "b": (n * 4, "in"), "out": (n * 2, "out")}


def cast_f32_to_bf16(**kw):
    return {"x": (kw["n"] * 4, "in"), "out": (kw["n"] * 2, "out")}


def cast_bf16_to_f32(**kw):
    return {"x": (kw["n"] * 2, "in"), "out": (kw["n"] * 4, "out")}


def _step_common(d, kw, coef_cols):
    batch, n, steps = kw["batch"], kw["n"], kw["num_steps"]
    _put(d, kw, "eps", (2 * batch if kw["guidance"] > 0 else batch) * n * 4)
    _put(d, kw, "latent", batch * n * 4, "inout")
    _put(d, kw, "coef", steps * coef_cols * 4)
    _put(d, kw, "step_ptr", 8 if int(kw.get("advance", 1)) == 2 else 4, "inout")   # advance 2: {step, ticket}
    _put(d, kw, "inpaint_init", n * 4)
    _put(d, kw, "inpaint_noise", batch * n * 4)
    _put(d, kw, "inpaint_mask", n * 4)
    _put(d, kw, "step_noise", steps * batch * n * 4)


def cfg_step(**kw):
    d = {}
    _step_common(d, kw, 4)
    _put(d, kw, "noise_coef", kw["num_steps"] * 4)
    return d


def sampler_step(**kw):
    d = {}
    _step_common(d, kw, 8)
    _put(d, kw, "denoised_prev", kw["batch"] * kw["n"] * 4, "inout")
    return d


def latent_resample(**kw):
    batch = kw["batch"]
    d = {}
    _put(d, kw, "x", batch * kw["h_in"] * kw["w_in"] * 16)
    _put(d, kw, "out", batch * kw["h_out"] * kw["w_out"] * 16, "out")
    _put(d, kw, "noise", batch * kw["h_out"] * kw["w_out"] * 16)
    _put(d, kw, "wx", kw["w_out"] * 32)                                     # MsdResampleRow [w_out]
    _put(d, kw, "wy", kw["h_out"] * 32)
    return d


def tile_consensus(**kw):
    batch, views = kw["batch"], len(kw["ys"]) * len(kw["xs"])
    d = {}
    _put(d, kw, "tiles", batch * views * kw["th"] * kw["tw"] * 16, "inout")
    _put(d, kw, "canvas", batch * kw["H"] * kw["W"] * 16, "in" if kw.get("mode", 0) == 1 else "out")
    _put(d, kw, "wy", kw["th"] * 4)
    _put(d, kw, "wx", kw["tw"] * 4)
    return d


def region_combine(**kw):
    regions, batch, n = kw["regions"], kw["batch"], kw["n"]
    d = {}
    _put(d, kw, "eps", regions * batch * n * 4)
    _put(d, kw, "w", regions * (n // 4) * 4)
    _put(d, kw, "out", batch * n * 4, "out")
    return d


# by the name of the ops.* function
EXTENTS = {f.__name__: f for f in (
    conv_gemm, conv_direct, group_norm, layer_norm, attention, cross_attention_q, attention_identity, softmax_rows, embedding_sum,
    replicate, memset_zero, add_bf16, add_f32_bf16, cast_f32_to_bf16, cast_bf16_to_f32, cfg_step, sampler_step, latent_resample,
    tile_consensus, region_combine)}

# Operand pairs that may be ONE buffer, as the header declares them (everything else of a launch is disjoint):
# msd_replicate "src == dst: replica 0 stays where it is"; msd_add_f32_bf16 "may run in place, out == a"; msd_conv_gemm "residual == out"
# (the ControlNet zero convs); msd_region_combine "out: may be eps itself".  The latent of the step kernels is one inout operand.
IN_PLACE = {
    "replicate": {("src", "dst")},
    "add_f32_bf16": {("a", "out")},
    "conv_gemm": {("residual", "out")},
    "region_combine": {("eps", "out")},
    "cfg_step": {("latent", "latent")},
    "sampler_step": {("latent", "latent")},
}


def may_share(op, a, b):
    pairs = IN_PLACE.get(op, ())
    return (a, b) in pairs or (b, a) in pairs


def extents(op, **kw):
    return EXTENTS[op](**kw)
