"""IP-Adapter image prompts without a GPU: the description and its table, the checkpoint map, the host projection, the float64
statement of the launch, the C ABI of the fifth library, what the engines record, and every refusal."""
import ctypes
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

import _extents_ipadapter as XI
import _layer_walk as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 8   # latent rows / columns of the stand-in engines
EMB = np.linspace(-1.0, 1.0, 1024)


# ------------------------------------------------------------------------------------------------------------ parse / table
def test_parse_defaults_and_forms():
    from minsdtf_amd import ipadapter as ip

    assert ip.parse(None) is None
    s = ip.parse(dict(embeds=EMB))
    assert (s.weight, s.start, s.end, s.weight_type, s.path, s.model, s.tokens, s.image) == (1.0, 0.0, 1.0, "linear", None, None, None, None)
    assert s.embeds.shape == (1024,) and s.embeds.dtype == np.float64
    assert ip.parse(s).weight == 1.0 and ip.parse(ip.IPAdapterSpec(tokens=np.zeros((16, 768)))).tokens.shape == (16, 768)
    assert ip.parse(dict(embeds=EMB[None], weight=-0.5)).weight == -0.5
    assert ip.parse(dict(image="picture.png", path="a.bin")).image == "picture.png"
    t = ip.table(dict(embeds=EMB), 5)
    assert t.shape == (5, 16) and t.dtype == np.float32 and (t == 1.0).all()


@pytest.mark.parametrize("bad,word", [
    (dict(), "exactly one of"), (dict(embeds=EMB, tokens=np.zeros((4, 768))), "exactly one of"), (dict(embeds=EMB[:100]), "embeds"),
    (dict(embeds=np.full(1024, np.nan)), "embeds"), (dict(tokens=np.zeros((17, 768))), "tokens"), (dict(tokens=np.zeros((4, 512))), "tokens"),
    (dict(embeds=EMB, weight="much"), "weight"), (dict(embeds=EMB, weight=float("inf")), "weight"), (dict(embeds=EMB, weight=True), "weight"),
    (dict(embeds=EMB, start=-0.1), "start"), (dict(embeds=EMB, end=1.5), "end"), (dict(embeds=EMB, start=0.8, end=0.2), "start"),
    (dict(embeds=EMB, weight_type="strong"), "weight_type"), (dict(embeds=EMB, weight_type={"up_blocks.9.attentions.0": 1.0}), "unknown attention block"),
    (dict(embeds=EMB, weight_type={"mid_block.attentions.0": "x"}), "weight_type"), (dict(embeds=EMB, path="a", model=object()), "path"),
    (dict(embeds=EMB, path=3), "path"), (dict(embeds=EMB, scale=1.0), "unknown field"), (dict(embeds=EMB, negative_tokens=np.zeros((4, 768))), "negative_tokens"),
    (dict(tokens=np.zeros((4, 768)), negative_tokens=np.zeros((5, 768))), "negative_tokens"), ("linear", "expected"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_parse_value_errors(bad, word):
    from minsdtf_amd import ipadapter as ip

    with pytest.raises(ValueError, match=f"^ip_adapter.*{word}"):
        ip.parse(bad)
    with pytest.raises(ValueError, match="^ip_adapter: num_steps"):
        ip.table(dict(embeds=EMB), 0)


@pytest.mark.parametrize("steps", [1, 4, 25])
def test_table_takes_the_step_range_by_the_control_units_rule(steps):
    from minsdtf_amd import control, ipadapter as ip

    for start, end in ((0.0, 1.0), (0.0, 0.75), (0.3, 0.6), (0.5, 0.5), (0.0, 0.0), (1.0, 1.0), (0.2, 1.0)):
        t = ip.table(dict(embeds=EMB, weight=0.7, start=start, end=end), steps)
        c = control.table(dict(weight=0.7, start=start, end=end), steps)   # fp32 [steps][1][13][2]
        assert np.array_equal(t, np.repeat(c[:, 0, :1, 1], 16, axis=1)), (start, end)
    assert (ip.table(dict(embeds=EMB, end=0.75), 4)[:, 0] == [1, 1, 1, 0]).all()


def test_weight_types_name_blocks_of_pag_layers():
    from minsdtf_amd import ipadapter as ip
    from minsdtf_amd.engine import PAG_LAYERS

    assert len(PAG_LAYERS) == ip.LAYERS == 16
    lin, style, comp = (ip.table(dict(embeds=EMB, weight=2.0, weight_type=w), 2)[0] for w in ip.WEIGHT_TYPES)
    assert (lin == 2.0).all()
    assert [n for n, v in zip(PAG_LAYERS, style) if v] == [f"up_blocks.1.attentions.{r}" for r in range(3)] and set(style) == {0.0, 2.0}
    assert [n for n, v in zip(PAG_LAYERS, comp) if v] == ["down_blocks.2.attentions.1"] and comp.sum() == 2.0
    d = ip.table(dict(embeds=EMB, weight=2.0, weight_type={"mid_block.attentions.0": 0.5, "up_blocks.3.attentions.2": -1.0}), 3)
    want = np.zeros(16, dtype=np.float32)
    want[PAG_LAYERS.index("mid_block.attentions.0")], want[PAG_LAYERS.index("up_blocks.3.attentions.2")] = 1.0, -2.0
    assert np.array_equal(d, np.tile(want, (3, 1)))


# --------------------------------------------------------------------------------------------------------------- the loader
def _state(tokens=4, seed=1):
    from minsdtf_amd.models import IPAdapter

    return IPAdapter.synthetic_state(seed, tokens)


def _nested(state):
    return {"image_proj": {k[len("image_proj."):]: torch.from_numpy(v) for k, v in state.items() if k.startswith("image_proj.")},
            "ip_adapter": {k[len("ip_adapter."):]: torch.from_numpy(v) for k, v in state.items() if k.startswith("ip_adapter.")}}


@pytest.mark.parametrize("form", ["flat", "nested"])
def test_loader_maps_the_checkpoint_indices_to_the_layers(form):
    """Index i = 1, 3, .. 31 in diffusers' attn_processors order: the down blocks, then the UP blocks, then the mid block."""
    from minsdtf_amd import ipadapter as ip
    from minsdtf_amd.engine import PAG_LAYERS, UNET_ATTN_LAYERS

    st = _state()
    named = ip.read_state(st if form == "flat" else _nested(st))
    order = ([f"down_blocks.{l}.attentions.{r}" for l in range(3) for r in range(2)]
             + [f"up_blocks.{u}.attentions.{r}" for u in (1, 2, 3) for r in range(3)] + ["mid_block.attentions.0"])
    assert sorted(order) == sorted(PAG_LAYERS)
    width = {n[:-len(".transformer_blocks.0.attn2")]: c for n, c in UNET_ATTN_LAYERS}
    for j, blk in enumerate(order):
        for m in ("to_k_ip", "to_v_ip"):
            src = st[f"ip_adapter.{2 * j + 1}.{m}.weight"]
            assert src.shape == (width[blk], 768) and np.array_equal(named[f"{blk}.{m}"], src), (j, blk, m)
    assert np.array_equal(named["proj.weight"], st["image_proj.proj.weight"]) and named["norm.bias"].shape == (768,)


def test_loader_raises_on_a_swapped_pair_and_on_missing_or_odd_keys():
    from minsdtf_amd import ipadapter as ip

    st = _state()
    swapped = dict(st)
    swapped["ip_adapter.11.to_k_ip.weight"], swapped["ip_adapter.19.to_k_ip.weight"] = st["ip_adapter.19.to_k_ip.weight"], st["ip_adapter.11.to_k_ip.weight"]
    with pytest.raises(ValueError, match=r"^ip_adapter: ip_adapter\.11\.to_k_ip\.weight has shape \(640, 768\), down_blocks\.2\.attentions\.1 takes \(1280, 768\)"):
        ip.read_state(swapped)
    missing = {k: v for k, v in st.items() if k != "ip_adapter.31.to_v_ip.weight"}
    with pytest.raises(ValueError, match="^ip_adapter: the checkpoint has no 'ip_adapter.31.to_v_ip.weight'"):
        ip.read_state(missing)
    with pytest.raises(ValueError, match="^ip_adapter: unexpected checkpoint keys"):
        ip.read_state(dict(st, **{"ip_adapter.33.to_k_ip.weight": st["ip_adapter.31.to_k_ip.weight"]}))
    with pytest.raises(ValueError, match="^ip_adapter: image_proj.proj.weight has shape"):
        ip.read_state(dict(st, **{"image_proj.proj.weight": np.zeros((768, 1280), dtype=np.float32)}))
    with pytest.raises(ValueError, match="^ip_adapter: image_proj.norm.weight has shape"):
        ip.read_state(dict(st, **{"image_proj.norm.weight": np.zeros((1024,), dtype=np.float32)}))


def test_model_packs_k_then_v_rows_and_reads_a_file(tmp_path):
    from minsdtf_amd import engine
    from minsdtf_amd.models import IPAdapter

    st = _state(tokens=16, seed=4)
    path = str(tmp_path / "ip-adapter.bin")
    torch.save(_nested(st), path)
    m = IPAdapter(path=path, device=torch.device("cpu"))
    assert m.tokens == 16 and m.weights_version == 1 and len(m._W) == 16
    for j, name in ((0, "down_blocks.0.attentions.0"), (15, "mid_block.attentions.0"), (6, "up_blocks.1.attentions.0")):
        key = name + ".transformer_blocks.0.attn2.kv_ip.w"
        w = m._W[key]
        C = st[f"ip_adapter.{2 * j + 1}.to_k_ip.weight"].shape[0]
        if m._W.layout(key) == 1:   # chunk-major [K/64][N][64] -> [N][K]
            w = w.permute(1, 0, 2).reshape(2 * C, 768)
        assert m._W.layout(key) == (1 if engine.W_CHUNK_MAJOR else 0) and w.dtype == torch.bfloat16
        want = np.concatenate([st[f"ip_adapter.{2 * j + 1}.to_k_ip.weight"], st[f"ip_adapter.{2 * j + 1}.to_v_ip.weight"]], axis=0)
        assert torch.equal(w, torch.from_numpy(want).to(torch.bfloat16)), name
    with pytest.raises(ValueError, match="^ip_adapter: checkpoint .* not found"):
        IPAdapter(path=str(tmp_path / "none.bin"), device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="no weights set"):
        IPAdapter(4, device=torch.device("cpu"))._require_weights()


def test_projection_against_torch_float64():
    from minsdtf_amd.models import IPAdapter

    for tokens in (4, 16):
        st = _state(tokens, seed=7)
        m = IPAdapter(tokens, device=torch.device("cpu"))
        m.set_state(st)
        lin, norm = torch.nn.Linear(1024, tokens * 768).double(), torch.nn.LayerNorm(768).double()
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(st["image_proj.proj.weight"]))
            lin.bias.copy_(torch.from_numpy(st["image_proj.proj.bias"]))
            norm.weight.copy_(torch.from_numpy(st["image_proj.norm.weight"]))
            norm.bias.copy_(torch.from_numpy(st["image_proj.norm.bias"]))
            for e in (EMB, np.zeros(1024)):
                want = norm(lin(torch.from_numpy(e)).reshape(tokens, 768)).numpy()
                got = m.project(e)
                assert got.dtype == np.float32 and got.shape == (tokens, 768)
                assert np.abs(got - want).max() <= 2.0 ** -22 * max(1.0, np.abs(want).max())


def test_unconditional_rows_get_the_zero_embeddings_tokens():
    from minsdtf_amd.models import IPAdapter
    from minsdtf_amd.stable_diffusion import StableDiffusionBase
    from minsdtf_amd import ipadapter as ip

    m = IPAdapter.synthetic(2, 4, device=torch.device("cpu"))
    sd = StableDiffusionBase(64, 64)
    model, (tok_u, tok_c) = sd._ip_inputs(ip.parse(dict(embeds=EMB, model=m)))
    assert model is m and np.array_equal(tok_u, m.project(np.zeros(1024))) and np.array_equal(tok_c, m.project(EMB))
    assert not np.array_equal(tok_u, tok_c)
    # `tokens` bypasses the projection; its negative defaults to zeros
    t = np.random.default_rng(0).standard_normal((4, 768))
    _m, (tu, tc) = sd._ip_inputs(ip.parse(dict(tokens=t, model=m)))
    assert np.array_equal(tc, t.astype(np.float32)) and not tu.any()
    # `image` goes through the pipeline's encoder, and says what works without one
    with pytest.raises(ValueError, match="^ip_adapter: `image` needs StableDiffusion.image_prompt_encoder.*`embeds`.*`tokens`"):
        sd._ip_inputs(ip.parse(dict(image=np.zeros((8, 8, 3)), model=m)))
    sd.image_prompt_encoder = lambda picture: EMB.astype(np.float32)
    _m, (_tu, tc2) = sd._ip_inputs(ip.parse(dict(image=np.zeros((8, 8, 3)), model=m)))
    assert np.array_equal(tc2, m.project(EMB.astype(np.float32)))
    with pytest.raises(ValueError, match="^ip_adapter: 16 `tokens`, the adapter takes 4"):
        sd._ip_inputs(ip.parse(dict(tokens=np.zeros((16, 768)), model=m)))
    with pytest.raises(ValueError, match="^ip_adapter: one of `path`"):
        sd._ip_inputs(ip.parse(dict(embeds=EMB)))


# ---------------------------------------------------------------------------------------------------- the float64 statement
def test_attention_reference_against_two_torch_softmaxes():
    from minsdtf_amd import ipadapter as ip

    gen = torch.Generator().manual_seed(0)
    B, H, d, S, T, N = 2, 2, 40, 9, 13, 4
    C = H * d
    q, k, v = (torch.randn(B, n, C, generator=gen, dtype=torch.float64) for n in (S, T, T))
    k_ip, v_ip = (torch.randn(B, N, C, generator=gen, dtype=torch.float64) for _ in range(2))
    q = q * (d ** -0.5 * 1.4426950408889634)

    def attn(kk, vv):
        qh, kh, vh = (x.view(B, -1, H, d).permute(0, 2, 1, 3) for x in (q, kk, vv))
        return (torch.softmax(qh @ kh.transpose(-1, -2) * np.log(2.0), -1) @ vh).permute(0, 2, 1, 3).reshape(B, S, C)

    for s in (1.0, -0.4, 2.5):
        got = ip.attention_reference(q.numpy(), k.numpy(), v.numpy(), k_ip.numpy(), v_ip.numpy(), s, H)
        assert np.abs(got - (attn(k, v) + s * attn(k_ip, v_ip)).numpy()).max() < 1e-12
    nan = np.full((B, N, C), np.nan)
    zero = ip.attention_reference(q.numpy(), k.numpy(), v.numpy(), nan, nan, 0.0, H)
    text = ip.attention_reference(q.numpy(), k.numpy(), v.numpy(), k_ip.numpy(), v_ip.numpy() * 0.0, 1.0, H)
    assert np.array_equal(zero, text) and np.abs(zero - attn(k, v).numpy()).max() < 1e-12


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_library_exports_its_header_and_the_others_are_untouched():
    from minsdtf_amd import _lib, _lib_control, _lib_dynthresh, _lib_ext, _lib_ipadapter

    assert os.path.exists(_lib_ipadapter.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    header = open(os.path.join(ROOT, "include", "minsdtf_hip_ipadapter.h")).read()
    declared = set(re.findall(r"^MSDI_API\s+(?:int|const char\*)\s+(msdi_\w+)\s*\(", header, flags=re.M))
    assert declared == set(_lib_ipadapter.SYMBOLS) == {"msdi_abi_version", "msdi_last_error", "msdi_attention_decoupled"}
    assert not re.search(r"^(?:int|const char\*)\s+msdi_\w+\s*\(", header, flags=re.M), "a declaration without MSDI_API"
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib_ipadapter.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert exported == declared, sorted(exported ^ declared)
    lib = _lib_ipadapter.load()
    assert lib.msdi_abi_version() == _lib_ipadapter.ABI_VERSION == int(re.search(r"#define MSDI_ABI_VERSION (\d+)", header).group(1))
    for name, value in (("MSDI_LAYERS", _lib_ipadapter.LAYERS), ("MSDI_KEYS", _lib_ipadapter.KEYS), ("MSDI_MAX_TOKENS", _lib_ipadapter.MAX_TOKENS)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value
    emap = open(os.path.join(ROOT, "minsdtf_amd", "csrc", "ipadapter", "exports_ipadapter.map")).read()
    assert set(re.findall(r"\b(msdi_\w+);", emap)) == declared and "*;" in emap and "msdi_*" not in emap
    counts = {}
    for other in (_lib, _lib_ext, _lib_dynthresh, _lib_control):
        table = subprocess.check_output(["nm", "-D", "--defined-only", other.LIB_PATH], text=True)
        assert "msdi_" not in table and not any(n.startswith("msdi_") for n in other.SYMBOLS)
        counts[other.LIB_NAME] = len([ln for ln in table.splitlines() if ln.strip()])
    assert list(counts.values()) == [31, 4, 3, 3], counts


def test_struct_layout_matches_the_header():
    from minsdtf_amd import _lib_ipadapter

    cls, struct = _lib_ipadapter.MsdiAttentionDecoupled, "MsdiAttentionDecoupled"
    fields = [n for n, _t in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "minsdtf_hip_ipadapter.h"\nint main(){printf("%zu", sizeof(' + struct + '));' + \
        "".join(f'printf(" %zu", offsetof({struct}, {f}));' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]


BASE = 1 << 24   # (addresses are only compared and checked for alignment: every bad call returns before a launch)
GOOD = dict(q=BASE, k=2 * BASE, vt=3 * BASE, k_ip=4 * BASE, vt_ip=5 * BASE, out=6 * BASE, scales=7 * BASE, step_ptr=8 * BASE, batch=2, heads=8,
            head_dim=40, s=64, t=77, n=4, q_ld=320, k_ld=320, vt_ld=80, kip_ld=320, vtip_ld=8, o_ld=320, layer=3, num_steps=4)
BAD = [dict(q=None), dict(k_ip=None), dict(vt_ip=None), dict(scales=None), dict(out=None), dict(q=BASE + 8), dict(vt_ip=5 * BASE + 2),
       dict(step_ptr=8 * BASE + 2), dict(head_dim=64), dict(t=0), dict(t=97), dict(n=0), dict(n=17), dict(t=81, vt_ld=88, n=16, vtip_ld=16),
       dict(t=96, vt_ld=96, n=1), dict(batch=0), dict(batch=65536), dict(heads=0), dict(s=0), dict(layer=-1), dict(layer=16), dict(num_steps=0),
       dict(q_ld=324), dict(vtip_ld=4), dict(q_ld=312), dict(kip_ld=312), dict(o_ld=312), dict(vt_ld=72), dict(vtip_ld=0), dict(n=16),
       dict(out=BASE), dict(out=4 * BASE), dict(out=5 * BASE), dict(out=7 * BASE), dict(out=8 * BASE - 16)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_argument_errors_without_a_device(bad):
    from minsdtf_amd import _lib_ipadapter, ops

    lib = _lib_ipadapter.load()
    call = ops.ip_attention(**dict(GOOD, **bad))
    assert call.name == "ip_attention" and call.fn(*call.args, None) == -1, bad   # MSD_E_ARG
    assert b"attention_decoupled" in lib.msdi_last_error()


def test_null_struct_and_the_limits_the_header_names():
    from minsdtf_amd import _lib_ipadapter

    lib = _lib_ipadapter.load()
    assert lib.msdi_attention_decoupled(None, None) == -1 and b"attention_decoupled: null" in lib.msdi_last_error()
    # T = 77 with N = 16 is exactly one tile; T = 81 with N = 16 is not (the message names the tile)
    assert 80 + 16 == _lib_ipadapter.KEYS


# ------------------------------------------------------------------------------------------------------------------ engines
class _Tensor(LW._Tensor):
    dtype = torch.bfloat16   # (emit_time_embedding reads it)


class _Weights(LW._AnyWeights):
    def __missing__(self, k):
        return _Tensor()


def _net(**kw):
    return types.SimpleNamespace(_require_weights=lambda: None, device=torch.device("cpu"), _W=_Weights(), **kw)


def _engine(monkeypatch, tokens, control=False, t_uncond=77, guidance=7.5, **kw):
    """A DenoiseEngine on the stand-ins, its Plan.rec calls as Rec records, per plan in recording order."""
    import minsdtf_amd.stable_diffusion as sdm
    from minsdtf_amd import engine

    monkeypatch.setattr(sdm, "CONTROLNET_OVERLAP", False)
    recs = []
    orig = engine.Plan.rec

    def rec(self, f, **k):
        recs.append(LW.Rec(f.__name__, k.get("name", ""), k, {n: LW._operand(v) for n, v in k.items() if LW._operand(v) is not None}))
        return orig(self, f, **k)

    monkeypatch.setattr(engine.Plan, "rec", rec)
    if tokens:
        kw.update(ip_tokens=tokens, ip_adapter=_net(tokens=tokens, weights_version=1))
    if control:
        kw.update(control_net=_net(), hint_net=_net())
    eng = sdm.DenoiseEngine(_net(h=SIZE, w=SIZE), 2, 77, t_uncond, 3, guidance, 0.7, **kw)
    monkeypatch.setattr(engine.Plan, "rec", orig)
    return eng, recs


@pytest.mark.parametrize("form", ["fused", "two_passes", "no_guidance", "controlnet"])
def test_engine_records_one_launch_per_attn2_and_the_kv_in_the_prep_plan(monkeypatch, form):
    from minsdtf_amd import engine

    kw = dict(t_uncond=40 if form == "two_passes" else 77, guidance=0.0 if form == "no_guidance" else 7.5, control=form == "controlnet")
    plain, plain_recs = _engine(monkeypatch, 0, **kw)
    eng, recs = _engine(monkeypatch, 4, **kw)
    passes = 2 if form == "two_passes" else 1
    B = 2
    nb = {"fused": [2 * B], "controlnet": [2 * B], "two_passes": [B, B], "no_guidance": [B]}[form]
    assert len(eng.passes) == passes and [p[1] for p in eng.passes] == nb
    # the plain engine: no ip launch, the fused cross-attention where it has the shape
    assert not any(r.op == "ip_attention" for r in plain_recs) and any(r.op == "cross_attention_q" for r in plain_recs)
    assert plain.ip_scales is None and not plain.ip_in
    # the UNet of the IP engine: 16 launches per pass, no fused cross-attention and no plain attn2 left in it
    mine = [r for r in recs if r.op == "ip_attention"]
    assert len(mine) == 16 * passes
    n_prep = len(eng.prep.calls) + len(eng.prep_t.calls)
    step = recs[n_prep:]
    assert all(r in step for r in mine) and len(step) == len(eng.calls)
    names = [n + ".transformer_blocks.0.attn2.ip" for n in engine.PAG_LAYERS]
    for p in range(passes):
        assert [r.name for r in mine[16 * p:16 * (p + 1)]] == names
    plain_step = plain_recs[len(plain.prep.calls) + len(plain.prep_t.calls):]
    fused = lambda rs: [r.name for r in rs if r.op == "cross_attention_q"]                          # noqa: E731
    parts = lambda rs: [r.name for r in rs if r.op == "attention" and r.name.endswith(".attn2")]    # noqa: E731
    assert len(fused(plain_step)) == (10 + (4 if form == "controlnet" else 0)) * passes
    if form == "controlnet":   # the ControlNet's own encoder keeps its plain records: 4 fused launches, 3 at head size 160
        assert len(fused(step)) == 4 and len(parts(step)) == 3 and len(parts(plain_step)) == 3 + 6
        assert all(n.startswith(("down_blocks.", "mid_block.")) for n in fused(step) + parts(step))
    else:
        assert not fused(step) and not parts(step)
    # 32 K / V matrices -> 16 split GEMMs per pass in the persistent prep plan, none in the step plan
    kv = [r for r in recs if r.op == "conv_gemm" and r.name.endswith(".kv_ip")]
    assert len(kv) == 16 * passes and all(r in recs[:n_prep] for r in kv)
    assert [r.name for r in kv[:16]] == [n + ".kv_ip" for n, _c in engine.UNET_ATTN_LAYERS]
    assert tuple(eng.ip_scales.shape) == (3, 16) and eng.ip_scales.dtype == torch.float32
    assert {t: tuple(v.shape) for t, v in eng.ip_in.items()} == {p[3]: (p[1], 4, 768) for p in eng.passes}
    for r, k in zip(mine, kv):
        a = r.kw
        # every operand inside its live buffer (tests/_extents_ipadapter.py); the image K / V^T are the outputs of this layer's GEMM
        dims = {x: a[x] for x in ("batch", "heads", "head_dim", "s", "t", "n", "q_ld", "k_ld", "vt_ld", "kip_ld", "vtip_ld", "o_ld", "num_steps")}
        ext = XI.ip_attention(q=1, k=1, vt=1, k_ip=1, vt_ip=1, out=1, scales=1, step_ptr=1, **dims)
        assert a["scales"] is eng.ip_scales and a["step_ptr"] is eng.step_ptr and a["num_steps"] == 3 and a["n"] == 4 and a["vtip_ld"] == 8
        assert a["layer"] == names.index(r.name) and (a["batch"], a["t"]) == (nb[mine.index(r) // 16], eng.passes[mine.index(r) // 16][2])
        ns0, ns1, out1, out1_ld, out2, out2_ld = k.kw["split"]   # (ops.conv_gemm's: k rows to out1, v transposed to out2)
        assert a["k_ip"] is out1 and a["vt_ip"] is out2 and (ns0, ns1, out1_ld, out2_ld) == (0, a["heads"] * a["head_dim"], a["kip_ld"], 8)
        assert set(r.operands) == set(ext) - {"scales", "step_ptr"}
        for name, o in r.operands.items():
            assert not o.freed and ext[name][0] <= o.avail, (r.name, name)
        assert ext["scales"][0] == eng.ip_scales.numel() * 4
    # nothing else moves: apart from attn2 the step plan's launch names are the plain job's
    strip = lambda rs: [r.name for r in rs if ".attn2" not in r.name or ".attn2.to_out" in r.name]   # noqa: E731
    assert strip(step) == strip(plain_recs[len(plain.prep.calls) + len(plain.prep_t.calls):])


def test_engine_options_key_and_checks():
    import minsdtf_amd.stable_diffusion as sdm
    from minsdtf_amd.jobopts import REFUSED, EngineOptions

    assert EngineOptions.of().key() == () and EngineOptions.of(ip_tokens=None) == EngineOptions.of(ip_tokens=0) == EngineOptions()
    assert EngineOptions.of(ip_tokens=4).key() == (("ip", 4),)
    assert EngineOptions.of(dynthresh=True, control_units=1, ip_tokens=16, sampler="euler_a").key() == (("dynthresh",), ("control", 1), ("ip", 16))
    assert "ip_adapter" not in REFUSED and "ip" not in REFUSED and len(REFUSED) == 8
    unet, ad = _net(h=SIZE, w=SIZE), _net(tokens=4, weights_version=1)
    args = (unet, 2, 77, 77, 3, 7.5, 0.7)
    for bad in (dict(ip_tokens=4), dict(ip_adapter=ad), dict(ip_tokens=16, ip_adapter=ad)):
        with pytest.raises(ValueError, match="^ip_adapter: an engine of ip_tokens"):
            sdm.DenoiseEngine(*args, **bad)
    with pytest.raises(ValueError, match="^ip_adapter: 17 image tokens"):
        sdm.DenoiseEngine(*args, ip_tokens=17, ip_adapter=_net(tokens=17))
    for kind, opts in (("pag", dict(pag=("mid_block.attentions.0",))), ("sag", dict(sag=True)), ("regions", dict(regions=2)),
                       ("regions", dict(regions=2, region_mode="attention")), ("hypertile", dict(hypertile=(2, 2, 0))),
                       ("reference_only", dict(reference=("mid_block.attentions.0",))), ("denoise_streams = 2", dict(streams=2))):
        wide = (_net(h=16, w=16),) + args[1:]   # (a latent whose level 0 splits into 2 x 2 windows of 8 tokens)
        with pytest.raises(ValueError, match=f"^ip_adapter: .*cannot be combined with.*{kind}"):
            sdm.DenoiseEngine(*(wide if kind == "hypertile" else args), ip_tokens=4, ip_adapter=ad, **opts)
    # a text context that does not fit the tile beside the image tokens: the limit by name
    with pytest.raises(ValueError, match=r"^ip_adapter: a text context of 154 tokens and 4 image tokens exceed the 96 keys.*roundup8\(T\) \+ N <= 96.*77 tokens"):
        sdm.DenoiseEngine(unet, 2, 154, 77, 3, 7.5, 0.7, ip_tokens=4, ip_adapter=ad)
    with pytest.raises(ValueError, match="^ip_adapter: a text context of 81 tokens and 16 image tokens"):
        sdm.DenoiseEngine(unet, 2, 77, 81, 3, 7.5, 0.7, ip_tokens=16, ip_adapter=_net(tokens=16))
    sdm.DenoiseEngine(unet, 2, 77, 80, 3, 7.5, 0.7, ip_tokens=16, ip_adapter=_net(tokens=16))   # 80 + 16: exactly one tile


def test_attn_variant_refuses_ip_with_regions():
    from minsdtf_amd import engine

    x = engine.Act(None, 2, 8, 8, 320)
    ipv = (_Tensor(), _Tensor(), 4, 8, _Tensor(), 3, 0)
    engine.AttnVariant(ip=ipv).check("blk", x, 8, 1)
    with pytest.raises(ValueError, match="ip .*does not go with regions"):
        engine.AttnVariant(ip=ipv, regions=2, region_rows=1, region_w=_Tensor()).check("blk", x, 8, 1)
    with pytest.raises(ValueError, match="ip with 17 image tokens"):
        engine.AttnVariant(ip=(_Tensor(), _Tensor(), 17, 24, _Tensor(), 3, 0)).check("blk", x, 8, 1)
    with pytest.raises(ValueError, match="ip .*does not go with pag"):
        engine.UNetVariant(ip=({}, 4, _Tensor(), 3), pag_layers=("mid_block.attentions.0",), perturbed=1).check(2, None, None)


def test_prepare_carries_the_goes_with_check(monkeypatch):
    eng, _ = _engine(monkeypatch, 4)
    plain, _ = _engine(monkeypatch, 0)
    tok, tab = np.zeros((4, 768), dtype=np.float32), np.ones((3, 16), dtype=np.float32)
    with pytest.raises(ValueError, match="`ip_adapter` goes with an engine built with ip_tokens=N"):
        eng.prepare({}, None, None, None)
    with pytest.raises(ValueError, match="`ip_adapter` goes with an engine built with ip_tokens=N"):
        plain.prepare({}, None, None, None, ip_adapter=(tok, tok, tab))
    with pytest.raises(ValueError, match="image tokens of shapes"):
        eng.prepare({}, None, None, None, ip_adapter=(tok[:2], tok, tab))
    with pytest.raises(ValueError, match="a table of shape"):
        eng.prepare({}, None, None, None, ip_adapter=(tok, tok, tab[:2]))


def test_engine_key_holds_the_token_count_and_the_adapter():
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    class Net:
        weights_version = 1
        tokens = 4

    sd = StableDiffusionBase(64, 64)
    sd.diffusion_model = Net()
    args = (1, 77, 77, 4, 7.5, 0.7, False)
    plain = sd._engine_key(*args)
    assert sd._engine_key(*args, ip_tokens=None, ip_adapter=None) == plain
    ad = Net()
    one = sd._engine_key(*args, ip_tokens=4, ip_adapter=ad)
    assert one[:len(plain)] == plain and one[-1] == ("ip", 4) and one[len(plain)][0] == "ip_adapter"
    assert one == sd._engine_key(*args, ip_tokens=4, ip_adapter=ad) != sd._engine_key(*args, ip_tokens=4, ip_adapter=Net())
    ad.weights_version = 2
    assert one != sd._engine_key(*args, ip_tokens=4, ip_adapter=ad)


# ------------------------------------------------------------------------------------------------- generate_image, no device
def test_generate_image_refusals():
    from minsdtf_amd.models import IPAdapter
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    ctx = np.zeros((77, 768), dtype=np.float32)
    sd = StableDiffusionBase(64, 64)   # (no models behind it: anything that reaches a model fails another way)
    sd.unconditional_context = ctx
    m = IPAdapter.synthetic(0, 4, device=torch.device("cpu"))
    ipa = dict(embeds=EMB, model=m)
    kw = dict(batch_size=1, num_steps=3, seed=0)
    mask = np.ones((64, 64), dtype=np.float32)
    kinds = dict(pag=dict(scale=3.0), regions=dict(regions=[dict(prompt=ctx, mask=mask)]), tiled=dict(size=(64, 128)), hires=dict(scale=2.0),
                 sag=dict(scale=0.75), hypertile=dict(tile=64), reference_only=dict(latent=np.zeros((1, 8, 8, 4), dtype=np.float32)))
    for kind, spec in kinds.items():
        for fn in (sd.generate_image, sd.text_to_image):
            with pytest.raises(ValueError, match=f"^ip_adapter: .*cannot be combined with {kind}$"):
                fn(ctx, ip_adapter=ipa, **{kind: spec}, **kw)
    with pytest.raises(ValueError, match="^ip_adapter: .*cannot be combined with pag, sag$"):
        sd.generate_image(ctx, ip_adapter=ipa, sag=dict(scale=0.75), pag=dict(scale=3.0), **kw)
    sd.denoise_streams = 2
    with pytest.raises(ValueError, match="^ip_adapter: .*cannot be combined with denoise_streams = 2$"):
        sd.generate_image(ctx, ip_adapter=ipa, **kw)
    sd.denoise_streams = None
    with pytest.raises(ValueError, match="^ip_adapter: weight_type"):
        sd.generate_image(ctx, ip_adapter=dict(ipa, weight_type="strong"), **kw)
    with pytest.raises(ValueError, match=r"^ip_adapter: a text context of 154 tokens.*roundup8\(T\) \+ N <= 96"):
        sd.generate_image(np.zeros((154, 768), dtype=np.float32), ip_adapter=ipa, **kw)
    with pytest.raises(ValueError, match="^ip_adapter: a text context of 154 tokens"):
        sd.generate_image(ctx, negative_prompt=np.zeros((154, 768), dtype=np.float32), ip_adapter=ipa, **kw)
    with pytest.raises(ValueError, match="^ip_adapter: `image` needs"):
        sd.generate_image(ctx, ip_adapter=dict(image=np.zeros((8, 8, 3)), model=m), **kw)
    assert not sd._engines
    for fn in (sd.text_to_image, sd.image_to_image, sd.inpaint, sd.generate_image):
        assert "ip_adapter" in fn.__doc__


def test_committed_fixtures_are_told_apart_from_the_plain_job():
    for size in (128, 256):
        path = os.path.join(ROOT, "tests", "golden", f"ip_adapter_{size}.npz")
        assert os.path.exists(path) and os.path.getsize(path) <= 1 << 20, path
        z = np.load(path)
        assert float(z["plain_psnr"]) < 35.0, (size, float(z["plain_psnr"]))
