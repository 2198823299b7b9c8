"""The CLIP ViT-H/14 vision tower without a GPU: the C ABI of the sixth library, the weight table against transformers' key names, the
float64 restatement against transformers' own model, the preprocessing against Pillow, the recorded launch plan and the pipeline's
image-prompt path."""
import ctypes
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

import _extents as X
import _extents_vision as XV
import _layer_walk as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_library_exports_its_header_and_the_others_are_untouched():
    from minsdtf_amd import _lib, _lib_control, _lib_dynthresh, _lib_ext, _lib_ipadapter, _lib_vision

    assert os.path.exists(_lib_vision.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    header = open(os.path.join(ROOT, "include", "minsdtf_hip_vision.h")).read()
    declared = set(re.findall(r"^MSDV_API\s+(?:int|const char\*)\s+(msdv_\w+)\s*\(", header, flags=re.M))
    assert declared == set(_lib_vision.SYMBOLS) == {"msdv_abi_version", "msdv_last_error", "msdv_patch_embed", "msdv_gelu", "msdv_pool_project"}
    assert not re.search(r"^(?:int|const char\*)\s+msdv_\w+\s*\(", header, flags=re.M), "a declaration without MSDV_API"
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib_vision.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert exported == declared, sorted(exported ^ declared)
    lib = _lib_vision.load()
    assert lib.msdv_abi_version() == _lib_vision.ABI_VERSION == int(re.search(r"#define MSDV_ABI_VERSION (\d+)", header).group(1)) == 1
    for name in ("IMAGE", "PATCH", "GRID", "TOKENS", "WIDTH", "PATCH_K", "PROJ", "MAX_BATCH"):
        assert int(re.search(rf"#define MSDV_{name} (\d+)", header).group(1)) == getattr(_lib_vision, name), name
    emap = open(os.path.join(ROOT, "minsdtf_amd", "csrc", "vision", "exports_vision.map")).read()
    assert set(re.findall(r"\b(msdv_\w+);", emap)) == declared and "*;" in emap and "msdv_*" not in emap
    counts = {}
    for other in (_lib, _lib_ext, _lib_dynthresh, _lib_control, _lib_ipadapter):
        table = subprocess.check_output(["nm", "-D", "--defined-only", other.LIB_PATH], text=True)
        assert "msdv_" not in table and not any(n.startswith("msdv_") for n in other.SYMBOLS)
        counts[other.LIB_NAME] = len([ln for ln in table.splitlines() if ln.strip()])
    assert list(counts.values()) == [31, 4, 3, 3, 3], counts


@pytest.mark.parametrize("struct", ["MsdvPatchEmbed", "MsdvPoolProject"])
def test_struct_layout_matches_the_header(struct):
    from minsdtf_amd import _lib_vision

    cls = getattr(_lib_vision, struct)
    fields = [n for n, _t in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "minsdtf_hip_vision.h"\nint main(){printf("%zu", sizeof(' + struct + '));' + \
        "".join(f'printf(" %zu", offsetof({struct}, {f}));' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]


BASE = 1 << 26   # (addresses are only compared and checked for alignment: every bad call returns before a launch)
PE_GOOD = dict(pixels=BASE, w=2 * BASE, cls=3 * BASE, pos=4 * BASE, gamma=5 * BASE, beta=6 * BASE, out=7 * BASE, batch=2, scale=(1.0, 1.0, 1.0),
               shift=(0.0, 0.0, 0.0), w_ld=592, o_ld=1280)
PE_BAD = [dict(pixels=None), dict(w=None), dict(cls=None), dict(pos=None), dict(gamma=None), dict(beta=None), dict(out=None), dict(pixels=BASE + 4),
          dict(w=2 * BASE + 8), dict(pos=4 * BASE + 2), dict(out=7 * BASE + 8), dict(batch=0), dict(batch=9), dict(w_ld=584), dict(w_ld=580),
          dict(w_ld=588), dict(o_ld=1272), dict(o_ld=1284), dict(eps=0.0), dict(out=BASE), dict(out=2 * BASE + 16), dict(out=4 * BASE),
          dict(out=5 * BASE - 64)]
GELU_GOOD = dict(x=BASE, out=2 * BASE, rows=257, cols=5120)
GELU_BAD = [dict(x=None), dict(out=None), dict(x=BASE + 4), dict(out=2 * BASE + 2), dict(rows=0), dict(cols=0), dict(cols=12), dict(cols=5124),
            dict(ld_in=5112), dict(ld_in=5122), dict(ld_out=5124), dict(ld_out=5112), dict(out=BASE), dict(out=BASE + 4096), dict(x=2 * BASE + 1024)]
PP_GOOD = dict(x=BASE, gamma=2 * BASE, beta=3 * BASE, w=4 * BASE, out=5 * BASE, batch=3, x_stride=257 * 1280)
PP_BAD = [dict(x=None), dict(gamma=None), dict(beta=None), dict(w=None), dict(out=None), dict(x=BASE + 2), dict(w=4 * BASE + 8), dict(out=5 * BASE + 4),
          dict(batch=0), dict(batch=9), dict(x_stride=1272), dict(x_stride=1284), dict(w_layout=2), dict(eps=-1.0), dict(out=BASE), dict(out=2 * BASE),
          dict(out=4 * BASE + 64), dict(out=BASE + 2 * 257 * 1280 * 2)]
_ids = lambda b: "-".join(f"{k}={v}" for k, v in b.items())   # noqa: E731


def _refused(op, entry, good, bad):
    from minsdtf_amd import _lib_vision, ops

    lib = _lib_vision.load()
    call = getattr(ops, op)(**dict(good, **bad))
    assert call.name == op and call.fn(*call.args, None) == -1, bad   # MSD_E_ARG, nothing launched (there is no device)
    assert entry in lib.msdv_last_error()


@pytest.mark.parametrize("bad", PE_BAD, ids=_ids)
def test_patch_embed_argument_errors_without_a_device(bad):
    _refused("patch_embed", b"patch_embed", PE_GOOD, bad)


@pytest.mark.parametrize("bad", GELU_BAD, ids=_ids)
def test_gelu_argument_errors_without_a_device(bad):
    _refused("gelu", b"gelu", GELU_GOOD, bad)


@pytest.mark.parametrize("bad", PP_BAD, ids=_ids)
def test_pool_project_argument_errors_without_a_device(bad):
    _refused("pool_project", b"pool_project", PP_GOOD, bad)


def test_null_structs_and_the_one_geometry():
    from minsdtf_amd import _lib_vision, ops

    lib = _lib_vision.load()
    assert lib.msdv_patch_embed(None, None) == -1 and b"patch_embed: null" in lib.msdv_last_error()
    assert lib.msdv_pool_project(None, None) == -1 and b"pool_project: null" in lib.msdv_last_error()
    for op, good, other in (("patch_embed", PE_GOOD, dict(image=336)), ("patch_embed", PE_GOOD, dict(patch=16)), ("patch_embed", PE_GOOD, dict(width=1024)),
                            ("pool_project", PP_GOOD, dict(width=1024)), ("pool_project", PP_GOOD, dict(proj=768))):
        call = getattr(ops, op)(**dict(good, **other))
        assert call.fn(*call.args, None) == -3 and b"ViT-H/14 only" in lib.msdv_last_error(), other   # MSD_E_UNSUPPORTED


# -------------------------------------------------------------------------------------------------------------------- weights
_HF = {}


def _hf(layers=2):
    """transformers' CLIPVisionModelWithProjection at the ViT-H/14 geometry with `layers` layers (random weights, built from a config:
    nothing is fetched), in float64, and its state as float32 arrays."""
    if layers not in _HF:
        from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection

        torch.manual_seed(7)
        cfg = CLIPVisionConfig(hidden_size=1280, intermediate_size=5120, num_attention_heads=16, image_size=224, patch_size=14,
                               projection_dim=1024, hidden_act="gelu", num_hidden_layers=layers)
        model = CLIPVisionModelWithProjection(cfg).eval()
        with torch.no_grad():   # (the default init leaves the norms at 1 / 0 and the biases at 0: move them, or those paths are vacuous)
            for n, p in model.named_parameters():
                if n.endswith(".bias"):
                    p.uniform_(-0.1, 0.1)
                elif "norm" in n and n.endswith(".weight"):
                    p.uniform_(0.8, 1.2)
        _HF[layers] = (model, {k: v.detach().clone().numpy() for k, v in model.state_dict().items()})
    return _HF[layers]


def test_table_keys_are_transformers_state_dict_keys():
    from minsdtf_amd import weights as W

    _model, state = _hf(2)
    specs = W.table("clip_vision", layers=2)
    keys = [s.key for s in specs]
    assert len(keys) == len(set(keys)) == 3 + 2 + 2 * 16 + 2 + 1
    assert set(keys) == {k for k in state if not k.endswith("position_ids")}
    for s in specs:
        assert tuple(state[s.key].shape) == s.torch_shape, s.key
    assert len(W.table("clip_vision")) == 3 + 2 + 32 * 16 + 2 + 1 and W.param_count("clip_vision") == sum(int(np.prod(s.shape)) for s in W.table("clip_vision"))
    assert "vision_model.pre_layrnorm.weight" in keys and "visual_projection.weight" in keys and "visual_projection.bias" not in keys
    for bad in (0, 33):
        with pytest.raises(ValueError, match="clip_vision: .* layers"):
            W.table("clip_vision", layers=bad)


def test_loader_raises_by_name_and_takes_fp16():
    from minsdtf_amd import weights as W

    state = W.clip_vision_synthetic_state(3, 1)
    arrays = W.clip_vision_arrays(dict(state, **{"vision_model.embeddings.position_ids": np.arange(257)[None]}), 1)   # (the buffer is ignored)
    specs = W.table("clip_vision", layers=1)
    assert [a.shape for a in arrays] == [s.shape for s in specs] and all(a.dtype == np.float32 for a in arrays)
    missing = {k: v for k, v in state.items() if k != "vision_model.encoder.layers.0.mlp.fc1.bias"}
    with pytest.raises(KeyError, match="vision_model.encoder.layers.0.mlp.fc1.bias"):
        W.clip_vision_arrays(missing, 1)
    with pytest.raises(KeyError, match="vision_model.encoder.layers.1.layer_norm1.weight"):
        W.clip_vision_arrays(state, 2)
    swapped = dict(state, **{"visual_projection.weight": state["visual_projection.weight"].T})
    with pytest.raises(ValueError, match=r"'visual_projection.weight' has shape \(1280, 1024\), expected \(1024, 1280\)"):
        W.clip_vision_arrays(swapped, 1)
    half = {k: torch.from_numpy(v).to(torch.float16) for k, v in state.items()}
    for a, b, s in zip(W.clip_vision_arrays(half, 1), arrays, specs):
        assert a.dtype == np.float32 and np.array_equal(a, b.astype(np.float16).astype(np.float32)), s.key


def test_layout_packs_the_tower_like_the_text_encoder():
    from minsdtf_amd import layout, packing
    from minsdtf_amd import weights as W

    specs = W.table("clip_vision", layers=1)
    table = {e.key: e for e in layout.layout(specs)}
    ln = "vision_model.encoder.layers.0."
    assert table[ln + "self_attn.qkv.w"].shape == (3840, 1280) and table[ln + "self_attn.qkv.b"].shape == (3840,) and table[ln + "self_attn.qkv.w"].chunk_major
    assert not any(k.startswith(ln + "self_attn." + m) for k in table for m in ("q_proj", "k_proj", "v_proj"))
    assert table[ln + "mlp.fc1.w"].shape == (5120, 1280) and table[ln + "layer_norm1.g"].store == layout.VEC
    pe = table["vision_model.embeddings.patch_embedding.w"]
    assert (pe.shape, pe.pad_k, pe.stored_shape, pe.chunk_major) == ((1280, 588), 592, (1280, 592), False)
    assert table["visual_projection.w"].stored_shape == (20, 1024, 64) and "visual_projection.b" not in table
    assert table["vision_model.embeddings.class_embedding"].shape == (1280,) and table["vision_model.embeddings.position_embedding"].shape == (257, 1280)
    assert all(e.pad_k is None for k, e in table.items() if k != pe.key)
    state = W.clip_vision_synthetic_state(0, 1)
    named = {(s.name, s.kind): a for s, a in zip(specs, W.clip_vision_arrays(state, 1))}
    packed, _ = packing.pack(list(table.values()), named, torch.device("cpu"))
    w = packed[pe.key].float().numpy()
    src = state["vision_model.embeddings.patch_embedding.weight"]   # OIHW
    assert w.shape == (1280, 592) and not w[:, 588:].any()
    want = torch.from_numpy(src).permute(0, 2, 3, 1).reshape(1280, 588).to(torch.bfloat16).float().numpy()   # k = (ky * 14 + kx) * 3 + c
    assert np.array_equal(w[:, :588], want)
    assert packed["vision_model.embeddings.class_embedding"].dtype == torch.float32


# ----------------------------------------------------------------------------------------------------------- host restatement
def test_forward_host_is_transformers_model_in_float64():
    from minsdtf_amd import vision

    model, state = _hf(2)
    rng = np.random.default_rng(5)
    px = rng.uniform(0.0, 255.0, (2, 224, 224, 3))
    mine = vision.forward_host(state, px, 2)
    mean, std = np.asarray(vision.MEAN), np.asarray(vision.STD)
    pv = torch.from_numpy(((px / 255.0 - mean) / std).transpose(0, 3, 1, 2).copy())
    with torch.no_grad():
        out = model.double()(pixel_values=pv, output_hidden_states=True)
    model.float()
    for name, ref in (("image_embeds", out.image_embeds), ("penultimate", out.hidden_states[-2]), ("last_hidden_state", out.hidden_states[-1])):
        err = float(np.abs(mine[name] - ref.numpy()).max())
        print(f"forward_host vs transformers (float64): {name} {err:.2e}")
        assert mine[name].dtype == np.float64 and err <= 1e-9, (name, err)
    one = vision.forward_host(state, px[0], 2)   # a single picture, and a sample does not depend on its batch
    assert np.abs(one["image_embeds"][0] - mine["image_embeds"][0]).max() <= 1e-12
    with pytest.raises(ValueError, match="clip_vision: pixels of shape"):
        vision.forward_host(state, px[:, :200], 2)


def _pillow_f(px, nh, nw):
    from PIL import Image

    return np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(px[..., c], dtype=np.float32), mode="F").resize((nw, nh), Image.BICUBIC))
                     for c in range(3)], axis=-1)


@pytest.mark.parametrize("h,w", [(300, 700), (120, 90), (224, 500), (1000, 224)])
def test_preprocess_is_pillow_bicubic_in_floating_point(h, w):
    from minsdtf_amd import vision

    rng = np.random.default_rng(h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    px = np.clip(127.5 + 90.0 * np.sin(yy[..., None] / 17.0 + np.arange(3)) * np.cos(xx[..., None] / 23.0) + 20.0 * rng.standard_normal((h, w, 3)), 0, 255)
    px = np.round(px).astype(np.uint8)
    nh, nw = vision.resize_size(h, w)
    short, long = min(h, w), max(h, w)
    assert min(nh, nw) == 224 and max(nh, nw) == int(long * 224 / short) and (nh >= nw) == (h >= w)
    got = vision.preprocess(px)
    assert got.shape == (224, 224, 3) and got.dtype == np.float32 and got.min() >= 0.0 and got.max() <= 255.0
    ref = np.clip(_pillow_f(px, nh, nw), 0.0, 255.0)
    top, left = (nh - 224) // 2, (nw - 224) // 2
    ref = ref[top:top + 224, left:left + 224]
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"preprocess {h}x{w} -> {nh}x{nw}: max difference to Pillow mode F {err:.2e} levels")
    assert err <= 1e-3, err
    assert np.array_equal(got, vision.preprocess(px.astype(np.float32))) and np.array_equal(got, vision.preprocess(px[None]))


def test_preprocess_passes_a_224_picture_unchanged_and_reads_files(tmp_path):
    from PIL import Image

    from minsdtf_amd import vision

    px = np.random.default_rng(2).integers(0, 256, (224, 224, 3)).astype(np.uint8)
    assert np.array_equal(vision.preprocess(px), px.astype(np.float32))
    path = str(tmp_path / "picture.png")
    Image.fromarray(px).save(path)
    assert np.array_equal(vision.preprocess(path), px.astype(np.float32))
    assert vision.digest(vision.preprocess(px)) == vision.digest(px.astype(np.float32)) != vision.digest(px[::-1].astype(np.float32))
    for bad in (np.zeros((8, 8, 2)), np.zeros((8,)), np.full((8, 8, 3), np.nan)):
        with pytest.raises(ValueError, match="^clip_vision: "):
            vision.preprocess(bad)
    sc, sh = vision.pixel_affine()
    assert np.allclose(np.asarray(sc) * 255.0 * np.asarray(vision.STD), 1.0, rtol=1e-15) and np.allclose(np.asarray(sh) * np.asarray(vision.STD), -np.asarray(vision.MEAN))


# ----------------------------------------------------------------------------------------------------------------------- plan
def _record(layers, B, output):
    """models.ClipVisionEncoder._build on stand-ins: its Plan.rec calls as LW.Rec records, in recording order."""
    from minsdtf_amd import engine
    from minsdtf_amd.models import ClipVisionEncoder

    recs = []
    orig = engine.Plan.rec

    def rec(self, fn, **kw):
        ops_ = {}
        for k, v in kw.items():
            if k == "split" and v is not None:
                ops_["out1"], ops_["out2"] = LW._operand(v[2]), LW._operand(v[4])
                continue
            if k == "workspace" and isinstance(v, engine._Lazy):
                continue
            o = LW._operand(v)
            if o is not None:
                ops_[k] = o
        recs.append(LW.Rec(fn.__name__, kw.get("name", ""), kw, ops_))
        return orig(self, fn, **kw)

    engine.Plan.rec = rec
    try:
        net = types.SimpleNamespace(device=torch.device("cpu"), _W=LW._AnyWeights(), layers=layers, _use_graph=False)
        bp = ClipVisionEncoder._build(net, B, output)
    finally:
        engine.Plan.rec = orig
    return recs, bp


LAYER_OPS = ["layer_norm", "conv_gemm", "attention", "conv_gemm", "layer_norm", "conv_gemm", "gelu", "conv_gemm"]
LAYER_NAMES = ["layer_norm1", "self_attn.qkv", "self_attn", "self_attn.out_proj", "layer_norm2", "mlp.fc1", "mlp.gelu", "mlp.fc2"]


@pytest.mark.parametrize("layers,B", [(2, 1), (3, 2), (32, 1)])
def test_plan_is_two_plus_eight_launches_per_layer(layers, B):
    from minsdtf_amd import ops

    recs, bp = _record(layers, B, "image_embeds")
    assert len(recs) == len(bp.plan.calls) == 2 + 8 * layers
    assert [r.op for r in recs] == ["patch_embed"] + LAYER_OPS * layers + ["pool_project"]
    assert [r.name for r in recs[1:-1]] == [f"vision_model.encoder.layers.{i}.{n}" for i in range(layers) for n in LAYER_NAMES]
    assert tuple(bp.io["pixels"].shape) == (B, 224, 224, 3) and tuple(bp.io["out"].shape) == (B, 1024) and bp.io["out"].dtype == torch.float32
    pe, pp = recs[0].kw, recs[-1].kw
    assert (pe["batch"], pe["w_ld"], pe["o_ld"]) == (B, 592, 1280) and (pp["batch"], pp["x_stride"], pp["w_layout"]) == (B, 257 * 1280, 1)
    for r in recs:
        a = r.kw
        if r.op == "attention":
            assert (a["batch"], a["heads"], a["head_dim"], a["s"], a["t"], a["vt_ld"], bool(a["causal"])) == (B, 16, 80, 257, 257, 264, False)
            assert a["scale"] == 80 ** -0.5 and a["q_ld"] == a["k_ld"] == a["o_ld"] == 1280
        if r.name.endswith("self_attn.qkv"):
            assert a["split"][:2] == (1280, 1280) and a["split"][5] == 264 and a["N"] == 3840
        if r.name.endswith("mlp.fc1"):
            assert a["out_dtype"] == ops.OUT_F32 and a["act"] == ops.ACT_NONE and a["bias"] is not None and a["N"] == 5120
        if r.op == "gelu":
            assert (a["rows"], a["cols"]) == (B * 257, 5120)
            fc1 = recs[recs.index(r) - 1]
            assert r.operands["x"].buf == fc1.operands["out"].buf   # fc1's fp32 output is what the GELU rounds
        if r.name.endswith(("out_proj", "fc2")):
            assert a["residual"] is not None and a["act"] == ops.ACT_NONE
    # every operand inside its live buffer (tests/_extents.py, tests/_extents_vision.py)
    for r in recs:
        dims = {k: (v if v is None or isinstance(v, (int, float, str, bool)) else (tuple(True if not isinstance(x, (int, float)) else x for x in v)
                                                                                   if isinstance(v, tuple) else True))
                for k, v in r.kw.items() if k != "name"}
        ext = XV.EXTENTS[r.op](**dims) if r.op in XV.EXTENTS else X.extents(r.op, **dims)
        assert r.operands, r.name
        for name, o in r.operands.items():
            assert name in ext, (r.name, name)
            if o.kind == "buf":
                assert not o.freed and ext[name][0] <= o.avail, (r.name, name, ext[name][0], o.avail)


def test_penultimate_drops_the_last_layer_and_the_pooled_head():
    full, _ = _record(3, 2, "image_embeds")
    recs, bp = _record(3, 2, "penultimate")
    assert len(recs) == len(full) - 8 == 2 + 8 * 3 - 8
    assert not any(r.op == "pool_project" for r in recs) and not any(".layers.2." in r.name for r in recs)
    assert [(r.op, r.name) for r in recs[:-1]] == [(r.op, r.name) for r in full[:1 + 8 * 2]]
    assert recs[-1].op == "cast_bf16_to_f32" and recs[-1].kw["n"] == 2 * 257 * 1280 and tuple(bp.io["out"].shape) == (2, 257, 1280)
    assert recs[-1].operands["x"].buf == recs[-2].operands["out"].buf   # the output of layer 1 = the input of the last layer
    hidden, bph = _record(3, 2, "last_hidden_state")
    assert len(hidden) == 2 + 8 * 3 and hidden[-1].op == "cast_bf16_to_f32" and tuple(bph.io["out"].shape) == (2, 257, 1280)


# ------------------------------------------------------------------------------------------------------------------- pipeline
class _Tower:
    """Stands in for models.ClipVisionEncoder: counts its calls, returns an embedding that depends on the pixels."""

    def __init__(self):
        self.weights_version, self.calls = 1, 0

    def predict_on_batch(self, px):
        assert px.shape == (1, 224, 224, 3) and px.dtype == np.float32
        self.calls += 1
        return (np.linspace(-1.0, 1.0, 1024) * (1.0 + px.mean() / 255.0) + self.weights_version)[None].astype(np.float32)


def test_image_prompt_precedence_refusal_and_cache():
    from minsdtf_amd import ipadapter as ip
    from minsdtf_amd.models import IPAdapter
    from minsdtf_amd.stable_diffusion import StableDiffusion, StableDiffusionBase

    sd = StableDiffusionBase(64, 64)
    assert sd.clip_vision is None and sd.clip_vision_path is None and "clip_vision_path" in StableDiffusion.__init__.__code__.co_varnames
    m = IPAdapter.synthetic(0, 4, device=torch.device("cpu"))
    pic, pic2 = np.full((32, 48, 3), 100, dtype=np.uint8), np.full((32, 48, 3), 200, dtype=np.uint8)
    spec = ip.parse(dict(image=pic, model=m))
    # neither a callable nor a tower: the unchanged error
    with pytest.raises(ValueError, match="^ip_adapter: `image` needs StableDiffusion.image_prompt_encoder.*`embeds`.*`tokens`"):
        sd._ip_inputs(spec)
    with pytest.raises(ValueError, match="^encode_image_prompt: no vision tower"):
        sd.encode_image_prompt(pic)
    # the tower encodes preprocess(image)
    tower = _Tower()
    sd.clip_vision = tower
    assert sd.clip_vision is tower
    model, (tok_u, tok_c) = sd._ip_inputs(spec)
    emb = sd.encode_image_prompt(pic)
    assert model is m and tower.calls == 1 and emb.shape == (1024,) and emb.dtype == np.float64
    assert np.array_equal(tok_c, m.project(emb)) and np.array_equal(tok_u, m.project(np.zeros(1024)))
    assert np.array_equal(sd._ip_inputs(ip.parse(dict(embeds=emb, model=m)))[1][1], tok_c) and tower.calls == 1
    # the same picture does not run the tower again; another one does, and so does a new weights_version
    sd._ip_inputs(spec)
    sd.encode_image_prompt(pic.astype(np.float32))
    assert tower.calls == 1
    assert not np.array_equal(sd.encode_image_prompt(pic2), emb) and tower.calls == 2
    sd.encode_image_prompt(pic)
    assert tower.calls == 3   # (one picture is kept)
    tower.weights_version = 2
    assert not np.array_equal(sd.encode_image_prompt(pic), emb) and tower.calls == 4
    emb[:] = 0.0   # (the caller's copy)
    assert sd.encode_image_prompt(pic).any() and tower.calls == 4
    # a "plus" adapter's resampler is not part of the package
    plus = IPAdapter.synthetic(0, 16, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="^ip_adapter: `image` with a \"plus\" adapter.*tokens="):
        sd._ip_inputs(ip.parse(dict(image=pic, model=plus)))
    assert tower.calls == 4
    # a callable that was set still wins
    sd.image_prompt_encoder = lambda picture: np.linspace(0.0, 1.0, 1024)
    assert np.array_equal(sd._ip_inputs(spec)[1][1], m.project(np.linspace(0.0, 1.0, 1024))) and tower.calls == 4
    assert sd._ip_inputs(ip.parse(dict(image=pic, model=plus)))[0] is plus
