"""The IP-Adapter "plus" Resampler without a GPU: the float64 statement against a torch.nn transcription of the public formula, the
checkpoint reader, the C ABI of the seventh library, the recorded launch plan and the pipeline's route from a picture to the image
tokens of a plus adapter."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _extents as X
import _extents_resampler as XR
import _extents_vision as XV
import _layer_walk as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------------- the float64 statement
class _Attention(nn.Module):
    def __init__(self, dim=768, heads=12, head=64):
        super().__init__()
        self.heads, self.head = heads, head
        self.norm1, self.norm2 = nn.LayerNorm(dim), nn.LayerNorm(dim)
        self.to_q = nn.Linear(dim, heads * head, bias=False)
        self.to_kv = nn.Linear(dim, 2 * heads * head, bias=False)
        self.to_out = nn.Linear(heads * head, dim, bias=False)

    def forward(self, x, latents):
        x, latents = self.norm1(x), self.norm2(latents)
        B, N, _ = latents.shape
        q = self.to_q(latents)
        k, v = self.to_kv(torch.cat([x, latents], dim=1)).chunk(2, dim=-1)
        q, k, v = (t.reshape(B, t.shape[1], self.heads, self.head).transpose(1, 2) for t in (q, k, v))
        f = self.head ** -0.25
        w = torch.softmax((q * f) @ (k * f).transpose(-2, -1), dim=-1)
        return self.to_out((w @ v).transpose(1, 2).reshape(B, N, -1))


class _Resampler(nn.Module):
    """The formula of the issue / of minsdtf_amd/resampler.py's docstring on torch.nn layers; its state_dict keys are the
    checkpoint's `image_proj.` keys."""

    def __init__(self, depth, tokens=16, dim=768, embed=1280, mult=4):
        super().__init__()
        self.latents = nn.Parameter(torch.zeros(1, tokens, dim))
        self.proj_in, self.proj_out, self.norm_out = nn.Linear(embed, dim), nn.Linear(dim, dim), nn.LayerNorm(dim)
        self.layers = nn.ModuleList([nn.ModuleList([_Attention(dim), nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, mult * dim, bias=False), nn.GELU(),
                                                                                   nn.Linear(mult * dim, dim, bias=False))]) for _ in range(depth)])

    def forward(self, hidden):
        x = self.proj_in(hidden)
        latents = self.latents.repeat(hidden.shape[0], 1, 1)
        for attn, ff in self.layers:
            latents = attn(x, latents) + latents
            y = ff[0](latents)
            latents = ff[3](F.gelu(ff[1](y))) + latents
        return self.norm_out(self.proj_out(latents))


@pytest.mark.parametrize("depth,B", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_forward_host_is_the_formula_in_float64(depth, B):
    from minsdtf_amd import resampler as R

    state = R.synthetic_state(3, depth)
    model = _Resampler(depth).double()
    assert set(model.state_dict()) == {k[len("image_proj."):] for k in state}                  # the checkpoint's key names
    model.load_state_dict({k[len("image_proj."):]: torch.from_numpy(v).double() for k, v in state.items()})
    hidden = 1.2 * np.random.default_rng(depth).standard_normal((B, 257, 1280))
    with torch.no_grad():
        ref = model(torch.from_numpy(hidden)).numpy()
    for form in (state, R.read_state(state)):                                                  # the file's layout, or the reader's result
        mine = R.forward_host(form, hidden, depth)
        err = float(np.abs(mine - ref).max())
        print(f"forward_host vs torch.nn (float64), depth {depth}, B = {B}: {err:.2e}")
        assert mine.dtype == np.float64 and mine.shape == (B, 16, 768) and err <= 1e-9, err
    one = R.forward_host(state, hidden[0])                                                      # a sample does not depend on its batch
    assert np.abs(one[0] - R.forward_host(state, hidden)[0]).max() <= 1e-12
    with pytest.raises(ValueError, match="ip_resampler: hidden states of shape"):
        R.forward_host(state, hidden[:, :, :1024])


def test_attention_reference_is_the_layer_s_softmax():
    from minsdtf_amd import resampler as R

    rng = np.random.default_rng(1)
    q, kl, vl = (rng.standard_normal((2, 5, 128)) for _ in range(3))
    kx, vx = (rng.standard_normal((2, 77, 128)) for _ in range(2))
    got = R.attention_reference(q, kx, vx, kl, vl, 64 ** -0.5 * 1.4426950408889634, 2)
    k, v = np.concatenate([kx, kl], 1), np.concatenate([vx, vl], 1)
    sp = lambda a: torch.from_numpy(a).reshape(2, -1, 2, 64).transpose(1, 2)   # noqa: E731
    ref = (torch.softmax(sp(q) @ sp(k).transpose(-2, -1) / 8.0, -1) @ sp(v)).transpose(1, 2).reshape(2, 5, 128).numpy()
    assert np.abs(got - ref).max() <= 1e-12


def test_synthetic_state_is_seeded_and_scaled():
    from minsdtf_amd import resampler as R

    a, b, c = R.synthetic_state(1, 2), R.synthetic_state(1, 2), R.synthetic_state(2, 2)
    assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) and a[k].dtype == np.float32 for k in a)
    assert not np.array_equal(a["image_proj.latents"], c["image_proj.latents"])
    assert len(a) == 7 + 11 * 2 and len(R.synthetic_state(0, 4)) == 7 + 11 * 4 and R.synthetic_state(0, 1, 8)["image_proj.latents"].shape == (1, 8, 768)
    for k, v in a.items():
        if k.endswith(("norm1.weight", "norm2.weight", "norm_out.weight", ".1.0.weight")):
            assert 0.8 <= v.min() and v.max() <= 1.2, k
        elif v.ndim == 2:
            lim = np.sqrt(6.0 / sum(v.shape))
            assert np.abs(v).max() <= lim and np.abs(v).max() > 0.9 * lim, k
        elif k.endswith("latents"):
            assert 0.8 / np.sqrt(768) < v.std() < 1.2 / np.sqrt(768)
        else:
            assert np.abs(v).max() <= 0.1 and v.any(), k


# ------------------------------------------------------------------------------------------------------------------ the reader
def _plus_state(depth=2, seed=4):
    from minsdtf_amd import resampler as R
    from minsdtf_amd.models import IPAdapter

    state = {k: v for k, v in IPAdapter.synthetic_state(seed, 16).items() if not k.startswith("image_proj.")}
    state.update(R.synthetic_state(seed, depth))
    return state


def test_reader_takes_flat_nested_and_fp16_states():
    from minsdtf_amd import ipadapter as ip
    from minsdtf_amd import resampler as R

    flat = _plus_state(2)
    named = R.read_state(flat)
    assert R.depth_of(named) == 2 and named["latents"].shape == (1, 16, 768) and set(named) == set(R.key_shapes(2))
    nested = {"image_proj": {k[len("image_proj."):]: torch.from_numpy(v) for k, v in flat.items() if k.startswith("image_proj.")},
              "ip_adapter": {k[len("ip_adapter."):]: torch.from_numpy(v) for k, v in flat.items() if k.startswith("ip_adapter.")}}
    for k, v in R.read_state(nested).items():
        assert v.dtype == np.float32 and np.array_equal(v, named[k]), k
    half = {k: torch.from_numpy(v).to(torch.float16) for k, v in flat.items()}
    for k, v in R.read_state(half).items():
        assert v.dtype == np.float32 and np.array_equal(v, named[k].astype(np.float16).astype(np.float32)), k
    assert R.depth_of(R.read_state(_plus_state(1))) == 1 and R.depth_of(R.read_state(_plus_state(4))) == 4
    eight = dict(flat, **{"image_proj.latents": flat["image_proj.latents"][:, :8]})
    assert R.read_state(eight)["latents"].shape == (1, 8, 768)
    # ipadapter.read_state recognises the layout by image_proj.latents: the resampler's keys and the 32 matrices, no projection
    both = ip.read_state(nested)
    assert {k for k in both if k.startswith("resampler.")} == {"resampler." + k for k in named} and "proj.weight" not in both
    assert sum(k.endswith((".to_k_ip", ".to_v_ip")) for k in both) == 32
    with pytest.raises(ValueError, match="the checkpoint has no 'image_proj.proj.weight'"):   # without `latents` it is read as a base checkpoint
        ip.read_state({k: v for k, v in flat.items() if k != "image_proj.latents"})


def test_reader_names_every_missing_key_and_wrong_shape():
    from minsdtf_amd import ipadapter as ip
    from minsdtf_amd import resampler as R

    flat = _plus_state(1)
    keys = [k for k in flat if k.startswith("image_proj.")]
    assert len(keys) == 7 + 11
    for k in keys:
        gone = {a: b for a, b in flat.items() if a != k}
        if k == "image_proj.latents":
            continue                                            # (without it the state is no plus checkpoint: the base reader's error, below)
        if k.startswith("image_proj.layers.") and sum(a.startswith("image_proj.layers.0.") for a in gone) == 0:
            continue
        with pytest.raises(ValueError, match=re.escape(f"the checkpoint has no {k!r}")):
            R.read_state(gone)
        with pytest.raises(ValueError, match=re.escape(f"the checkpoint has no {k!r}")):
            ip.read_state(gone)
        wrong = dict(flat, **{k: np.zeros(tuple(s + 1 for s in flat[k].shape), dtype=np.float32)})
        with pytest.raises(ValueError, match=re.escape(k.rsplit(".", 1)[0])):
            R.read_state(wrong)
    with pytest.raises(ValueError, match=r"image_proj.latents has shape \(1, 17, 768\)"):
        R.read_state(dict(flat, **{"image_proj.latents": np.zeros((1, 17, 768), dtype=np.float32)}))
    with pytest.raises(ValueError, match=r"image_proj.latents has shape \(16, 768\)"):
        R.read_state(dict(flat, **{"image_proj.latents": np.zeros((16, 768), dtype=np.float32)}))
    # the head count is not in the file: another inner width is refused
    wide = dict(flat, **{"image_proj.layers.0.0.to_q.weight": np.zeros((1024, 768), dtype=np.float32),
                         "image_proj.layers.0.0.to_kv.weight": np.zeros((2048, 768), dtype=np.float32),
                         "image_proj.layers.0.0.to_out.weight": np.zeros((768, 1024), dtype=np.float32)})
    with pytest.raises(ValueError, match=r"to_q.weight has shape \(1024, 768\): an inner width of 768 = 12 heads of 64"):
        R.read_state(wide)
    # a gap in the layer indices
    gap = dict(flat, **{k.replace("layers.0.", "layers.2."): v for k, v in flat.items() if ".layers.0." in k})
    with pytest.raises(ValueError, match=r"layers has the indices \[0, 2\]"):
        R.read_state(gap)
    # a missing to_k_ip of a plus checkpoint: the same error as for a base one
    with pytest.raises(ValueError, match="the checkpoint has no 'ip_adapter.5.to_k_ip.weight'"):
        ip.read_state({a: b for a, b in flat.items() if a != "ip_adapter.5.to_k_ip.weight"})


def test_adapters_with_and_without_a_resampler():
    from minsdtf_amd import resampler as R
    from minsdtf_amd.models import IPAdapter, IPResampler

    base = IPAdapter.synthetic(0, 4, device=CPU)
    sixteen = IPAdapter.synthetic(0, 16, device=CPU)
    assert base.resampler is None and sixteen.resampler is None and sixteen.tokens == 16 and sixteen.projection is not None
    assert base.project(np.zeros(1024)).shape == (4, 768)
    plus = IPAdapter.synthetic_plus(3, depth=2, device=CPU)
    assert isinstance(plus.resampler, IPResampler) and plus.tokens == 16 and plus.resampler.depth == 2 and plus.projection is None
    assert plus.resampler.kind == "ip_resampler" and plus.resampler.weights_version == 1 and plus.weights_version == 1
    with pytest.raises(ValueError, match="^ip_adapter: a \"plus\" adapter has no projection.*`image`.*`tokens`"):
        plus.project(np.zeros(1024))
    # the 32 matrices load exactly as a base adapter's
    same = IPAdapter.synthetic(3, 16, device=CPU)
    assert sorted(plus._W.keys()) == sorted(same._W.keys())
    for k in same._W.keys():
        assert torch.equal(plus._W[k], same._W[k]), k
    # the resampler's packed image: layout.py's keys, the latents as an fp32 constant, q | k | v of the latents stacked
    W = plus.resampler._W
    assert W["latents"].dtype == torch.float32 and tuple(W["latents"].shape) == (16, 768)
    assert W["layers.0.attn.qkv.w"].dtype == torch.bfloat16 and W["layers.0.attn.qkv.w"].numel() == 2304 * 768 and W["layers.1.attn.to_kv.w"].numel() == 1536 * 768
    assert "layers.0.attn.to_q.w" not in W.keys() and W["proj_in.b"].shape == (768,) and "layers.0.ff.fc1.b" not in W.keys()
    st = plus.resampler.state
    assert set(st) == set(R.key_shapes(2)) and R.forward_host(st, np.zeros((1, 257, 1280))).shape == (1, 16, 768)
    # a state of another depth / token count is adopted; a base state on a plus adapter drops the resampler
    rs = IPResampler(depth=4, device=CPU)
    rs.set_state(R.synthetic_state(0, 1, 8))
    assert (rs.depth, rs.tokens, rs.weights_version) == (1, 8, 1) and len(rs.weights) == len(rs._specs)
    assert rs.load_synthetic(2).keys() == R.synthetic_state(2, 1, 8).keys() and rs.weights_version == 2
    plus.set_state(IPAdapter.synthetic_state(0, 4))
    assert plus.resampler is None and plus.tokens == 4 and plus.weights_version == 2
    with pytest.raises(ValueError, match="ip_resampler: .* layers"):
        IPResampler(depth=0, device=CPU)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_library_exports_its_header_and_the_others_are_untouched():
    from minsdtf_amd import _lib, _lib_control, _lib_dynthresh, _lib_ext, _lib_ipadapter, _lib_resampler, _lib_vision

    assert os.path.exists(_lib_resampler.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    header = open(os.path.join(ROOT, "include", "minsdtf_hip_resampler.h")).read()
    declared = set(re.findall(r"^MSDR_API\s+(?:int|const char\*)\s+(msdr_\w+)\s*\(", header, flags=re.M))
    assert declared == set(_lib_resampler.SYMBOLS) == {"msdr_abi_version", "msdr_last_error", "msdr_perceiver_attention"}
    assert not re.search(r"^(?:int|const char\*)\s+msdr_\w+\s*\(", header, flags=re.M), "a declaration without MSDR_API"
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib_resampler.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert exported == declared, sorted(exported ^ declared)
    lib = _lib_resampler.load()
    assert lib.msdr_abi_version() == _lib_resampler.ABI_VERSION == int(re.search(r"#define MSDR_ABI_VERSION (\d+)", header).group(1)) == 1
    for name in ("HEAD_DIM", "MAX_QUERIES", "MAX_TX", "KEY_TILE"):
        assert int(re.search(rf"#define MSDR_{name} (\d+)", header).group(1)) == getattr(_lib_resampler, name), name
    assert _lib_resampler.MAX_TX >= 264 and _lib_resampler.MAX_QUERIES == 16
    emap = open(os.path.join(ROOT, "minsdtf_amd", "csrc", "resampler", "exports_resampler.map")).read()
    assert set(re.findall(r"\b(msdr_\w+);", emap)) == declared and "*;" in emap and "msdr_*" not in emap
    counts = {}
    for other in (_lib, _lib_ext, _lib_dynthresh, _lib_control, _lib_ipadapter, _lib_vision):
        table = subprocess.check_output(["nm", "-D", "--defined-only", other.LIB_PATH], text=True)
        assert "msdr_" not in table and not any(n.startswith("msdr_") for n in other.SYMBOLS)
        counts[other.LIB_NAME] = len([ln for ln in table.splitlines() if ln.strip()])
    assert list(counts.values()) == [31, 4, 3, 3, 3, 5], counts


def test_struct_layout_matches_the_header():
    from minsdtf_amd import _lib_resampler

    struct = "MsdrPerceiverAttention"
    cls = getattr(_lib_resampler, struct)
    fields = [n for n, _t in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "minsdtf_hip_resampler.h"\nint main(){printf("%zu", sizeof(' + struct + '));' + \
        "".join(f'printf(" %zu", offsetof({struct}, {f}));' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]


BASE = 1 << 26   # (addresses are only compared and checked for alignment: every bad call returns before a launch)
PA_GOOD = dict(q=BASE, k_x=2 * BASE, vt_x=3 * BASE, k_l=4 * BASE, vt_l=5 * BASE, out=6 * BASE, batch=2, heads=12, n=16, t_x=257, q_ld=768, kx_ld=768,
               vtx_ld=264, kl_ld=768, vtl_ld=16, o_ld=768, scale=0.18)
PA_BAD = [(dict(q=None), -1, b"null"), (dict(vt_l=None), -1, b"null"), (dict(out=None), -1, b"null"), (dict(k_x=2 * BASE + 8), -1, b"16-byte"),
          (dict(out=6 * BASE + 2), -1, b"16-byte"), (dict(n=17), -1, b"n = 17"), (dict(n=0), -1, b"n = 0"), (dict(head_dim=80), -3, b"head_dim 80"),
          (dict(head_dim=128), -3, b"head_dim 128"), (dict(t_x=273, vtx_ld=280), -1, b"t_x = 273"), (dict(t_x=0), -1, b"t_x = 0"),
          (dict(batch=0), -1, b"batch 0"), (dict(heads=0), -1, b"heads 0"), (dict(heads=65536), -1, b"heads 65536"),
          (dict(q_ld=772), -1, b"q_ld = 772"), (dict(kx_ld=770), -1, b"kx_ld = 770"), (dict(vtx_ld=268), -1, b"vtx_ld = 268"),
          (dict(kl_ld=780), -1, b"kl_ld = 780"), (dict(vtl_ld=20), -1, b"vtl_ld = 20"), (dict(o_ld=769), -1, b"o_ld = 769"),
          (dict(q_ld=760), -1, b"smaller than heads"), (dict(o_ld=704), -1, b"smaller than heads"), (dict(vtx_ld=256), -1, b"vtx_ld = 256 < t_x = 257"),
          (dict(vtl_ld=8), -1, b"vtl_ld = 8 < n = 16"), (dict(scale=float("inf")), -1, b"scale"), (dict(scale=float("nan")), -1, b"scale"),
          (dict(out=BASE), -1, b"overlaps"), (dict(out=2 * BASE + 4096), -1, b"overlaps"), (dict(out=3 * BASE + 64), -1, b"overlaps"),
          (dict(out=4 * BASE), -1, b"overlaps"), (dict(out=5 * BASE + 16), -1, b"overlaps")]


@pytest.mark.parametrize("bad,rc,text", PA_BAD, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_perceiver_attention_argument_errors_without_a_device(bad, rc, text):
    from minsdtf_amd import _lib_resampler, ops

    lib = _lib_resampler.load()
    call = ops.perceiver_attention(**dict(PA_GOOD, **bad))
    assert call.name == "perceiver_attention" and call.fn(*call.args, None) == rc, bad   # nothing launched (there is no device)
    msg = lib.msdr_last_error()
    assert b"perceiver_attention" in msg and text in msg, msg
    assert lib.msdr_perceiver_attention(None, None) == -1 and b"perceiver_attention: null" in lib.msdr_last_error()


# ----------------------------------------------------------------------------------------------------------------------- plan
def _record(depth, B, tokens=16):
    """models.IPResampler._build on stand-ins: its Plan.rec calls as LW.Rec records, in recording order."""
    from minsdtf_amd import engine
    from minsdtf_amd.models import IPResampler

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
        net = types.SimpleNamespace(device=CPU, _W=LW._AnyWeights(), depth=depth, tokens=tokens, _use_graph=False)
        bp = IPResampler._build(net, B)
    finally:
        engine.Plan.rec = orig
    return recs, bp


LAYER_OPS = ["layer_norm", "conv_gemm", "layer_norm", "conv_gemm", "perceiver_attention", "conv_gemm", "layer_norm", "conv_gemm", "gelu", "conv_gemm"]
LAYER_NAMES = ["attn.norm1", "attn.to_kv", "attn.norm2", "attn.qkv", "attn", "attn.to_out", "ff.norm", "ff.fc1", "ff.gelu", "ff.fc2"]


@pytest.mark.parametrize("depth,B", [(1, 1), (1, 2), (2, 1), (2, 2), (4, 1), (4, 2)])
def test_plan_launch_count_is_the_docstring_s_formula(depth, B):
    from minsdtf_amd import engine, ops

    recs, bp = _record(depth, B)
    assert "6 + 10 * depth" in engine.emit_ip_resampler.__doc__ and "6 + 10 * depth" in engine.ip_resampler_launches.__doc__
    assert len(recs) == len(bp.plan.calls) == engine.ip_resampler_launches(depth, B) == 6 + 10 * depth + (1 if B > 1 else 0)
    head = ["cast_f32_to_bf16", "conv_gemm", "cast_f32_to_bf16"] + (["replicate"] if B > 1 else [])
    assert [r.op for r in recs] == head + LAYER_OPS * depth + ["conv_gemm", "layer_norm", "cast_bf16_to_f32"]
    assert [r.name for r in recs[len(head):-3]] == [f"layers.{i}.{n}" for i in range(depth) for n in LAYER_NAMES]
    assert [r.name for r in recs[:len(head)]] == ["hidden.bf16", "proj_in", "latents.bf16", "latents.replicate"][:len(head)]
    assert [r.name for r in recs[-3:]] == ["proj_out", "norm_out", "tokens.f32"]
    assert tuple(bp.io["hidden"].shape) == (B, 257, 1280) and tuple(bp.io["out"].shape) == (B, 16, 768) and bp.io["out"].dtype == torch.float32
    for r in recs:
        a = r.kw
        if r.op == "perceiver_attention":
            assert (a["batch"], a["heads"], a["head_dim"], a["n"], a["t_x"], a["vtx_ld"], a["vtl_ld"]) == (B, 12, 64, 16, 257, 264, 16)
            assert a["q_ld"] == a["kx_ld"] == a["kl_ld"] == a["o_ld"] == 768 and a["scale"] == 64 ** -0.5 * 1.4426950408889634
            kv, qkv = recs[recs.index(r) - 3], recs[recs.index(r) - 1]      # the two segments are read where their GEMMs wrote them
            assert (r.operands["k_x"].buf, r.operands["vt_x"].buf) == (kv.operands["out1"].buf, kv.operands["out2"].buf)
            assert (r.operands["q"].buf, r.operands["k_l"].buf, r.operands["vt_l"].buf) == (qkv.operands["out"].buf, qkv.operands["out1"].buf, qkv.operands["out2"].buf)
        if r.name.endswith("attn.to_kv"):
            assert a["split"][:2] == (0, 768) and a["split"][5] == 264 and a["N"] == 1536 and a["bias"] is None and (a["batch"], a["h_in"]) == (B, 257)
        if r.name.endswith("attn.qkv"):
            assert a["split"][:2] == (768, 768) and a["split"][5] == 16 and a["N"] == 2304 and a["bias"] is None and (a["batch"], a["h_in"]) == (B, 16)
        if r.name.endswith("ff.fc1"):
            assert a["out_dtype"] == ops.OUT_F32 and a["act"] == ops.ACT_NONE and a["bias"] is None and a["N"] == 3072
        if r.op == "gelu":
            assert (a["rows"], a["cols"]) == (B * 16, 3072)
            assert r.operands["x"].buf == recs[recs.index(r) - 1].operands["out"].buf   # fc1's fp32 output is what the GELU rounds
        if r.name.endswith(("attn.to_out", "ff.fc2")):
            assert a["residual"] is not None and a["bias"] is None and a["act"] == ops.ACT_NONE
        if r.name in ("proj_in", "proj_out"):
            assert a["bias"] is not None and a["residual"] is None
        if r.op == "replicate":
            assert (a["nbytes"], a["copies"]) == (16 * 768 * 2, B)
    # every operand inside its live buffer (tests/_extents.py, tests/_extents_vision.py, tests/_extents_resampler.py)
    for r in recs:
        dims = {k: (v if v is None or isinstance(v, (int, float, str, bool)) else (tuple(True if not isinstance(x, (int, float)) else x for x in v)
                                                                                   if isinstance(v, tuple) else True))
                for k, v in r.kw.items() if k != "name"}
        ext = XR.EXTENTS[r.op](**dims) if r.op in XR.EXTENTS else (XV.EXTENTS[r.op](**dims) if r.op in XV.EXTENTS else X.extents(r.op, **dims))
        assert r.operands, r.name
        for name, o in r.operands.items():
            assert name in ext, (r.name, name)
            if o.kind == "buf":
                assert not o.freed and ext[name][0] <= o.avail, (r.name, name, ext[name][0], o.avail)


def test_plan_digests_are_the_parent_commit_s():
    """tools/plan_digest.py on this tree against its output on the parent commit (tests/golden/plan_digests_before_resampler.txt):
    no existing job's plan moved a launch."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import plan_digest as PD
    finally:
        sys.path.pop(0)
    want = [ln.split() for ln in open(os.path.join(ROOT, "tests", "golden", "plan_digests_before_resampler.txt")).read().splitlines() if ln.strip()]
    kinds = PD.cpu_kinds() + PD.model_kinds()
    assert len(want) == len(kinds) == 27
    for (kind, build), line in zip(kinds, want):
        n, sha = PD.record(build)
        assert " ".join(line[:-2]) == kind and (str(n), sha) == (line[-2], line[-1]), kind


# ------------------------------------------------------------------------------------------------------------------- pipeline
class _Tower:
    """Stands in for models.ClipVisionEncoder: counts its calls, returns seeded hidden states that depend on the pixels."""

    def __init__(self):
        self.weights_version, self.calls = 1, 0

    def predict_on_batch(self, px, output="image_embeds"):
        assert px.shape == (1, 224, 224, 3) and px.dtype == np.float32 and output == "penultimate"
        self.calls += 1
        seed = int(np.float64(px.astype(np.float64).sum()) * 1000) % (1 << 31)
        return (1.2 * np.random.default_rng([seed, self.weights_version]).standard_normal((1, 257, 1280))).astype(np.float32)


def _pipeline():
    from minsdtf_amd import resampler as R
    from minsdtf_amd.models import IPAdapter
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    sd = StableDiffusionBase(64, 64)
    plus = IPAdapter.synthetic_plus(0, depth=1, device=CPU)
    rs = plus.resampler
    rs.calls = 0

    def predict(hidden):
        rs.calls += 1
        return (R.forward_host(rs.state, hidden) + (rs.weights_version - 1)).astype(np.float32)

    rs.predict_on_batch = predict
    return sd, plus, _Tower()


PIC, PIC2 = np.full((32, 48, 3), 100, dtype=np.uint8), np.full((32, 48, 3), 200, dtype=np.uint8)


def test_a_picture_and_a_plus_adapter_give_the_image_tokens():
    """The test that shows the feature exists: on the parent commit `_ip_inputs` raises "its resampler over the tower's hidden states
    is not part of the package" here.  The adapter is built the way the parent can: 16 tokens, and a settable `resampler`."""
    from minsdtf_amd import ipadapter as ip
    from minsdtf_amd.models import IPAdapter
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    sd = StableDiffusionBase(64, 64)
    m = IPAdapter.synthetic(0, 16, device=CPU)
    m.resampler = types.SimpleNamespace(weights_version=1, predict_on_batch=lambda hidden: np.tanh(hidden[:, :16, :768]).astype(np.float32))
    tower = _Tower()
    sd.clip_vision = tower
    model, (tok_u, tok_c) = sd._ip_inputs(ip.parse(dict(image=PIC, model=m)))
    assert model is m and tower.calls == 2
    assert tok_u.shape == tok_c.shape == (16, 768) and tok_u.dtype == tok_c.dtype == np.float32 and not np.array_equal(tok_u, tok_c)


def test_image_prompt_tokens_cache_and_refusals():
    from minsdtf_amd import ipadapter as ip
    from minsdtf_amd import resampler as R
    from minsdtf_amd import vision
    from minsdtf_amd.models import IPAdapter

    sd, plus, tower = _pipeline()
    rs = plus.resampler
    spec = ip.parse(dict(image=PIC, model=plus))
    # no tower: refused, also when a callable is set (it returns the pooled embedding)
    for enc in (None, lambda picture: np.zeros(1024)):
        sd.image_prompt_encoder = enc
        with pytest.raises(ValueError, match=r"^ip_adapter: `image` with a \"plus\" adapter needs.*clip_vision .*clip_vision_path=.*pooled embedding"):
            sd._ip_inputs(spec)
    sd.image_prompt_encoder = None
    with pytest.raises(ValueError, match=r"^ip_adapter: `embeds` with a \"plus\" adapter.*`image`.*`tokens`"):
        sd._ip_inputs(ip.parse(dict(embeds=np.zeros(1024), model=plus)))
    assert rs.calls == 0
    # tokens= works as today
    tk = np.random.default_rng(0).standard_normal((16, 768))
    model, (neg, pos) = sd._ip_inputs(ip.parse(dict(tokens=tk, model=plus)))
    assert model is plus and np.array_equal(pos, tk.astype(np.float32)) and not neg.any() and rs.calls == 0
    # the picture: both networks on it and on the zero-normalised picture
    sd.clip_vision = tower
    tok_u, tok_c = sd.image_prompt_tokens(PIC, plus)
    assert (tower.calls, rs.calls) == (2, 2) and tok_u.shape == tok_c.shape == (16, 768) and tok_u.dtype == tok_c.dtype == np.float32
    px = vision.preprocess(PIC)
    seedless = _Tower()
    assert np.array_equal(tok_c, R.forward_host(rs.state, seedless.predict_on_batch(px[None], output="penultimate")).astype(np.float32)[0])
    assert np.array_equal(tok_u, R.forward_host(rs.state, seedless.predict_on_batch(vision.zero_normalised_pixels()[None], output="penultimate")).astype(np.float32)[0])
    model, (u2, c2) = sd._ip_inputs(spec)
    assert model is plus and np.array_equal(u2, tok_u) and np.array_equal(c2, tok_c)
    # the same picture runs nothing; the caller's copies are its own
    tok_c[:] = 0.0
    assert sd.image_prompt_tokens(PIC.astype(np.float32), plus)[1].any() and (tower.calls, rs.calls) == (2, 2)
    # another picture runs each network once: not the negative
    u3, c3 = sd.image_prompt_tokens(PIC2, plus)
    assert (tower.calls, rs.calls) == (3, 3) and np.array_equal(u3, tok_u) and not np.array_equal(c3, c2)
    sd.image_prompt_tokens(PIC, plus)
    assert (tower.calls, rs.calls) == (4, 4)   # (one picture is kept)
    # a new weights_version on either model, or on the adapter, invalidates both entries
    tower.weights_version = 2
    u4, c4 = sd.image_prompt_tokens(PIC, plus)
    assert (tower.calls, rs.calls) == (6, 6) and not np.array_equal(u4, tok_u) and not np.array_equal(c4, c2)
    rs.weights_version += 1
    u5, _c5 = sd.image_prompt_tokens(PIC, plus)
    assert (tower.calls, rs.calls) == (8, 8) and not np.array_equal(u5, u4)
    plus.weights_version += 1
    sd.image_prompt_tokens(PIC, plus)
    assert (tower.calls, rs.calls) == (10, 10)
    sd.image_prompt_tokens(PIC, plus)
    assert (tower.calls, rs.calls) == (10, 10)
    # 16 tokens and no resampler: today's error
    sixteen = IPAdapter.synthetic(0, 16, device=CPU)
    with pytest.raises(ValueError, match="^ip_adapter: `image` with a \"plus\" adapter.*tokens="):
        sd._ip_inputs(ip.parse(dict(image=PIC, model=sixteen)))
    with pytest.raises(ValueError, match="^image_prompt_tokens: the adapter has no resampler"):
        sd.image_prompt_tokens(PIC, sixteen)
    with pytest.raises(ValueError, match="17 `tokens`|tokens"):
        sd._ip_inputs(ip.parse(dict(tokens=tk[:4], model=plus)))
    assert (tower.calls, rs.calls) == (10, 10)


def test_the_negative_picture_is_zero_to_fp32_rounding():
    from minsdtf_amd import vision

    px = vision.zero_normalised_pixels()
    scale, shift = vision.pixel_affine()
    assert px.shape == (224, 224, 3) and px.dtype == np.float32 and np.array_equal(px, np.broadcast_to(px[0, 0], px.shape))
    x = px.astype(np.float64) * np.asarray(scale) + np.asarray(shift)
    # pixel = 255 mean rounded to fp32: relative 2^-24, so |x| <= 2^-24 |shift|
    assert float(np.abs(x).max()) <= 2.0 ** -24 * max(abs(s) for s in shift)
    assert np.allclose(px[0, 0], 255.0 * np.asarray(vision.MEAN), rtol=1e-6)
    assert vision.digest(vision.preprocess(px)) == vision.digest(px)   # a 224 x 224 float picture passes preprocess unchanged
