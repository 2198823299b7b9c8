"""Perturbed-attention guidance without a GPU: the job description and every ValueError of minsdtf_amd/pag.py, the two weight
planes, the host combine against float64, generate_image's refusals and size cap (raised before any device work), the library's
export, the struct layout and the argument checks of msd_attention_identity, and the two oracle fixture files."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


# ------------------------------------------------------------------------------------------------------------------ parse
def test_parse_accepts():
    from minsdtf_amd import engine, pag

    assert pag.parse(None) is None
    d = pag.parse(pag.PagSpec())
    assert d.scale == 3.0 and d.layers == frozenset({"mid_block.attentions.0"}) and d.key == ("mid_block.attentions.0",)
    assert pag.parse({}) == d and pag.parse(dict(scale=3, layers=["mid"])) == d and pag.parse(d) is d
    assert pag.parse(dict(layers="mid_block.attentions.0")) == d
    names = pag.layer_names()
    assert len(names) == 16 == len(set(names)) and tuple(names) == tuple(engine.PAG_LAYERS)
    assert [n + ".transformer_blocks.0.attn2" for n in names] == [n for n, _c in engine.UNET_ATTN_LAYERS]
    every = pag.parse(pag.PagSpec(scale=0.5, layers=list(names) + ["mid"]))
    assert every.layers == frozenset(names) and every.scale == 0.5 and every.key == tuple(sorted(names))
    assert pag.parse(dict(scale=0)).scale == 0.0
    assert pag.parse(dict(scale=np.float32(1.5), layers=("up_blocks.2.attentions.2", "mid"))).key == \
        ("mid_block.attentions.0", "up_blocks.2.attentions.2")


@pytest.mark.parametrize("bad, match", [
    (dict(scale=3.0, layer="mid"), "unknown field"), (dict(strength=1.0), "unknown field"),
    (dict(scale=float("nan")), "scale"), (dict(scale=float("inf")), "scale"), (dict(scale=-0.5), "scale"), (dict(scale="much"), "scale"),
    (dict(scale=None), "scale"),
    (dict(layers="middle"), "unknown layer"), (dict(layers=["mid", "up_blocks.0.attentions.0"]), "unknown layer"),
    (dict(layers=["down_blocks.3.attentions.0"]), "unknown layer"), (dict(layers=[7]), "unknown layer"),
    (dict(layers="mid_block.attentions.0.transformer_blocks.0.attn1"), "unknown layer"),
    (dict(layers=[]), "no layer"), (dict(layers=None), "no layer"),
    ("mid", "PagSpec"), (3.0, "PagSpec"),
])
def test_parse_rejects(bad, match):
    from minsdtf_amd import pag

    with pytest.raises(ValueError, match=match):
        pag.parse(bad)


# ---------------------------------------------------------------------------------------------------------------- weights
@pytest.mark.parametrize("scale, guidance", [(3.0, 7.5), (0.7, 1.0), (5.0, 0.3), (3.0, 0.0), (0.1, 0.0), (0.0, 7.5)])
def test_weight_planes(scale, guidance):
    """fp32(1 + k) and fp32(-k), k = s / g in float64 with guidance and s without."""
    from minsdtf_amd import pag

    k = np.float64(scale) / np.float64(guidance) if guidance > 0 else np.float64(scale)
    w = pag.weights(scale, guidance, 5, 7)
    assert w.dtype == np.float32 and w.shape == (2, 5, 7) and pag.factor(scale, guidance) == k
    np.testing.assert_array_equal(w[0], np.full((5, 7), np.float32(1.0 + k)))
    np.testing.assert_array_equal(w[1], np.full((5, 7), np.float32(-k)))


def test_combine_host_against_float64():
    """c' = fp32(fma(w1, p, fp32(w0 * c))): two roundings.  With s_1 = w0 c and s_2 = w0 c + w1 p exact: |v_1 - s_1| <= u |s_1|,
    |v_2 - s_2| <= (1 + u) u |s_1| + u |s_2| <= u (2 + u) (|w0| + |w1|) max(|c|, |p|), u = 2^-24 - held to 3 u of that magnitude.
    (The reference reads the same fp32 planes, so their own rounding is no part of the error.)"""
    from minsdtf_amd import pag

    rng = np.random.default_rng(5)
    c, p = (rng.standard_normal((3, 5, 7, 4)).astype(np.float32) for _ in range(2))
    for scale, guidance in ((3.0, 7.5), (2.5, 0.0), (0.3, 12.0)):
        w = pag.weights(scale, guidance, 5, 7)
        got = pag.combine_host(c, p, w)
        assert got.dtype == np.float32 and got.shape == c.shape
        w64 = w.astype(np.float64)
        want = w64[0][None, :, :, None] * c.astype(np.float64) + w64[1][None, :, :, None] * p.astype(np.float64)
        mag = (abs(w64[0, 0, 0]) + abs(w64[1, 0, 0])) * max(np.abs(c).max(), np.abs(p).max())
        assert np.abs(got - want).max() <= 3 * 2.0 ** -24 * mag
        k = pag.factor(scale, guidance)   # and it is the formula: c + k (c - p)
        np.testing.assert_allclose(got, c.astype(np.float64) + k * (c.astype(np.float64) - p), rtol=0, atol=1e-6 * mag)
    # p == c: the planes sum to 1 within fp32 rounding of each
    same = pag.combine_host(c, c, pag.weights(3.0, 7.5, 5, 7))
    assert np.abs(same - c).max() <= 4 * 2.0 ** -24 * 1.8 * np.abs(c).max()


# ------------------------------------------------------------------------------------------------- generate_image, no device
def test_refused_names_every_excluded_argument():
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    what, arguments, states = StableDiffusionBase._REFUSED["pag"]
    assert "text-to-image" in what
    assert set(arguments) == {"regions", "tiled", "hires", "control_net_image", "reference_image", "inpaint_mask"}
    assert tuple(states) == ("denoise_streams = 2",)


def test_refusals_and_the_cap_come_before_any_device_work():
    from minsdtf_amd import regions, tiled
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    ctx = np.zeros((77, 768), dtype=np.float32)
    img = np.zeros((64, 64, 3), dtype=np.uint8)
    sd = StableDiffusionBase(64, 64)   # (no models behind it: anything that reaches a model fails another way)
    kw = dict(batch_size=1, num_steps=3, seed=0, pag=dict(scale=3.0))
    halves = dict(regions=[dict(prompt=ctx, mask=m) for m in regions.boxes(8, 8, 1, 2)])
    for extra, names in ((dict(tiled=dict(size=(64, 128))), ["tiled"]), (dict(hires=dict(scale=2)), ["hires"]),
                         (dict(regions=halves), ["regions"]),
                         (dict(control_net_image=img.astype(np.float32)), ["control_net_image"]),
                         (dict(reference_image=img), ["reference_image"]), (dict(inpaint_mask=img[..., 0]), ["inpaint_mask"]),
                         (dict(reference_image=img, inpaint_mask=img[..., 0]), ["reference_image", "inpaint_mask"])):
        with pytest.raises(ValueError, match="pag is") as e:
            sd.generate_image(ctx, **kw, **extra)
        assert all(n in str(e.value) for n in names), str(e.value)
    two = StableDiffusionBase(64, 64)
    two.denoise_streams = 2
    with pytest.raises(ValueError, match="pag.*denoise_streams"):
        two.generate_image(ctx, **kw)
    with pytest.raises(ValueError, match="pag is"):
        sd.text_to_image(ctx, tiled=dict(size=(64, 128)), **kw)
    # the cap: 3 * batch_size (2 * batch_size without guidance) <= 2 * tiled.MAX_VIEW_BATCH UNet rows
    assert 2 * tiled.MAX_VIEW_BATCH == 12
    with pytest.raises(ValueError, match=r"15 UNet rows.*MAX_VIEW_BATCH = 12"):
        sd.generate_image(ctx, **{**kw, "batch_size": 5})
    with pytest.raises(ValueError, match=r"14 UNet rows.*MAX_VIEW_BATCH = 12"):
        sd.generate_image(ctx, unconditional_guidance_scale=0.0, **{**kw, "batch_size": 7})
    # a bad description is a ValueError of its own
    with pytest.raises(ValueError, match="unknown field"):
        sd.generate_image(ctx, batch_size=1, num_steps=3, pag=dict(scales=3.0))
    with pytest.raises(ValueError, match="unknown layer"):
        sd.generate_image(ctx, batch_size=1, num_steps=3, pag=dict(layers="top"))
    assert not sd._engines


def test_engine_key_holds_the_layers_and_never_the_scale():
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    class Net:
        weights_version = 1

    sd = StableDiffusionBase(64, 64)
    sd.diffusion_model = Net()
    args = (1, 77, 77, 4, 7.5, 0.0, False)
    plain = sd._engine_key(*args)
    assert sd._engine_key(*args, pag=None) == plain
    mid = sd._engine_key(*args, pag=("mid_block.attentions.0",))
    assert mid != plain and mid[:len(plain)] == plain and mid[-1] == ("pag", ("mid_block.attentions.0",))
    two = sd._engine_key(*args, pag=frozenset({"up_blocks.2.attentions.2", "mid_block.attentions.0"}))
    assert two[-1] == ("pag", ("mid_block.attentions.0", "up_blocks.2.attentions.2")) and two != mid
    assert not any(isinstance(v, float) and v == 3.0 for v in mid)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_library_exports_attention_identity():
    from minsdtf_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    assert "msd_attention_identity" in _lib.SYMBOLS and _lib.ABI_VERSION == 12
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "msd_attention_identity" in {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "minsdtf_hip.h")).read()
    assert "#define MSD_ABI_VERSION 12" in header and "MSD_API int msd_attention_identity(" in header
    lib = _lib.load()
    assert lib.msd_abi_version() == 12


def _block(**kw):
    from minsdtf_amd import _lib

    s = _lib.MsdAttentionIdentity()
    good = dict(vt=1 << 20, out=1 << 24, batch=2, channels=320, s=35, vt_ld=40, o_ld=320)
    for k, v in {**good, **kw}.items():
        setattr(s, k, v)
    return s


@pytest.mark.parametrize("bad, word", [
    (dict(vt=None), b"null"), (dict(out=None), b"null"), (dict(vt=(1 << 20) + 8), b"aligned"), (dict(out=(1 << 24) + 2), b"aligned"),
    (dict(batch=0), b"batch"), (dict(batch=65536), b"batch"), (dict(s=0), b"s = 0"), (dict(channels=0), b"channels"),
    (dict(channels=324), b"channels"), (dict(vt_ld=36), b"vt_ld"), (dict(vt_ld=32), b"vt_ld"), (dict(o_ld=312), b"o_ld"),
    (dict(o_ld=324), b"o_ld"), (dict(batch=4096, channels=1280, s=512, vt_ld=512, o_ld=1280), b"2^31"),
    (dict(batch=4096, channels=8, s=2048, vt_ld=2048, o_ld=320), b"2^31"),
    (dict(out=1 << 20), b"overlaps"), (dict(out=(1 << 20) + 2 * 320 * 40 * 2 - 16), b"overlaps"),
    (dict(vt=(1 << 24) + 2 * 35 * 320 * 2 - 16), b"overlaps"),
])
def test_argument_errors_need_no_device(bad, word):
    """Every bad call returns MSD_E_ARG (-1) with a message before anything is launched (the pointers are never followed)."""
    from minsdtf_amd import _lib

    lib = _lib.load()
    assert lib.msd_attention_identity(None, None) == -1 and b"null" in lib.msd_last_error()
    assert lib.msd_attention_identity(ctypes.byref(_block(**bad)), None) == -1, bad
    assert word in lib.msd_last_error(), (bad, lib.msd_last_error())


def test_struct_layout_matches_header():
    from minsdtf_amd import _lib

    fields = ("out", "batch", "channels", "s", "vt_ld", "o_ld")
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "minsdtf_hip.h"\nint main(){printf("%zu' + " %zu" * len(fields) + \
          '\\n", sizeof(MsdAttentionIdentity)' + "".join(f", offsetof(MsdAttentionIdentity, {f})" for f in fields) + ");return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    t = _lib.MsdAttentionIdentity
    assert sizes == [ctypes.sizeof(t)] + [getattr(t, f).offset for f in fields]


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("tag, size, layers, sampler, batch, rescale", [
    ("a", 128, ("mid_block.attentions.0",), "", 1, 0.0),
    ("b", 64, ("down_blocks.1.attentions.0", "mid_block.attentions.0", "up_blocks.2.attentions.2"), "dpmpp_2m", 2, 0.7),
])
def test_fixture_files(tag, size, layers, sampler, batch, rescale):
    """tools/make_pag_fixtures.py's two files: the recorded inputs are the issue's, and the plain job lies below 30 dB of the PAG
    latent, so the 40 dB bar of tests/test_pag_gpu.py tells a PAG job from a job without PAG."""
    from minsdtf_amd import pag

    path = os.path.join(GOLD, f"oracle_pag_{tag}.npz")
    assert os.path.exists(path) and os.path.getsize(path) < (1 << 20)
    g = np.load(path)
    assert float(g["plain_psnr"]) < 30.0
    assert (int(g["weight_seed"]), float(g["bias_scale"]), int(g["context_seed"]), int(g["noise_seed"])) == (0, 0.05, 1234, 0)
    assert (float(g["guidance"]), int(g["steps"]), float(g["guidance_rescale"])) == (7.5, 4, rescale)
    assert (int(g["size"]), str(g["sampler"]), int(g["batch"])) == (size, sampler, batch)
    assert tuple(str(n) for n in g["layers"]) == layers and float(g["scale"]) >= 3.0
    assert pag.parse(dict(scale=float(g["scale"]), layers=[str(n) for n in g["layers"]])).layers == frozenset(layers)
    assert g["latent"].shape == (batch, size // 8, size // 8, 4) and g["latent"].dtype == np.float32
    assert np.all(np.isfinite(g["latent"]))


# ------------------------------------------------------------------------------------------------------------- the recorded plan
def _walk(latent_mod, nb, **kw):
    """Every call emit_unet records at 16 x 16 (tests/_layer_walk.py's tensor-less walk: nothing is launched), as (op, name,
    batch, vt / out byte offsets of the attention calls)."""
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from _layer_walk import _AnyWeights, _Tensor

    from minsdtf_amd import engine

    out, orig = [], engine.Plan.rec

    def rec(self, fn, **k):   # (a whole buffer is an engine.Buf, a part of one an engine.BufView with its byte offset in .off)
        extra = tuple(getattr(k[n], "off", 0) for n in ("vt", "out")) if fn.__name__.startswith("attention") else ()
        out.append((fn.__name__, k.get("name"), k.get("batch")) + extra)
        return orig(self, fn, **k)

    engine.Plan.rec = rec
    try:
        p = engine.Plan("cpu")
        e = engine.Emitter(p, _AnyWeights())
        ctx = engine.Act(p.alloc(nb * 77 * 768 * 2), nb, 77, 1, 768)
        kv = engine.emit_context_kv(e, ctx, engine.UNET_ATTN_LAYERS, p)
        out.clear()
        engine.emit_unet(e, _Tensor(), latent_mod, nb, 16, 16, (_Tensor(), 0, 0, engine.temb_columns(False)), kv, 77, _Tensor(), None, variant=engine.UNetVariant(**kw))
    finally:
        engine.Plan.rec = orig
    return out


def test_no_perturbed_rows_record_the_plain_plan():
    plain = _walk(2, 6)
    assert _walk(2, 6, pag_layers=None, perturbed=0) == plain
    assert _walk(2, 6, pag_layers=frozenset({"mid_block.attentions.0"}), perturbed=0) == plain
    assert not any(op == "attention_identity" for op, *_ in plain)
    assert sum(name.endswith(".replicate") for _op, name, *_ in plain) == 3   # the shared prefix (resnet, to_out rows, their moments)


def test_perturbed_rows_in_the_recorded_plan():
    """The last 2 of 6 rows perturbed in two blocks (8 x 8 = 64 tokens at C = 640; 2 x 2 = 4 tokens, padded to 8, at C = 1280):
    msd_attention on the first 4 rows at the base pointers, msd_attention_identity on the last 2 at the offset pointers, every
    other call as in the plain plan."""
    layers = frozenset({"down_blocks.1.attentions.1", "mid_block.attentions.0"})
    plain, got = _walk(2, 6), _walk(2, 6, pag_layers=layers, perturbed=2)
    rest = [c for c in got if c[0] != "attention_identity"]
    assert len(rest) == len(plain) and len(got) == len(plain) + 2
    for a, b in zip(plain, rest):
        blk = (a[1] or "").split(".transformer_blocks.0.attn1")[0]
        if a[0] == "attention" and a[1].endswith(".attn1") and blk in layers:
            assert b == (a[0], a[1], 4, 0, 0) and a[2] == 6
        else:
            assert a == b
    tb = ".transformer_blocks.0.attn1"
    i = got.index(("attention", "down_blocks.1.attentions.1" + tb, 4, 0, 0))
    assert got[i + 1] == ("attention_identity", "down_blocks.1.attentions.1" + tb + ".identity", 2, 4 * 640 * 64 * 2, 4 * 64 * 640 * 2)
    i = got.index(("attention", "mid_block.attentions.0" + tb, 4, 0, 0))
    assert got[i + 1] == ("attention_identity", "mid_block.attentions.0" + tb + ".identity", 2, 4 * 1280 * 8 * 2, 4 * 4 * 1280 * 2)
    # every row perturbed (predict_perturbed): the attention launch is gone
    every = _walk(2, 2, pag_layers=layers, perturbed=2)
    names = [(op, name) for op, name, *_ in every]
    for blk in layers:
        assert ("attention", blk + tb) not in names and ("attention_identity", blk + tb + ".identity") in names
    assert len(every) == len(_walk(2, 2))


def test_first_block_selected_shares_nothing():
    from minsdtf_amd import engine

    first = engine.PAG_LAYERS[0]
    got = _walk(2, 6, pag_layers=frozenset({first}), perturbed=2)
    assert not any((name or "").endswith(".replicate") for _op, name, *_ in got)
    tb = first + ".transformer_blocks.0.attn1"
    assert ("attention", tb, 4, 0, 0) in got and ("attention_identity", tb + ".identity", 2, 4 * 320 * 256 * 2, 4 * 256 * 320 * 2) in got
    with pytest.raises(ValueError, match="unknown attention block"):
        _walk(2, 6, pag_layers=frozenset({"mid"}), perturbed=2)
