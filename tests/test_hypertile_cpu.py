"""HyperTile without a GPU: the job description and its errors, the refusal table, the per-level geometry, the float64 statement of
the kernel against a plain loop over windows, the C ABI (export, struct layout, argument checks), the recorded plan of a windowed
job and the operand extents of every windowed launch, and the committed oracle fixtures."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _extents_hypertile as XH
import _layer_walk as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


# ------------------------------------------------------------------------------------------------------------- the description
def test_parse_accepts():
    from minsdtf_amd import hypertile as HT

    assert HT.parse(None) is None
    r = HT.parse({"tile": 512})
    assert r == HT.Resolved((512, 512), 0) and HT.parse(r) is r
    assert HT.parse(HT.HypertileSpec()) == r
    assert HT.parse(dict(tile=(256, 128), depth=1)) == HT.Resolved((256, 128), 1)
    assert HT.parse(dict(tile=np.int64(256), depth=np.int32(2))) == HT.Resolved((256, 256), 2)
    assert HT.parse(dict(tile=[64, 192])).tile == (64, 192)
    assert r.windows(1024, 1536) == (2, 3) and r.key(1024, 512) == (2, 1, 0)
    assert r.key(512, 512) == (1, 1, 0)   # one window: generate_image runs the plain job


@pytest.mark.parametrize("bad, match", [
    (dict(tile=512, depht=0), "unknown field"),
    ("512", "HypertileSpec, a dict or None"),
    (dict(tile=512, depth=3), "depth"), (dict(tile=512, depth=-1), "depth"), (dict(tile=512, depth=0.0), "depth"),
    (dict(tile=512, depth=True), "depth"),
    (dict(tile="512"), "tile"), (dict(tile=(512,)), "tile"), (dict(tile=(512, 512, 512)), "tile"), (dict(tile=0), "tile"),
    (dict(tile=-64), "tile"), (dict(tile=512.0), "tile"), (dict(tile=None), "tile"),
    (dict(tile=96), r"not a multiple of 64 px.*64, 128"),
    (dict(tile=32), r"not a multiple of 64 px.*nearest valid tiles are 64$"),
    (dict(tile=64, depth=1), r"not a multiple of 128 px.*nearest valid tiles are 128$"),
    (dict(tile=(256, 384), depth=2), r"384 is not a multiple of 256 px.*256, 512"),
])
def test_parse_rejects(bad, match):
    from minsdtf_amd import hypertile as HT

    with pytest.raises(ValueError, match=match):
        HT.parse(bad)


def test_a_tile_that_does_not_divide_the_picture_names_the_nearest_valid_tiles():
    from minsdtf_amd import hypertile as HT

    assert HT.valid_tiles(768, 0) == [64, 128, 192, 256, 384, 768] and HT.valid_tiles(768, 2) == [256, 768]
    assert HT.valid_tiles(1024, 1) == [128, 256, 512, 1024] and HT.valid_tiles(200, 0) == []
    assert HT.nearest_tiles(768, 320, 0) == [256, 384] and HT.nearest_tiles(768, 832, 0) == [768] and HT.nearest_tiles(768, 32, 0) == [64]
    with pytest.raises(ValueError, match=r"tile height 320 does not divide the picture's height 768 px.*256, 384"):
        HT.parse(dict(tile=320)).windows(768, 640)
    with pytest.raises(ValueError, match=r"tile width 512 does not divide the picture's width 768 px.*depth 1 are 384, 768"):
        HT.parse(dict(tile=512, depth=1)).windows(1024, 768)
    with pytest.raises(ValueError, match="none"):
        HT.parse(dict(tile=128)).windows(200, 200)


def test_level_geometry():
    from minsdtf_amd import hypertile as HT

    # a 1024 x 1024 picture with tile 512 at depth 2: 2 x 2 windows at every level
    assert HT.level_geometry(128, 128, 2, 2, 2) == [(128, 128, 64, 64), (64, 64, 32, 32), (32, 32, 16, 16)]
    assert HT.level_geometry(32, 16, 4, 2, 0) == [(32, 16, 8, 8)]
    assert HT.level_geometry(32, 32, 2, 2, 1) == [(32, 32, 16, 16), (16, 16, 8, 8)]
    assert HT.level_geometry(24, 16, 3, 1, 0) == [(24, 16, 8, 16)]
    # every accepted spec gives windows whose width is a multiple of 8 tokens at its deepest level
    for depth in range(3):
        unit = 64 << depth
        spec = HT.parse(dict(tile=(unit, 2 * unit), depth=depth))
        nh, nw, d = spec.key(4 * unit, 4 * unit)
        geo = HT.level_geometry(4 * unit // 8, 4 * unit // 8, nh, nw, d)
        assert len(geo) == depth + 1 and geo[-1][2:] == (8, 16) and all(g[3] % 8 == 0 for g in geo)
    for bad in ((16, 16, 4, 4, 0), (16, 16, 2, 2, 1), (16, 16, 3, 1, 0), (16, 16, 1, 1, 3), (16, 16, 0, 1, 0), (12, 16, 1, 1, 2)):
        with pytest.raises(ValueError, match="hypertile"):
            HT.level_geometry(*bad)


def test_window_tokens():
    from minsdtf_amd import hypertile as HT

    t = HT.window_tokens(4, 6, 2, 3)
    assert t.shape == (4, 6)
    assert t[0].tolist() == [0, 1, 2, 6, 7, 8] and t[1].tolist() == [3, 4, 5, 9, 10, 11] and t[3].tolist() == [15, 16, 17, 21, 22, 23]
    assert sorted(t.ravel().tolist()) == list(range(24))
    with pytest.raises(ValueError):
        HT.window_tokens(4, 6, 3, 3)


@pytest.mark.parametrize("h, w, wh, ww", [(16, 16, 8, 8), (24, 16, 12, 8), (8, 48, 8, 24), (9, 8, 9, 8), (6, 4, 3, 2)])
def test_float64_reference_against_a_plain_loop_over_windows(h, w, wh, ww):
    """The statement against the definition, token by token: token (y, x) belongs to window (y / wh, x / ww), and a query's
    result is the base-2 softmax average of v over the keys of its own window."""
    from minsdtf_amd import hypertile as HT

    rng = np.random.default_rng(7)
    B, H, d = 2, 2, 5
    S, C = h * w, H * d
    q, k, v = (rng.standard_normal((B, S, C)) for _ in range(3))
    got = HT.attention_windowed_reference(q, k, v, H, h, w, wh, ww)
    assert got.shape == (B, S, C) and got.dtype == np.float64
    want = np.empty_like(got)
    for b in range(B):
        for hd in range(H):
            sl = slice(hd * d, (hd + 1) * d)
            for y in range(h):
                for x in range(w):
                    keys = [yy * w + xx for yy in range(y // wh * wh, y // wh * wh + wh) for xx in range(x // ww * ww, x // ww * ww + ww)]
                    s = k[b, keys, sl] @ q[b, y * w + x, sl]
                    p = np.exp2(s - s.max())
                    want[b, y * w + x, sl] = (p / p.sum()) @ v[b, keys, sl]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    # one window is the plain attention
    whole = HT.attention_windowed_reference(q, k, v, H, h, w, h, w)
    s = np.einsum("bshd,bthd->bhst", q.reshape(B, S, H, d), k.reshape(B, S, H, d))
    p = np.exp2(s - s.max(-1, keepdims=True))
    plain = np.einsum("bhst,bthd->bshd", p / p.sum(-1, keepdims=True), v.reshape(B, S, H, d)).reshape(B, S, C)
    np.testing.assert_allclose(whole, plain, rtol=0, atol=1e-12)
    if (wh, ww) != (h, w):
        assert np.abs(got - plain).max() > 1e-3
    with pytest.raises(ValueError):
        HT.attention_windowed_reference(q, k, v, H, h + 1, w, wh, ww)


# ------------------------------------------------------------------------------------------------- generate_image, no device
def test_refused_names_every_excluded_argument():
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    what, arguments, states = StableDiffusionBase._REFUSED["hypertile"]
    assert "text-to-image" in what
    assert set(arguments) == {"tiled", "regions", "pag", "reference_only", "control_net_image", "inpaint_mask", "reference_image"}
    assert set(states) == {"denoise_streams = 2"}   # (host_loop=True and a TCD pipeline are served)


def test_refusals_come_before_any_device_work():
    from minsdtf_amd import regions
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    ctx = np.zeros((77, 768), dtype=np.float32)
    img = np.zeros((128, 128, 3), dtype=np.uint8)
    sd = StableDiffusionBase(128, 128)   # (no models behind it: anything that reaches a model fails another way)
    kw = dict(batch_size=1, num_steps=3, seed=0, hypertile=dict(tile=64))
    halves = dict(regions=[dict(prompt=ctx, mask=m) for m in regions.boxes(16, 16, 1, 2)])
    z = np.zeros((1, 16, 16, 4), dtype=np.float32)
    for extra, names in ((dict(tiled=dict(size=(128, 256))), ["tiled"]), (dict(regions=halves), ["regions"]),
                         (dict(pag=dict(scale=3.0)), ["pag"]), (dict(reference_only=dict(latent=z)), ["reference_only"]),
                         (dict(control_net_image=img.astype(np.float32)), ["control_net_image"]),
                         (dict(reference_image=img), ["reference_image"]), (dict(inpaint_mask=img[..., 0]), ["inpaint_mask"]),
                         (dict(pag=dict(scale=3.0), inpaint_mask=img[..., 0]), ["pag", "inpaint_mask"])):
        with pytest.raises(ValueError, match="hypertile is") as e:
            sd.generate_image(ctx, **kw, **extra)
        assert all(n in str(e.value) for n in names), str(e.value)
    two = StableDiffusionBase(128, 128)
    two.denoise_streams = 2
    with pytest.raises(ValueError, match="hypertile.*denoise_streams"):
        two.generate_image(ctx, **kw)
    with pytest.raises(ValueError, match="hypertile is"):
        sd.text_to_image(ctx, tiled=dict(size=(128, 256)), **kw)
    # a bad description and a tile the picture does not take are ValueErrors of their own
    with pytest.raises(ValueError, match="unknown field"):
        sd.generate_image(ctx, batch_size=1, num_steps=3, hypertile=dict(tile=64, deep=1))
    with pytest.raises(ValueError, match="not a multiple of 64"):
        sd.generate_image(ctx, batch_size=1, num_steps=3, hypertile=dict(tile=48))
    with pytest.raises(ValueError, match=r"does not divide the picture's height 128 px.*are 128$"):
        sd.generate_image(ctx, batch_size=1, num_steps=3, hypertile=dict(tile=(192, 64)))
    # with hires the geometry is the target size's: 192 divides 384 but not 128
    with pytest.raises(ValueError, match=r"does not divide the picture's height 256 px.*128, 256"):
        sd.generate_image(ctx, batch_size=1, num_steps=3, hires=dict(scale=2), hypertile=dict(tile=192))
    assert not sd._engines


def test_engine_refuses_direct_construction():
    from minsdtf_amd.jobopts import EngineOptions

    def check(control_net=None, streams=None, inpaint=False, tcd=False, **kw):
        """The options as an engine of batch 2 at 16 x 16 keeps them, behind the check it makes before it allocates anything."""
        e = EngineOptions.of(**kw)
        e.check(16, 16, 2, 7.5, control_net is not None, inpaint, tcd, streams)
        return e

    assert check(hypertile=(2, 2, 0)).hypertile == (2, 2, 0) and check().hypertile is None
    assert check(hypertile=(2, 2, 0), tcd=True, sampler=None).hypertile == (2, 2, 0)
    for kw in (dict(control_net=object()), dict(inpaint=True), dict(streams=2), dict(regions=2), dict(pag=("mid_block.attentions.0",)),
               dict(reference=("mid_block.attentions.0",))):
        with pytest.raises(ValueError, match="hypertile"):
            check(hypertile=(2, 2, 0), **kw)
    with pytest.raises(ValueError, match="hypertile"):
        check(hypertile=(4, 4, 0))     # 4-token windows
    with pytest.raises(ValueError, match="hypertile"):
        check(hypertile=(2, 2, 1))     # 8 x 8 level: 4-token windows
    with pytest.raises(ValueError, match="hypertile"):
        check(hypertile=(2, 2))


def test_engine_key_holds_the_windows_and_the_depth():
    from minsdtf_amd import hypertile as HT
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    class Net:
        weights_version = 1

    sd = StableDiffusionBase(128, 128)
    sd.diffusion_model = Net()
    args = (1, 77, 77, 4, 7.5, 0.0, False)
    plain = sd._engine_key(*args)
    assert sd._engine_key(*args, hypertile=None) == plain
    ka = sd._engine_key(*args, hypertile=HT.parse(dict(tile=64)).key(128, 128))
    assert ka != plain and ka[:len(plain)] == plain and ka[-1] == ("hypertile", 2, 2, 0)
    assert sd._engine_key(*args, hypertile=HT.parse(dict(tile=(64, 64))).key(128, 128)) == ka
    assert sd._engine_key(*args, hypertile=(2, 1, 0)) != ka and sd._engine_key(*args, hypertile=(2, 2, 1)) != ka
    assert sd._engine_key(*args, pag=("mid_block.attentions.0",)) != ka


# ------------------------------------------------------------------------------------------------------------------ the C ABI
NEW = "msd_attention_windowed"
FIELDS = ("q", "k", "vt", "out", "batch", "heads", "head_dim", "h", "w", "wh", "ww", "q_ld", "k_ld", "vt_ld", "o_ld")


def test_library_exports_the_new_entry_point():
    from minsdtf_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    assert NEW in _lib.SYMBOLS and _lib.ABI_VERSION == 12
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "minsdtf_hip.h")).read()
    assert "#define MSD_ABI_VERSION 12" in header
    assert NEW in exported and f"MSD_API int {NEW}(" in header
    assert _lib.load().msd_abi_version() == 12


def test_struct_layout_matches_header():
    from minsdtf_amd import _lib

    struct = "MsdAttentionWindowed"
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "minsdtf_hip.h"\nint main(){printf("%zu' + " %zu" * len(FIELDS) + \
          f'\\n", sizeof({struct})' + "".join(f", offsetof({struct}, {f})" for f in FIELDS) + ");return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    t = getattr(_lib, struct)
    assert [f for f, _t in t._fields_] == list(FIELDS)
    assert sizes == [ctypes.sizeof(t)] + [getattr(t, f).offset for f in FIELDS]


def _windowed(**kw):
    from minsdtf_amd import _lib

    s = _lib.MsdAttentionWindowed()
    # B = 2, H = 2, d = 40, 16 x 16 tokens in 8 x 8 windows: q / k / out 2*256*80*2 = 81920 bytes, vt 2*80*256*2 = 81920
    good = dict(q=1 << 20, k=2 << 20, vt=3 << 20, out=4 << 20, batch=2, heads=2, head_dim=40, h=16, w=16, wh=8, ww=8,
                q_ld=80, k_ld=80, vt_ld=256, o_ld=80)
    for k, v in {**good, **kw}.items():
        setattr(s, k, v)
    return s


@pytest.mark.parametrize("bad, word", [
    (dict(q=None), b"null"), (dict(k=None), b"null"), (dict(vt=None), b"null"), (dict(out=None), b"null"),
    (dict(q=(1 << 20) + 8), b"aligned"), (dict(k=(2 << 20) + 2), b"aligned"), (dict(vt=(3 << 20) + 4), b"aligned"),
    (dict(out=(4 << 20) + 8), b"aligned"),
    (dict(head_dim=64), b"head_dim"), (dict(head_dim=0), b"head_dim"),
    (dict(h=0), b"h = 0"), (dict(w=0), b"w = 0"), (dict(wh=0), b"wh = 0"), (dict(ww=0), b"ww = 0"), (dict(ww=-8), b"ww = -8"),
    (dict(wh=6), b"h % wh"), (dict(ww=24, vt_ld=256), b"w % ww"), (dict(w=12, ww=4, vt_ld=192), b"ww % 8"),
    (dict(w=12, ww=12, vt_ld=192), b"ww % 8"),
    (dict(batch=0), b"batch"), (dict(batch=65536), b"batch"), (dict(heads=0), b"heads"), (dict(heads=65536), b"heads"),
    (dict(q_ld=84), b"multiples of 8"), (dict(vt_ld=260), b"multiples of 8"), (dict(q_ld=72), b"smaller"), (dict(k_ld=72), b"smaller"),
    (dict(o_ld=72), b"smaller"), (dict(vt_ld=248), b"vt_ld"), (dict(h=32, wh=8), b"vt_ld"),
    (dict(batch=65535, heads=65535, q_ld=2621400, k_ld=2621400, o_ld=2621400), b"2^31"),
    (dict(out=1 << 20), b"overlaps"), (dict(out=(1 << 20) + 81920 - 16), b"overlaps"), (dict(out=(2 << 20) - 16), b"overlaps"),
    (dict(out=(2 << 20) + 16), b"overlaps"), (dict(out=(3 << 20) + 81920 - 16), b"overlaps"), (dict(out=(3 << 20) - 81920 + 16), b"overlaps"),
])
def test_argument_errors_need_no_device(bad, word):
    """Every bad call returns MSD_E_ARG (-1) with a message before anything is launched (the pointers are never followed)."""
    from minsdtf_amd import _lib

    lib = _lib.load()
    assert lib.msd_attention_windowed(None, None) == -1 and b"null" in lib.msd_last_error()
    assert lib.msd_attention_windowed(ctypes.byref(_windowed(**bad)), None) == -1, bad
    assert word in lib.msd_last_error(), (bad, lib.msd_last_error())


# ------------------------------------------------------------------------------------------------------------- the recorded plan
GEO = ("batch", "heads", "head_dim", "h", "w", "wh", "ww", "s", "t", "q_ld", "k_ld", "vt_ld", "o_ld")


def _walk(latent_mod, nb, hw=16, **kw):
    """Every recorded call of emit_unet: (op, name, its dimensions, the byte offsets of q / k / vt / out)."""
    from minsdtf_amd import engine

    out, orig = [], engine.Plan.rec

    def rec(self, fn, **k):
        names = ("q", "k", "vt", "out") if fn.__name__.startswith("attention") else ()
        out.append((fn.__name__, k.get("name"), tuple((g, k[g]) for g in GEO if isinstance(k.get(g), int))) + tuple(getattr(k[n], "off", 0) for n in names if n in k))
        return orig(self, fn, **k)

    engine.Plan.rec = rec
    try:
        p = engine.Plan("cpu")
        e = engine.Emitter(p, LW._AnyWeights())
        ctx = engine.Act(p.alloc(nb * 77 * 768 * 2), nb, 77, 1, 768)
        kv = engine.emit_context_kv(e, ctx, engine.UNET_ATTN_LAYERS, p)
        out.clear()
        engine.emit_unet(e, LW._Tensor(), latent_mod, nb, hw, hw, (LW._Tensor(), 0, 0, engine.temb_columns(False)), kv, 77, LW._Tensor(), None, variant=engine.UNetVariant(**kw))
    finally:
        engine.Plan.rec = orig
    return out


LEVEL0 = ["down_blocks.0.attentions.0", "down_blocks.0.attentions.1", "up_blocks.3.attentions.0", "up_blocks.3.attentions.1",
          "up_blocks.3.attentions.2"]
TB = ".transformer_blocks.0.attn1"


def test_no_window_records_the_plain_plan():
    """window=None is the parent's plan call for call, at the 512 x 512 default job's shape too (64 x 64 latent, 2 rows, the shared
    prefix): the same launches as tests/test_pag_cpu.py's walk of the plain forward."""
    import test_pag_cpu

    plain = _walk(2, 4)
    assert _walk(2, 4, window=None) == plain and _walk(2, 4, window=None, window_depth=2) == plain
    assert [c[:2] for c in plain] == [c[:2] for c in test_pag_cpu._walk(2, 4)]
    assert not any(op == "attention_windowed" for op, *_ in plain)
    big = _walk(1, 2, hw=64)
    assert _walk(1, 2, hw=64, window=None) == big and not any(op == "attention_windowed" for op, *_ in big)
    assert sum(name.endswith(".replicate") for _op, name, *_ in big) == 3


def test_windowed_job_in_the_recorded_plan():
    """A 128 x 128 px job (16 x 16 latent) with tile 64, 4 rows with the shared prefix: exactly the five level-0 attn1 are
    `.attn1.windowed` with h = w = 16, wh = ww = 8 - the first on the ONE copy of the shared prefix - and every other call is the
    plain plan's."""
    from minsdtf_amd import hypertile as HT

    nh, nw, depth = HT.parse(dict(tile=64)).key(128, 128)
    plain = _walk(2, 4)
    got = _walk(2, 4, window=(nh, nw), window_depth=depth)
    assert len(got) == len(plain)
    wins = [c for c in got if c[0] == "attention_windowed"]
    assert [c[1] for c in wins] == [b + TB + ".windowed" for b in LEVEL0]
    for c in wins:
        geo = dict(c[2])
        assert (geo["h"], geo["w"], geo["wh"], geo["ww"], geo["heads"], geo["head_dim"]) == (16, 16, 8, 8, 8, 40)
        assert (geo["q_ld"], geo["k_ld"], geo["o_ld"], geo["vt_ld"]) == (320, 320, 320, 256)
    assert [dict(c[2])["batch"] for c in wins] == [2, 4, 4, 4, 4]   # (the first block's front runs on one copy of the 2 + 2 rows)
    changed = 0
    for a, b in zip(plain, got):
        if b[0] == "attention_windowed":
            ga, gb = dict(a[2]), dict(b[2])
            assert a[0] == "attention" and a[1] + ".windowed" == b[1] and a[3:] == b[3:]
            assert all(ga[k] == gb[k] for k in ("batch", "heads", "head_dim", "q_ld", "k_ld", "vt_ld", "o_ld")) and ga["s"] == gb["h"] * gb["w"]
            changed += 1
        else:
            assert a == b
    assert changed == 5
    # depth 1 on a 32 x 32 latent with 2 x 2 windows: ten launches, 16- and 8-token windows at d = 40 / 80
    deep = [dict(c[2]) for c in _walk(1, 2, hw=32, window=(2, 2), window_depth=1) if c[0] == "attention_windowed"]
    assert sorted((g["h"], g["wh"], g["ww"], g["head_dim"]) for g in deep) == [(16, 8, 8, 80)] * 5 + [(32, 16, 16, 40)] * 5
    assert sum(c[0] == "attention_windowed" for c in _walk(1, 2, hw=64, window=(2, 2), window_depth=2)) == 15


def test_window_is_not_combined():
    from minsdtf_amd import engine

    with pytest.raises(ValueError, match="window"):
        _walk(2, 4, window=(2, 2), pag_layers=frozenset({"mid_block.attentions.0"}), perturbed=1)
    with pytest.raises(ValueError, match="window"):
        _walk(2, 4, window=(2, 2), region_attn=(2, 2, {}))
    with pytest.raises(ValueError, match="window"):
        _walk(2, 5, window=(2, 2), reference=(frozenset({"mid_block.attentions.0"}), LW._Tensor(), None))
    with pytest.raises(ValueError, match="window_depth"):
        _walk(2, 4, window=(2, 2), window_depth=3)
    with pytest.raises(ValueError, match="windows"):
        _walk(2, 4, window=(4, 4))          # 4-token windows
    with pytest.raises(ValueError, match="windows"):
        _walk(2, 4, window=(2, 2), window_depth=1)
    p = engine.Plan("cpu")
    e = engine.Emitter(p, LW._AnyWeights())
    kv = {"b.transformer_blocks.0.attn2": (LW._Tensor(), LW._Tensor(), 80)}
    for kw in (dict(perturbed=1), dict(reference=1), dict(window=(3, 1)), dict(window=(1, 3)), dict(window=(0, 1))):
        with pytest.raises(ValueError, match="window"):
            e.attentions(p.act(4, 16, 16, 320), "b", kv, 77, variant=engine.AttnVariant(**{"window": (2, 2), **kw}))
    with pytest.raises(ValueError, match="head size"):
        e.attentions(p.act(4, 16, 16, 512), "b", kv, 77, variant=engine.AttnVariant(window=(2, 2)))


def test_every_windowed_launch_fits_its_buffers():
    """tests/test_plan_extents_cpu.py's Fits / Live / Disjoint over a windowed plan: 4 rows at 48 x 64, 3 x 2 windows at depth 2
    (16 x 32, 8 x 16 and 4 x 8 token windows)."""
    from minsdtf_amd import engine

    recs, orig = [], engine.Plan.rec

    def rec(self, fn, **kw):
        ops_ = {k: o for k, o in ((k, LW._operand(v)) for k, v in kw.items() if k != "split") if o is not None}
        recs.append(LW.Rec(fn.__name__, kw.get("name", ""), kw, ops_))
        return orig(self, fn, **kw)

    engine.Plan.rec = rec
    try:
        p = engine.Plan("cpu")
        e = engine.Emitter(p, LW._AnyWeights())
        ctx = engine.Act(p.alloc(4 * 77 * 768 * 2), 4, 77, 1, 768)
        kv = engine.emit_context_kv(e, ctx, engine.UNET_ATTN_LAYERS, p)
        recs.clear()
        engine.emit_unet(e, LW._Tensor(), 2, 4, 48, 64, (LW._Tensor(), 0, 0, engine.temb_columns(False)), kv, 77, LW._Tensor(), None,
                         variant=engine.UNetVariant(window=(3, 2), window_depth=2))
    finally:
        engine.Plan.rec = orig
    checked = 0
    for r in recs:
        if r.op != "attention_windowed":
            continue
        dims = {k: (v if v is None or isinstance(v, (int, float, str)) else True) for k, v in r.kw.items() if k != "name"}
        ext = XH.attention_windowed(**dims)
        seen = []
        assert {"q", "k", "vt", "out"} <= set(r.operands)
        for name, o in r.operands.items():
            assert name in ext, f"{r.name}: operand '{name}' has no extent"
            if o.kind != "buf":
                continue
            need, role = ext[name]
            assert need <= o.avail, f"{r.name}: operand '{name}' needs {need} bytes, its buffer has {o.avail} from the operand's address"
            assert not o.freed, f"{r.name}: operand '{name}' lies in a freed buffer"
            seen.append((name, role, o.offset, o.offset + need))
        for i, (na, ra, lo_a, hi_a) in enumerate(seen):   # out apart from every input
            for nb_, rb, lo_b, hi_b in seen[i + 1:]:
                if "out" in (ra, rb):
                    assert not (lo_a < hi_b and lo_b < hi_a), f"{r.name}: '{na}' and '{nb_}' share bytes"
        kw = r.kw
        assert kw["h"] % kw["wh"] == 0 and kw["w"] % kw["ww"] == 0 and kw["ww"] % 8 == 0
        assert kw["vt_ld"] >= kw["h"] * kw["w"] and kw["vt_ld"] % 8 == 0 and (kw["h"] // kw["wh"], kw["w"] // kw["ww"]) == (3, 2)
        checked += 1
    assert checked == 15


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("tag, height, width, tile, depth, windows, batch", [
    ("a", 256, 128, 64, 0, (4, 2), 2),
    ("b", 256, 256, 128, 1, (2, 2), 1),
])
def test_fixture_files(tag, height, width, tile, depth, windows, batch):
    """tools/make_hypertile_fixtures.py's two files: the recorded inputs are the issue's, and the plain job lies below 30 dB of the
    windowed latent, so the 40 dB bar of tests/test_hypertile_gpu.py tells the two jobs apart."""
    from minsdtf_amd import hypertile as HT

    path = os.path.join(GOLD, f"oracle_hypertile_{tag}.npz")
    assert os.path.exists(path) and os.path.getsize(path) < (1 << 20)
    g = np.load(path)
    assert float(g["plain_psnr"]) < 30.0
    assert (int(g["weight_seed"]), float(g["bias_scale"]), int(g["context_seed"]), int(g["noise_seed"])) == (0, 0.05, 1234, 0)
    assert (float(g["guidance"]), int(g["steps"]), float(g["guidance_rescale"]), str(g["sampler"])) == (7.5, 4, 0.0, "")
    assert (int(g["height"]), int(g["width"]), int(g["tile"]), int(g["depth"]), int(g["batch"])) == (height, width, tile, depth, batch)
    assert tuple(int(v) for v in g["windows"]) == windows
    assert HT.parse(dict(tile=tile, depth=depth)).key(height, width) == windows + (depth,)
    assert g["latent"].shape == (batch, height // 8, width // 8, 4) and g["latent"].dtype == np.float32
