"""Tiled diffusion, host side (no GPU): view offsets, view order and blend weight rows, the job description's errors, the C
struct and the host validation of msd_tile_consensus, the float64 statement of the kernel, the refused combinations and the
per-step draws of a stochastic sampler on overlapping views."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from minsdtf_amd import samplers as smp
from minsdtf_amd import tiled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ geometry, hand-written cases
def test_one_view():
    g = tiled.parse(dict(size=(512, 512)), 512, 512)
    assert (g.ys, g.xs, g.rows, g.cols, g.views) == ((0,), (0,), 1, 1, 1)
    assert (g.th, g.tw, g.H, g.W, g.height, g.width, g.blend) == (64, 64, 64, 64, 512, 512, "uniform")
    assert g.offsets() == [(0, 0)]


def test_exact_multiples_and_the_default_stride():
    g = tiled.parse(dict(size=(512, 1024)), 512, 512)   # default stride: half the tile = 256 px = 32 latent
    assert g.ys == (0,) and g.xs == (0, 32, 64) and (g.H, g.W) == (64, 128)
    g = tiled.parse(tiled.TiledSpec(size=(1024, 768), stride=256), 512, 512)   # the 3 x 2 job of tiled.MAX_VIEW_BATCH
    assert g.ys == (0, 32, 64) and g.xs == (0, 32) and g.views == 6
    # row-major view order: v = r * cols + c
    assert g.offsets() == [(0, 0), (0, 32), (32, 0), (32, 32), (64, 0), (64, 32)]
    g = tiled.parse(dict(size=(384, 384), stride=(128, 64)), 256, 256)
    assert g.ys == (0, 16) and g.xs == (0, 8, 16)


def test_snapped_last_view():
    # L = 96, t = 64, s = 24: n = ceil(32 / 24) + 1 = 3, offsets 0, 24, min(48, 32)
    g = tiled.parse(dict(size=(512, 768), stride=192), 512, 512)
    assert g.xs == (0, 24, 32) and g.ys == (0,)
    assert tiled.axis_offsets(96, 64, 24) == (0, 24, 32)
    assert tiled.axis_offsets(100, 64, 32) == (0, 32, 36)
    assert tiled.axis_offsets(64, 64, 32) == (0,)


def test_stride_equal_to_the_tile():
    g = tiled.parse(dict(size=(512, 1024), stride=512), 512, 512)
    assert g.xs == (0, 64) and g.ys == (0,)   # no overlap
    g = tiled.parse(dict(size=(512, 1280), stride=(512, 512)), 512, 512)
    assert g.xs == (0, 64, 96)   # 160 = 2.5 tiles: the last view snapped back over the second


def test_weight_rows():
    g = tiled.parse(dict(size=(512, 768)), 512, 256)
    assert g.wy.dtype == np.float32 and g.wx.dtype == np.float32
    np.testing.assert_array_equal(g.wy, np.ones(64, np.float32))
    np.testing.assert_array_equal(g.wx, np.ones(32, np.float32))
    g = tiled.parse(dict(size=(512, 768), blend="gaussian"), 512, 256)
    for row, t in ((g.wy, 64), (g.wx, 32)):
        i = np.arange(t, dtype=np.float64)
        want = np.exp(-(((i - (t - 1) / 2) / t) ** 2) / (2 * 0.01)).astype(np.float32)
        np.testing.assert_array_equal(row, want)
        np.testing.assert_array_equal(row, row[::-1])           # symmetric about the tile's middle
        assert row.min() > 0 and row.argmax() in (t // 2 - 1, t // 2) and row[0] < 0.05 * row.max()
    # hand-computed entries for t = 4: exp(-((i - 1.5) / 4)^2 / 0.02)
    np.testing.assert_allclose(tiled.weight_row(4, "gaussian"), np.exp(-np.array([0.140625, 0.015625, 0.015625, 0.140625]) / 0.02),
                               rtol=1e-7)


@pytest.mark.parametrize("bad,match", [
    (dict(size=(500, 512)), "multiple of 64"),
    (dict(size=(512, 1000)), "multiple of 64"),
    (dict(size=(448, 1024)), "smaller than the tile"),
    (dict(size=(1024, 448)), "smaller than the tile"),
    (dict(size=(512, 1024), stride=100), "multiple of 8"),
    (dict(size=(512, 1024), stride=0), "multiple of 8"),
    (dict(size=(512, 1024), stride=-8), "multiple of 8"),
    (dict(size=(512, 1024), stride=(256, 520)), "exceeds the tile"),
    (dict(size=(512, 1024), stride=(256,)), "stride must be"),
    (dict(size=(512, 1024), stride=25.5), "stride must be"),
    (dict(size=(512, 1024), blend="cosine"), "unknown blend"),
    (dict(size=1024), "size must be"),
    (dict(size=(512.5, 1024)), "size must be"),
    (dict(), "give the canvas"),
    (dict(size=(512, 1024), overlap=64), "unknown field"),
    (dict(size=(512, 8192), stride=8), "per axis"),
])
def test_parse_errors(bad, match):
    with pytest.raises(ValueError, match=match):
        tiled.parse(bad, 512, 512)
    if "overlap" not in bad:
        with pytest.raises(ValueError, match=match):
            tiled.parse(tiled.TiledSpec(**bad), 512, 512)


def test_parse_none_and_wrong_types():
    assert tiled.parse(None, 512, 512) is None
    with pytest.raises(ValueError, match="must be a TiledSpec"):
        tiled.parse("2x1", 512, 512)
    g = tiled.parse(dict(size=(512, 1024)), 512, 512)
    assert tiled.parse(g, 512, 512) is g
    with pytest.raises(ValueError, match="tile is"):
        tiled.parse(g, 256, 256)
    assert g.key == tiled.parse(tiled.TiledSpec(size=(512, 1024), stride=(256, 256)), 512, 512).key
    assert g.key != tiled.parse(dict(size=(512, 1024), blend="gaussian"), 512, 512).key
    for bad in (dict(ys=(0, 8), xs=(1,)), dict(ys=(0, 9, 8), xs=(0,)), dict(ys=(0, 8, 8), xs=(0,)), dict(ys=(8,), xs=(0,))):
        with pytest.raises(ValueError, match="tiled"):
            tiled.geometry(8, 8, 16, 8, **bad)
    with pytest.raises(ValueError, match="at most the tile length"):
        tiled.geometry(8, 8, 24, 8, (0, 16), (0,))   # rows 8 .. 15 uncovered


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_is_still_12_and_the_symbol_is_declared():
    from minsdtf_amd import _lib

    assert "msd_tile_consensus" in _lib.SYMBOLS and _lib.ABI_VERSION == 12
    assert _lib.load().msd_abi_version() == 12
    assert _lib.TILE_MAX_VIEWS == tiled.MAX_AXIS_VIEWS == 64


def test_struct_matches_header():
    from minsdtf_amd import _lib

    fields = ["tiles", "canvas", "ys", "xs", "rows", "cols", "th", "tw", "H", "W", "batch", "wy", "wx", "mode"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "minsdtf_hip.h"\nint main(){printf("%zu %d", sizeof(MsdTileConsensus), '
           'MSD_TILE_MAX_VIEWS);\n' + "".join(f'printf(" %zu", offsetof(MsdTileConsensus, {f}));\n' for f in fields) + 'return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    S = _lib.MsdTileConsensus
    assert got == [ctypes.sizeof(S), _lib.TILE_MAX_VIEWS] + [getattr(S, f).offset for f in fields]
    assert [f for f, _t in S._fields_] == fields


def _good_struct():
    from minsdtf_amd import _lib

    s = _lib.MsdTileConsensus()
    s.tiles, s.canvas, s.wy, s.wx = 1 << 20, 8 << 20, 3 << 20, 4 << 20
    s.rows, s.cols, s.th, s.tw, s.H, s.W, s.batch, s.mode = 2, 3, 8, 8, 12, 20, 2, 0
    s.ys[:2] = [0, 4]
    s.xs[:3] = [0, 8, 12]
    return s


def test_argument_errors_without_a_gpu():
    """Every bad field comes back as -1 with a message before anything is launched (no device needed)."""
    from minsdtf_amd import _lib

    lib = _lib.load()
    assert lib.msd_tile_consensus(None, None) == -1
    assert b"null" in lib.msd_last_error()
    n_tiles_bytes = 2 * 6 * 8 * 8 * 16
    for field, value in (("tiles", None), ("canvas", None), ("wy", None), ("wx", None),
                         ("tiles", (1 << 20) + 4), ("canvas", (8 << 20) + 8), ("wy", (3 << 20) + 4), ("wx", (4 << 20) + 12),
                         ("batch", 0), ("batch", -1), ("batch", 1 << 20), ("th", 0), ("tw", 0), ("H", 7), ("W", 7), ("rows", 0), ("cols", 0),
                         ("rows", 65), ("cols", 65), ("mode", 2), ("mode", -1),
                         ("canvas", 1 << 20), ("canvas", (1 << 20) + n_tiles_bytes - 16), ("tiles", (8 << 20) + 16)):
        s = _good_struct()
        setattr(s, field, value)
        assert lib.msd_tile_consensus(ctypes.byref(s), None) == -1, (field, value)
        assert lib.msd_last_error(), field
    for axis, n, bad in (("ys", 2, [1, 4]), ("ys", 2, [0, 3]), ("ys", 2, [0, 5]), ("ys", 2, [4, 0]), ("xs", 3, [0, 0, 12]),
                         ("xs", 3, [0, 12, 8]), ("xs", 3, [0, 3, 12]), ("xs", 3, [0, 8, 11]), ("xs", 3, [-1, 8, 12])):
        s = _good_struct()
        getattr(s, axis)[:n] = bad
        assert lib.msd_tile_consensus(ctypes.byref(s), None) == -1, (axis, bad)
        assert axis.encode() in lib.msd_last_error()
    s = _good_struct()   # a gap wider than the tile leaves pixels uncovered
    s.W, s.cols = 20, 2
    s.xs[:2] = [0, 12]
    assert lib.msd_tile_consensus(ctypes.byref(s), None) == -1 and b"xs" in lib.msd_last_error()
    s = _good_struct()   # 2^31 elements
    s.rows, s.cols, s.th, s.tw, s.H, s.W, s.batch = 1, 1, 16384, 16384, 16384, 16384, 2
    s.ys[0] = s.xs[0] = 0
    s.canvas = 1 << 44
    assert lib.msd_tile_consensus(ctypes.byref(s), None) == -1 and b"2^31" in lib.msd_last_error()


def test_ops_record_fills_the_struct():
    from minsdtf_amd import ops

    c = ops.tile_consensus(tiles=1 << 20, canvas=8 << 20, wy=3 << 20, wx=4 << 20, ys=(0, 4), xs=(0, 8, 12), th=8, tw=8, H=12, W=20,
                           batch=2, mode=1)
    s = c.keep
    assert (s.rows, s.cols, s.th, s.tw, s.H, s.W, s.batch, s.mode) == (2, 3, 8, 8, 12, 20, 2, 1)
    assert list(s.ys[:3]) == [0, 4, 0] and list(s.xs[:4]) == [0, 8, 12, 0]
    with pytest.raises(ValueError, match="views"):
        ops.tile_consensus(tiles=1, canvas=2, wy=3, wx=4, ys=(), xs=(0,), th=8, tw=8, H=8, W=8, batch=1)


# ------------------------------------------------------------------------------------------------ the float64 reference
def _geo(th, tw, H, W, sy, sx, blend="uniform"):
    return tiled.geometry(th, tw, H, W, tiled.axis_offsets(H, th, sy), tiled.axis_offsets(W, tw, sx), blend)


def test_reference_single_cover_is_the_identity():
    rng = np.random.default_rng(0)
    g = _geo(8, 8, 8, 8, 4, 4)
    t = rng.standard_normal((3, 8, 8, 4)).astype(np.float32)
    canvas, out = tiled.consensus_reference(t, g)
    np.testing.assert_array_equal(canvas, t.astype(np.float64))
    np.testing.assert_array_equal(out, t.astype(np.float64))
    for blend in tiled.BLENDS:   # no overlap: every pixel has one cover, whatever the weights
        g = _geo(8, 6, 16, 12, 8, 6, blend)
        t = rng.standard_normal((2 * 4, 8, 6, 4))
        canvas, out = tiled.consensus_reference(t, g)
        np.testing.assert_array_equal(out, t)
        np.testing.assert_array_equal(canvas[1, 8:, :6], t[4 + 2])   # sample-major rows, row-major views


def test_reference_uniform_is_the_arithmetic_mean():
    rng = np.random.default_rng(1)
    g = _geo(8, 8, 12, 8, 4, 8)   # two views, rows 4 .. 7 under both
    t = rng.standard_normal((2, 8, 8, 4))
    canvas, _ = tiled.consensus_reference(t, g)
    np.testing.assert_array_equal(canvas[0, :4], t[0, :4])
    np.testing.assert_array_equal(canvas[0, 8:], t[1, 4:])
    np.testing.assert_allclose(canvas[0, 4:8], 0.5 * (t[0, 4:] + t[1, :4]), rtol=0, atol=1e-15)
    g = _geo(8, 8, 12, 12, 4, 4)   # 2 x 2 views: the centre 4 x 4 block lies under all four
    t = rng.standard_normal((4, 8, 8, 4))
    canvas, _ = tiled.consensus_reference(t, g)
    want = (t[0, 4:, 4:] + t[1, 4:, :4] + t[2, :4, 4:] + t[3, :4, :4]) / 4.0
    np.testing.assert_allclose(canvas[0, 4:8, 4:8], want, rtol=0, atol=1e-15)


@pytest.mark.parametrize("blend", tiled.BLENDS)
def test_reference_writes_the_canvas_back_into_every_view(blend):
    rng = np.random.default_rng(2)
    g = _geo(8, 6, 20, 16, 4, 4, blend)   # snapped last views on the columns
    assert g.xs == (0, 4, 8, 10)
    t = rng.standard_normal((2 * g.views, 8, 6, 4))
    canvas, out = tiled.consensus_reference(t, g)
    np.testing.assert_array_equal(out, tiled.slice_views(canvas, g))
    again, out2 = tiled.consensus_reference(out, g)   # a fixed point: views that agree stay as they are
    np.testing.assert_allclose(again, canvas, rtol=0, atol=1e-14)
    lo, hi = t.min(), t.max()
    assert canvas.min() >= lo - 1e-12 and canvas.max() <= hi + 1e-12   # a mean with positive weights
    if blend == "gaussian":   # weighted towards the view whose centre is nearer
        g2 = _geo(8, 8, 8, 12, 8, 4, "gaussian")
        t2 = np.zeros((2, 8, 8, 1))
        t2[1] = 1.0
        c2, _ = tiled.consensus_reference(t2, g2)
        assert c2[0, 0, 4, 0] < 0.5 < c2[0, 0, 7, 0]


# ------------------------------------------------------------------------------------------------ the pipeline's host logic
def test_refused_combinations_raise_before_any_model_is_built():
    from minsdtf_amd.stable_diffusion import StableDiffusion

    p = StableDiffusion(64, 64, device=torch.device("cpu"))
    ctx = np.zeros((77, 768), dtype=np.float32)
    p.unconditional_context = ctx
    img = np.zeros((64, 64, 3), dtype=np.uint8)
    kw = dict(batch_size=1, num_steps=4, seed=0, tiled=dict(size=(64, 128)))
    for extra in (dict(reference_image=img), dict(inpaint_mask=img[..., 0]), dict(control_net_image=img.astype(np.float32)),
                  dict(hires=dict(scale=2)), dict(host_loop=True)):
        with pytest.raises(ValueError, match="tiled"):
            p.generate_image(ctx, **kw, **extra)
    with pytest.raises(ValueError, match="tiled"):
        StableDiffusion(64, 64, device=torch.device("cpu"), active_tcd=True).generate_image(ctx, **kw)
    with pytest.raises(ValueError, match="tiled"):
        p.image_to_image(ctx, reference_image=img, **kw)
    with pytest.raises(ValueError, match="tiled"):
        p.text_to_image(ctx, hires=dict(scale=2), **kw)
    with pytest.raises(ValueError, match="MAX_VIEW_BATCH"):
        p.generate_image(ctx, **{**kw, "batch_size": tiled.MAX_VIEW_BATCH // 3 + 1})   # 3 views per image
    with pytest.raises(ValueError, match="MAX_VIEW_BATCH"):
        p.generate_image(ctx, **{**kw, "tiled": dict(size=(256, 256), stride=32)})   # 7 x 7 views
    with pytest.raises(ValueError, match="multiple of 64"):
        p.text_to_image(ctx, batch_size=1, num_steps=4, seed=0, tiled=dict(size=(64, 100)))
    with pytest.raises(ValueError, match="diffusion_noise has shape"):
        p.generate_image(ctx, batch_size=1, num_steps=4, tiled=dict(size=(64, 128)), diffusion_noise=np.zeros((1, 8, 8, 4), np.float32))
    assert not p._engines and p._diffusion_model is None and p._image_decoder is None
    assert tiled.MAX_VIEW_BATCH >= 6


@pytest.mark.parametrize("sampler", [None, "dpmpp_2m_karras", "euler_a"])
def test_draws_are_made_at_canvas_shape_and_agree_on_overlaps(monkeypatch, sampler):
    """The start noise and a stochastic sampler's per-step draws are made for the canvas and travel - under shard_batch too - as
    canvas-shaped arrays of the global batch; cut per view, two views hold the same numbers where they overlap."""
    from minsdtf_amd import dist as mdist
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sent = {}

    def fake_sharded(local, context, uncond_context, noise, device, per_sample=(), shared=(), shard=True):
        sent["noise"], sent["per_sample"], sent["shared"], sent["shard"] = np.asarray(noise), [np.asarray(a) for a in per_sample], list(shared), shard
        return torch.zeros(int(noise.shape[0]), 64, 128, 3, dtype=torch.uint8)

    monkeypatch.setattr(mdist, "world_size", lambda: 2)
    monkeypatch.setattr(mdist, "generate_sharded", fake_sharded)
    p = StableDiffusion(64, 64, device=torch.device("cpu"))
    p.shard_batch = True
    rng = np.random.default_rng(4)
    ctx, unc = rng.standard_normal((2, 77, 768)).astype(np.float32), rng.standard_normal((2, 77, 768)).astype(np.float32)
    spec = dict(size=(64, 128), stride=32)   # 8 x 16 latent, views at columns 0, 4, 8
    out = p.generate_image(ctx, negative_prompt=unc, batch_size=2, num_steps=5, seed=3, sampler=sampler, tiled=spec)
    assert out.shape == (2, 64, 128, 3) and sent["shard"] and sent["shared"] == []
    np.testing.assert_array_equal(sent["noise"], np.random.default_rng(3).standard_normal((2, 8, 16, 4)).astype(np.float32))
    if sampler != "euler_a":
        assert sent["per_sample"] == []
        return
    assert [a.shape for a in sent["per_sample"]] == [(2, 5, 8 * 16 * 4)]
    z = sent["per_sample"][0].reshape(2, 5, 8, 16, 4)
    np.testing.assert_array_equal(z, smp.draw_step_noise(2, 5, 8, 16, 3))
    g = tiled.parse(spec, 64, 64)
    views = tiled.slice_views(z, g)
    assert views.shape == (2 * 3, 5, 8, 8, 4)
    for b in range(2):
        np.testing.assert_array_equal(views[b * 3 + 0][:, :, 4:], views[b * 3 + 1][:, :, :4])   # columns 4 .. 7 of the canvas
        np.testing.assert_array_equal(views[b * 3 + 1][:, :, 4:], views[b * 3 + 2][:, :, :4])   # columns 8 .. 11
        np.testing.assert_array_equal(views[b * 3 + 2], z[b][:, :, 8:16])
    tv = tiled.slice_views(torch.from_numpy(z), g)   # (tensors - a sharded rank's slice - are cut the same way)
    np.testing.assert_array_equal(tv.numpy(), views)
    # sample 0's draws do not depend on the batch size
    np.testing.assert_array_equal(smp.draw_step_noise(1, 5, 8, 16, 3)[0], z[0])
