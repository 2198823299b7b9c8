"""Regional prompting without a GPU: the normalised weights, the masks and every ValueError of minsdtf_amd/regions.py, the float64
statement of msd_region_combine, generate_image's refusals and size cap (raised before any device work), the library's export
and the struct layout."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _soft_masks(R, h, w, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.random((h, w)) + 0.01 for _ in range(R)]


# ------------------------------------------------------------------------------------------------------------------ weights
@pytest.mark.parametrize("R", [1, 2, 5, 16])
def test_weights_sum_to_one(R):
    """Every weight is a float64 quotient rounded once to fp32: its error is at most 2^-24 of itself, and the quotients sum
    to 1, so the fp32 weights sum to 1 within 2^-24 (+ the float64 sum's own rounding): 2^-23 holds with room."""
    from minsdtf_amd import regions

    w = regions.weights(_soft_masks(R, 5, 7, seed=R), region_weights=[1.0 + 0.5 * r for r in range(R)])
    assert w.dtype == np.float32 and w.shape == (R, 5, 7) and w.min() >= 0.0
    assert np.abs(w.astype(np.float64).sum(axis=0) - 1.0).max() <= 2.0 ** -23
    based = regions.weights(_soft_masks(R - 1, 5, 7), base_weight=0.3) if R > 1 else None
    if based is not None:
        assert based.shape == (R, 5, 7)
        assert np.abs(based.astype(np.float64).sum(axis=0) - 1.0).max() <= 2.0 ** -23


def test_weights_are_the_float64_quotient_rounded_once():
    from minsdtf_amd import regions

    masks = _soft_masks(3, 4, 6, seed=9)
    rw = [0.5, 2.0, 1.25]
    m = np.stack([v * np.asarray(x, dtype=np.float64) for v, x in zip(rw, masks)])
    np.testing.assert_array_equal(regions.weights(masks, rw), (m / m.sum(axis=0)[None]).astype(np.float32))
    mb = np.concatenate([np.full((1, 4, 6), 0.3), m])
    np.testing.assert_array_equal(regions.weights(masks, rw, base_weight=0.3), (mb / mb.sum(axis=0)[None]).astype(np.float32))


def test_single_cover_is_exactly_one_and_zero():
    from minsdtf_amd import regions

    masks = regions.boxes(5, 7, 2, 3)
    w = regions.weights(masks, region_weights=[0.3, 1.7, 2.9, 0.7, 1.1, 5.3])   # (any weight: m / m == 1.0)
    for r, m in enumerate(masks):
        np.testing.assert_array_equal(w[r], m)
    assert set(np.unique(w).tolist()) == {0.0, 1.0}
    # partly overlapping soft masks: where one mask alone is non-zero it is still exactly 1.0
    a, b = np.zeros((4, 8)), np.zeros((4, 8))
    a[:, :5], b[:, 3:] = 0.37, 0.91
    w = regions.weights([a, b])
    np.testing.assert_array_equal(w[0][:, :3], 1.0)
    np.testing.assert_array_equal(w[1][:, :3], 0.0)
    np.testing.assert_array_equal(w[1][:, 5:], 1.0)
    np.testing.assert_array_equal(w[0][:, 5:], 0.0)
    assert np.all((w[0][:, 3:5] > 0.0) & (w[0][:, 3:5] < 1.0))


def test_image_resolution_masks_take_the_block_mean():
    from minsdtf_amd import regions

    rng = np.random.default_rng(4)
    big = rng.random((40, 56)) + 0.05
    small = regions.latent_mask(big, 5, 7)
    assert small.dtype == np.float64 and small.shape == (5, 7)
    for y in range(5):
        for x in range(7):
            assert small[y, x] == pytest.approx(big[8 * y:8 * y + 8, 8 * x:8 * x + 8].astype(np.float64).mean(), rel=1e-15)
    other = rng.random((5, 7)) + 0.05
    w = regions.weights([big, other], h=5, w=7)
    m = np.stack([small, other])
    np.testing.assert_array_equal(w, (m / m.sum(axis=0)[None]).astype(np.float32))
    # a binary image-resolution mask whose edge cuts an 8 x 8 block: the fraction of the block
    edge = np.zeros((16, 16))
    edge[:, :12] = 1.0
    np.testing.assert_array_equal(regions.latent_mask(edge, 2, 2), [[1.0, 0.5], [1.0, 0.5]])


def test_boxes():
    from minsdtf_amd import regions

    got = regions.boxes(5, 7, 2, 3)
    assert len(got) == 6 and all(m.shape == (5, 7) for m in got)
    np.testing.assert_array_equal(sum(got), np.ones((5, 7)))   # a partition
    assert got[0][:2, :2].all() and got[0].sum() == 4            # rows [0, 2), columns [0, 2)
    assert got[5][2:, 4:].all() and got[5].sum() == 9            # rows [2, 5), columns [4, 7)
    left, right = regions.boxes(8, 8, 1, 2)
    assert left[:, :4].all() and not left[:, 4:].any() and right[:, 4:].all() and not right[:, :4].any()
    for bad in ((0, 1), (1, 0), (6, 1), (1, 8)):
        with pytest.raises(ValueError, match="grid"):
            regions.boxes(5, 7, *bad)


def test_value_errors():
    from minsdtf_amd import regions

    ctx = np.zeros((77, 768), dtype=np.float32)
    ok = np.ones((8, 8))

    def job(*masks, **kw):
        return dict(regions=[dict(prompt=ctx, mask=m) for m in masks], **kw)

    assert regions.parse(None, 64, 64) is None
    hole = np.ones((8, 8))
    hole[3, 5] = 0.0
    hole[6, 1] = 0.0
    with pytest.raises(ValueError, match=r"\(3, 5\)"):   # the first uncovered pixel, row-major
        regions.parse(job(hole, hole), 64, 64)
    assert regions.parse(job(hole, hole, base_weight=0.2), 64, 64).count == 3   # (the base prompt covers every pixel)
    with pytest.raises(ValueError, match="shape"):
        regions.parse(job(ok, np.ones((8, 9))), 64, 64)
    with pytest.raises(ValueError, match="shape"):
        regions.parse(job(np.ones((8, 8, 1))), 64, 64)
    with pytest.raises(ValueError, match="shape"):
        regions.parse(job(np.ones((32, 32))), 64, 64)
    neg = np.ones((8, 8))
    neg[0, 0] = -0.5
    with pytest.raises(ValueError, match="negative"):
        regions.parse(job(ok, neg), 64, 64)
    for v in (np.nan, np.inf):
        bad = np.ones((8, 8))
        bad[2, 2] = v
        with pytest.raises(ValueError, match="non-finite"):
            regions.parse(job(bad), 64, 64)
    with pytest.raises(ValueError, match="MAX_REGIONS"):
        regions.parse(job(*[ok] * 17), 64, 64)
    with pytest.raises(ValueError, match="MAX_REGIONS"):
        regions.parse(job(*[ok] * 16, base_weight=0.1), 64, 64)
    assert regions.parse(job(*[ok] * 16), 64, 64).count == 16
    for wt in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="weight"):
            regions.parse(dict(regions=[dict(prompt=ctx, mask=ok, weight=wt)]), 64, 64)
    for bw in (-0.1, np.inf):
        with pytest.raises(ValueError, match="base_weight"):
            regions.parse(job(ok, base_weight=bw), 64, 64)
    with pytest.raises(ValueError, match="no region"):
        regions.parse(dict(regions=[]), 64, 64)
    with pytest.raises(ValueError, match="unknown field"):
        regions.parse(dict(regions=[dict(prompt=ctx, mask=ok)], blend="x"), 64, 64)
    with pytest.raises(ValueError, match="unknown field"):
        regions.parse(dict(regions=[dict(prompt=ctx, mask=ok, feather=2)]), 64, 64)
    with pytest.raises(ValueError, match="no prompt"):
        regions.parse(dict(regions=[dict(mask=ok)]), 64, 64)
    with pytest.raises(ValueError, match="no mask"):
        regions.parse(dict(regions=[dict(prompt=ctx)]), 64, 64)
    with pytest.raises(ValueError, match="Regions"):
        regions.parse([ok], 64, 64)
    # the object forms
    r = regions.parse(regions.Regions([regions.RegionSpec(ctx, ok), regions.RegionSpec(ctx, np.ones((64, 64)), 2.0)], 0.5), 64, 64)
    assert r.count == 3 and r.weights().shape == (3, 8, 8)
    np.testing.assert_array_equal(r.weights(), np.broadcast_to(np.float32([0.5, 1.0, 2.0])[:, None, None] / np.float32(3.5), (3, 8, 8)))
    assert regions.parse(r, 64, 64) is r
    with pytest.raises(ValueError, match="latent"):
        regions.parse(r, 128, 64)


def test_combine_reference_is_the_weighted_sum():
    from minsdtf_amd import regions

    rng = np.random.default_rng(2)
    R, B, h, w = 5, 3, 5, 7
    eps = rng.standard_normal((R * B, h, w, 4)).astype(np.float32)
    wt = regions.weights(_soft_masks(R, h, w))
    want = np.einsum("ryx,rbyxc->byxc", wt.astype(np.float64), eps.astype(np.float64).reshape(R, B, h, w, 4))
    got = regions.combine_reference(eps, wt)
    assert got.dtype == np.float64 and got.shape == (B, h, w, 4)
    np.testing.assert_allclose(got, want, rtol=0, atol=8 * 2.0 ** -53 * np.abs(eps).max())
    # the host loop's fp32 form of it: R roundings (see test_regions_gpu.test_combine_vs_float64)
    host = regions.combine_host([eps[r * B:(r + 1) * B] for r in range(R)], wt)
    assert host.dtype == np.float32
    assert np.abs(host - want).max() <= (R + 1) * 2.0 ** -24 * np.abs(eps).max()
    with pytest.raises(ValueError, match="shape"):
        regions.combine_reference(eps[:-1], wt)
    with pytest.raises(ValueError, match="shape"):
        regions.combine_reference(eps, wt[:, :4])


# ------------------------------------------------------------------------------------------------- generate_image, no device
def _job(R, ctx):
    from minsdtf_amd import regions

    masks = regions.boxes(8, 8, 1, R) if R <= 8 else [np.ones((8, 8))] * R
    return dict(regions=[dict(prompt=ctx, mask=m) for m in masks])


def test_refusals_and_the_cap_come_before_any_device_work():
    from minsdtf_amd import tiled
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    ctx = np.zeros((77, 768), dtype=np.float32)
    img = np.zeros((64, 64, 3), dtype=np.uint8)
    sd = StableDiffusionBase(64, 64)   # (no models behind it: anything that reaches a model fails another way)
    kw = dict(batch_size=1, num_steps=3, seed=0, regions=_job(2, ctx))
    for extra, names in ((dict(tiled=dict(size=(64, 128))), ["tiled"]), (dict(hires=dict(scale=2)), ["hires"]),
                         (dict(control_net_image=img.astype(np.float32)), ["control_net_image"]),
                         (dict(reference_image=img), ["reference_image"]), (dict(inpaint_mask=img[..., 0]), ["inpaint_mask"]),
                         (dict(reference_image=img, inpaint_mask=img[..., 0], hires=dict(scale=2)),
                          ["hires", "reference_image", "inpaint_mask"])):
        with pytest.raises(ValueError, match="regions") as e:
            sd.generate_image(ctx, **kw, **extra)
        assert all(n in str(e.value) for n in names), str(e.value)
    with pytest.raises(ValueError, match="regions.*active_tcd"):
        StableDiffusionBase(64, 64, active_tcd=True).generate_image(ctx, **kw)
    two = StableDiffusionBase(64, 64)
    two.denoise_streams = 2
    with pytest.raises(ValueError, match="regions.*denoise_streams"):
        two.generate_image(ctx, **kw)
    with pytest.raises(ValueError, match="regions"):
        sd.text_to_image(ctx, tiled=dict(size=(64, 128)), **kw)
    # the cap: (1 + R) * batch_size <= 2 * tiled.MAX_VIEW_BATCH UNet rows, and the message names the numbers
    cap = 2 * tiled.MAX_VIEW_BATCH
    assert cap == 12
    with pytest.raises(ValueError, match=r"14 UNet\s+rows.*MAX_VIEW_BATCH = 12"):
        sd.generate_image(ctx, batch_size=2, num_steps=3, seed=0, regions=_job(6, ctx))
    with pytest.raises(ValueError, match="MAX_VIEW_BATCH"):
        sd.generate_image(ctx, batch_size=1, num_steps=3, seed=0, regions=_job(12, ctx))
    with pytest.raises(ValueError, match="MAX_VIEW_BATCH"):   # the base prompt counts when it is evaluated
        sd.generate_image(ctx, batch_size=2, num_steps=3, seed=0, regions=dict(base_weight=0.5, **_job(5, ctx)))
    # a bad description is a ValueError of its own
    with pytest.raises(ValueError, match="unknown field"):
        sd.generate_image(ctx, batch_size=1, num_steps=3, regions=dict(regions=[], masks=[]))
    assert not sd._engines


def test_region_contexts_must_share_one_token_length():
    from minsdtf_amd import regions
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    sd = StableDiffusionBase(64, 64)
    sd.unconditional_context = np.zeros((77, 768), dtype=np.float32)
    short, long_ = np.zeros((77, 768), dtype=np.float32), np.zeros((154, 768), dtype=np.float32)
    left, right = regions.boxes(8, 8, 1, 2)
    job = dict(regions=[dict(prompt=short, mask=left), dict(prompt=long_, mask=right)])
    with pytest.raises(ValueError, match="share one token length.*77.*154"):
        sd.generate_image(short, batch_size=1, num_steps=3, seed=0, regions=job)
    job = dict(regions=[dict(prompt=long_, mask=left), dict(prompt=long_, mask=right)], base_weight=0.5)
    with pytest.raises(ValueError, match="share one token length.*base prompt: 77"):
        sd.generate_image(short, batch_size=1, num_steps=3, seed=0, regions=job)
    assert not sd._engines


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_library_exports_region_combine():
    from minsdtf_amd import _lib, regions

    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    assert "msd_region_combine" in _lib.SYMBOLS
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "msd_region_combine" in {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "minsdtf_hip.h")).read()
    assert "#define MSD_REGION_MAX 16" in header and _lib.REGION_MAX == regions.MAX_REGIONS == 16
    lib = _lib.load()
    # argument validation works without a GPU: nothing is launched for a bad call
    assert lib.msd_region_combine(None, None) == -1
    assert b"null" in lib.msd_last_error()
    s = _lib.MsdRegionCombine()
    s.eps, s.w, s.out, s.regions, s.batch, s.n = 4096, 65536, 4096, 17, 1, 64
    assert lib.msd_region_combine(ctypes.byref(s), None) == -1
    assert b"regions" in lib.msd_last_error()


def test_struct_layout_matches_header():
    from minsdtf_amd import _lib

    src = '#include <stdio.h>\n#include <stddef.h>\n#include "minsdtf_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", ' \
          'sizeof(MsdRegionCombine), offsetof(MsdRegionCombine, w), offsetof(MsdRegionCombine, out), ' \
          'offsetof(MsdRegionCombine, regions), offsetof(MsdRegionCombine, n));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    t = _lib.MsdRegionCombine
    assert sizes == [ctypes.sizeof(t), t.w.offset, t.out.offset, t.regions.offset, t.n.offset]
