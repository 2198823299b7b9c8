"""Regional prompting inside cross-attention, everything that needs no GPU: the job description (mode), the per-level weight planes,
the recorded plans (tensor-less, as tests/_layer_walk.py walks them), msd_region_attention's argument checks through the library,
and generate_image's refusals and cap arithmetic, which come before any device work."""
import ctypes

import numpy as np
import pytest

import _extents as X
import _extents_region_attention as XR
import _layer_walk as LW


def _halves(h=8, w=8):
    from minsdtf_amd import regions

    return regions.boxes(h, w, 1, 2)


# ------------------------------------------------------------------------------------------------------------------ parse
def test_mode_round_trips_and_defaults_to_latent():
    from minsdtf_amd import regions

    left, right = _halves()
    specs = [dict(prompt="a", mask=left), dict(prompt="b", mask=right)]
    assert regions.Regions().mode == "latent"
    assert regions.parse(dict(regions=specs), 64, 64).mode == "latent"
    for mode in ("latent", "attention"):
        res = regions.parse(dict(regions=specs, mode=mode), 64, 64)
        assert res.mode == mode
        assert regions.parse(res, 64, 64) is res
        assert regions.parse(regions.Regions([regions.RegionSpec("a", left), regions.RegionSpec("b", right)], 0.0, mode), 64, 64).mode == mode
    # the fields stay positional: mode is the last one
    assert regions.Resolved(("a",), np.ones((1, 8, 8)), 0.0).mode == "latent"
    assert regions.Resolved(("a",), np.ones((1, 8, 8)), 0.0, "attention").mode == "attention"


@pytest.mark.parametrize("mode", ["Attention", "couple", "", None, 1])
def test_bad_mode_raises(mode):
    from minsdtf_amd import regions

    left, right = _halves()
    with pytest.raises(ValueError, match="mode"):
        regions.parse(dict(regions=[dict(prompt="a", mask=left), dict(prompt="b", mask=right)], mode=mode), 64, 64)


# ---------------------------------------------------------------------------------------------------------- level_weights
def _levels(h, w):
    from minsdtf_amd import engine

    return engine.unet_levels(h, w)


def _soft(h, w, R, seed, base=0.0):
    from minsdtf_amd import regions

    rng = np.random.default_rng(seed)
    return regions._resolve([regions.RegionSpec(f"p{i}", rng.random((h, w)) + 0.01, 0.5 + i) for i in range(R)], base, h, w, "attention")


@pytest.mark.parametrize("hw,R,base", [((8, 8), 3, 0.0), ((9, 13), 2, 0.3), ((64, 64), 16, 0.0), ((1, 1), 1, 0.0)])
def test_level_zero_is_weights_and_every_plane_sums_to_one(hw, R, base):
    res = _soft(hw[0], hw[1], R, 7, base)
    levels = _levels(*hw)
    planes = res.level_weights(levels)
    assert [p.shape for p in planes] == [(res.count,) + lv for lv in levels] and all(p.dtype == np.float32 for p in planes)
    np.testing.assert_array_equal(planes[0], res.weights())
    for p in planes:
        assert p.min() >= 0.0
        # every weight is one rounding (relative 2^-24) of a float64 quotient; the quotients sum to 1: within 2 fp32 ulp of 1
        assert float(np.abs(p.astype(np.float64).sum(axis=0) - 1.0).max()) <= 2 * 2.0 ** -23


def test_engine_levels():
    assert _levels(64, 64) == [(64, 64), (32, 32), (16, 16), (8, 8)]
    assert _levels(9, 13) == [(9, 13), (5, 7), (3, 4), (2, 2)]


def test_halves_are_exact():
    """Left / right halves on 8 x 8: exactly 0 / 1 at levels 0 to 2, exactly 0.5 / 0.5 at the 1 x 1 level."""
    from minsdtf_amd import regions

    res = regions.parse(dict(regions=[dict(prompt="a", mask=m) for m in _halves()], mode="attention"), 64, 64)
    planes = res.level_weights(_levels(8, 8))
    for l in range(3):
        wl = 8 >> l
        want = np.zeros((2, wl, wl), dtype=np.float32)
        want[0, :, :wl // 2] = 1.0
        want[1, :, wl // 2:] = 1.0
        np.testing.assert_array_equal(planes[l], want)
    np.testing.assert_array_equal(planes[3], np.full((2, 1, 1), 0.5, dtype=np.float32))


def test_single_cover_blocks_are_exact_and_odd_latents_use_clipped_blocks():
    """9 x 13: region 0 covers rows 0 .. 3 alone (weight 2.5), region 1 the rest (soft).  A level pixel whose whole block lies in rows
    0 .. 3 has exactly 1.0 / 0.0.  The last row / column blocks are clipped: level 1's pixel (4, 6) is latent pixel (8, 12) alone,
    level 3's pixel (1, 1) the 1 x 5 block of row 8, columns 8 .. 12 - the float64 mean over what exists, not over 2^l x 2^l."""
    from minsdtf_amd import regions

    h, w = 9, 13
    rng = np.random.default_rng(3)
    m0 = np.zeros((h, w))
    m0[:4] = 1.0
    m1 = rng.random((h, w)) + 0.1
    m1[:4] = 0.0
    m2 = rng.random((h, w)) + 0.1
    m2[:4] = 0.0
    res = regions._resolve([regions.RegionSpec("a", m0, 2.5), regions.RegionSpec("b", m1, 1.0), regions.RegionSpec("c", m2, 0.7)], 0.0, h, w, "attention")
    levels = _levels(h, w)
    assert levels == [(9, 13), (5, 7), (3, 4), (2, 2)]
    planes = res.level_weights(levels)
    for l, p in enumerate(planes):
        f = 1 << l
        for y in range(p.shape[1]):
            if (y + 1) * f <= 4:   # the whole block inside region 0's rows
                np.testing.assert_array_equal(p[0, y], np.ones(p.shape[2], dtype=np.float32))
                np.testing.assert_array_equal(p[1:, y], np.zeros((2, p.shape[2]), dtype=np.float32))
    masks = res.masks   # float64, region weights multiplied in

    def want(l, y, x):
        f = 1 << l
        blk = masks[:, y * f:min((y + 1) * f, h), x * f:min((x + 1) * f, w)].mean(axis=(1, 2))
        return (blk / blk.sum()).astype(np.float32)

    np.testing.assert_array_equal(planes[1][:, 4, 6], want(1, 4, 6))
    np.testing.assert_array_equal(planes[1][:, 4, 6], res.weights()[:, 8, 12])
    np.testing.assert_array_equal(planes[3][:, 1, 1], want(3, 1, 1))
    np.testing.assert_array_equal(planes[2][:, 2, 3], want(2, 2, 3))
    np.testing.assert_array_equal(planes[2][:, 1, 1], want(2, 1, 1))   # an unclipped block that straddles rows 3 | 4
    with pytest.raises(ValueError, match="level"):
        res.level_weights([(9, 13), (4, 6), (2, 3), (1, 1)])


def test_pack_levels():
    from minsdtf_amd import regions

    res = _soft(9, 13, 3, 1)
    levels = _levels(9, 13)
    planes = res.level_weights(levels)
    flat = regions.pack_levels(planes)
    offs = regions.level_offsets(3, levels)
    assert flat.dtype == np.float32 and flat.shape == (offs[-1],) and all(o % 4 == 0 for o in offs)
    for p, o in zip(planes, offs):
        np.testing.assert_array_equal(flat[o:o + p.size].reshape(p.shape), p)


def test_attention_reference_is_the_weighted_sum_of_softmaxes():
    from minsdtf_amd import regions

    rng = np.random.default_rng(0)
    B, S, T, H, d, R = 2, 5, 7, 2, 4, 3
    q, k, v = rng.standard_normal((B, S, H * d)), rng.standard_normal((R * B, T, H * d)), rng.standard_normal((R * B, T, H * d))
    w = rng.random((R, S))
    w[1, :2] = 0.0
    w /= w.sum(0)
    got = regions.attention_reference(q, k, v, w, H)
    want = np.zeros_like(got)
    for b in range(B):
        for h in range(H):
            c = slice(h * d, (h + 1) * d)
            for r in range(R):
                s = q[b, :, c] @ k[r * B + b, :, c].T * np.log(2.0)
                p = np.exp(s - s.max(1, keepdims=True))
                want[b, :, c] += w[r][:, None] * ((p / p.sum(1, keepdims=True)) @ v[r * B + b, :, c])
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    k[2:4] = np.nan   # region 1 of both samples: where it is nowhere positive it may hold anything
    w2 = np.stack([w[0] + w[1], np.zeros(S), w[2]])
    assert np.all(np.isfinite(regions.attention_reference(q, k, v, w2, H)))


# ------------------------------------------------------------------------------------------------------------------ plans
def _walk_unet(nb, h, w, R=0, rows=0, ctx_rows=None):
    """Every Plan.rec call of emit_unet at fused batch nb (tests/_layer_walk.py walk_all's hook), the last `rows` rows conditional
    rows over R regions; the planes live in a Buf of the plan so that their extents can be checked."""
    from minsdtf_amd import engine, regions

    out = []
    orig = engine.Plan.rec

    def rec(self, fn, **kw):
        ops_ = {}
        for k, v in kw.items():
            if k == "split" and v is not None:
                continue
            o = LW._operand(v)
            if o is not None:
                ops_[k] = o
        out.append(LW.Rec(fn.__name__, kw.get("name", ""), kw, ops_))
        return orig(self, fn, **kw)

    engine.Plan.rec = rec
    try:
        p = engine.Plan("cpu")
        e = engine.Emitter(p, LW._AnyWeights())
        T = LW._Tensor
        cr = nb if ctx_rows is None else ctx_rows
        ctx = engine.Act(p.alloc(cr * 77 * 768 * 2), cr, 77, 1, 768)
        kv = engine.emit_context_kv(e, ctx, engine.UNET_ATTN_LAYERS, p)
        temb = (T(), 0, 0, engine.temb_columns(False))
        ra = None
        if R:
            levels = engine.unet_levels(h, w)
            offs = regions.level_offsets(R, levels)
            wbuf = p.alloc(offs[-1] * 4)
            ra = (R, rows, {lv: wbuf.at(o * 4) for lv, o in zip(levels, offs)})
        n0 = len(out)
        engine.emit_unet(e, T(), max(rows, 1) if R else nb, nb, h, w, temb, kv, 77, T(), None, variant=engine.UNetVariant(region_attn=ra))
    finally:
        engine.Plan.rec = orig
    return out[n0:], p


def _sig(recs):
    def one(v):
        return v if v is None or isinstance(v, (int, float, str, bool, tuple)) and not isinstance(v, tuple) else type(v).__name__

    return [(r.op, r.name, sorted((k, one(v)) for k, v in r.kw.items())) for r in recs]


def test_regions_zero_records_the_plain_plan():
    plain = LW.walk_all("unet", 2, 8, 8)[0]
    mine = _walk_unet(2, 8, 8)[0]
    tail = plain[len(plain) - len(mine):]
    assert _sig(mine) == _sig(tail) and len(mine) > 200
    assert not any(r.op == "region_attention" for r in mine)


@pytest.mark.parametrize("hw", [(64, 64), (8, 8)])
@pytest.mark.parametrize("nb,B", [(2, 1), (1, 1), (4, 2)])
def test_attention_mode_plan(hw, nb, B):
    """R = 3: exactly 16 msd_region_attention launches with batch = B, at every level's own plane, no msd_region_combine; every
    operand of every launch fits its Buf from the operand's address and lies in a live Buf."""
    h, w = hw
    R = 3
    bu = nb - B
    recs, _plan = _walk_unet(nb, h, w, R=R, rows=B, ctx_rows=bu + R * B)
    ra = [r for r in recs if r.op == "region_attention"]
    assert len(ra) == 16 and not any(r.op in ("region_combine", "cross_attention_q") for r in recs)
    assert all(r.kw["batch"] == B and r.kw["regions"] == R and r.kw["t"] == 77 and r.kw["w_ld"] == r.kw["s"] for r in ra)
    assert sorted({r.kw["s"] for r in ra}) == sorted({a * b for a, b in _levels(h, w)[:3]} | {_levels(h, w)[3][0] * _levels(h, w)[3][1]})
    plain_attn2 = [r for r in recs if r.op == "attention" and r.name.endswith(".attn2")]
    assert len(plain_attn2) == (16 if bu else 0) and all(r.kw["batch"] == bu for r in plain_attn2)
    for r in recs:
        ext_fn = XR.EXTENTS.get(r.op) or X.EXTENTS[r.op]
        dims = {k: (v if v is None or isinstance(v, (int, float, str, bool)) else
                    (tuple(x if x is None or isinstance(x, (int, float)) else True for x in v) if isinstance(v, tuple) else True))
                for k, v in r.kw.items() if k != "name"}
        ext = ext_fn(**dims)
        seen = []
        for name, o in r.operands.items():
            assert name in ext, f"{r.op} '{r.name}': operand '{name}' has no extent"
            need, role = ext[name]
            if o.kind != "buf":
                continue
            assert need <= o.avail, f"{r.op} '{r.name}': operand '{name}' needs {need} bytes, its buffer has {o.avail}"
            assert not o.freed, f"{r.op} '{r.name}': operand '{name}' lies in a freed buffer"
            seen.append((name, role, o.offset, o.offset + need))
        if r.op == "region_attention":
            assert set(r.operands) == {"q", "k", "vt", "w", "out"} and all(o.kind == "buf" for o in r.operands.values())
            for i, (na, _ra, lo_a, hi_a) in enumerate(seen):
                for nb_, _rb, lo_b, hi_b in seen[i + 1:]:
                    assert not (lo_a < hi_b and lo_b < hi_a), f"'{r.name}': operands '{na}' and '{nb_}' share bytes"


def test_attention_mode_plan_refuses_long_contexts():
    from minsdtf_amd import engine

    p = engine.Plan("cpu")
    e = engine.Emitter(p, LW._AnyWeights())
    ctx = engine.Act(p.alloc(3 * 154 * 768 * 2), 3, 154, 1, 768)
    kv = engine.emit_context_kv(e, ctx, engine.UNET_ATTN_LAYERS, p)
    with pytest.raises(ValueError, match="context tokens"):
        engine.emit_unet(e, LW._Tensor(), 1, 1, 8, 8, (LW._Tensor(), 0, 0, engine.temb_columns(False)), kv, 154, LW._Tensor(), None,
                         variant=engine.UNetVariant(region_attn=(3, 1, {lv: LW._Tensor() for lv in engine.unet_levels(8, 8)})))


# ---------------------------------------------------------------------------------------------------- argument checks
BASE = 1 << 20   # (addresses are only compared and checked for alignment: every bad call returns before a launch)


def _args(**over):
    from minsdtf_amd import _lib

    B, H, d, S, T, R = 2, 8, 40, 64, 77, 3
    C = H * d
    a = dict(q=BASE, k=2 * BASE, vt=4 * BASE, w=6 * BASE, out=7 * BASE, batch=B, heads=H, head_dim=d, s=S, t=T, regions=R, q_ld=C,
             k_ld=C, vt_ld=80, w_ld=S, o_ld=C)
    a.update(over)
    s = _lib.MsdRegionAttention()
    for k, v in a.items():
        setattr(s, k, v)
    return s


BAD = [dict(q=None), dict(k=None), dict(vt=None), dict(w=None), dict(out=None),
       dict(q=BASE + 8), dict(k=2 * BASE + 2), dict(vt=4 * BASE + 4), dict(w=6 * BASE + 4), dict(out=7 * BASE + 8),
       dict(head_dim=64), dict(head_dim=0), dict(head_dim=320), dict(t=0), dict(t=97), dict(t=-1), dict(regions=0), dict(regions=17),
       dict(batch=0), dict(batch=65536), dict(w_ld=63), dict(o_ld=312), dict(o_ld=324), dict(q_ld=324), dict(k_ld=324), dict(vt_ld=84),
       dict(vt_ld=72), dict(s=0),
       dict(out=BASE), dict(out=BASE + 64), dict(out=2 * BASE + 320 * 2 * 77), dict(out=4 * BASE + 16), dict(out=6 * BASE),
       dict(out=6 * BASE + 2 * 64 * 4 + 16), dict(out=BASE - 16)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_argument_errors_without_a_device(bad):
    from minsdtf_amd import _lib

    lib = _lib.load()
    assert lib.msd_region_attention(ctypes.byref(_args(**bad)), None) == -1, bad   # MSD_E_ARG
    assert b"region_attention" in lib.msd_last_error()


def test_null_struct_is_an_argument_error():
    from minsdtf_amd import _lib

    assert _lib.load().msd_region_attention(None, None) == -1


def test_struct_layout_matches_the_header():
    import os
    import subprocess
    import tempfile

    from minsdtf_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [n for n, _t in _lib.MsdRegionAttention._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "minsdtf_hip.h"\nint main(){printf("%zu", sizeof(MsdRegionAttention));' + \
        "".join(f'printf(" %zu", offsetof(MsdRegionAttention, {f}));' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(_lib.MsdRegionAttention)] + [getattr(_lib.MsdRegionAttention, f).offset for f in fields]


# ------------------------------------------------------------------------------------------- generate_image: refusals
@pytest.fixture()
def pipe(monkeypatch):
    """A pipeline whose device work raises: everything checked here must come before it."""
    from minsdtf_amd import stable_diffusion as sdm

    class Reached(Exception):
        pass

    sd = sdm.StableDiffusion(64, 64, jit_compile=True, device="cpu")
    sd.unconditional_context = np.zeros((77, 768), dtype=np.float32)

    def boom(*a, **k):
        raise Reached()

    monkeypatch.setattr(sdm.StableDiffusionBase, "_run_sharded", boom)
    return sd, Reached


def _job(prompts, masks, mode="attention", base_weight=0.0):
    return dict(regions=[dict(prompt=p, mask=m) for p, m in zip(prompts, masks)], base_weight=base_weight, mode=mode)


def test_cap_arithmetic_and_refusals(pipe):
    from minsdtf_amd import regions
    from minsdtf_amd import tiled as tiled_mod

    sd, Reached = pipe
    assert tiled_mod.MAX_VIEW_BATCH == 6
    ctx = np.zeros((77, 768), dtype=np.float32)
    sixteen = _job([ctx] * 16, regions.boxes(8, 8, 4, 4))
    kw = dict(num_steps=2, seed=1)
    # sixteen regions at batch 6: 12 UNet rows, accepted (the device work is reached)
    with pytest.raises(Reached):
        sd.generate_image(ctx, regions=sixteen, batch_size=6, **kw)
    with pytest.raises(ValueError, match=r'mode="attention" are 14 UNet rows per step, more than 2 \* tiled.MAX_VIEW_BATCH = 12'):
        sd.generate_image(ctx, regions=sixteen, batch_size=7, **kw)
    # latent mode: its cap and its message are what they were
    three = _job([ctx] * 3, regions.boxes(8, 8, 1, 3), mode="latent")
    with pytest.raises(ValueError) as ei:
        sd.generate_image(ctx, regions=three, batch_size=4, **kw)
    assert str(ei.value) == ("regions: 4 image(s) of 1 + 3 prompts are 16 UNet rows per step, more than 2 * tiled.MAX_VIEW_BATCH = 12: "
                             "use fewer regions or a smaller batch")
    with pytest.raises(Reached):   # ... and attention mode takes that job
        sd.generate_image(ctx, regions=dict(three, mode="attention"), batch_size=4, **kw)
    # contexts above 96 tokens
    long_ctx = np.zeros((154, 768), dtype=np.float32)
    with pytest.raises(ValueError, match='mode="latent"'):
        sd.generate_image(long_ctx, regions=_job([long_ctx] * 2, _halves()), **kw)
    # the refusal rules are those of regions
    with pytest.raises(ValueError, match="regions is text-to-image on one stream only: it cannot be combined with tiled"):
        sd.generate_image(ctx, regions=_job([ctx] * 2, _halves()), tiled=dict(height=128, width=128), **kw)
    with pytest.raises(ValueError, match="mode"):
        sd.generate_image(ctx, regions=_job([ctx] * 2, _halves(), mode="both"), **kw)

