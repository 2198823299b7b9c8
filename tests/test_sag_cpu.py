"""Self-attention guidance, everything that needs no GPU: the job description, the host statements of the two device steps
(against a torch restatement of diffusers' sag_masking written here, and against the formula), the recorded plans on tensor-less
stand-ins with the operand extents of every new launch, the extension library's C ABI (symbols, struct layouts, argument checks
through the library) and generate_image's refusals, cap and engine key, which come before any device work."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _extents as X
import _extents_sag as XS
import _layer_walk as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ parse
def test_parse_accepts():
    from minsdtf_amd import sag

    assert sag.parse(None) is None
    d = sag.parse({})
    assert (d.scale, d.blur_sigma, d.threshold) == (0.75, 1.0, 1.0) == tuple(getattr(sag.SagSpec(), f) for f in ("scale", "blur_sigma", "threshold"))
    assert sag.parse(True) == d and sag.parse(sag.SagSpec()) == d and sag.parse(d) is d
    r = sag.parse(dict(scale=3, blur_sigma=3.0, threshold=0.0))
    assert r == sag.Resolved(3.0, 3.0, 0.0) and isinstance(r.scale, float)
    assert sag.parse(sag.SagSpec(scale=0.1, threshold=-1.0)).threshold == -1.0


@pytest.mark.parametrize("bad, match", [
    (dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"), (dict(scale=float("nan")), "scale"), (dict(scale="much"), "scale"),
    (dict(scale=True), "scale"), (dict(blur_sigma=0.0), "blur_sigma"), (dict(blur_sigma=3.5), "blur_sigma"),
    (dict(blur_sigma=float("inf")), "blur_sigma"), (dict(threshold=float("nan")), "threshold"), (dict(threshold=None), "threshold"),
    (dict(scales=1.0), "unknown field"), ("mid", "SagSpec"), (0.75, "SagSpec"), (False, "SagSpec")])
def test_parse_rejects(bad, match):
    from minsdtf_amd import sag

    with pytest.raises(ValueError, match=match):
        sag.parse(bad)


def test_taps_and_params():
    from minsdtf_amd import sag

    for s in (0.3, 1.0, 3.0):
        t = sag.taps(s)
        i = np.arange(9, dtype=np.float64) - 4
        want = np.exp(-0.5 * (i / s) ** 2)
        assert t.dtype == np.float32 and t.shape == (9,)
        np.testing.assert_array_equal(t, (want / want.sum()).astype(np.float32))
        np.testing.assert_array_equal(t, t[::-1])
        assert abs(float(t.astype(np.float64).sum()) - 1.0) <= 9 * 2.0 ** -25
    p = sag.params(sag.parse(dict(blur_sigma=2.0, threshold=1.25)))
    assert p.dtype == np.float32 and p.shape == (10,) and p[9] == np.float32(1.25)
    np.testing.assert_array_equal(p[:9], sag.taps(2.0))


# --------------------------------------------------------------------------------------------------------------- degrade_host
def _sag_masking_torch(x, e, alpha, sigma, A, map_hw, blur_sigma, threshold):
    """diffusers' sag_masking and its re-noising, restated: the mask reshaped to the map and F.interpolate'd (nearest), a reflect
    pad of 4, ONE conv2d with the 9 x 9 outer-product kernel, degraded = blur * mask + x0 * (1 - mask), then alpha * degraded +
    sigma * e EVERYWHERE (NHWC float64 in and out)."""
    import torch
    import torch.nn.functional as F

    B, h, w, C = x.shape
    x0 = torch.from_numpy((x - sigma * e) / alpha).permute(0, 3, 1, 2)
    mask = (torch.from_numpy(np.asarray(A, dtype=np.float32)) > np.float32(threshold)).reshape(B, 1, *map_hw).to(torch.float64)
    mask = F.interpolate(mask, (h, w)).expand(B, C, h, w)
    i = torch.arange(9, dtype=torch.float64) - 4
    t = torch.exp(-0.5 * (i / blur_sigma) ** 2)
    t = t / t.sum()
    kern = (t[:, None] * t[None, :]).expand(C, 1, 9, 9)
    blur = F.conv2d(F.pad(x0, (4, 4, 4, 4), mode="reflect"), kern, groups=C)
    deg = blur * mask + x0 * (1 - mask)
    return alpha * deg.permute(0, 2, 3, 1).numpy() + sigma * e, mask[:, 0].numpy() > 0.5


@pytest.mark.parametrize("hw, map_hw", [((8, 8), (1, 1)), ((16, 24), (2, 3)), ((64, 64), (8, 8))])
@pytest.mark.parametrize("blur_sigma", [1.0, 2.5])
def test_degrade_host_against_diffusers_masking(hw, map_hw, blur_sigma):
    """Inside the mask: rounding only (float64 against float64 in another order, fp32 taps against float64 taps: 1e-6 of the
    values).  Outside: degrade_host returns x ITSELF where diffusers recomputes alpha * x0 + sigma * e - the documented deviation -
    which is x up to float64 rounding."""
    from minsdtf_amd import sag

    h, w = hw
    rng = np.random.default_rng(h * 100 + w)
    B = 2
    x = rng.standard_normal((B, h, w, 4)).astype(np.float32)
    e = rng.standard_normal((B, h, w, 4)).astype(np.float32)
    A = rng.uniform(0.5, 1.5, (B, map_hw[0] * map_hw[1])).astype(np.float32)
    A[0, 0], A[1, -1] = 1.5, 0.5   # (both sides of the threshold in every case, the 1 x 1 map included)
    alpha, sigma = 0.8, 0.6
    got = sag.degrade_host(x, e, alpha, sigma, A, map_hw, sag.taps(blur_sigma), 1.0)
    want, mask = _sag_masking_torch(x.astype(np.float64), e.astype(np.float64), alpha, sigma, A, map_hw, blur_sigma, 1.0)
    assert got.dtype == np.float64 and got.shape == x.shape
    np.testing.assert_array_equal(mask, sag.mask_host(A, map_hw, h, w, 1.0))   # the integer nearest map is torch's here: h % mh == 0
    assert mask.any() and not mask.all()
    np.testing.assert_array_equal(got[~mask], x.astype(np.float64)[~mask])            # bit for bit the latent
    np.testing.assert_allclose(want[~mask], x.astype(np.float64)[~mask], rtol=0, atol=1e-14)   # ... which diffusers' form only rounds
    np.testing.assert_allclose(got[mask], want[mask], rtol=0, atol=2e-6)              # fp32 taps against float64 taps
    assert np.abs(got[mask] - x[mask]).max() > 1e-2


def test_degrade_host_reflect_limit_and_the_non_integer_map():
    from minsdtf_amd import sag

    x = np.random.default_rng(0).standard_normal((1, 5, 5, 4))
    out = sag.degrade_host(x, np.zeros_like(x), 1.0, 0.0, np.full((1, 1), 2.0), (1, 1), sag.taps(1.0), 1.0)
    assert out.shape == x.shape and np.all(np.isfinite(out))
    with pytest.raises(ValueError, match="reflect"):
        sag.degrade_host(x[:, :4], np.zeros_like(x[:, :4]), 1.0, 0.0, np.full((1, 1), 2.0), (1, 1), sag.taps(1.0), 1.0)
    # 9 x 9 latent over a 2 x 2 map: rows 0 .. 4 read map row 0 (floor(y * 2 / 9)), rows 5 .. 8 map row 1
    m = sag.mask_host(np.asarray([[2.0, 0.0, 0.0, 2.0]]), (2, 2), 9, 9, 1.0)[0]
    assert m[:5, :5].all() and not m[:5, 5:].any() and not m[5:, :5].any() and m[5:, 5:].all()
    # exactly the threshold is not above it
    assert not sag.mask_host(np.ones((1, 1), dtype=np.float32), (1, 1), 8, 8, 1.0).any()


def test_combine_host_against_the_formula():
    """eps = u + g (c - u) + s (u - d) == u + g (c' - u) with c' = k u + c - k d, k = s / g; without guidance (1 + s) c - s d.  In fp32
    in the kernel's order; against float64 within a few fp32 roundings of the largest term."""
    from minsdtf_amd import sag

    rng = np.random.default_rng(1)
    u, c, d = (rng.standard_normal((2, 8, 8, 4)).astype(np.float32) for _ in range(3))
    g, s = 7.5, 3.0
    w = sag.weights(s, g, 8, 8)
    assert w.shape == (3, 8, 8) and w.dtype == np.float32
    k = np.float32(s / g)
    np.testing.assert_array_equal(w[:, 0, 0], np.asarray([k, 1.0, -k], dtype=np.float32))
    got = sag.combine_host(u, c, d, w)
    assert got.dtype == np.float32
    u6, c6, d6 = (a.astype(np.float64) for a in (u, c, d))
    want = float(k) * u6 + c6 - float(k) * d6
    assert np.abs(got - want).max() <= 3 * 2.0 ** -24 * np.abs(want).max() + 2.0 ** -24 * (np.abs(u6).max() + np.abs(d6).max())
    # the pinned order: v = k u; v = fma(1, c, v); v = fma(-k, d, v)
    v = (k * u).astype(np.float32)
    v = (c.astype(np.float64) + v.astype(np.float64)).astype(np.float32)
    v = ((-float(k)) * d6 + v.astype(np.float64)).astype(np.float32)
    np.testing.assert_array_equal(got, v)
    full = u6 + g * (want - u6)
    np.testing.assert_allclose(full, u6 + g * (c6 - u6) + g * float(k) * (u6 - d6), rtol=1e-12, atol=1e-12)
    # no guidance
    w0 = sag.weights(s, 0.0, 8, 8)
    np.testing.assert_array_equal(w0[:, 0, 0], np.asarray([1.0 + s, -s], dtype=np.float32))
    got0 = sag.combine_host(None, c, d, w0)
    np.testing.assert_allclose(got0, (1 + s) * c6 - s * d6, rtol=0, atol=4 * 2.0 ** -24 * (1 + s) * np.abs(c6).max())


# ------------------------------------------------------------------------------------------------------------------ plans
def _record(fn):
    """Run fn(plan, emitter, T) with engine.Plan.rec hooked: the Rec records of tests/_layer_walk.py, and the plan."""
    from minsdtf_amd import engine

    out = []
    orig = engine.Plan.rec

    def rec(self, f, **kw):
        ops_ = {}
        for k, v in kw.items():
            if k == "split" and v is not None:
                continue
            o = LW._operand(v)
            if o is not None:
                ops_[k] = o
        out.append(LW.Rec(f.__name__, kw.get("name", ""), kw, ops_))
        return orig(self, f, **kw)

    engine.Plan.rec = rec
    try:
        p = engine.Plan("cpu")
        e = engine.Emitter(p, LW._AnyWeights(), step_ptr=LW._Tensor())
        fn(p, e, LW._Tensor)
    finally:
        engine.Plan.rec = orig
    return out, p


def _sag_step(B, h, w, cfg=True, sampler=False):
    """A whole SAG step as DenoiseEngine records it, every buffer of its own a Buf of the plan: pass 1 with the map, the degrade,
    pass 2, the combine, the step kernel."""
    from minsdtf_amd import engine, ops

    def build(p, e, T):
        NB = 2 * B if cfg else B
        n = h * w * 4
        mh, mw = engine.unet_levels(h, w)[3]
        ctx = engine.Act(p.alloc(NB * 77 * 768 * 2), NB, 77, 1, 768)
        kv = engine.emit_context_kv(e, ctx, engine.UNET_ATTN_LAYERS, p)
        temb = (T(), 0, 0, engine.temb_columns(False))
        latent, degraded = p.alloc(B * n * 4), p.alloc(B * n * 4)
        eps = p.alloc((5 if cfg else 2) * B * n * 4)
        A, params, coef = p.alloc(B * mh * mw * 4), p.alloc(10 * 4), p.alloc(4 * (8 if sampler else 4) * 4)
        planes = p.alloc((3 if cfg else 2) * h * w * 4)
        ws = p.alloc(ops.colsum_workspace_floats(B, 8, mh * mw) * 4)
        build.first = len(p.recs)
        engine.emit_unet(e, latent, B, NB, h, w, temb, kv, 77, eps, variant=engine.UNetVariant(sag=(A, ws, 0, B)))
        p.free(ws)
        engine.emit_sag_pass(e, latent, eps, coef, 8 if sampler else 4, 4, A, params, degraded, B, h, w, temb, kv, 77,
                             eps.at((2 if cfg else 1) * B * n * 4))
        group = engine.emit_sag_combine(p, lambda g: eps.at(g * B * n * 4), lambda i: planes.at(i * h * w * 4), B, n, cfg)
        assert group == (3 if cfg else 0)
        p.rec(ops.cfg_step, eps=eps.at(group * B * n * 4), latent=latent, coef=coef, step_ptr=T(), batch=B, n=n, num_steps=4, guidance=7.5,
              guidance_rescale=0.0, advance=2)

    recs, plan = _record(build)
    return recs[build.first:], plan


def _sig(recs):
    def one(v):
        return v if v is None or isinstance(v, (int, float, str, bool)) else type(v).__name__

    return [(r.op, r.name, sorted((k, one(v)) for k, v in r.kw.items())) for r in recs]


def test_sag_none_records_the_plain_plan():
    """emit_unet without `sag` (and with sag=None) records what the parent's plain walk records, name by name, keyword by keyword."""
    from minsdtf_amd import engine

    plain = LW.walk_all("unet", 2, 8, 8)[0]

    def build(p, e, T):
        ctx = engine.Act(p.alloc(2 * 77 * 768 * 2), 2, 77, 1, 768)
        kv = engine.emit_context_kv(e, ctx, engine.UNET_ATTN_LAYERS, p)
        build.first = len(p.recs)
        engine.emit_unet(e, T(), 2, 2, 8, 8, (T(), 0, 0, engine.temb_columns(False)), kv, 77, T(), None, variant=engine.UNetVariant(sag=None))

    mine = _record(build)[0][build.first:]
    tail = plain[len(plain) - len(mine):]
    assert len(mine) > 200 and [(r.op, r.name) for r in mine] == [(r.op, r.name) for r in tail]
    assert not any(r.op in ("attention_colsum", "sag_degrade") for r in mine)
    # ... and the pass with the map is that plan plus ONE launch, right behind the mid block's attn1
    recs, _plan = _sag_step(2, 8, 8, cfg=False)
    first_pass = recs[:len(mine) + 1]
    names = [r.name for r in first_pass]
    mid = "mid_block.attentions.0.transformer_blocks.0.attn1"
    i = names.index(mid)
    assert names[i + 1] == mid + ".colsum" and first_pass[i + 1].op == "attention_colsum"
    assert [(r.op, r.name) for r in first_pass[:i + 1] + first_pass[i + 2:]] == [(r.op, r.name) for r in mine]


@pytest.mark.parametrize("cfg, sampler", [(True, False), (True, True), (False, False)])
@pytest.mark.parametrize("B, hw", [(1, (16, 16)), (2, (64, 64)), (2, (8, 8)), (1, (8, 16))])
def test_sag_step_plan(B, hw, cfg, sampler):
    """The launch-name sequence of a step - ... mid_block ... attn1, attn1.colsum, ..., sag.degrade, a second conv_in, ..., the
    combine, the step kernel - and the operand extents of every launch inside live buffers of the plan."""
    from minsdtf_amd import engine

    h, w = hw
    recs, _plan = _sag_step(B, h, w, cfg, sampler)
    names = [r.name or r.op for r in recs]   # (the step kernel is recorded without a name: its Call takes the op's)
    mid = "mid_block.attentions.0.transformer_blocks.0.attn1"
    i, j = names.index(mid), names.index("sag.degrade")
    assert names[i + 1] == mid + ".colsum" and names.count(mid + ".colsum") == 1 and i + 1 < j
    assert names[j - 1] == "conv_out" and names[j + 1] == "conv_in" and names.count("conv_in") == 2 and names.count("conv_out") == 2
    assert names.index(mid, i + 1) > j   # the second pass: a plain mid block
    tail = ["sag.copy_u", "sag.combine", "cfg_step"] if cfg else ["sag.combine", "cfg_step"]
    assert names[-len(tail):] == tail and names[-len(tail) - 1] == "conv_out"
    mh, mw = engine.unet_levels(h, w)[3]
    cs = recs[i + 1]
    assert cs.op == "attention_colsum" and (cs.kw["batch"], cs.kw["heads"], cs.kw["head_dim"], cs.kw["s"]) == (B, 8, 160, mh * mw)
    dg = recs[j]
    assert dg.op == "sag_degrade" and (dg.kw["batch"], dg.kw["h"], dg.kw["w"], dg.kw["mh"], dg.kw["mw"]) == (B, h, w, mh, mw)
    assert dg.kw["coef_stride"] == (8 if sampler else 4) and dg.kw["step_ptr"] is not None
    second_conv_in = recs[j + 1]
    assert second_conv_in.kw["batch"] == B and second_conv_in.kw["in_batch_mod"] == B
    assert second_conv_in.operands["x"].buf == dg.operands["out"].buf   # the second pass reads the degraded latent
    combine = recs[-2]
    assert combine.kw["regions"] == (3 if cfg else 2) and combine.kw["batch"] == B
    if cfg:
        assert recs[-3].kw["regions"] == 1
        assert combine.operands["out"].offset == combine.operands["eps"].offset + 4 * B * h * w * 16
        assert recs[-1].operands["eps"].offset == combine.operands["eps"].offset + 3 * B * h * w * 16
    else:
        assert combine.operands["out"].offset == combine.operands["eps"].offset == recs[-1].operands["eps"].offset
    checked = 0
    for r in recs:
        ext_fn = XS.EXTENTS.get(r.op) or X.EXTENTS[r.op]
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
        if r.op in XS.EXTENTS:   # the new launches: every operand a buffer of the plan, outputs apart from everything else
            checked += 1
            want = {"attention_colsum": {"q", "k", "out", "workspace"},
                    "sag_degrade": {"latent", "eps", "coef", "colsum", "params", "out", "step_ptr"}}[r.op]
            assert set(r.operands) == want
            for a, (na, ra, lo_a, hi_a) in enumerate(seen):
                for nb_, rb, lo_b, hi_b in seen[a + 1:]:
                    if "out" in (ra, rb):
                        assert not (lo_a < hi_b and lo_b < hi_a), f"'{r.name}': operands '{na}' and '{nb_}' share bytes"
    assert checked == 2


def test_colsum_is_refused_where_it_cannot_run():
    from minsdtf_amd import engine

    def build(p, e, T):
        x = p.act(2, 8, 8, 320)   # head size 40
        e.attentions(x, "down_blocks.0.attentions.0", {"down_blocks.0.attentions.0.transformer_blocks.0.attn2": (T(), T(), 80)}, 77,
                     variant=engine.AttnVariant(colsum=(T(), T(), 0, 2)))

    with pytest.raises(ValueError, match="colsum"):
        _record(build)

    def rows(p, e, T):
        x = p.act(2, 2, 2, 1280)
        e.attentions(x, "mid_block.attentions.0", {"mid_block.attentions.0.transformer_blocks.0.attn2": (T(), T(), 80)}, 77,
                     variant=engine.AttnVariant(colsum=(T(), T(), 1, 2)))

    with pytest.raises(ValueError, match="colsum"):
        _record(rows)


# -------------------------------------------------------------------------------------------------------------- the C ABI
def test_extension_library_exports_its_header_and_the_core_is_untouched():
    from minsdtf_amd import _lib, _lib_ext

    assert os.path.exists(_lib_ext.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    header = open(os.path.join(ROOT, "include", "minsdtf_hip_ext.h")).read()
    declared = set(re.findall(r"^MSDX_API\s+(?:int|const char\*)\s+(msdx_\w+)\s*\(", header, flags=re.M))
    assert declared == set(_lib_ext.SYMBOLS) == {"msdx_abi_version", "msdx_last_error", "msdx_attention_colsum", "msdx_sag_degrade"}
    assert not re.search(r"^(?:int|const char\*)\s+msdx_\w+\s*\(", header, flags=re.M), "a declaration without MSDX_API"
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib_ext.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert exported == declared, sorted(exported ^ declared)
    lib = _lib_ext.load()
    assert lib.msdx_abi_version() == _lib_ext.ABI_VERSION == int(re.search(r"#define MSDX_ABI_VERSION (\d+)", header).group(1))
    # the core library exports no msdx_ symbol and its binding knows none
    core = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert "msdx_" not in core and not any(n.startswith("msdx_") for n in _lib.SYMBOLS)


@pytest.mark.parametrize("struct", ["MsdxAttentionColsum", "MsdxSagDegrade"])
def test_struct_layout_matches_the_header(struct):
    from minsdtf_amd import _lib_ext

    cls = getattr(_lib_ext, struct)
    fields = [n for n, _t in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "minsdtf_hip_ext.h"\nint main(){printf("%zu", sizeof(' + struct + '));' + \
        "".join(f'printf(" %zu", offsetof({struct}, {f}));' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]


BASE = 1 << 20   # (addresses are only compared and checked for alignment: every bad call returns before a launch)


def _colsum(**over):
    from minsdtf_amd import _lib_ext

    a = dict(q=BASE, k=2 * BASE, out=3 * BASE, workspace=4 * BASE, workspace_floats=2 * 8 * 64 * 2, batch=2, heads=8, head_dim=160, s=64,
             q_ld=1280, k_ld=1280)
    a.update(over)
    s = _lib_ext.MsdxAttentionColsum()
    for k, v in a.items():
        setattr(s, k, v)
    return s


COLSUM_BAD = [dict(q=None), dict(k=None), dict(out=None), dict(workspace=None), dict(q=BASE + 8), dict(k=2 * BASE + 2), dict(out=3 * BASE + 4),
              dict(workspace=4 * BASE + 8), dict(head_dim=40), dict(head_dim=80), dict(head_dim=0), dict(heads=0), dict(heads=65), dict(s=0),
              dict(s=4097), dict(s=-1), dict(batch=0), dict(batch=65536), dict(q_ld=1272), dict(q_ld=1284), dict(k_ld=1272), dict(k_ld=1284),
              dict(workspace_floats=2 * 8 * 64 * 2 - 1), dict(workspace_floats=0), dict(out=BASE), dict(out=2 * BASE + 64), dict(out=4 * BASE),
              dict(workspace=BASE + 1280 * 2 * 127), dict(workspace=3 * BASE + 2 * 64 * 4 - 16), dict(workspace=2 * BASE - 16)]


@pytest.mark.parametrize("bad", COLSUM_BAD, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_colsum_argument_errors_without_a_device(bad):
    from minsdtf_amd import _lib_ext

    lib = _lib_ext.load()
    assert lib.msdx_attention_colsum(ctypes.byref(_colsum(**bad)), None) == -1, bad   # MSD_E_ARG
    assert b"attention_colsum" in lib.msdx_last_error()


def _degrade(**over):
    from minsdtf_amd import _lib_ext

    a = dict(latent=BASE, eps=2 * BASE, coef=3 * BASE, step_ptr=4 * BASE, colsum=5 * BASE, params=6 * BASE, out=7 * BASE, batch=2, h=16,
             w=24, mh=2, mw=3, coef_stride=4, num_steps=3)
    a.update(over)
    s = _lib_ext.MsdxSagDegrade()
    for k, v in a.items():
        setattr(s, k, v)
    return s


N_DEG = 2 * 16 * 24 * 16
DEGRADE_BAD = [dict(latent=None), dict(eps=None), dict(coef=None), dict(colsum=None), dict(params=None), dict(out=None),
               dict(latent=BASE + 8), dict(eps=2 * BASE + 4), dict(out=7 * BASE + 8), dict(coef=3 * BASE + 2), dict(colsum=5 * BASE + 1),
               dict(params=6 * BASE + 2), dict(step_ptr=4 * BASE + 2), dict(h=4), dict(w=4), dict(h=0), dict(h=4097), dict(w=4097),
               dict(mh=0), dict(mw=0), dict(mh=17), dict(mw=25), dict(batch=0), dict(batch=65536), dict(coef_stride=1), dict(coef_stride=0),
               dict(num_steps=0), dict(out=BASE), dict(out=BASE + N_DEG - 16), dict(out=2 * BASE + 16), dict(out=3 * BASE), dict(out=4 * BASE),
               dict(out=5 * BASE + 16), dict(out=6 * BASE + 32), dict(out=BASE - 16)]


@pytest.mark.parametrize("bad", DEGRADE_BAD, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_degrade_argument_errors_without_a_device(bad):
    from minsdtf_amd import _lib_ext

    lib = _lib_ext.load()
    assert lib.msdx_sag_degrade(ctypes.byref(_degrade(**bad)), None) == -1, bad   # MSD_E_ARG
    assert b"sag_degrade" in lib.msdx_last_error()


def test_null_structs_are_argument_errors():
    from minsdtf_amd import _lib_ext

    lib = _lib_ext.load()
    assert lib.msdx_attention_colsum(None, None) == -1 and b"null" in lib.msdx_last_error()
    assert lib.msdx_sag_degrade(None, None) == -1 and b"null" in lib.msdx_last_error()


# ------------------------------------------------------------------------------------------------- generate_image, no device
def test_refused_names_every_excluded_argument():
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    what, arguments, states = StableDiffusionBase._REFUSED["sag"]
    assert what == "text-to-image on one stream only"
    assert set(arguments) == {"regions", "tiled", "hires", "pag", "reference_only", "hypertile", "control_net_image", "reference_image",
                              "inpaint_mask"}
    assert tuple(states) == ("denoise_streams = 2",)
    # the entries that were there keep their words
    assert StableDiffusionBase._REFUSED["pag"] == ("text-to-image on one stream only",
                                                   ("regions", "tiled", "hires", "control_net_image", "reference_image", "inpaint_mask"),
                                                   ("denoise_streams = 2",))


def test_refusals_and_the_cap_come_before_any_device_work():
    from minsdtf_amd import regions, tiled
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    ctx = np.zeros((77, 768), dtype=np.float32)
    img = np.zeros((64, 64, 3), dtype=np.uint8)
    sd = StableDiffusionBase(64, 64)   # (no models behind it: anything that reaches a model fails another way)
    kw = dict(batch_size=1, num_steps=3, seed=0, sag=dict(scale=1.0))
    halves = dict(regions=[dict(prompt=ctx, mask=m) for m in regions.boxes(8, 8, 1, 2)])
    for extra, names in ((dict(tiled=dict(size=(64, 128))), ["tiled"]), (dict(hires=dict(scale=2)), ["hires"]),
                         (dict(regions=halves), ["regions"]), (dict(pag=dict(scale=3.0)), ["pag"]),
                         (dict(hypertile=dict(tile=32)), ["hypertile"]),
                         (dict(reference_only=dict(latent=np.zeros((1, 8, 8, 4), dtype=np.float32))), ["reference_only"]),
                         (dict(control_net_image=img.astype(np.float32)), ["control_net_image"]),
                         (dict(reference_image=img), ["reference_image"]), (dict(inpaint_mask=img[..., 0]), ["inpaint_mask"]),
                         (dict(pag=dict(scale=3.0), inpaint_mask=img[..., 0]), ["pag", "inpaint_mask"])):
        with pytest.raises(ValueError, match="sag is text-to-image on one stream only: it cannot be combined with") as e:
            sd.generate_image(ctx, **kw, **extra)
        assert all(n in str(e.value) for n in names), str(e.value)
    two = StableDiffusionBase(64, 64)
    two.denoise_streams = 2
    with pytest.raises(ValueError, match="sag is.*denoise_streams = 2"):
        two.generate_image(ctx, **kw)
    with pytest.raises(ValueError, match="sag is"):
        sd.text_to_image(ctx, tiled=dict(size=(64, 128)), **kw)
    # the cap, in PAG's words: 3 * batch_size (2 * batch_size without guidance) <= 2 * tiled.MAX_VIEW_BATCH UNet rows
    assert 2 * tiled.MAX_VIEW_BATCH == 12
    with pytest.raises(ValueError) as e:
        sd.generate_image(ctx, **{**kw, "batch_size": 5})
    assert str(e.value) == "sag: 5 image(s) are 15 UNet rows per step, more than 2 * tiled.MAX_VIEW_BATCH = 12: use a smaller batch"
    with pytest.raises(ValueError, match=r"14 UNet rows.*MAX_VIEW_BATCH = 12"):
        sd.generate_image(ctx, unconditional_guidance_scale=0.0, **{**kw, "batch_size": 7})
    with pytest.raises(ValueError, match="unknown field"):
        sd.generate_image(ctx, batch_size=1, num_steps=3, sag=dict(sigma=3.0))
    with pytest.raises(ValueError, match="blur_sigma"):
        sd.generate_image(ctx, batch_size=1, num_steps=3, sag=dict(blur_sigma=4.0))
    assert not sd._engines


def test_engine_key_holds_the_fact_and_never_the_numbers():
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    class Net:
        weights_version = 1

    sd = StableDiffusionBase(64, 64)
    sd.diffusion_model = Net()
    args = (1, 77, 77, 4, 7.5, 0.0, False)
    plain = sd._engine_key(*args)
    assert sd._engine_key(*args, sag=None) == plain
    key = sd._engine_key(*args, sag=True)
    assert key != plain and key[:len(plain)] == plain and key[-1] == ("sag",)
    assert sd._engine_key(*args, sampler="euler_a", sag=True)[-1] == ("sag",)
