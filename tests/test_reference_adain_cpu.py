"""Reference AdaIN without a GPU: the `adain` field of the reference-only description and its site table, the float64 statement
of the kernel against torch, the library's export, the struct layout and the argument checks of msd_reference_adain, the recorded
plan and its operand extents, emit_unet's and generate_image's refusals, and the two oracle fixture files."""
import ctypes
import os
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import _extents_reference_adain as XA
import _layer_walk as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
Z = np.zeros((1, 8, 8, 4), dtype=np.float32)
SEVEN = ("down_blocks.3.resnets.0", "down_blocks.3.resnets.1", "mid_block.resnets.1", "up_blocks.0.resnets.0", "up_blocks.0.resnets.1",
         "up_blocks.0.upsamplers.0.conv", "up_blocks.1.attentions.0")
FIFTEEN = ("down_blocks.1.attentions.0", "down_blocks.1.attentions.1", "down_blocks.2.attentions.0", "down_blocks.2.attentions.1",
           "down_blocks.3.resnets.0", "down_blocks.3.resnets.1", "mid_block.resnets.1", "up_blocks.0.resnets.0", "up_blocks.0.resnets.1",
           "up_blocks.0.upsamplers.0.conv", "up_blocks.1.attentions.0", "up_blocks.1.attentions.1", "up_blocks.1.upsamplers.0.conv",
           "up_blocks.2.attentions.0", "up_blocks.2.attentions.1")


# ------------------------------------------------------------------------------------------------------------------ parse
def test_site_table_and_its_fifteen_weights():
    from minsdtf_amd import reference

    assert tuple(n for n, _gw in reference.ADAIN_SITES) == FIFTEEN
    gw = [g for _n, g in reference.ADAIN_SITES]
    assert gw[:6] == [Fraction(2 * (6 - i), 6) for i in range(6)] and gw[6] == 0 and gw[7:] == [Fraction(2 * i, 8) for i in range(8)]
    assert [float(g) for g in gw[7:]] == [0, .25, .5, .75, 1, 1.25, 1.5, 1.75]
    np.testing.assert_allclose([float(g) for g in gw[:6]], [2, 5 / 3, 4 / 3, 1, 2 / 3, 1 / 3], rtol=1e-15)
    assert not any(n.startswith(("down_blocks.0", "up_blocks.3")) or "downsamplers" in n for n in FIFTEEN)


def test_auto_is_weight_one_is_the_seven_sites_and_one_is_strict():
    from minsdtf_amd import reference

    assert reference.adain_sites(1.0) == frozenset(SEVEN)
    assert reference.parse(dict(latent=Z, adain="auto")).adain == frozenset(SEVEN)
    # gw == 1 is excluded at weight 1 and included just above it
    ones = {"down_blocks.2.attentions.1", "up_blocks.1.attentions.1"}
    assert not ones & reference.adain_sites(1.0) and ones <= reference.adain_sites(float(np.nextafter(1.0, 2.0)))
    # thirds compare exactly: float(1/3) lies below 1/3, so it does not select the site of gw = 1/3; the next float up does
    third = 1.0 / 3.0
    assert Fraction(third) < Fraction(1, 3)
    assert "down_blocks.3.resnets.1" not in reference.adain_sites(third)
    assert "down_blocks.3.resnets.1" in reference.adain_sites(float(np.nextafter(third, 1.0)))
    assert reference.adain_sites(2.0) == frozenset(FIFTEEN) - {"down_blocks.1.attentions.0"}
    assert reference.adain_sites(1e-300) == frozenset({"mid_block.resnets.1", "up_blocks.0.resnets.0"})


def test_parse_accepts():
    from minsdtf_amd import engine, reference

    off = reference.parse(dict(latent=Z))
    assert off.adain is None and off.adain_key is None and off.key == tuple(sorted(engine.PAG_LAYERS))
    assert reference.parse(dict(latent=Z, adain=None)).key == off.key
    every = reference.parse(dict(latent=Z, adain="all"))
    assert every.adain == frozenset(FIFTEEN) and every.layers == frozenset(engine.PAG_LAYERS)
    assert every.key == off.key + (("adain",) + tuple(sorted(FIFTEEN)),) and every.adain_key == tuple(sorted(FIFTEEN))
    for w in (1, 1.0, np.float32(1.0), np.int64(1)):
        assert reference.parse(dict(latent=Z, adain=w)).adain == frozenset(SEVEN)
    assert reference.parse(dict(latent=Z, adain=0.5)).adain == frozenset({"mid_block.resnets.1", "up_blocks.0.resnets.0", "up_blocks.0.resnets.1",
                                                                           "down_blocks.3.resnets.1"})
    assert reference.parse(dict(latent=Z, adain="mid_block.resnets.1")).adain == frozenset({"mid_block.resnets.1"})
    two = reference.parse(dict(latent=Z, adain=(n for n in FIFTEEN[:2]), layers="mid"))
    assert two.adain == frozenset(FIFTEEN[:2]) and two.layers == frozenset({"mid_block.attentions.0"})
    # AdaIN without the attention part
    for none in ([], None, ()):
        alone = reference.parse(dict(latent=Z, adain="auto", layers=none))
        assert alone.layers == frozenset() and alone.adain == frozenset(SEVEN) and alone.key == (("adain",) + tuple(sorted(SEVEN)),)
    assert reference.parse(reference.ReferenceSpec(latent=Z, adain="all")).key == every.key
    assert "adain" in reference.FIELDS


@pytest.mark.parametrize("bad, match", [
    (dict(latent=Z, adain=0.0), "adain"), (dict(latent=Z, adain=-1.0), "adain"), (dict(latent=Z, adain=2.5), "adain"),
    (dict(latent=Z, adain=float("nan")), "adain"), (dict(latent=Z, adain=float("inf")), "adain"), (dict(latent=Z, adain=True), "adain"),
    (dict(latent=Z, adain="mid"), "adain.*unknown site"), (dict(latent=Z, adain="down_blocks.0.attentions.0"), "adain.*unknown site"),
    (dict(latent=Z, adain=["mid_block.resnets.1", "up_blocks.0.resnets.2"]), "adain.*unknown site"),
    (dict(latent=Z, adain=["all"]), "adain.*unknown site"), (dict(latent=Z, adain=[1.0]), "adain.*unknown site"),
    (dict(latent=Z, adain=[]), "adain selects no site"), (dict(latent=Z, adain=()), "adain selects no site"),
    (dict(latent=Z, adain=object()), "adain"),
    (dict(latent=Z, layers=[]), "no layer"), (dict(latent=Z, layers=None), "no layer"), (dict(latent=Z, layers=[], adain=None), "no layer"),
    (dict(latent=Z, adain="auto", layers="middle"), "unknown layer"), (dict(latent=Z, adan="auto"), "unknown field"),
])
def test_parse_rejects(bad, match):
    from minsdtf_amd import reference

    with pytest.raises(ValueError, match=match):
        reference.parse(bad)
    for w in (0.0, 2.0000001, float("nan"), "much", None):
        with pytest.raises(ValueError, match="adain"):
            reference.adain_sites(w)


def test_engine_key_holds_the_sites_and_never_the_image_the_draw_or_the_fidelity():
    from minsdtf_amd import reference
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    class Net:
        weights_version = 1

    sd = StableDiffusionBase(64, 64)
    sd.diffusion_model = Net()
    args = (1, 77, 77, 4, 7.5, 0.0, False)
    plain = sd._engine_key(*args)

    def key(spec):
        r = reference.parse(spec)
        return sd._engine_key(*args, reference=tuple(sorted(r.layers)), adain=r.adain_key)

    off = key(dict(latent=Z, layers="mid", fidelity=0.25))
    assert off == sd._engine_key(*args, reference=("mid_block.attentions.0",)) and off[-1] == ("reference", ("mid_block.attentions.0",))
    assert sd._engine_key(*args, reference=None, adain=None) == plain
    a = key(dict(latent=Z, layers="mid", fidelity=0.25, adain="auto"))
    b = key(dict(latent=Z + 3, layers="mid", fidelity=1.0, noise=Z + 1, adain=1.0))
    assert a == b and a != off and a != plain and a[:len(plain)] == plain
    assert a[-1] == ("reference", ("mid_block.attentions.0",), ("adain",) + tuple(sorted(SEVEN)))
    assert not any(isinstance(v, float) and v in (0.25, 1.0) for v in a[-1]) and not any(isinstance(v, np.ndarray) for v in a)
    every = key(dict(latent=Z, layers="mid", adain="all"))
    alone = key(dict(latent=Z, layers=[], adain="auto"))
    assert len({a, every, alone, off, plain}) == 5 and alone[-1] == ("reference", (), ("adain",) + tuple(sorted(SEVEN)))


# ------------------------------------------------------------------------------------------------- the float64 reference
def test_float64_reference_against_torch_var_mean():
    import torch

    from minsdtf_amd import reference

    rng = np.random.default_rng(3)
    rows, hw, C = 3, 37, 16
    x = rng.standard_normal((rows, hw, C)) * rng.uniform(0.5, 3.0, (rows, 1, C)) + rng.standard_normal((rows, 1, C)) * 4
    ref = rng.standard_normal((hw, C)) * 2.0 - 5.0
    mix = np.array([0.0, 0.5, 1.0])
    got = reference.adain_reference(x, ref, mix)
    assert got.dtype == np.float64 and got.shape == x.shape
    xt, rt = torch.from_numpy(x), torch.from_numpy(ref)[None]
    var, mean = torch.var_mean(xt, dim=1, keepdim=True, correction=0)
    var_acc, mean_acc = torch.var_mean(rt, dim=1, keepdim=True, correction=0)
    std, std_acc = torch.sqrt(var.clamp_min(0) + 1e-6), torch.sqrt(var_acc.clamp_min(0) + 1e-6)
    y = (((xt - mean) / std) * std_acc + mean_acc).numpy()   # diffusers' form
    for b, f in enumerate(mix):
        np.testing.assert_allclose(got[b], f * x[b] + (1 - f) * y[b], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(got[2], x[2])
    # fidelity 0: the row takes the reference's statistics
    np.testing.assert_allclose(got[0].mean(0), ref.mean(0), rtol=0, atol=1e-12)
    np.testing.assert_allclose(got[0].var(0), ref.var(0), rtol=1e-5)
    np.testing.assert_array_equal(reference.adain_reference(x, ref, None), reference.adain_reference(x, ref, np.zeros(rows)))
    nan = x.copy()
    nan[2] = np.nan
    out = reference.adain_reference(nan, ref, mix)
    assert np.isfinite(out[:2]).all() and np.isnan(out[2]).all()
    np.testing.assert_allclose(reference.adain_reference(ref[None], ref, [0.3])[0], ref, rtol=0, atol=1e-12)
    assert "var_mean" in reference.adain_reference.__doc__ and "style_fidelity" in reference.adain_reference.__doc__


# ------------------------------------------------------------------------------------------------------------------ the C ABI
FIELDS = ("x", "ref", "mix", "rows", "hw", "c", "eps")


def test_library_exports_the_new_entry_point():
    import re

    from minsdtf_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    assert "msd_reference_adain" in _lib.SYMBOLS and _lib.ABI_VERSION == 12
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "minsdtf_hip.h")).read()
    assert "#define MSD_ABI_VERSION 12" in header
    assert "msd_reference_adain" in exported and "MSD_API int msd_reference_adain(" in header
    assert len(re.findall(r"^MSD_API ", header, flags=re.M)) == 31 == len(_lib.SYMBOLS)
    assert _lib.load().msd_abi_version() == 12


def test_struct_layout_matches_header():
    from minsdtf_amd import _lib

    src = '#include <stdio.h>\n#include <stddef.h>\n#include "minsdtf_hip.h"\nint main(){printf("%zu' + " %zu" * len(FIELDS) + \
          '\\n", sizeof(MsdReferenceAdain)' + "".join(f", offsetof(MsdReferenceAdain, {f})" for f in FIELDS) + ");return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    t = _lib.MsdReferenceAdain
    assert [f for f, _t in t._fields_] == list(FIELDS)
    assert sizes == [ctypes.sizeof(t)] + [getattr(t, f).offset for f in FIELDS]


def _adain(**kw):
    from minsdtf_amd import _lib

    s = _lib.MsdReferenceAdain()
    # rows 2, hw 70, c 24: x is 2 * 70 * 24 * 2 = 6720 bytes, ref 3360 directly behind it (the engine's layout)
    good = dict(x=1 << 20, ref=(1 << 20) + 6720, mix=2 << 20, rows=2, hw=70, c=24, eps=1e-6)
    for k, v in {**good, **kw}.items():
        setattr(s, k, v)
    return s


@pytest.mark.parametrize("bad, word", [
    (dict(x=None), b"null"), (dict(ref=None), b"null"),
    (dict(x=(1 << 20) + 8, ref=3 << 20), b"aligned"), (dict(ref=(3 << 20) + 2), b"aligned"), (dict(mix=(2 << 20) + 4), b"aligned"),
    (dict(rows=0), b"rows"), (dict(rows=-1), b"rows"), (dict(rows=65536, ref=1 << 30), b"rows"), (dict(hw=0), b"hw"), (dict(hw=-5), b"hw"),
    (dict(c=0), b"c = 0"), (dict(c=20), b"c = 20"), (dict(c=-8), b"c = -8"),
    (dict(eps=0.0), b"eps"), (dict(eps=-1e-6), b"eps"), (dict(eps=float("nan")), b"eps"), (dict(eps=float("inf")), b"eps"),
    (dict(hw=1 << 20, c=2048, ref=1 << 40), b"2^31"),
    (dict(ref=1 << 20), b"overlaps"), (dict(ref=(1 << 20) + 3360), b"overlaps"), (dict(ref=(1 << 20) + 6720 - 16), b"overlaps"),
    (dict(ref=(1 << 20) - 3360 + 16), b"overlaps"), (dict(mix=(1 << 20) + 16), b"overlaps"),
])
def test_argument_errors_need_no_device(bad, word):
    """Every bad call returns MSD_E_ARG (-1) with a message before anything is launched (the pointers are never followed)."""
    from minsdtf_amd import _lib

    lib = _lib.load()
    assert lib.msd_reference_adain(None, None) == -1 and b"null" in lib.msd_last_error()
    assert lib.msd_reference_adain(ctypes.byref(_adain(**bad)), None) == -1, bad
    assert word in lib.msd_last_error(), (bad, lib.msd_last_error())


# ------------------------------------------------------------------------------------------------------------- the recorded plan
def _record(nb, hw, **kw):
    """emit_unet at nb rows and hw x hw latents on the CPU -> (LW.Rec list, the plan, (ref_latent, mix) buffers)."""
    from minsdtf_amd import engine

    recs, orig = [], engine.Plan.rec

    def rec(self, fn, **k):
        ops_ = {n: o for n, o in ((n, LW._operand(v)) for n, v in k.items() if n != "split") if o is not None}
        recs.append(LW.Rec(fn.__name__, k.get("name", ""), k, ops_))
        return orig(self, fn, **k)

    engine.Plan.rec = rec
    try:
        p = engine.Plan("cpu")
        e = engine.Emitter(p, LW._AnyWeights())
        ctx = engine.Act(p.alloc(nb * 77 * 768 * 2), nb, 77, 1, 768)
        kv = engine.emit_context_kv(e, ctx, engine.UNET_ATTN_LAYERS, p)
        recs.clear()
        mix, ref_latent = p.alloc((nb - 1) * 4), p.alloc(hw * hw * 4 * 4)
        if "reference" in kw:
            kw["reference"] = (kw["reference"], ref_latent, mix)
        engine.emit_unet(e, LW._Tensor(), 2, nb, hw, hw, (LW._Tensor(), 0, 0, engine.temb_columns(False)), kv, 77, LW._Tensor(),
                         kw.pop("controls", None), variant=engine.UNetVariant(**kw))
    finally:
        engine.Plan.rec = orig
    return recs


def _sig(recs):
    return [(r.op, r.name, r.kw.get("batch"), tuple(sorted((n, o.kind, o.offset) for n, o in r.operands.items()))) for r in recs]


def test_no_adain_records_the_reference_only_plan():
    from minsdtf_amd import engine

    layers = frozenset(engine.PAG_LAYERS)
    base = _sig(_record(5, 24, reference=layers))
    assert _sig(_record(5, 24, reference=layers, adain=None)) == base
    assert _sig(_record(5, 24, reference=layers, adain=frozenset())) == base
    assert not any(op == "reference_adain" for op, *_ in base)
    # the sites add their records and change no other
    every = _sig(_record(5, 24, reference=layers, adain=frozenset(FIFTEEN)))
    assert [s[:3] for s in every if s[0] != "reference_adain"] == [s[:3] for s in base]


def test_fifteen_sites_in_the_recorded_plan():
    """5 rows at 24 x 24 (hw 144, 36, 9): each msd_reference_adain directly behind the record that writes its site, before any
    record that reads it, on 4 rows with ref at the last row of the same buffer; the upsampler sites sit on the conv's output."""
    recs = _record(5, 24, reference=frozenset(), adain=frozenset(FIFTEEN))
    at = [i for i, r in enumerate(recs) if r.op == "reference_adain"]
    assert [recs[i].name for i in at] == [n + ".adain" for n in FIFTEEN]
    shapes = {"down_blocks.1": (144, 640), "down_blocks.2": (36, 1280), "down_blocks.3": (9, 1280), "mid_block": (9, 1280),
              "up_blocks.0.resnets": (9, 1280), "up_blocks.0.upsamplers": (36, 1280), "up_blocks.1.attentions": (36, 1280),
              "up_blocks.1.upsamplers": (144, 1280), "up_blocks.2": (144, 640)}
    for i in at:
        r = recs[i]
        site = r.name[:-len(".adain")]
        hw, c = next(v for k, v in shapes.items() if site.startswith(k))
        assert (r.kw["rows"], r.kw["hw"], r.kw["c"], r.kw["eps"]) == (4, hw, c, 1e-6), r.name
        x, ref, mix = r.operands["x"], r.operands["ref"], r.operands["mix"]
        assert ref.offset == x.offset + 4 * hw * c * 2 and ref.avail == x.avail - 4 * hw * c * 2, r.name
        assert mix.kind == "buf" and not x.freed
        # the record in front of it wrote this very buffer, and is the site's own call
        prod = recs[i - 1]
        assert prod.name.startswith(site), (r.name, prod.name)
        assert prod.operands["out"].offset == x.offset, (r.name, prod.name)
        if "upsamplers" in site:
            assert prod.name == site and prod.kw.get("upsample")
        # (directly behind the site's last writer: whatever reads the site's value comes after the AdaIN record)
        assert not any(o.kind == "buf" and o.offset == x.offset and n == "out" for k in range(i + 1, min(i + 4, len(recs)))
                       for n, o in recs[k].operands.items()), f"{r.name}: the site is written again behind its AdaIN"
        # and the site IS read afterwards (the onward path)
        assert any(o.kind == "buf" and o.offset == x.offset and n != "out" for n, o in recs[i + 1].operands.items()), (r.name, recs[i + 1].name)
    # "auto": the seven sites, all at C = 1280
    seven = [r for r in _record(5, 24, reference=frozenset({"mid_block.attentions.0"}), adain=frozenset(SEVEN)) if r.op == "reference_adain"]
    assert [r.name for r in seven] == [n + ".adain" for n in FIFTEEN if n in SEVEN] and all(r.kw["c"] == 1280 for r in seven)


def test_every_new_launch_fits_its_buffers():
    """tests/test_plan_extents_cpu.py's Fits / Live / Disjoint over the fifteen records: x and ref inside their buffer and live,
    ref and mix apart from the rows that are rewritten."""
    from minsdtf_amd import engine

    recs = _record(5, 24, reference=frozenset(engine.PAG_LAYERS), adain=frozenset(FIFTEEN))
    checked = 0
    for r in recs:
        if r.op != "reference_adain":
            continue
        dims = {k: (v if v is None or isinstance(v, (int, float, str)) else True) for k, v in r.kw.items() if k != "name"}
        ext = XA.reference_adain(**dims)
        seen = []
        assert {"x", "ref", "mix"} <= set(r.operands)
        for name, o in r.operands.items():
            assert name in ext, f"{r.name}: operand '{name}' has no extent"
            if o.kind != "buf":
                continue
            need, role = ext[name]
            assert need <= o.avail, f"{r.name}: operand '{name}' needs {need} bytes, its buffer has {o.avail} from the operand's address"
            assert not o.freed, f"{r.name}: operand '{name}' lies in a freed buffer"
            seen.append((name, role, o.offset, o.offset + need))
        for i, (na, ra, lo_a, hi_a) in enumerate(seen):   # the rewritten rows apart from every input
            for nb_, rb, lo_b, hi_b in seen[i + 1:]:
                if "inout" in (ra, rb):
                    assert not (lo_a < hi_b and lo_b < hi_a), f"{r.name}: '{na}' and '{nb_}' share bytes"
        checked += 1
    assert checked == 15


def test_emit_unet_refusals():
    from minsdtf_amd import engine

    sites = frozenset(SEVEN)
    mid = frozenset({"mid_block.attentions.0"})
    with pytest.raises(ValueError, match="adain goes with a reference row"):
        _record(4, 16, adain=sites)
    with pytest.raises(ValueError, match="reference"):
        _record(5, 16, reference=mid, adain=sites, pag_layers=mid, perturbed=1)
    with pytest.raises(ValueError, match="reference"):
        _record(5, 16, reference=mid, adain=sites, region_attn=(2, 2, {}))
    with pytest.raises(ValueError, match="window|adain"):
        _record(5, 16, reference=mid, adain=sites, window=(2, 2))
    with pytest.raises(ValueError, match="reference"):
        _record(5, 16, reference=mid, adain=sites, controls=[LW._Tensor()] * 13)
    with pytest.raises(ValueError, match="unknown adain site"):
        _record(5, 16, reference=mid, adain=frozenset({"mid_block.resnets.0"}))
    with pytest.raises(ValueError, match="unknown adain site"):
        _record(5, 16, reference=mid, adain=frozenset({"up_blocks.1.attentions.2"}))
    # layers may be empty with adain; the 3-tuple with an empty set and no adain still raises
    assert sum(r.op == "reference_adain" for r in _record(5, 16, reference=frozenset(), adain=sites)) == 7
    with pytest.raises(ValueError, match="reference layers"):
        _record(5, 16, reference=frozenset())
    with pytest.raises(ValueError, match="reference layers"):
        _record(5, 16, reference=frozenset(), adain=None)
    assert engine.PAG_LAYERS   # (the names the refusals speak of)


def test_generate_image_refusals_and_the_cap_come_before_any_device_work():
    from minsdtf_amd import regions, tiled
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    ctx = np.zeros((77, 768), dtype=np.float32)
    img = np.zeros((64, 64, 3), dtype=np.uint8)
    sd = StableDiffusionBase(64, 64)   # (no models behind it: anything that reaches a model fails another way)
    for spec in (dict(latent=Z, adain="auto"), dict(latent=Z, adain="all", layers=[])):
        kw = dict(batch_size=1, num_steps=3, seed=0, reference_only=spec)
        halves = dict(regions=[dict(prompt=ctx, mask=m) for m in regions.boxes(8, 8, 1, 2)])
        for extra, names in ((dict(tiled=dict(size=(64, 128))), ["tiled"]), (dict(hires=dict(scale=2)), ["hires"]),
                             (dict(regions=halves), ["regions"]), (dict(pag=dict(scale=3.0)), ["pag"]),
                             (dict(control_net_image=img.astype(np.float32)), ["control_net_image"]),
                             (dict(reference_image=img), ["reference_image"]), (dict(inpaint_mask=img[..., 0]), ["inpaint_mask"])):
            with pytest.raises(ValueError, match="reference_only is") as e:
                sd.generate_image(ctx, **kw, **extra)
            assert all(n in str(e.value) for n in names), str(e.value)
        two = StableDiffusionBase(64, 64)
        two.denoise_streams = 2
        with pytest.raises(ValueError, match="reference_only.*denoise_streams"):
            two.generate_image(ctx, **kw)
        tcd = StableDiffusionBase(64, 64, active_tcd=True)
        with pytest.raises(ValueError, match="reference_only.*TCD"):
            tcd.generate_image(ctx, **kw)
        assert 2 * tiled.MAX_VIEW_BATCH == 12
        with pytest.raises(ValueError, match=r"13 UNet rows.*MAX_VIEW_BATCH = 12"):
            sd.generate_image(ctx, **{**kw, "batch_size": 6})
        sd.unconditional_context = np.zeros((77, 768), dtype=np.float32)
        with pytest.raises(ValueError, match="token length"):
            sd.generate_image(np.zeros((154, 768), dtype=np.float32), **kw)
    for bad, match in ((dict(latent=Z, adain=3.0), "adain"), (dict(latent=Z, adain="top"), "unknown site"), (dict(latent=Z, adain=[]), "no site")):
        with pytest.raises(ValueError, match=match):
            sd.generate_image(ctx, batch_size=1, num_steps=3, reference_only=bad)
        with pytest.raises(ValueError, match=match):
            sd.text_to_image(ctx, batch_size=1, num_steps=3, reference_only=bad)
    assert not sd._engines


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("tag, size, adain, sites, layers, fidelity, sampler, batch, rescale", [
    ("a", 128, "auto", SEVEN, None, 0.5, "", 1, 0.0),
    ("b", 64, "all", FIFTEEN, (), 1.0, "dpmpp_2m", 2, 0.7),
])
def test_fixture_files(tag, size, adain, sites, layers, fidelity, sampler, batch, rescale):
    """tools/make_reference_adain_fixtures.py's two files: the recorded inputs are the issue's, and both the plain job and the job
    with adain off lie below 30 dB of the AdaIN latent, so the 40 dB bar of tests/test_reference_adain_gpu.py tells them apart."""
    from minsdtf_amd import engine, reference

    layers = tuple(engine.PAG_LAYERS) if layers is None else layers
    path = os.path.join(GOLD, f"oracle_reference_adain_{tag}.npz")
    assert os.path.exists(path) and os.path.getsize(path) < (1 << 20)
    g = np.load(path)
    assert float(g["plain_psnr"]) < 30.0 and float(g["attn_only_psnr"]) < 30.0
    if not layers:
        assert float(g["attn_only_psnr"]) == float(g["plain_psnr"])
    assert (int(g["weight_seed"]), float(g["bias_scale"]), int(g["context_seed"]), int(g["noise_seed"])) == (0, 0.05, 1234, 0)
    assert (float(g["guidance"]), int(g["steps"]), float(g["guidance_rescale"])) == (7.5, 4, rescale)
    assert (int(g["size"]), str(g["sampler"]), int(g["batch"])) == (size, sampler, batch)
    old = np.load(os.path.join(GOLD, "oracle_reference_only_a.npz"))
    assert (int(g["reference_seed"]), int(g["reference_noise_seed"])) == (int(old["reference_seed"]), int(old["reference_noise_seed"]))
    assert float(g["reference_scale"]) in (1.0, 2.0, 4.0)
    assert tuple(str(n) for n in g["layers"]) == layers and float(g["fidelity"]) == fidelity
    assert str(g["adain"]) == adain and tuple(str(n) for n in g["sites"]) == tuple(n for n in FIFTEEN if n in sites)
    r = reference.parse(dict(latent=np.zeros((1, size // 8, size // 8, 4)), layers=[str(n) for n in g["layers"]], adain=str(g["adain"])))
    assert r.adain == frozenset(sites) and r.layers == frozenset(layers)
    assert g["latent"].shape == (batch, size // 8, size // 8, 4) and g["latent"].dtype == np.float32
    assert np.all(np.isfinite(g["latent"]))
