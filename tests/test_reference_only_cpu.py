"""Reference-only control without a GPU: the job description and every ValueError of minsdtf_amd/reference.py, the rate table, the
float64 statement of the kernel against torch, generate_image's refusals and size cap (raised before any device work), the
library's exports, the struct layouts and the argument checks of msd_attention_joint / msd_reference_latent, the recorded plan and
its operand extents, and the two oracle fixture files."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _extents as X
import _extents_reference_only as XR
import _layer_walk as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
Z = np.zeros((1, 8, 8, 4), dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------------ parse
def test_parse_accepts():
    from minsdtf_amd import engine, reference

    assert reference.parse(None) is None
    d = reference.parse(dict(latent=Z))
    assert d.fidelity == 0.5 and d.layers == frozenset(engine.PAG_LAYERS) and d.key == tuple(sorted(engine.PAG_LAYERS))
    assert d.image is None and d.noise is None and d.latent.shape == (1, 8, 8, 4) and d.latent.dtype == np.float32
    assert reference.parse(d) is d
    assert reference.parse(reference.ReferenceSpec(latent=Z)).key == d.key
    m = reference.parse(dict(latent=Z.astype(np.float64), layers="mid", fidelity=1, noise=Z + 1))
    assert m.key == ("mid_block.attentions.0",) and m.fidelity == 1.0 and m.noise.dtype == np.float32 and m.noise[0, 0, 0, 0] == 1.0
    two = reference.parse(dict(image=np.zeros((64, 64, 3), np.uint8), layers=("up_blocks.1.attentions.2", "mid"), fidelity=np.float32(0)))
    assert two.key == ("mid_block.attentions.0", "up_blocks.1.attentions.2") and two.latent is None and two.image is not None
    assert reference.parse(dict(latent=Z, layers=list(engine.PAG_LAYERS))).key == d.key
    assert tuple(reference.layer_names()) == tuple(engine.PAG_LAYERS)


@pytest.mark.parametrize("bad, match", [
    (dict(latent=Z, layer="mid"), "unknown field"), (dict(latent=Z, strength=1.0), "unknown field"),
    (dict(), "exactly one"), (dict(latent=Z, image=np.zeros((64, 64, 3), np.uint8)), "exactly one"), (dict(fidelity=0.3), "exactly one"),
    (dict(latent=Z, fidelity=float("nan")), "fidelity"), (dict(latent=Z, fidelity=-0.1), "fidelity"), (dict(latent=Z, fidelity=1.5), "fidelity"),
    (dict(latent=Z, fidelity="much"), "fidelity"), (dict(latent=Z, fidelity=None), "fidelity"),
    (dict(latent=Z, layers="middle"), "unknown layer"), (dict(latent=Z, layers=["mid", "up_blocks.0.attentions.0"]), "unknown layer"),
    (dict(latent=Z, layers=[7]), "unknown layer"), (dict(latent=Z, layers=["all"]), "unknown layer"),
    (dict(latent=Z, layers=[]), "no layer"), (dict(latent=Z, layers=None), "no layer"),
    (dict(latent=Z[0]), r"\(1, h, w, 4\)"), (dict(latent=np.zeros((2, 8, 8, 4))), r"\(1, h, w, 4\)"), (dict(latent=np.zeros((1, 8, 8, 3))), r"\(1, h, w, 4\)"),
    (dict(latent=Z + np.float32("nan")), "not finite"),
    (dict(latent=Z, noise=np.zeros((1, 4, 8, 4))), "differ in shape"), (dict(latent=Z, noise=np.zeros((8, 8, 4))), r"\(1, h, w, 4\)"),
    ("mid", "ReferenceSpec"), (0.5, "ReferenceSpec"),
])
def test_parse_rejects(bad, match):
    from minsdtf_amd import reference

    with pytest.raises(ValueError, match=match):
        reference.parse(bad)


def test_noise_draw_follows_the_hires_convention():
    from minsdtf_amd import reference

    a = reference.draw_noise(8, 16, seed=7)
    assert a.shape == (1, 8, 16, 4) and a.dtype == np.float32
    np.testing.assert_array_equal(a, np.random.default_rng([7, 3]).standard_normal((1, 8, 16, 4)).astype(np.float32))
    np.random.seed(5)
    b = reference.draw_noise(8, 16)
    np.random.seed(5)
    np.testing.assert_array_equal(b, np.random.randn(1, 8, 16, 4).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ rates
def test_rate_table_against_the_scheduler_and_a_schedule():
    from minsdtf_amd import reference, samplers
    from minsdtf_amd.scheduler import Scheduler

    s = Scheduler()
    s.set_timesteps(7)
    r = reference.rates(s)
    assert r.dtype == np.float64 and r.shape == (7, 2)
    for i, t in enumerate(s.timesteps):
        assert r[i, 0] == s.signal_rates[t] and r[i, 1] == s.noise_rates[t]
    np.testing.assert_allclose(r[:, 0] ** 2 + r[:, 1] ** 2, 1.0, rtol=0, atol=1e-15)
    assert s.timesteps[0] > s.timesteps[-1] and r[0, 1] > r[-1, 1]
    r2 = reference.rates(s, 3)
    np.testing.assert_array_equal(r2[3:], r[3:])
    np.testing.assert_array_equal(r2[:3], np.tile([1.0, 0.0], (3, 1)))
    for name in ("dpmpp_2m", "euler_a_karras"):
        sched = samplers.schedule(samplers.parse(name), s, 6)
        rs = reference.rates(sched, 1)
        rows = samplers.rows(sched, 1)
        assert rs.shape == (6, 2) and rs.dtype == np.float64
        np.testing.assert_array_equal(rs, rows[:, :2])   # the alpha / sigma the device step itself reads for evaluation i
        np.testing.assert_array_equal(rs[1:, 0], sched.alphas[1:6])
        np.testing.assert_array_equal(rs[1:, 1], (sched.sigmas * sched.alphas)[1:6])


def test_reference_latent_host_is_one_product_and_one_fma():
    from minsdtf_amd import reference

    rng = np.random.default_rng(2)
    z, n = rng.standard_normal((1, 4, 4, 4)).astype(np.float32), rng.standard_normal((1, 4, 4, 4)).astype(np.float32)
    a, b = 0.73, 0.41
    got = reference.reference_latent_host(z, n, (a, b))
    assert got.dtype == np.float32 and got.shape == z.shape
    want = np.float64(np.float32(a)) * z + np.float64(np.float32(b)) * n
    assert np.abs(got - want).max() <= 2 * 2.0 ** -24 * (np.abs(z).max() + np.abs(n).max())
    np.testing.assert_array_equal(reference.reference_latent_host(z, n, (1.0, 0.0)), z)


# ------------------------------------------------------------------------------------------------- the float64 reference
def test_float64_reference_against_torch_softmax_over_concatenated_keys():
    import torch

    from minsdtf_amd import reference

    rng = np.random.default_rng(3)
    B, H, d, S, T, Tr = 3, 2, 8, 5, 7, 4
    C = H * d
    q, k, v = rng.standard_normal((B, S, C)), rng.standard_normal((B, T, C)), rng.standard_normal((B, T, C))
    kr, vr = rng.standard_normal((Tr, C)), rng.standard_normal((Tr, C))
    mix = np.array([0.0, 0.3, 1.0])

    def attend(qb, kb, vb):
        qh, kh, vh = (torch.from_numpy(x).view(-1, H, d).permute(1, 0, 2) for x in (qb, kb, vb))
        p = torch.softmax((qh @ kh.transpose(-1, -2)) * np.log(2.0), -1)   # base-2 scores
        return (p @ vh).permute(1, 0, 2).reshape(-1, C).numpy()

    got = reference.joint_attention_reference(q, k, v, kr, vr, mix, H)
    assert got.dtype == np.float64 and got.shape == (B, S, C)
    for b in range(B):
        plain = attend(q[b], k[b], v[b])
        joint = attend(q[b], np.concatenate([k[b], kr]), np.concatenate([v[b], vr]))
        np.testing.assert_allclose(got[b], mix[b] * plain + (1 - mix[b]) * joint, rtol=0, atol=1e-12)
    none = reference.joint_attention_reference(q, k, v, kr, vr, None, H)
    np.testing.assert_array_equal(none, reference.joint_attention_reference(q, k, v, kr, vr, np.zeros(B), H))
    nan = reference.joint_attention_reference(q, k, v, kr * np.nan, vr * np.nan, [1.0, 1.0, 1.0], H)
    assert np.isfinite(nan).all()
    np.testing.assert_array_equal(nan[2], got[2])
    # duplicated keys leave the softmax average unchanged
    dup = reference.joint_attention_reference(q[:1], k[:1], v[:1], k[0], v[0], None, H)
    np.testing.assert_allclose(dup[0], attend(q[0], k[0], v[0]), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------- generate_image, no device
def test_refused_names_every_excluded_argument():
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    what, arguments, states = StableDiffusionBase._REFUSED["reference_only"]
    assert "text-to-image" in what
    assert set(arguments) == {"regions", "pag", "tiled", "hires", "control_net_image", "reference_image", "inpaint_mask"}
    assert set(states) == {"a TCD pipeline (active_tcd=True)", "denoise_streams = 2"}


def test_refusals_and_the_cap_come_before_any_device_work():
    from minsdtf_amd import regions, tiled
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    ctx = np.zeros((77, 768), dtype=np.float32)
    img = np.zeros((64, 64, 3), dtype=np.uint8)
    sd = StableDiffusionBase(64, 64)   # (no models behind it: anything that reaches a model fails another way)
    kw = dict(batch_size=1, num_steps=3, seed=0, reference_only=dict(latent=Z))
    halves = dict(regions=[dict(prompt=ctx, mask=m) for m in regions.boxes(8, 8, 1, 2)])
    for extra, names in ((dict(tiled=dict(size=(64, 128))), ["tiled"]), (dict(hires=dict(scale=2)), ["hires"]),
                         (dict(regions=halves), ["regions"]), (dict(pag=dict(scale=3.0)), ["pag"]),
                         (dict(control_net_image=img.astype(np.float32)), ["control_net_image"]),
                         (dict(reference_image=img), ["reference_image"]), (dict(inpaint_mask=img[..., 0]), ["inpaint_mask"]),
                         (dict(pag=dict(scale=3.0), inpaint_mask=img[..., 0]), ["pag", "inpaint_mask"])):
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
    with pytest.raises(ValueError, match="reference_only is"):
        sd.text_to_image(ctx, tiled=dict(size=(64, 128)), **kw)
    # the cap: 2 * batch_size + 1 <= 2 * tiled.MAX_VIEW_BATCH UNet rows
    assert 2 * tiled.MAX_VIEW_BATCH == 12
    with pytest.raises(ValueError, match=r"13 UNet rows.*MAX_VIEW_BATCH = 12"):
        sd.generate_image(ctx, **{**kw, "batch_size": 6})
    # a bad description is a ValueError of its own
    with pytest.raises(ValueError, match="unknown field"):
        sd.generate_image(ctx, batch_size=1, num_steps=3, reference_only=dict(latent=Z, fidelty=0.5))
    with pytest.raises(ValueError, match="unknown layer"):
        sd.generate_image(ctx, batch_size=1, num_steps=3, reference_only=dict(latent=Z, layers="top"))
    # a negative prompt of another token length, and a latent of another size than the job's
    sd.unconditional_context = np.zeros((77, 768), dtype=np.float32)
    with pytest.raises(ValueError, match="token length"):
        sd.generate_image(np.zeros((154, 768), dtype=np.float32), **kw)
    with pytest.raises(ValueError, match=r"shape \(1, 4, 4, 4\)"):
        sd.generate_image(ctx, batch_size=1, num_steps=3, seed=0, reference_only=dict(latent=np.zeros((1, 4, 4, 4), np.float32)))
    assert not sd._engines


def test_engine_key_holds_the_layers_and_never_the_image_the_draw_or_the_fidelity():
    from minsdtf_amd import reference
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    class Net:
        weights_version = 1

    sd = StableDiffusionBase(64, 64)
    sd.diffusion_model = Net()
    args = (1, 77, 77, 4, 7.5, 0.0, False)
    plain = sd._engine_key(*args)
    assert sd._engine_key(*args, reference=None) == plain
    a = reference.parse(dict(latent=Z, layers="mid", fidelity=0.25))
    b = reference.parse(dict(latent=Z + 3, layers="mid", fidelity=1.0, noise=Z + 1))
    ka, kb = sd._engine_key(*args, reference=a.key), sd._engine_key(*args, reference=b.key)
    assert ka == kb and ka != plain and ka[:len(plain)] == plain and ka[-1] == ("reference", ("mid_block.attentions.0",))
    assert not any(isinstance(v, float) and v in (0.25, 1.0) for v in ka) and not any(isinstance(v, np.ndarray) for v in ka)
    every = sd._engine_key(*args, reference=reference.parse(dict(latent=Z)).key)
    assert every != ka and len(every[-1][1]) == 16
    assert sd._engine_key(*args, pag=("mid_block.attentions.0",)) != ka


# ------------------------------------------------------------------------------------------------------------------ the C ABI
NEW = ("msd_attention_joint", "msd_reference_latent")


def test_library_exports_the_new_entry_points():
    from minsdtf_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    assert all(n in _lib.SYMBOLS for n in NEW) and _lib.ABI_VERSION == 12
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "minsdtf_hip.h")).read()
    assert "#define MSD_ABI_VERSION 12" in header
    for n in NEW:
        assert n in exported and f"MSD_API int {n}(" in header
    assert _lib.load().msd_abi_version() == 12


JOINT_FIELDS = ("q", "k", "vt", "k_ref", "vt_ref", "mix", "out", "batch", "heads", "head_dim", "s", "t", "t_ref", "q_ld", "k_ld", "vt_ld", "o_ld")
LATENT_FIELDS = ("z", "noise", "coef", "step_ptr", "out", "n", "num_steps")


@pytest.mark.parametrize("struct, fields", [("MsdAttentionJoint", JOINT_FIELDS), ("MsdReferenceLatent", LATENT_FIELDS)])
def test_struct_layout_matches_header(struct, fields):
    from minsdtf_amd import _lib

    src = '#include <stdio.h>\n#include <stddef.h>\n#include "minsdtf_hip.h"\nint main(){printf("%zu' + " %zu" * len(fields) + \
          f'\\n", sizeof({struct})' + "".join(f", offsetof({struct}, {f})" for f in fields) + ");return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    t = getattr(_lib, struct)
    assert [f for f, _t in t._fields_] == list(fields)
    assert sizes == [ctypes.sizeof(t)] + [getattr(t, f).offset for f in fields]


def _joint(**kw):
    from minsdtf_amd import _lib

    s = _lib.MsdAttentionJoint()
    # B = 2, H = 2, d = 40, S = T = 35, T_ref = 20: q 2*35*80*2 = 11200 bytes, vt 2*80*40*2 = 12800, vt_ref 6400
    good = dict(q=1 << 20, k=2 << 20, vt=3 << 20, k_ref=4 << 20, vt_ref=5 << 20, mix=6 << 20, out=7 << 20, batch=2, heads=2, head_dim=40,
                s=35, t=35, t_ref=20, q_ld=80, k_ld=80, vt_ld=40, o_ld=80)
    for k, v in {**good, **kw}.items():
        setattr(s, k, v)
    return s


@pytest.mark.parametrize("bad, word", [
    (dict(q=None), b"null"), (dict(k=None), b"null"), (dict(vt=None), b"null"), (dict(k_ref=None), b"null"), (dict(vt_ref=None), b"null"),
    (dict(out=None), b"null"),
    (dict(q=(1 << 20) + 8), b"aligned"), (dict(k_ref=(4 << 20) + 2), b"aligned"), (dict(vt_ref=(5 << 20) + 4), b"aligned"),
    (dict(out=(7 << 20) + 8), b"aligned"), (dict(mix=(6 << 20) + 4), b"mix"),
    (dict(head_dim=64), b"head_dim"), (dict(head_dim=0), b"head_dim"),
    (dict(s=0), b"s = 0"), (dict(t=0), b"t = 0"), (dict(t_ref=0), b"t_ref = 0"), (dict(t_ref=-3), b"t_ref"),
    (dict(batch=0), b"batch"), (dict(batch=65536), b"batch"), (dict(heads=0), b"heads"), (dict(heads=65536), b"heads"),
    (dict(q_ld=84), b"multiples of 8"), (dict(vt_ld=36), b"multiples of 8"), (dict(q_ld=72), b"smaller"), (dict(k_ld=72), b"smaller"),
    (dict(o_ld=72), b"smaller"), (dict(vt_ld=32), b"vt_ld"), (dict(t_ref=48), b"vt_ld"),
    (dict(batch=65535, heads=65535, s=64, q_ld=2621400, k_ld=2621400, o_ld=2621400), b"2^31"),
    (dict(out=1 << 20), b"overlaps"), (dict(out=(1 << 20) + 11200 - 16), b"overlaps"), (dict(out=(2 << 20) - 16), b"overlaps"),
    (dict(out=(3 << 20) + 12800 - 16), b"overlaps"), (dict(out=(4 << 20) + 16), b"overlaps"), (dict(out=(5 << 20) + 6400 - 16), b"overlaps"),
    (dict(out=6 << 20), b"overlaps"),
])
def test_joint_argument_errors_need_no_device(bad, word):
    """Every bad call returns MSD_E_ARG (-1) with a message before anything is launched (the pointers are never followed)."""
    from minsdtf_amd import _lib

    lib = _lib.load()
    assert lib.msd_attention_joint(None, None) == -1 and b"null" in lib.msd_last_error()
    assert lib.msd_attention_joint(ctypes.byref(_joint(**bad)), None) == -1, bad
    assert word in lib.msd_last_error(), (bad, lib.msd_last_error())


def _latent(**kw):
    from minsdtf_amd import _lib

    s = _lib.MsdReferenceLatent()
    good = dict(z=1 << 20, noise=2 << 20, coef=3 << 20, step_ptr=4 << 20, out=5 << 20, n=1024, num_steps=4)
    for k, v in {**good, **kw}.items():
        setattr(s, k, v)
    return s


@pytest.mark.parametrize("bad, word", [
    (dict(z=None), b"null"), (dict(noise=None), b"null"), (dict(coef=None), b"null"), (dict(out=None), b"null"),
    (dict(z=(1 << 20) + 4), b"aligned"), (dict(noise=(2 << 20) + 8), b"aligned"), (dict(out=(5 << 20) + 4), b"aligned"),
    (dict(n=0), b"n = 0"), (dict(n=1022), b"n = 1022"), (dict(num_steps=0), b"num_steps"),
    (dict(out=1 << 20), b"distinct"), (dict(out=(2 << 20) + 4080), b"distinct"), (dict(noise=(1 << 20) + 4080), b"distinct"),
    (dict(out=(3 << 20) + 16), b"distinct"), (dict(out=(4 << 20) - 4080), b"step_ptr"),
])
def test_reference_latent_argument_errors_need_no_device(bad, word):
    from minsdtf_amd import _lib

    lib = _lib.load()
    assert lib.msd_reference_latent(None, None) == -1 and b"null" in lib.msd_last_error()
    assert lib.msd_reference_latent(ctypes.byref(_latent(**bad)), None) == -1, bad
    assert word in lib.msd_last_error(), (bad, lib.msd_last_error())


# ------------------------------------------------------------------------------------------------------------- the recorded plan
def _walk(latent_mod, nb, **kw):
    """tests/test_pag_cpu.py's walk with the attention calls' q / k / vt / k_ref / vt_ref / out byte offsets and conv_in's out offset."""
    from minsdtf_amd import engine

    out, orig = [], engine.Plan.rec

    def rec(self, fn, **k):
        names = ("q", "k", "vt", "k_ref", "vt_ref", "out") if fn.__name__.startswith("attention") else \
            ("out",) if (k.get("name") or "").startswith("conv_in") else ()
        out.append((fn.__name__, k.get("name"), k.get("batch")) + tuple(getattr(k[n], "off", 0) for n in names if n in k))
        return orig(self, fn, **k)

    engine.Plan.rec = rec
    try:
        p = engine.Plan("cpu")
        e = engine.Emitter(p, LW._AnyWeights())
        ctx = engine.Act(p.alloc(nb * 77 * 768 * 2), nb, 77, 1, 768)
        kv = engine.emit_context_kv(e, ctx, engine.UNET_ATTN_LAYERS, p)
        out.clear()
        engine.emit_unet(e, LW._Tensor(), latent_mod, nb, 16, 16, (LW._Tensor(), 0, 0, engine.temb_columns(False)), kv, 77, LW._Tensor(), None, variant=engine.UNetVariant(**kw))
    finally:
        engine.Plan.rec = orig
    return out


def test_no_reference_records_the_plain_plan():
    import test_pag_cpu

    plain = _walk(2, 4)
    assert _walk(2, 4, reference=None) == plain
    assert [c[:3] for c in plain] == [c[:3] for c in test_pag_cpu._walk(2, 4)]
    assert not any(op in ("attention_joint", "reference_latent") for op, *_ in plain)
    assert sum(name.endswith(".replicate") for _op, name, *_ in plain) == 3


def test_reference_row_in_the_recorded_plan():
    """5 rows at 16 x 16 (u, u, c, c, r), two blocks selected (8 x 8 = 64 tokens at C = 640; 2 x 2 = 4 tokens, V^T padded to 8, at
    C = 1280): ONE msd_attention_joint on 4 rows whose k_ref / vt_ref are row 4 of k / vt, ONE msd_attention on 1 row at the offset
    pointers, a second conv_in at row 4, no replicate; every other call as in a plain 5-row plan with nothing shared."""
    from minsdtf_amd import engine

    layers = frozenset({"down_blocks.1.attentions.1", "mid_block.attentions.0"})
    mix = LW._Tensor()
    got = _walk(2, 5, reference=(layers, LW._Tensor(), mix))
    assert not any((name or "").endswith(".replicate") for _op, name, *_ in got)
    assert got[0] == ("conv_direct", "conv_in", 4, 0) and got[1] == ("conv_direct", "conv_in.reference", 1, 4 * 16 * 16 * 320 * 2)
    tb = ".transformer_blocks.0.attn1"
    joints = [c for c in got if c[0] == "attention_joint"]
    assert [c[1] for c in joints] == ["down_blocks.1.attentions.1" + tb + ".joint", "mid_block.attentions.0" + tb + ".joint"]
    for blk, C, S, sp in (("down_blocks.1.attentions.1", 640, 64, 64), ("mid_block.attentions.0", 1280, 4, 8)):
        i = got.index(("attention_joint", blk + tb + ".joint", 4, 0, 0, 0, 4 * S * C * 2, 4 * C * sp * 2, 0))
        assert got[i + 1] == ("attention", blk + tb, 1, 4 * S * C * 2, 4 * S * C * 2, 4 * C * sp * 2, 4 * S * C * 2)
    # the blocks that are not selected: msd_attention on all 5 rows
    plain_attn1 = [c for c in got if c[0] == "attention" and c[1].endswith(tb) and c[1][:-len(tb)] not in layers]
    assert len(plain_attn1) == 14 and all(c[2:] == (5, 0, 0, 0, 0) for c in plain_attn1)
    # against the 5-row plan that shares nothing (latent_batch_mod 5): the same calls but conv_in and the two selected attn1
    plain = _walk(5, 5)
    rest = [c for c in got if c[0] != "attention_joint" and c[1] != "conv_in.reference"]
    assert len(rest) == len(plain)
    for a, b in zip(plain, rest):
        if a[1] == "conv_in":
            assert b[:3] == ("conv_direct", "conv_in", 4)
        elif a[0] == "attention" and a[1].endswith(tb) and a[1][:-len(tb)] in layers:
            assert b[:3] == (a[0], a[1], 1) and a[2] == 5
        else:
            assert a == b
    # every block
    every = _walk(1, 3, reference=(frozenset(engine.PAG_LAYERS), LW._Tensor(), None))
    assert sum(c[0] == "attention_joint" and c[2] == 2 for c in every) == 16
    assert sum(c[0] == "attention" and c[1].endswith(tb) and c[2] == 1 for c in every) == 16


def test_reference_is_not_combined():
    from minsdtf_amd import engine

    ref = (frozenset({"mid_block.attentions.0"}), LW._Tensor(), None)
    with pytest.raises(ValueError, match="reference"):
        _walk(2, 5, reference=ref, pag_layers=frozenset({"mid_block.attentions.0"}), perturbed=1)
    with pytest.raises(ValueError, match="reference"):
        _walk(2, 5, reference=ref, region_attn=(2, 2, {}))
    with pytest.raises(ValueError, match="reference"):
        _walk(1, 1, reference=ref)
    with pytest.raises(ValueError, match="reference layers"):
        _walk(2, 5, reference=(frozenset({"mid"}), LW._Tensor(), None))
    with pytest.raises(ValueError, match="reference layers"):
        _walk(2, 5, reference=(frozenset(), LW._Tensor(), None))
    p = engine.Plan("cpu")
    e = engine.Emitter(p, LW._AnyWeights())
    kv = {"b.transformer_blocks.0.attn2": (LW._Tensor(), LW._Tensor(), 80)}
    for kw in (dict(shared=2), dict(perturbed=1), dict(regions=2, region_rows=2, region_w=LW._Tensor()), dict(reference=2)):
        with pytest.raises(ValueError, match="reference"):
            e.attentions(p.act(4, 8, 8, 640), "b", kv, 77, shared=kw.pop("shared", 1), variant=engine.AttnVariant(**{"reference": 1, **kw}))


def test_every_new_launch_fits_its_buffers():
    """tests/test_plan_extents_cpu.py's Fits / Live / Disjoint over a reference plan: 5 rows at 24 x 24 (levels 24, 12, 6, 3: the
    3 x 3 level's 9 keys in a V^T row of 16)."""
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
        ctx = engine.Act(p.alloc(5 * 77 * 768 * 2), 5, 77, 1, 768)
        kv = engine.emit_context_kv(e, ctx, engine.UNET_ATTN_LAYERS, p)
        recs.clear()
        mix, ref_latent = p.alloc(4 * 4), p.alloc(24 * 24 * 4 * 4)
        engine.emit_unet(e, LW._Tensor(), 2, 5, 24, 24, (LW._Tensor(), 0, 0, engine.temb_columns(False)), kv, 77, LW._Tensor(), None,
                         variant=engine.UNetVariant(reference=(frozenset(engine.PAG_LAYERS), ref_latent, mix)))
    finally:
        engine.Plan.rec = orig
    checked = 0
    for r in recs:
        new = r.op == "attention_joint" or r.name == "conv_in.reference" or (r.op == "attention" and r.kw["batch"] == 1)
        if not new:
            continue
        dims = {k: (v if v is None or isinstance(v, (int, float, str)) else True) for k, v in r.kw.items() if k != "name"}
        ext = XR.attention_joint(**dims) if r.op == "attention_joint" else X.extents(r.op, **dims)
        seen = []
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
        if r.op == "attention_joint":
            assert {"q", "k", "vt", "k_ref", "vt_ref", "mix", "out"} <= set(r.operands)
            assert r.kw["vt_ld"] >= max(r.kw["t"], r.kw["t_ref"]) and r.kw["vt_ld"] % 8 == 0 and r.kw["batch"] == 4
        checked += 1
    assert checked == 16 + 16 + 1


# ---------------------------------------------------------------------------------------------------------------- fixtures
MID_UP1 = ("mid_block.attentions.0", "up_blocks.1.attentions.0", "up_blocks.1.attentions.1", "up_blocks.1.attentions.2")


@pytest.mark.parametrize("tag, size, layers, fidelity, sampler, batch, rescale", [
    ("a", 128, None, 0.5, "", 1, 0.0),
    ("b", 64, MID_UP1, 1.0, "dpmpp_2m", 2, 0.7),
])
def test_fixture_files(tag, size, layers, fidelity, sampler, batch, rescale):
    """tools/make_reference_only_fixtures.py's two files: the recorded inputs are the issue's, and the plain job lies below 30 dB
    of the reference-only latent, so the 40 dB bar of tests/test_reference_only_gpu.py tells the two jobs apart."""
    from minsdtf_amd import engine, reference

    layers = tuple(engine.PAG_LAYERS) if layers is None else layers
    path = os.path.join(GOLD, f"oracle_reference_only_{tag}.npz")
    assert os.path.exists(path) and os.path.getsize(path) < (1 << 20)
    g = np.load(path)
    assert float(g["plain_psnr"]) < 30.0
    assert (int(g["weight_seed"]), float(g["bias_scale"]), int(g["context_seed"]), int(g["noise_seed"])) == (0, 0.05, 1234, 0)
    assert (float(g["guidance"]), int(g["steps"]), float(g["guidance_rescale"])) == (7.5, 4, rescale)
    assert (int(g["size"]), str(g["sampler"]), int(g["batch"])) == (size, sampler, batch)
    assert int(g["reference_seed"]) == 77 and float(g["reference_scale"]) >= 1.0 and int(g["reference_noise_seed"]) >= 0
    assert tuple(str(n) for n in g["layers"]) == layers and float(g["fidelity"]) == fidelity
    assert reference.parse(dict(latent=np.zeros((1, size // 8, size // 8, 4)), layers=[str(n) for n in g["layers"]])).layers == frozenset(layers)
    assert g["latent"].shape == (batch, size // 8, size // 8, 4) and g["latent"].dtype == np.float32
    assert np.all(np.isfinite(g["latent"]))
