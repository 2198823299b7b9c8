"""Dynamic thresholding, everything that needs no GPU: the job description, the scale schedules, the rank of the order statistic,
the float64 host statement against a torch.quantile restatement written here, the degenerate plane, the library's C ABI (symbols,
struct layout, argument checks through the library), generate_image's refusals and engine key, and the recorded tail of a step on
tensor-less stand-ins with the operand extents of the new launch."""
import ctypes
import math
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

import _extents as X
import _extents_dynthresh as XD
import _layer_walk as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ parse
def test_parse_accepts():
    from minsdtf_amd import dynthresh as D

    assert D.parse(None) is None
    d = D.parse({})
    assert d == D.Resolved(7.0, 1.0, "constant", "constant", 0.0, 0.0, 1.0, "ad", "mean", 1.0)
    assert D.parse(True) == d and D.parse(D.DynThreshSpec()) == d and D.parse(d) is d
    r = D.parse(dict(mimic_scale=5, percentile=0, mimic_mode="cosine_up", cfg_mode="power_down", mimic_scale_min=1, cfg_scale_min=2,
                     sched_val=3, measure="std", startpoint="zero", phi=0))
    assert r == D.Resolved(5.0, 0.0, "cosine_up", "power_down", 1.0, 2.0, 3.0, "std", "zero", 0.0) and isinstance(r.mimic_scale, float)
    for mode in D.MODES:
        assert D.parse(dict(cfg_mode=mode, mimic_mode=mode)).cfg_mode == mode
    assert len(D.MODES) == 9


@pytest.mark.parametrize("bad, match", [
    (dict(mimic_scale=0.0), "mimic_scale"), (dict(mimic_scale=-1.0), "mimic_scale"), (dict(mimic_scale=float("nan")), "mimic_scale"),
    (dict(mimic_scale="low"), "mimic_scale"), (dict(mimic_scale=True), "mimic_scale"), (dict(percentile=1.5), "percentile"),
    (dict(percentile=-0.1), "percentile"), (dict(percentile=99.0), "percentile"), (dict(percentile=None), "percentile"),
    (dict(mimic_mode="sine"), "mimic_mode"), (dict(mimic_mode=1), "mimic_mode"), (dict(cfg_mode="Constant"), "cfg_mode"),
    (dict(mimic_scale_min=-1.0), "mimic_scale_min"), (dict(mimic_scale_min=float("inf")), "mimic_scale_min"),
    (dict(cfg_scale_min=-0.5), "cfg_scale_min"), (dict(cfg_scale_min="x"), "cfg_scale_min"), (dict(sched_val=0.0), "sched_val"),
    (dict(sched_val=float("nan")), "sched_val"), (dict(measure="var"), "measure"), (dict(measure=None), "measure"),
    (dict(startpoint="median"), "startpoint"), (dict(phi=1.01), "phi"), (dict(phi=-0.01), "phi"), (dict(phi=False), "phi"),
    (dict(mimic=7.0), "unknown field"), ("ad", "DynThreshSpec"), (7.0, "DynThreshSpec"), (False, "DynThreshSpec")])
def test_parse_rejects(bad, match):
    from minsdtf_amd import dynthresh as D

    with pytest.raises(ValueError, match=match) as e:
        D.parse(bad)
    assert str(e.value).startswith("dynamic_threshold")


# ----------------------------------------------------------------------------------------------------------------- scales
def test_scales_end_points_of_every_mode():
    from minsdtf_amd import dynthresh as D

    g, m, gmin, mmin, sv, N = 14.0, 6.0, 2.0, 1.0, 2.0, 5
    first = dict(constant=1.0, linear_down=1.0, linear_up=0.0, cosine_down=1.0, cosine_up=0.0, half_cosine_down=1.0, half_cosine_up=0.0,
                 power_up=0.0, power_down=1.0)
    last = dict(constant=1.0, linear_down=0.0, linear_up=1.0, cosine_down=math.cos(1.5707), cosine_up=1.0 - math.cos(1.5707),
                half_cosine_down=math.cos(1.0), half_cosine_up=1.0 - math.cos(1.0), power_up=1.0, power_down=0.0)
    mid = dict(constant=1.0, linear_down=0.5, linear_up=0.5, cosine_down=math.cos(1.5707 * 0.5), cosine_up=1.0 - math.cos(1.5707 * 0.5),
               half_cosine_down=math.cos(0.5), half_cosine_up=1.0 - math.cos(0.5), power_up=0.25, power_down=0.75)
    assert set(first) == set(D.MODES)
    for mode in D.MODES:
        t = D.scales(dict(mimic_scale=m, cfg_mode=mode, mimic_mode=mode, cfg_scale_min=gmin, mimic_scale_min=mmin, sched_val=sv), g, N)
        assert t.dtype == np.float64 and t.shape == (N, 2)
        for row, f in ((0, first), (2, mid), (N - 1, last)):
            assert t[row, 0] == pytest.approx(gmin + (g - gmin) * f[mode], abs=1e-14), (mode, row)
            assert t[row, 1] == pytest.approx(mmin + (m - mmin) * f[mode], abs=1e-14), (mode, row)
    # the extension's own constant: cosine_down does not quite reach the minimum
    assert D.HALF_PI == 1.5707 and D.scales(dict(cfg_mode="cosine_down"), 10.0, 3)[2, 0] == 10.0 * math.cos(1.5707) > 0.0
    # the two modes are independent
    t = D.scales(dict(cfg_mode="linear_down", mimic_mode="constant"), 12.0, 4)
    np.testing.assert_allclose(t[:, 0], [12.0, 8.0, 4.0, 0.0], rtol=0, atol=1e-14)
    np.testing.assert_array_equal(t[:, 1], 7.0)


def test_scales_of_one_step_and_bad_counts():
    from minsdtf_amd import dynthresh as D

    for mode in D.MODES:   # frac = 0: the first end point
        t = D.scales(dict(cfg_mode=mode, mimic_mode=mode), 12.0, 1)
        up = mode.endswith("_up")
        assert t.shape == (1, 2) and t[0, 0] == (0.0 if up else 12.0) and t[0, 1] == (0.0 if up else 7.0)
    with pytest.raises(ValueError, match="steps"):
        D.scales(True, 12.0, 0)


# ------------------------------------------------------------------------------------------------------------------- rank
@pytest.mark.parametrize("P", [2, 9, 64, 1023, 1024, 4096])
def test_rank(P):
    from minsdtf_amd import dynthresh as D

    assert D.rank(0.0, P) == (0, np.float32(0.0))
    assert D.rank(1.0, P) == (P - 1, np.float32(0.0))
    lo, frac = D.rank(0.5, P)
    assert isinstance(frac, np.float32)
    assert (lo, frac) == ((P - 1) // 2, np.float32(0.0 if P % 2 else 0.5))
    lo, frac = D.rank(0.95, P)
    pos = 0.95 * (P - 1)
    assert lo == math.floor(pos) and frac == np.float32(pos - lo) and 0 <= lo <= P - 1
    p = D.params(dict(percentile=0.95, measure="std", startpoint="zero", phi=0.25), P)
    assert p.dtype == np.int32 and p.nbytes == D.PARAM_BYTES == 32
    assert (p[0], p[1], p[2]) == (lo, 1, 1) and not p[5:].any()
    np.testing.assert_array_equal(p[3:5].view(np.float32), np.asarray([frac, 0.25], dtype=np.float32))
    q = D.params(True, P)
    assert (q[0], q[1], q[2]) == (P - 1, 0, 0) and q[3:5].view(np.float32).tolist() == [0.0, 1.0]
    with pytest.raises(ValueError):
        D.rank(1.5, P)
    with pytest.raises(ValueError):
        D.rank(0.5, 0)


# --------------------------------------------------------------------------------------------------------- dynthresh_host
def _dynthresh_torch(u, c, g, m, percentile, measure, startpoint, phi):
    """The extension's dynthresh() with sep_feat_channels = True, restated with torch in float64 on NHWC arrays: flatten(2) per
    (sample, channel), torch.quantile, the clamp, the blend.  Nothing of the product is used."""
    import torch

    u, c = (torch.from_numpy(np.asarray(a, dtype=np.float64)).permute(0, 3, 1, 2) for a in (u, c))
    d = c - u
    cfg, mim = u + g * d, u + m * d
    cfg_flat, mim_flat = cfg.flatten(2), mim.flatten(2)
    cfg_means, mim_means = cfg_flat.mean(dim=2, keepdim=True), mim_flat.mean(dim=2, keepdim=True)
    cfg_c, mim_c = cfg_flat - cfg_means, mim_flat - mim_means
    if measure == "ad":
        mim_ref = mim_c.abs().max(dim=2, keepdim=True).values
        cfg_ref = torch.quantile(cfg_c.abs(), percentile, dim=2, keepdim=True)
    else:
        mim_ref, cfg_ref = mim_c.std(dim=2, keepdim=True), cfg_c.std(dim=2, keepdim=True)
    if startpoint == "zero":
        r = cfg_flat * (mim_ref / cfg_ref)
    elif measure == "ad":
        mx = torch.maximum(mim_ref, cfg_ref)
        r = torch.minimum(torch.maximum(cfg_c, -mx), mx) / mx * mim_ref + cfg_means
    else:
        r = cfg_c / cfg_ref * mim_ref + cfg_means
    out = phi * r + (1.0 - phi) * cfg_flat
    return out.reshape(cfg.shape).permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("hw", [(2, 1), (3, 3), (8, 8), (13, 7), (32, 32)])
@pytest.mark.parametrize("measure, startpoint", [("ad", "mean"), ("ad", "zero"), ("std", "mean"), ("std", "zero")])
def test_host_statement_against_torch_quantile(hw, measure, startpoint):
    """float64 against float64 on identical inputs: 1e-12 of the largest |cfg|."""
    from minsdtf_amd import dynthresh as D

    h, w = hw
    rng = np.random.default_rng(100 * h + w)
    u = rng.standard_normal((2, h, w, 4)).astype(np.float32)
    c = (u + 0.3 * rng.standard_normal((2, h, w, 4))).astype(np.float32)
    c[0, 0, 0] = c[0, -1, -1]   # (a tie)
    for q in (0.0, 0.5, 0.95, 0.999, 1.0):
        for phi in (1.0, 0.4):
            got = D.dynthresh_host(u, c, 14.0, 6.5, dict(percentile=q, measure=measure, startpoint=startpoint, phi=phi))
            want = _dynthresh_torch(u, c, 14.0, 6.5, q, measure, startpoint, phi)
            assert got.dtype == np.float64 and got.shape == u.shape
            S = np.abs(u.astype(np.float64) + 14.0 * (c.astype(np.float64) - u)).max()
            assert np.abs(got - want).max() <= 1e-12 * S, (q, phi)
    # it thresholds: with the maximum as the reference a plane's spread is the mimic prediction's
    got = D.dynthresh_host(u, c, 14.0, 6.5, dict(measure="ad"))
    cfg = u.astype(np.float64) + 14.0 * (c.astype(np.float64) - u)
    mim = u.astype(np.float64) + 6.5 * (c.astype(np.float64) - u)
    dev = lambda a: np.abs(a - a.mean(axis=(1, 2), keepdims=True)).max(axis=(1, 2))
    np.testing.assert_allclose(dev(got), dev(mim), rtol=1e-12)
    assert (dev(cfg) > 1.5 * dev(mim)).all()


def test_degenerate_plane_keeps_cfg():
    """A plane without spread (divisor exactly 0): the extension divides 0 by 0; here that plane is cfg itself, the others are
    thresholded."""
    from minsdtf_amd import dynthresh as D

    rng = np.random.default_rng(4)
    u = rng.standard_normal((2, 6, 5, 4))
    c = rng.standard_normal((2, 6, 5, 4))
    u[1, :, :, 2], c[1, :, :, 2] = 0.25, 0.75   # cfg = 0.25 + g * 0.5 everywhere: cc = 0, mc = 0
    for measure in D.MEASURES:
        for startpoint in D.STARTPOINTS:
            got = D.dynthresh_host(u, c, 4.0, 2.0, dict(measure=measure, startpoint=startpoint, percentile=0.9))
            assert np.all(np.isfinite(got))
            np.testing.assert_array_equal(got[1, :, :, 2], np.full((6, 5), 0.25 + 4.0 * 0.5))
            want = _dynthresh_torch(u, c, 4.0, 2.0, 0.9, measure, startpoint, 1.0)
            assert np.isnan(want[1, :, :, 2]).all()
            keep = np.ones(u.shape, dtype=bool)
            keep[1, :, :, 2] = False
            np.testing.assert_allclose(got[keep], want[keep], rtol=0, atol=1e-12 * np.abs(want[keep]).max())
    with pytest.raises(ValueError, match="shape"):
        D.dynthresh_host(u, c[:1], 4.0, 2.0, True)


# -------------------------------------------------------------------------------------------------------------- the C ABI
def test_library_exports_its_header_and_the_others_are_untouched():
    from minsdtf_amd import _lib, _lib_dynthresh, _lib_ext

    assert os.path.exists(_lib_dynthresh.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    header = open(os.path.join(ROOT, "include", "minsdtf_hip_dynthresh.h")).read()
    declared = set(re.findall(r"^MSDT_API\s+(?:int|const char\*)\s+(msdt_\w+)\s*\(", header, flags=re.M))
    assert declared == set(_lib_dynthresh.SYMBOLS) == {"msdt_abi_version", "msdt_last_error", "msdt_dynamic_threshold"}
    assert not re.search(r"^(?:int|const char\*)\s+msdt_\w+\s*\(", header, flags=re.M), "a declaration without MSDT_API"
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib_dynthresh.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert exported == declared, sorted(exported ^ declared)
    lib = _lib_dynthresh.load()
    assert lib.msdt_abi_version() == _lib_dynthresh.ABI_VERSION == int(re.search(r"#define MSDT_ABI_VERSION (\d+)", header).group(1))
    # the export map names the header's functions one by one
    emap = open(os.path.join(ROOT, "minsdtf_amd", "csrc", "dynthresh", "exports_dynthresh.map")).read()
    assert set(re.findall(r"\b(msdt_\w+);", emap)) == declared and "*;" in emap and "msdt_*" not in emap
    for other in (_lib, _lib_ext):
        table = subprocess.check_output(["nm", "-D", "--defined-only", other.LIB_PATH], text=True)
        assert "msdt_" not in table and not any(n.startswith("msdt_") for n in other.SYMBOLS)


def test_struct_layout_matches_the_header():
    from minsdtf_amd import _lib_dynthresh

    cls, struct = _lib_dynthresh.MsdtDynamicThreshold, "MsdtDynamicThreshold"
    fields = [n for n, _t in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "minsdtf_hip_dynthresh.h"\nint main(){printf("%zu", sizeof(' + struct + '));' + \
        "".join(f'printf(" %zu", offsetof({struct}, {f}));' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]


BASE = 1 << 20   # (addresses are only compared and checked for alignment: every bad call returns before a launch)
ROW = 2 * 8 * 8 * 16   # bytes of the u rows (batch 2, 8 x 8): eps is 2 * ROW


def _call(**over):
    from minsdtf_amd import _lib_dynthresh

    a = dict(eps=BASE, out=BASE, scales=2 * BASE, step_ptr=3 * BASE, params=4 * BASE, batch=2, h=8, w=8, num_steps=4)
    a.update(over)
    s = _lib_dynthresh.MsdtDynamicThreshold()
    for k, v in a.items():
        setattr(s, k, v)
    return s


BAD = [dict(eps=None), dict(out=None), dict(scales=None), dict(params=None), dict(eps=BASE + 8, out=BASE + 8), dict(out=5 * BASE + 4),
       dict(scales=2 * BASE + 4), dict(params=4 * BASE + 8), dict(step_ptr=3 * BASE + 2), dict(batch=0), dict(batch=-1), dict(batch=65536),
       dict(h=0), dict(w=0), dict(h=-8), dict(h=1, w=1), dict(h=32768, w=16384), dict(h=65536, w=65536), dict(num_steps=0),
       dict(out=BASE + 16), dict(out=BASE + ROW), dict(out=BASE + 2 * ROW - 16), dict(out=BASE - 16), dict(out=BASE - ROW + 16),
       dict(out=2 * BASE), dict(out=2 * BASE + 16), dict(out=2 * BASE - 16), dict(out=4 * BASE), dict(out=4 * BASE + 16),
       dict(out=4 * BASE - ROW + 16), dict(out=3 * BASE), dict(out=3 * BASE - 16)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_argument_errors_without_a_device(bad):
    from minsdtf_amd import _lib_dynthresh

    lib = _lib_dynthresh.load()
    assert lib.msdt_dynamic_threshold(ctypes.byref(_call(**bad)), None) == -1, bad   # MSD_E_ARG
    assert b"dynamic_threshold" in lib.msdt_last_error()


def test_null_struct_is_an_argument_error():
    from minsdtf_amd import _lib_dynthresh

    lib = _lib_dynthresh.load()
    assert lib.msdt_dynamic_threshold(None, None) == -1 and b"dynamic_threshold: null" in lib.msdt_last_error()


# ------------------------------------------------------------------------------------------------- generate_image, no device
def test_refused_entry_and_the_others_keep_their_words():
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    what, arguments, states = StableDiffusionBase._REFUSED["dynamic_threshold"]
    assert what == "guided text-to-image on one stream only"
    assert set(arguments) == {"tiled", "control_net_image", "reference_image", "inpaint_mask"}
    assert tuple(states) == ("a TCD pipeline (active_tcd=True)", "denoise_streams = 2")
    assert StableDiffusionBase._REFUSED["sag"] == (
        "text-to-image on one stream only",
        ("regions", "tiled", "hires", "pag", "reference_only", "hypertile", "control_net_image", "reference_image", "inpaint_mask"),
        ("denoise_streams = 2",))
    assert StableDiffusionBase._REFUSED["pag"] == ("text-to-image on one stream only",
                                                   ("regions", "tiled", "hires", "control_net_image", "reference_image", "inpaint_mask"),
                                                   ("denoise_streams = 2",))
    assert set(StableDiffusionBase._REFUSED) == {"regions", "tiled", "hires", "pag", "hypertile", "reference_only", "sag", "dynamic_threshold"}


def test_refusals_come_before_any_device_work():
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    ctx = np.zeros((77, 768), dtype=np.float32)
    img = np.zeros((64, 64, 3), dtype=np.uint8)
    sd = StableDiffusionBase(64, 64)   # (no models behind it: anything that reaches a model fails another way)
    kw = dict(batch_size=1, num_steps=3, seed=0, dynamic_threshold=dict(mimic_scale=5.0))
    for extra, names in ((dict(tiled=dict(size=(64, 128))), ["tiled"]), (dict(control_net_image=img.astype(np.float32)), ["control_net_image"]),
                         (dict(reference_image=img), ["reference_image"]), (dict(inpaint_mask=img[..., 0]), ["inpaint_mask"]),
                         (dict(reference_image=img, inpaint_mask=img[..., 0]), ["reference_image", "inpaint_mask"])):
        with pytest.raises(ValueError, match="dynamic_threshold is guided text-to-image on one stream only: it cannot be combined with") as e:
            sd.generate_image(ctx, **kw, **extra)
        assert all(n in str(e.value) for n in names), str(e.value)
    two = StableDiffusionBase(64, 64)
    two.denoise_streams = 2
    with pytest.raises(ValueError, match="dynamic_threshold is.*denoise_streams = 2"):
        two.generate_image(ctx, **kw)
    tcd = StableDiffusionBase(64, 64, active_tcd=True)
    with pytest.raises(ValueError, match=r"dynamic_threshold is.*a TCD pipeline \(active_tcd=True\)"):
        tcd.generate_image(ctx, **kw)
    with pytest.raises(ValueError, match="dynamic_threshold is"):
        sd.text_to_image(ctx, tiled=dict(size=(64, 128)), **kw)
    for g in (0.0, -1.0):
        with pytest.raises(ValueError, match="nothing to threshold"):
            sd.generate_image(ctx, unconditional_guidance_scale=g, **kw)
    with pytest.raises(ValueError, match="unknown field"):
        sd.generate_image(ctx, batch_size=1, num_steps=3, dynamic_threshold=dict(mimic=3.0))
    with pytest.raises(ValueError, match="percentile"):
        sd.generate_image(ctx, batch_size=1, num_steps=3, dynamic_threshold=dict(percentile=99.0))
    assert not sd._engines


def test_engine_key_holds_the_fact_and_never_the_numbers():
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    class Net:
        weights_version = 1

    sd = StableDiffusionBase(64, 64)
    sd.diffusion_model = Net()
    args = (1, 77, 77, 4, 12.0, 0.0, False)
    plain = sd._engine_key(*args)
    assert sd._engine_key(*args, dynthresh=None) == plain
    key = sd._engine_key(*args, dynthresh=True)
    assert key != plain and key[:len(plain)] == plain and key[len(plain):] == (("dynthresh",),)
    assert sd._engine_key(*args, sampler="euler_a", dynthresh=True)[-1] == ("dynthresh",)
    both = sd._engine_key(*args, sag=True, dynthresh=True)
    assert both[-2:] == (("sag",), ("dynthresh",)) and both[:-1] == sd._engine_key(*args, sag=True)
    assert sd._engine_key(*args, pag=("mid_block.attentions.0",), dynthresh=True)[-1] == ("dynthresh",)


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


def _tail(dynthresh, sampler=None, B=2, h=8, w=8, steps=4, **state):
    """DenoiseEngine._build_tail itself on a stand-in engine whose buffers are Bufs of a host plan: the records of the tail."""
    import torch

    from minsdtf_amd import samplers as smp
    from minsdtf_amd.stable_diffusion import DenoiseEngine

    from minsdtf_amd import engine

    class Buf(engine.Buf):   # (the tail takes addresses inside eps and the SAG planes through data_ptr(): here the arena offset)
        def data_ptr(self):
            return self.offset

    def build(p, e, T):
        n = h * w * 4
        groups = 5 if state.get("sag") else 3 if (state.get("pag") or state.get("regions")) else 2

        def alloc(nbytes):
            b = p.alloc(nbytes)
            return Buf(b.arena, b.offset, b.nbytes)

        me = types.SimpleNamespace(B=B, num_steps=steps, h=h, w=w, regions=state.get("regions", 0), tiled=None, dual=False, cfg=True,
                                   unet=types.SimpleNamespace(device=torch.device("cpu")), sampler=smp.parse(sampler), region_attn=False,
                                   pag=state.get("pag"), sag=bool(state.get("sag")), dynthresh=dynthresh,
                                   eps=alloc(groups * B * n * 4), latent=p.alloc(B * n * 4), coef=p.alloc(steps * 8 * 4), step_ptr=p.alloc(8),
                                   region_w=p.alloc(3 * h * w * 4), pag_w=p.alloc(2 * h * w * 4), sag_w=alloc(3 * h * w * 4))
        build.me = me
        DenoiseEngine._build_tail(me, p, 12.0, 0.7, False, False)

    recs, plan = _record(build)
    return recs, build.me


@pytest.mark.parametrize("sampler", [None, "dpmpp_2m", "euler_a"])
def test_the_tail_records_one_more_launch_and_a_step_without_guidance(sampler):
    plain, _me = _tail(False, sampler)
    recs, me = _tail(True, sampler)
    step = "cfg_step" if sampler is None else "sampler_step"
    assert [r.op for r in plain] == [step] and [r.op for r in recs] == ["dynamic_threshold", step]
    assert (plain[0].kw["guidance"], plain[0].kw["guidance_rescale"]) == (12.0, 0.7)
    assert (recs[1].kw["guidance"], recs[1].kw["guidance_rescale"]) == (0.0, 0.0)
    scalar = lambda r: {k: v for k, v in r.kw.items() if isinstance(v, (int, float, str, bool)) and not k.startswith("guidance")}
    assert scalar(recs[1]) == scalar(plain[0]) and set(recs[1].kw) == set(plain[0].kw)   # nothing else of the step moves
    dt = recs[0]
    assert dt.name == "dynthresh" and (dt.kw["batch"], dt.kw["h"], dt.kw["w"], dt.kw["num_steps"]) == (2, 8, 8, 4)
    assert dt.kw["eps"] is dt.kw["out"] is recs[1].kw["eps"] is me.eps and dt.kw["step_ptr"] is me.step_ptr
    assert tuple(me.dt_scales.shape) == (4, 2) and me.dt_params.numel() * me.dt_params.element_size() == 32
    assert dt.kw["scales"] is me.dt_scales and dt.kw["params"] is me.dt_params
    assert _tail(False, sampler)[1].dt_scales is None


@pytest.mark.parametrize("state, front", [(dict(pag=frozenset(["mid_block.attentions.0"])), ["pag_combine"]),
                                          (dict(regions=2), ["region_combine"]), (dict(sag=True), ["sag.copy_u", "sag.combine"])])
def test_the_launch_goes_behind_the_other_combines(state, front):
    """pag / regions write c' over the c rows and the launch reads (u, c') from the base of eps; a SAG job's step reads group 3 on
    (the copy of u, c'), and so does the launch, which overwrites the copy."""
    recs, me = _tail(True, **state)
    names = [r.name or r.op for r in recs]
    assert names == front + ["dynthresh", "cfg_step"]
    dt, step = recs[-2], recs[-1]
    n = 8 * 8 * 4
    if state.get("sag"):   # (an address inside eps, not a buffer of the plan)
        first = me.eps.data_ptr() + 3 * 2 * n * 4
        assert dt.kw["eps"].ptr == dt.kw["out"].ptr == step.kw["eps"].ptr == first and dt.kw["eps"] is dt.kw["out"] is step.kw["eps"]
    else:
        for r in (dt, step):
            assert r.operands["eps"].offset == me.eps.offset
        assert dt.operands["out"].offset == dt.operands["eps"].offset
    assert (step.kw["guidance"], step.kw["guidance_rescale"]) == (0.0, 0.0)
    # every operand of every launch of the tail inside its buffer; the new launch's output apart from its small inputs
    for r in recs:
        ext_fn = XD.EXTENTS.get(r.op) or X.EXTENTS[r.op]
        dims = {k: (v if v is None or isinstance(v, (int, float, str, bool)) else True) for k, v in r.kw.items() if k != "name"}
        ext = ext_fn(**dims)
        for name, o in r.operands.items():
            assert name in ext, f"{r.op} '{r.name}': operand '{name}' has no extent"
            assert ext[name][0] <= o.avail and not o.freed, f"{r.op} '{r.name}': operand '{name}'"
    assert set(dt.operands) == ({"step_ptr"} if state.get("sag") else {"eps", "out", "step_ptr"})   # (scales, params: the engine's tensors)
    ext = XD.dynamic_threshold(**{k: (v if isinstance(v, int) else True) for k, v in dt.kw.items() if k != "name"})
    assert set(ext) == {"eps", "out", "scales", "params", "step_ptr"} and ext["eps"][0] == 2 * ext["out"][0] == 2 * 2 * n * 4
    assert XD.IN_PLACE["dynamic_threshold"] == {("eps", "out")}


def test_emit_records_exactly_the_launch():
    from minsdtf_amd import engine

    def build(p, e, T):
        eps = p.alloc(2 * 3 * 5 * 7 * 16)
        build.eps = eps
        build.ret = engine.emit_dynamic_threshold(p, eps, p.alloc(6 * 8), p.alloc(32), p.alloc(8), 3, 5, 7, 6)

    recs, _plan = _record(build)
    assert build.ret is build.eps and len(recs) == 1
    r = recs[0]
    assert (r.op, r.name) == ("dynamic_threshold", "dynthresh") and set(r.operands) == {"eps", "out", "scales", "params", "step_ptr"}
    ext = XD.dynamic_threshold(**{k: (v if isinstance(v, int) else True) for k, v in r.kw.items() if k != "name"})
    seen = {}
    for name, o in r.operands.items():
        assert ext[name][0] <= o.avail
        seen[name] = (o.offset, o.offset + ext[name][0])
    for a in seen:
        for b in seen:
            if a < b and "out" in (a, b) and (a, b) != ("eps", "out"):
                assert not (seen[a][0] < seen[b][1] and seen[b][0] < seen[a][1]), (a, b)
