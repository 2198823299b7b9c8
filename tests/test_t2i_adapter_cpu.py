"""T2I-Adapters without a GPU: the float64 statement against a torch.nn transcription of the public definition, the checkpoint
reader, the description / table / refusals, the C ABI of the eighth library, the recorded plans of the adapter and of a job, and the
pipeline's route from a picture to the features."""
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

import _extents as X
import _extents_t2i as XT
import _layer_walk as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
CH = (320, 640, 1280, 1280)
SITES = ("down_blocks.0.attentions.1", "down_blocks.1.attentions.1", "down_blocks.2.attentions.1", "down_blocks.3.resnets.1")


# ------------------------------------------------------------------------------------------------------- the float64 statement
class _Block(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.block1, self.act, self.block2 = nn.Conv2d(c, c, 3, padding=1), nn.ReLU(), nn.Conv2d(c, c, 1)

    def forward(self, x):
        return self.block2(self.act(self.block1(x))) + x


class _Level(nn.Module):
    def __init__(self, cin, cout, down):
        super().__init__()
        self.downsample = nn.AvgPool2d(2, 2) if down else None
        self.in_conv = nn.Conv2d(cin, cout, 1) if cin != cout else None
        self.resnets = nn.Sequential(_Block(cout), _Block(cout))

    def forward(self, x):
        if self.downsample is not None:
            x = self.downsample(x)
        if self.in_conv is not None:
            x = self.in_conv(x)
        return self.resnets(x)


class _FullAdapter(nn.Module):
    """The definition of the issue / of minsdtf_amd/t2iadapter.py's docstring on torch.nn layers (NCHW); under `adapter.` its
    state_dict keys are diffusers' checkpoint keys."""

    def __init__(self, cin):
        super().__init__()
        self.unshuffle = nn.PixelUnshuffle(8)
        self.conv_in = nn.Conv2d(64 * cin, CH[0], 3, padding=1)
        self.body = nn.ModuleList([_Level(CH[max(l - 1, 0)], CH[l], l > 0) for l in range(4)])

    def forward(self, x):
        x = self.conv_in(self.unshuffle(x))
        out = []
        for level in self.body:
            x = level(x)
            out.append(x)
        return out


@pytest.mark.parametrize("cin", [1, 3])
@pytest.mark.parametrize("hw", [(64, 64), (64, 128)])
def test_forward_host_is_the_definition_in_float64(cin, hw):
    from minsdtf_amd import t2iadapter as T

    state = T.synthetic_state(3, cin)
    model = _FullAdapter(cin).double()
    assert {"adapter." + k for k in model.state_dict()} == set(state)                    # diffusers' key names
    model.load_state_dict({k[len("adapter."):]: torch.from_numpy(v).double() for k, v in state.items()})
    pic = np.random.default_rng(cin).random((1,) + hw + (cin,))
    with torch.no_grad():
        ref = [f.permute(0, 2, 3, 1).numpy() for f in model(torch.from_numpy(pic).permute(0, 3, 1, 2))]
    for form in (state, T.read_state(state), T.synthetic_state(3, cin, layout="original")):   # both file layouts, or the reader's result
        got = T.forward_host(form, pic)
        assert [g.shape for g in got] == [(1, hw[0] // 8 >> l, hw[1] // 8 >> l, CH[l]) for l in range(4)] and got[0].dtype == np.float64
        for l, (g, r) in enumerate(zip(got, ref)):
            err = float(np.abs(g - r).max() / np.abs(r).max())
            assert err <= 1e-9, (l, err)
    assert [g.shape for g in T.forward_host(state, pic[0])] == [r.shape for r in ref]   # a picture without the batch axis
    with pytest.raises(ValueError, match="multiples of 64"):
        T.forward_host(state, np.zeros((1, 72, 64, cin)))
    with pytest.raises(ValueError, match=f"for an adapter of {cin} input channel"):
        T.forward_host(state, np.zeros((1, 64, 64, 4 - cin)))


@pytest.mark.parametrize("cin", [1, 3])
def test_unshuffle_channel_order_on_an_index_valued_picture(cin):
    """Every pixel holds its own (y, x, c) index: channel c * 64 + dy * 8 + dx of output pixel (Y, X) is picture pixel (8 Y + dy,
    8 X + dx, c) - a transposed (dy, dx), or c as the fastest index, cannot pass."""
    from minsdtf_amd import t2iadapter as T

    H, W = 16, 24
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(cin), indexing="ij")
    pic = (y * 1000 + x * 10 + c).astype(np.float64)[None]
    got = T.unshuffle_host(pic)
    assert got.shape == (1, 2, 3, 64 * cin)
    for Y in range(2):
        for Xp in range(3):
            for ch in range(64 * cin):
                cc, dy, dx = ch // 64, (ch % 64) // 8, ch % 8
                assert got[0, Y, Xp, ch] == (8 * Y + dy) * 1000 + (8 * Xp + dx) * 10 + cc
    ref = nn.PixelUnshuffle(8)(torch.from_numpy(pic).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).numpy()
    np.testing.assert_array_equal(got, ref)


def test_add_reference_is_the_statement():
    from minsdtf_amd import t2iadapter as T

    rng = np.random.default_rng(0)
    x, f0, f1 = rng.standard_normal((3, 16)), rng.standard_normal(16), np.full(16, np.nan)
    np.testing.assert_array_equal(T.add_reference(x, [f0, f1], [0.5, 0.0]), x + 0.5 * f0)
    keep = np.array(x)
    keep[1, 3] = np.nan
    got = T.add_reference(keep, [f1, f1], [0.0, 0.0])
    assert np.array_equal(got, keep, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------ the checkpoint
def test_reader_takes_both_layouts_and_fp16():
    from minsdtf_amd import t2iadapter as T

    for cin in (1, 3):
        d, o = T.synthetic_state(5, cin, layout="diffusers"), T.synthetic_state(5, cin, layout="original")
        assert len(d) == len(o) == 38 and "adapter.body.1.in_conv.weight" in d and "body.2.in_conv.weight" in o and "body.7.block2.bias" in o
        assert "adapter.body.0.in_conv.weight" not in d and "adapter.body.3.in_conv.weight" not in d
        a, b = T.read_state(d), T.read_state(o)
        assert set(a) == set(b) and len(a) == 38 and T.in_channels_of(a) == cin
        for k in a:
            np.testing.assert_array_equal(a[k], b[k])
            assert a[k].dtype == np.float32
        assert a["conv_in.weight"].shape == (320, 64 * cin, 3, 3) and a["body.2.resnets.1.block2.weight"].shape == (1280, 1280, 1, 1)
        np.testing.assert_array_equal(a["body.3.resnets.0.block1.bias"], o["body.6.block1.bias"])
        half = T.read_state({k: torch.from_numpy(v).half() for k, v in d.items()})
        for k in a:
            assert half[k].dtype == np.float32
            np.testing.assert_array_equal(half[k], a[k].astype(np.float16).astype(np.float32))


def test_reader_names_what_it_refuses():
    from minsdtf_amd import t2iadapter as T

    d = T.synthetic_state(5, 3)
    bad = dict(d)
    bad["adapter.body.2.resnets.0.block1.weight"] = np.zeros((1280, 640, 3, 3), dtype=np.float32)
    with pytest.raises(ValueError, match=r"adapter.body.2.resnets.0.block1.weight has shape \(1280, 640, 3, 3\), expected \(1280, 1280, 3, 3\)"):
        T.read_state(bad)
    bad = dict(d)
    del bad["adapter.body.1.in_conv.bias"]
    with pytest.raises(ValueError, match="has no 'adapter.body.1.in_conv.bias'"):
        T.read_state(bad)
    o = T.synthetic_state(5, 3, layout="original")
    with pytest.raises(ValueError, match=r"`skep` keys \(body.0.skep.weight"):
        T.read_state(dict(o, **{"body.0.skep.weight": np.zeros((320, 320, 1, 1), dtype=np.float32)}))
    with pytest.raises(ValueError, match=r"conv_in.weight has shape \(320, 768, 3, 3\).*SDXL"):
        T.read_state(dict(d, **{"adapter.conv_in.weight": np.zeros((320, 768, 3, 3), dtype=np.float32)}))
    with pytest.raises(ValueError, match="has no 'conv_in.weight'"):
        T.read_state({"body.0.block1.weight": o["body.0.block1.weight"]})
    # a light adapter: resnets at other channel sets, more blocks per level
    light = dict(d, **{"adapter.body.0.resnets.2.block1.weight": np.zeros((320, 320, 3, 3), dtype=np.float32)})
    with pytest.raises(ValueError, match=r"unexpected checkpoint keys \['adapter.body.0.resnets.2.block1.weight'\]"):
        T.read_state(light)


def test_model_packs_through_the_layout_table_and_reads_a_file(tmp_path):
    from minsdtf_amd import t2iadapter as T
    from minsdtf_amd.models import T2IAdapter

    m = T2IAdapter.synthetic(2, 1, device=CPU)
    assert (m.kind, m.in_channels, m.weights_version) == ("t2i_adapter", 1, 1) and len(m._W) == 38
    w = m._W["adapter.body.1.in_conv.w"]
    assert w.dtype == torch.bfloat16 and m._W.layout("adapter.body.1.in_conv.w") == 1 and tuple(w.shape) == (320 // 64, 640, 64)
    assert m._W["adapter.conv_in.b"].dtype == torch.float32 and tuple(m._W["adapter.conv_in.w"].shape) == (9, 320, 64)
    # chunk-major image of the logical [N][K] rows, K = (ky * 3 + kx) * C_in + c
    src = m.state["body.1.in_conv.weight"][:, :, 0, 0]
    np.testing.assert_array_equal(w.permute(1, 0, 2).reshape(640, 320).float().numpy(), torch.from_numpy(src).bfloat16().float().numpy())
    m.set_state(T.synthetic_state(2, 3, layout="original"))
    assert (m.in_channels, m.weights_version) == (3, 2) and tuple(m._W["adapter.conv_in.w"].shape) == (27, 320, 64)
    path = os.path.join(tmp_path, "adapter.pt")
    torch.save({k: torch.from_numpy(v).half() for k, v in T.synthetic_state(4, 1).items()}, path)
    f = T2IAdapter(path=path, device=CPU)
    assert f.in_channels == 1 and f.state["conv_in.weight"].shape == (320, 64, 3, 3)
    with pytest.raises(ValueError, match="not found"):
        T2IAdapter(path=os.path.join(tmp_path, "none.pt"), device=CPU)
    import pathlib

    assert T2IAdapter(path=pathlib.Path(path), device=CPU).in_channels == 1
    f.compile(jit_compile=True)
    assert f._use_graph and not f._plans
    with pytest.raises(ValueError, match="in_channels = 2"):
        T2IAdapter(2, device=CPU)
    with pytest.raises(RuntimeError, match="no weights set"):
        T2IAdapter(3, device=CPU).features(np.zeros((1, 64, 64, 3), dtype=np.float32))


# ------------------------------------------------------------------------------------------- description, table and refusals
PIC = np.zeros((64, 64, 3), dtype=np.uint8)


def test_parse_defaults_and_forms():
    from minsdtf_amd import t2iadapter as T

    assert T.parse(None) is None and T.MAX_UNITS == 3 and T.SITES == 4 and T.SITE_NAMES == SITES
    (u,) = T.parse(dict(image=PIC, path="a.pth"))
    assert (u.weight, u.start, u.end, u.path, u.model) == ((1.0,) * 4, 0.0, 1.0, "a.pth", None)
    (u,) = T.parse(T.T2IAdapterSpec(image=PIC, model=object(), weight=[1, 0.5, 0.25, 0], start=0.25, end=0.5))
    assert u.weight == (1.0, 0.5, 0.25, 0.0) and (u.start, u.end) == (0.25, 0.5)
    assert len(T.parse([dict(image=PIC, path="a")] * 3)) == 3
    assert T.parse(T.parse(dict(image=PIC, path="a"))) == T.parse(dict(image=PIC, path="a"))   # idempotent


@pytest.mark.parametrize("bad,word", [
    (dict(path="a"), "`image`"), (dict(image=PIC), "one of `path`"), (dict(image=PIC, path="a", model=1), "should not both"),
    (dict(image=PIC, path=3), "path = 3"), (dict(image=PIC, path="a", weight=-1), "weight = -1"),
    (dict(image=PIC, path="a", weight=float("nan")), "weight"), (dict(image=PIC, path="a", weight=[1, 2, 3]), "four of them"),
    (dict(image=PIC, path="a", weight=[1, 2, 3, -4]), r"weight\[3\]"), (dict(image=PIC, path="a", weight=True), "weight"),
    (dict(image=PIC, path="a", start=0.6, end=0.5), "start = 0.6 > end = 0.5"), (dict(image=PIC, path="a", end=1.5), "end = 1.5"),
    (dict(image=PIC, path="a", strength=1), "unknown field"), (3, "int"), ([dict(image=PIC, path="a")] * 4, "4 units"), ([], "0 units")])
def test_parse_value_errors(bad, word):
    from minsdtf_amd import t2iadapter as T

    with pytest.raises(ValueError, match="^t2i_adapter: .*" + word):
        T.parse(bad)


@pytest.mark.parametrize("steps", [1, 4, 10])
def test_table_is_weight_times_keep(steps):
    from minsdtf_amd import control, t2iadapter as T

    units = [dict(image=PIC, path="a", weight=[1.5, 1.0, 0.5, 0.25], start=0.25, end=0.75), dict(image=PIC, path="b", weight=0.7)]
    t = T.table(units, steps)
    assert t.shape == (steps, 2, 4) and t.dtype == np.float32
    for i in range(steps):
        k = control.keep(i, steps, 0.25, 0.75)
        np.testing.assert_array_equal(t[i, 0], np.asarray([1.5, 1.0, 0.5, 0.25], dtype=np.float32) * np.float32(k))
        np.testing.assert_array_equal(t[i, 1], np.full(4, np.float32(0.7)))
    # keep at the range ends (diffusers' rule): start = end = 1 keeps nothing, [0, 1] everything, end = 0.75 of 4 steps drops the last
    assert not T.table(dict(image=PIC, path="a", start=1.0), 4).any()
    assert T.table(dict(image=PIC, path="a"), 4).all()
    np.testing.assert_array_equal(T.table(dict(image=PIC, path="a", end=0.75), 4)[:, 0, 0], [1, 1, 1, 0])
    np.testing.assert_array_equal(T.table(dict(image=PIC, path="a", start=0.5), 4)[:, 0, 0], [0, 0, 1, 1])
    with pytest.raises(ValueError, match="num_steps = 0"):
        T.table(dict(image=PIC, path="a"), 0)


def test_picture_channel_counts_and_resize():
    from minsdtf_amd import t2iadapter as T
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    rs = StableDiffusionBase.resize
    a = T.picture(np.full((64, 64, 3), 255, dtype=np.uint8), 3, 64, 64)
    assert a.shape == (1, 64, 64, 3) and a.dtype == np.float32 and float(a.min()) == float(a.max()) == 1.0
    assert T.picture(np.full((32, 48), 51.0), 1, 64, 128, rs).shape == (1, 64, 128, 1)
    np.testing.assert_allclose(T.picture(np.full((32, 48, 1), 51.0), 1, 64, 128, rs), 0.2, rtol=1e-6)
    with pytest.raises(ValueError, match=r"\(3 channel\(s\)\) for an adapter of 1 input channel"):
        T.picture(np.zeros((64, 64, 3)), 1, 64, 64)
    with pytest.raises(ValueError, match=r"\(1 channel\(s\)\) for an adapter of 3 input channel"):
        T.picture(np.zeros((64, 64)), 3, 64, 64)
    with pytest.raises(ValueError, match="multiples of 64"):
        T.check_size(96, 64)


def test_picture_from_a_file_name_a_path_object_and_an_open_file(tmp_path):
    """A file goes the way a ControlNet hint's does: decoded, converted to the adapter's channels and resized by PIL - whatever
    names it: a str, an os.PathLike, an open binary file."""
    import pathlib

    from PIL import Image

    from minsdtf_amd import t2iadapter as T

    rgb = np.random.default_rng(0).integers(0, 256, (32, 48, 3)).astype(np.uint8)
    name = os.path.join(tmp_path, "pose.png")
    Image.fromarray(rgb).save(name)
    want3 = np.asarray(Image.open(name).convert("RGB").resize((128, 64)), dtype=np.float32)[None] / np.float32(255.0)
    want1 = np.asarray(Image.open(name).convert("L").resize((128, 64)), dtype=np.float32)[None, ..., None] / np.float32(255.0)
    with open(name, "rb") as fh:
        forms = [T.picture(name, 3, 64, 128), T.picture(pathlib.Path(name), 3, 64, 128), T.picture(fh, 3, 64, 128)]
    for got in forms:
        assert got.shape == (1, 64, 128, 3) and got.dtype == np.float32
        np.testing.assert_array_equal(got, want3)
    np.testing.assert_array_equal(T.picture(pathlib.Path(name), 1, 64, 128), want1)   # an RGB file for a 1-channel adapter: converted
    (u,) = T.parse(dict(image=pathlib.Path(name), path=pathlib.Path("adapter.pth")))
    assert isinstance(u.path, pathlib.Path)


def test_refusals_by_name_and_the_shared_table_keeps_its_rows():
    from minsdtf_amd import jobopts, t2iadapter as T

    names = ("control_net_image", "regions", "pag", "sag", "reference_only", "hypertile", "tiled", "hires")
    assert T.REFUSED == (names, ("denoise_streams = 2",))
    T.refuse({})
    T.refuse(dict(ip_adapter=1, dynamic_threshold=1, inpaint_mask=1, reference_image=1), streams=1)
    for n in names:
        with pytest.raises(ValueError, match=f"^t2i_adapter: .*cannot be combined with {n}$"):
            T.refuse({n: 1})
    with pytest.raises(ValueError, match="cannot be combined with regions, pag, denoise_streams = 2$"):
        T.refuse(dict(pag=1, regions=1), streams=2)
    assert len(jobopts.REFUSED) == 8 and "t2i_adapter" not in jobopts.REFUSED


def test_engine_options_key_and_checks():
    from minsdtf_amd.jobopts import EngineOptions, job_options

    assert EngineOptions.of(t2i_units=None) == EngineOptions.of(t2i_units=0) == EngineOptions() and EngineOptions.of().key() == ()
    assert EngineOptions.of(t2i_units=2).key() == (("t2i", 2),)
    assert EngineOptions.of(ip_tokens=4, t2i_units=1, dynthresh=True).key() == (("dynthresh",), ("ip", 4), ("t2i", 1))
    assert job_options() == {} and job_options(t2i_units=2) == dict(t2i_units=2)
    ok = EngineOptions.of(t2i_units=3, ip_tokens=4, dynthresh=True, sampler="euler_a")
    ok.check(16, 16, 1, 7.5, False, False, False, None)
    EngineOptions.of(t2i_units=2, ip_tokens=4, sampler="dpmpp_2m").check(16, 16, 1, 7.5, False, True, False, None)   # inpainting
    EngineOptions.of(t2i_units=1).check(8, 16, 2, 0.0, False, False, True, 1)   # a TCD pipeline, no guidance, inpainting
    with pytest.raises(ValueError, match="^t2i_adapter: 4 units"):
        EngineOptions.of(t2i_units=4).check(8, 8, 1, 7.5, False, False, False, None)
    with pytest.raises(ValueError, match="^t2i_adapter: a 72 x 64 job"):
        EngineOptions.of(t2i_units=1).check(9, 8, 1, 7.5, False, False, False, None)
    for kind, opts, kw in (("control_net_image", {}, dict(control=True)), ("pag", dict(pag=("mid_block.attentions.0",)), {}),
                           ("sag", dict(sag=True), {}), ("regions", dict(regions=2), {}), ("hypertile", dict(hypertile=(2, 2, 0)), {}),
                           ("reference_only", dict(reference=("mid_block.attentions.0",)), {}), ("denoise_streams = 2", {}, dict(streams=2))):
        with pytest.raises(ValueError, match=f"^t2i_adapter: .*cannot be combined with.*{kind}"):
            EngineOptions.of(t2i_units=1, **opts).check(16, 16, 1, 7.5, kw.get("control", False), False, False, kw.get("streams"))


# ------------------------------------------------------------------------------------------------------------------ the C ABI
NAMES = {"msda_abi_version", "msda_last_error", "msda_feature_add", "msda_unshuffle", "msda_relu", "msda_avgpool2"}


def test_library_exports_its_header_and_the_others_are_untouched():
    from minsdtf_amd import _lib, _lib_control, _lib_dynthresh, _lib_ext, _lib_ipadapter, _lib_resampler, _lib_t2i, _lib_vision

    assert os.path.exists(_lib_t2i.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    header = open(os.path.join(ROOT, "include", "minsdtf_hip_t2i.h")).read()
    declared = set(re.findall(r"^MSDA_API\s+(?:int|const char\*)\s+(msda_\w+)\s*\(", header, flags=re.M))
    assert declared == set(_lib_t2i.SYMBOLS) == NAMES
    assert not re.search(r"^(?:int|const char\*)\s+msda_\w+\s*\(", header, flags=re.M), "a declaration without MSDA_API"
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib_t2i.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert exported == declared, sorted(exported ^ declared)
    lib = _lib_t2i.load()
    assert lib.msda_abi_version() == _lib_t2i.ABI_VERSION == int(re.search(r"#define MSDA_ABI_VERSION (\d+)", header).group(1)) == 1
    for name in ("MAX_UNITS", "SITES", "CHUNK"):
        assert int(re.search(rf"#define MSDA_{name} (\d+)", header).group(1)) == getattr(_lib_t2i, name), name
    assert (_lib_t2i.MAX_UNITS, _lib_t2i.SITES) == (3, 4)
    emap = open(os.path.join(ROOT, "minsdtf_amd", "csrc", "t2i", "exports_t2i.map")).read()
    assert set(re.findall(r"\b(msda_\w+);", emap)) == declared and "*;" in emap and "msda_*" not in emap
    counts = {}
    for other in (_lib, _lib_ext, _lib_dynthresh, _lib_control, _lib_ipadapter, _lib_vision, _lib_resampler):
        table = subprocess.check_output(["nm", "-D", "--defined-only", other.LIB_PATH], text=True)
        assert "msda_" not in table and not any(n.startswith("msda_") for n in other.SYMBOLS)
        counts[other.LIB_NAME] = len([ln for ln in table.splitlines() if ln.strip()])
    assert list(counts.values()) == [31, 4, 3, 3, 3, 5, 3], counts
    mk = open(os.path.join(ROOT, "minsdtf_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\$\(TA_OUT\)", mk, flags=re.M) and re.search(r"rm -rf .*\$\(TA_OUT\)", mk)


def test_struct_layout_matches_the_header():
    from minsdtf_amd import _lib_t2i

    struct = "MsdaFeatureAdd"
    cls = getattr(_lib_t2i, struct)
    fields = [n for n, _t in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "minsdtf_hip_t2i.h"\nint main(){printf("%zu", sizeof(' + struct + '));' + \
        "".join(f'printf(" %zu", offsetof({struct}, {f}));' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]


BASE = 1 << 26   # (addresses are only compared and checked for alignment: every bad call returns before a launch)
FA_GOOD = dict(x=BASE, feats=[2 * BASE, 3 * BASE], scales=4 * BASE, step_ptr=5 * BASE, rows=2, n=2048, site=1, num_steps=3)
FA_BAD = [(dict(x=None), b"x must be non-null"), (dict(x=BASE + 8), b"16-byte"), (dict(feats=[2 * BASE, None]), b"feat[1] must be non-null"),
          (dict(feats=[2 * BASE + 2]), b"feat[0] must be non-null and 16-byte"), (dict(scales=None), b"scales must be non-null"),
          (dict(scales=4 * BASE + 4), b"scales must be non-null and 16-byte"), (dict(step_ptr=5 * BASE + 2), b"step_ptr must be 4-byte"),
          (dict(n=2044), b"n 2044"), (dict(n=0), b"n 0"), (dict(n=-8), b"n -8"), (dict(rows=0), b"rows 0"), (dict(rows=65536), b"rows 65536"),
          (dict(site=4), b"site 4"), (dict(site=-1), b"site -1"), (dict(num_steps=0), b"num_steps 0"),
          (dict(feats=[BASE + 4096]), b"x overlaps feat[0]"), (dict(feats=[2 * BASE, BASE + 2 * 2048 * 2 - 16]), b"x overlaps feat[1]"),
          (dict(scales=BASE + 64), b"overlaps scales"), (dict(step_ptr=BASE + 4), b"overlaps scales / step_ptr")]


@pytest.mark.parametrize("bad,text", FA_BAD, ids=lambda v: "-".join(f"{k}" for k in v) if isinstance(v, dict) else None)
def test_feature_add_argument_errors_without_a_device(bad, text):
    from minsdtf_amd import _lib_t2i, ops

    lib = _lib_t2i.load()
    call = ops.feature_add(**dict(FA_GOOD, **bad))
    assert call.name == "feature_add" and call.fn(*call.args, None) == -1, bad   # nothing launched (there is no device)
    msg = lib.msda_last_error()
    assert b"feature_add" in msg and text in msg, msg


def test_units_limits_and_the_other_kernels_argument_errors():
    from minsdtf_amd import _lib_t2i, ops

    lib = _lib_t2i.load()
    assert lib.msda_feature_add(None, None) == -1 and b"feature_add: null" in lib.msda_last_error()
    a = _lib_t2i.MsdaFeatureAdd()
    a.x, a.scales, a.rows, a.n, a.site, a.num_steps = BASE, 4 * BASE, 1, 8, 0, 1
    for units in (0, 4):
        a.units = units
        assert lib.msda_feature_add(ctypes.byref(a), None) == -1 and f"units {units}".encode() in lib.msda_last_error()
    with pytest.raises(ValueError, match="4 features"):
        ops.feature_add(**dict(FA_GOOD, feats=[BASE] * 4))
    for kw, text in ((dict(h=12), b"12 x 16"), (dict(w=20), b"16 x 20"), (dict(h=0), b"0 x 16"), (dict(cin=0), b"cin 0"), (dict(cin=5), b"cin 5"),
                     (dict(batch=0), b"batch 0"), (dict(x=None), b"non-null"), (dict(out=2 * BASE + 8), b"16-byte"), (dict(out=BASE + 64), b"overlaps"),
                     (dict(batch=1 << 15, h=1 << 10, w=1 << 6, cin=1), b"fewer than 2^31")):
        call = ops.unshuffle(**dict(dict(x=BASE, out=2 * BASE, batch=2, h=16, w=16, cin=3), **kw))
        assert call.fn(*call.args, None) == -1 and b"unshuffle" in lib.msda_last_error() and text in lib.msda_last_error(), (kw, lib.msda_last_error())
    for kw, text in ((dict(n=12), b"n 12"), (dict(n=0), b"n 0"), (dict(x=None), b"non-null"), (dict(x=BASE + 2), b"16-byte")):
        call = ops.relu(**dict(dict(x=BASE, n=64), **kw))
        assert call.fn(*call.args, None) == -1 and b"relu" in lib.msda_last_error() and text in lib.msda_last_error(), kw
    for kw, text in ((dict(h=3), b"3 x 4"), (dict(w=5), b"4 x 5"), (dict(h=0), b"0 x 4"), (dict(c=12), b"c 12"), (dict(c=0), b"c 0"), (dict(batch=0), b"batch 0"),
                     (dict(out=None), b"non-null"), (dict(x=BASE + 4), b"16-byte"), (dict(out=BASE + 16), b"overlaps")):
        call = ops.avgpool2(**dict(dict(x=BASE, out=2 * BASE, batch=2, h=4, w=4, c=320), **kw))
        assert call.fn(*call.args, None) == -1 and b"avgpool2" in lib.msda_last_error() and text in lib.msda_last_error(), kw


# ----------------------------------------------------------------------------------------------------------------------- plans
def _recording():
    """(the records, a Plan.rec that keeps every launch as an LW.Rec - a list of features as operands feats.<u> - and the original)"""
    from minsdtf_amd import engine

    recs = []
    orig = engine.Plan.rec

    def rec(self, fn, **kw):
        ops_ = {}
        for k, v in kw.items():
            if k == "workspace" and isinstance(v, engine._Lazy):
                continue
            if k == "feats":
                for u, f in enumerate(v):
                    if LW._operand(f) is not None:
                        ops_[f"feats.{u}"] = LW._operand(f)
                continue
            o = LW._operand(v)
            if o is not None:
                ops_[k] = o
        recs.append(LW.Rec(fn.__name__, kw.get("name", ""), kw, ops_))
        return orig(self, fn, **kw)

    return recs, rec, orig


def _dims(kw):
    return {k: (v if v is None or isinstance(v, (int, float, str, bool)) else (tuple(True if not isinstance(x, (int, float)) else x for x in v)
                                                                              if isinstance(v, (tuple, list)) else True))
            for k, v in kw.items() if k != "name"}


BLOCK_OPS = ["conv_gemm", "relu", "conv_gemm"]


@pytest.mark.parametrize("cin,hw", [(3, (128, 128)), (1, (128, 192)), (3, (512, 512))])
def test_adapter_plan_records_31_launches(cin, hw):
    from minsdtf_amd import engine, t2iadapter as T
    from minsdtf_amd.models import T2IAdapter

    recs, rec, orig = _recording()
    engine.Plan.rec = rec
    try:
        net = types.SimpleNamespace(device=CPU, _W=LW._AnyWeights(), in_channels=cin, _use_graph=False)
        bp = T2IAdapter._build(net, *hw)
    finally:
        engine.Plan.rec = orig
    assert len(recs) == len(bp.plan.calls) == T.LAUNCHES == engine.T2I_ADAPTER_LAUNCHES == 31 and "31 launches" in engine.emit_t2i_adapter.__doc__
    want_ops = ["unshuffle", "conv_gemm"] + BLOCK_OPS * 2
    want_names = ["adapter.unshuffle", "adapter.conv_in"] + [f"adapter.body.0.resnets.{j}.{n}" for j in range(2) for n in ("block1", "act", "block2")]
    for l in (1, 2, 3):
        want_ops += ["avgpool2"] + (["conv_gemm"] if l < 3 else []) + BLOCK_OPS * 2
        want_names += [f"adapter.body.{l}.downsample"] + ([f"adapter.body.{l}.in_conv"] if l < 3 else [])
        want_names += [f"adapter.body.{l}.resnets.{j}.{n}" for j in range(2) for n in ("block1", "act", "block2")]
    assert [r.op for r in recs] == want_ops and [r.name for r in recs] == want_names
    H, W = hw[0] // 8, hw[1] // 8
    a = recs[0].kw
    assert (a["batch"], a["h"], a["w"], a["cin"]) == (1,) + hw + (cin,)
    a = recs[1].kw
    assert (a["h_in"], a["w_in"], a["c0"], a["N"], a["ksize"]) == (H, W, 64 * cin, 320, 3) and (9 * a["c0"]) % 64 == 0 and a["bias"] is not None
    feats = []
    for i, r in enumerate(recs):
        a = r.kw
        if r.op == "relu":      # in place on block1's output, which block2 then reads; block2 adds the block's input
            b1, b2 = recs[i - 1], recs[i + 1]
            assert r.operands["x"].buf == b1.operands["out"].buf == b2.operands["a0"].buf and a["n"] == b1.kw["batch"] * b1.kw["h_in"] * b1.kw["w_in"] * b1.kw["N"]
            assert b1.kw["ksize"] == 3 and b2.kw["ksize"] == 1 and b1.kw["residual"] is None and b1.kw["act"] == 0 and b2.kw["act"] == 0
            assert b2.operands["residual"].buf == b1.operands["a0"].buf and b2.kw["res_ld"] == b2.kw["N"] == b1.kw["N"] == b1.kw["c0"]
            if r.name.endswith("resnets.1.act"):
                feats.append(b2)
        if r.op == "avgpool2":  # reads the previous level's feature where block2 wrote it: nothing is copied
            assert r.operands["x"].buf == feats[-1].operands["out"].buf
            assert (a["h"], a["w"], a["c"]) == (feats[-1].kw["h_in"], feats[-1].kw["w_in"], feats[-1].kw["N"])
    assert [(f.kw["h_in"], f.kw["w_in"], f.kw["N"]) for f in feats] == [(H >> l, W >> l, CH[l]) for l in range(4)]
    for l, f in enumerate(feats):   # the io tensors ARE those buffers, and no later launch writes or recycles them
        t = bp.io[f"feature.{l}"]
        assert t.dtype == torch.bfloat16 and tuple(t.shape) == (1, H >> l, W >> l, CH[l])
        assert t.data_ptr() == bp.plan.arena.base + f.operands["out"].offset
        later = recs[recs.index(f) + 1:]
        lo, hi = f.operands["out"].offset, f.operands["out"].offset + t.numel() * 2
        for r in later:
            for name, o in r.operands.items():
                writes = name in ("out",) or (r.op == "relu" and name == "x")
                if writes and o.kind == "buf":
                    ext = (XT.EXTENTS[r.op] if r.op in XT.EXTENTS else lambda **k: X.extents(r.op, **k))(**_dims(r.kw))
                    assert o.offset >= hi or o.offset + ext[name][0] <= lo, (r.name, name, l)
    assert tuple(bp.io["picture"].shape) == (1,) + hw + (cin,) and bp.io["picture"].dtype == torch.float32
    # every operand inside its live buffer (tests/_extents.py, tests/_extents_t2i.py)
    for r in recs:
        ext = XT.EXTENTS[r.op](**_dims(r.kw)) if r.op in XT.EXTENTS else X.extents(r.op, **_dims(r.kw))
        assert r.operands, r.name
        for name, o in r.operands.items():
            assert name in ext, (r.name, name)
            if o.kind == "buf":
                assert not o.freed and ext[name][0] <= o.avail, (r.name, name, ext[name][0], o.avail)


class _Tensor(LW._Tensor):
    dtype = torch.bfloat16   # (emit_time_embedding reads it)


class _Weights(LW._AnyWeights):
    def __missing__(self, k):
        return _Tensor()


def _net(**kw):
    return types.SimpleNamespace(_require_weights=lambda: None, device=CPU, _W=_Weights(), **kw)


def _engine(monkeypatch, units, size=16, t_uncond=77, guidance=7.5, **kw):
    """A DenoiseEngine on the stand-ins (a 128 x 128 job: a 16 x 16 latent), its Plan.rec calls as Rec records in recording order."""
    import minsdtf_amd.stable_diffusion as sdm
    from minsdtf_amd import engine

    recs, rec, orig = _recording()
    monkeypatch.setattr(engine.Plan, "rec", rec)
    if units:
        kw.update(t2i_units=units)
    eng = sdm.DenoiseEngine(_net(h=size, w=size), 1, 77, t_uncond, 3, guidance, 0.7, **kw)
    monkeypatch.setattr(engine.Plan, "rec", orig)
    return eng, recs


@pytest.mark.parametrize("form", ["fused", "two_passes", "no_guidance", "three_units", "with_ip"])
def test_job_records_four_adds_per_unet_pass_at_the_four_sites(monkeypatch, form):
    kw = dict(t_uncond=40 if form == "two_passes" else 77, guidance=0.0 if form == "no_guidance" else 7.5)
    if form == "with_ip":
        kw.update(ip_tokens=4, ip_adapter=_net(tokens=4, weights_version=1))
    U = 3 if form == "three_units" else 1
    plain, plain_recs = _engine(monkeypatch, 0, **kw)
    eng, recs = _engine(monkeypatch, U, **kw)
    passes = 2 if form == "two_passes" else 1
    nb = {"two_passes": [1, 1], "no_guidance": [1]}.get(form, [2])
    assert [p[1] for p in eng.passes] == nb and plain.t2i_scales is None and plain.t2i_feat is None
    assert not any(r.op == "feature_add" for r in plain_recs)
    n_prep = len(eng.prep.calls) + len(eng.prep_t.calls)
    step = recs[n_prep:]
    mine = [r for r in step if r.op == "feature_add"]
    assert len(mine) == 4 * passes and not any(r.op == "feature_add" for r in recs[:n_prep]) and len(step) == len(eng.calls)
    assert tuple(eng.t2i_scales.shape) == (3, U, 4) and eng.t2i_scales.dtype == torch.float32
    sizes = [16 * 16 * 320, 8 * 8 * 640, 4 * 4 * 1280, 2 * 2 * 1280]
    assert [[tuple(f.shape) for f in fs] for fs in eng.t2i_feat] == [[(n,) for n in sizes]] * U and eng.t2i_feat[0][0].dtype == torch.bfloat16
    for p in range(passes):
        group = mine[4 * p:4 * (p + 1)]
        assert [r.name for r in group] == [s + ".t2i" for s in SITES]
        for l, r in enumerate(group):
            a = r.kw
            assert (a["site"], a["rows"], a["n"], a["num_steps"]) == (l, nb[p], sizes[l], 3)
            assert a["scales"] is eng.t2i_scales and a["step_ptr"] is eng.step_ptr and len(a["feats"]) == U
            assert all(a["feats"][u] is eng.t2i_feat[u][l] for u in range(U))
            ext = XT.feature_add(**_dims(a))
            assert ext["x"][0] <= r.operands["x"].avail and not r.operands["x"].freed and ext["scales"][0] == eng.t2i_scales.numel() * 4
            assert all(ext[f"feats.{u}"][0] == eng.t2i_feat[u][l].numel() * 2 for u in range(U))
            # right behind the call that produced the site, in place on its output, and before the skip's and the downsampler's reads
            i = step.index(r)
            producer = step[i - 1]
            assert producer.name.startswith(SITES[l]) and producer.operands["out"].buf == r.operands["x"].buf, (producer.name, r.name)
            readers = [q for q in step[i + 1:] if any(o.kind == "buf" and o.buf == r.operands["x"].buf for n, o in q.operands.items() if n != "out")]
            assert readers, r.name
            if l < 3:
                assert readers[0].name == f"down_blocks.{l}.downsamplers.0.conv"
            else:
                assert readers[0].name.startswith("mid_block.resnets.0")
            assert any(q.name.startswith("up_blocks.") for q in readers)   # the skip connection reads the sum too
    # nothing else moves: without the adds the step plan is the plain job's, launch for launch
    strip = lambda rs: [(r.op, r.name) for r in rs if r.op != "feature_add"]   # noqa: E731
    assert strip(step) == strip(plain_recs[len(plain.prep.calls) + len(plain.prep_t.calls):])
    assert strip(recs[:n_prep]) == strip(plain_recs[:n_prep])


def test_unet_variant_refuses_t2i_with_what_it_excludes():
    from minsdtf_amd import engine

    t = ([[_Tensor()] * 4], _Tensor(), 3)
    engine.UNetVariant(t2i=t).check(2, None, None)
    engine.UNetVariant(t2i=t, ip=({}, 4, _Tensor(), 3)).check(2, None, None)
    for kw in (dict(pag_layers=("mid_block.attentions.0",), perturbed=1), dict(window=(2, 2)), dict(sag=(1, 2, 0, 1)),
               dict(region_attn=(2, 1, {})), dict(reference=(("mid_block.attentions.0",), _Tensor(), _Tensor()))):
        with pytest.raises(ValueError, match="t2i .*does not go with"):
            engine.UNetVariant(t2i=t, **kw).check(3, None, None)
    with pytest.raises(ValueError, match="t2i .*does not go with"):
        engine.UNetVariant(t2i=t).check(2, [1] * 13, None)
    with pytest.raises(ValueError, match=r"t2i with 4 unit\(s\)"):
        engine.UNetVariant(t2i=([[_Tensor()] * 4] * 4, _Tensor(), 3)).check(2, None, None)
    with pytest.raises(ValueError, match=r"of \[3\] features"):
        engine.UNetVariant(t2i=([[_Tensor()] * 3], _Tensor(), 3)).check(2, None, None)
    assert engine.T2I_SITES == SITES


def test_prepare_carries_the_goes_with_check(monkeypatch):
    eng, _ = _engine(monkeypatch, 1)
    plain, _ = _engine(monkeypatch, 0)
    feats = [[torch.zeros(n, dtype=torch.bfloat16) for n in (16 * 16 * 320, 8 * 8 * 640, 4 * 4 * 1280, 2 * 2 * 1280)]]
    tab = np.ones((3, 1, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="`t2i_adapter` goes with an engine built with t2i_units=U"):
        eng.prepare({}, None, None, None)
    with pytest.raises(ValueError, match="`t2i_adapter` goes with an engine built with t2i_units=U"):
        plain.prepare({}, None, None, None, t2i_adapter=(feats, tab))
    with pytest.raises(ValueError, match="adapter features of .* and a table of shape"):
        eng.prepare({}, None, None, None, t2i_adapter=([feats[0][:3] + [torch.zeros(8, dtype=torch.bfloat16)]], tab))
    with pytest.raises(ValueError, match=r"a table of shape \(2, 1, 4\)"):
        eng.prepare({}, None, None, None, t2i_adapter=(feats, tab[:2]))


def test_engine_key_of_a_job_without_an_adapter_is_the_parent_s():
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    class Net:
        weights_version = 1

    sd = StableDiffusionBase(64, 64)
    sd.diffusion_model = Net()
    args = (1, 77, 77, 4, 7.5, 0.7, False)
    plain = sd._engine_key(*args)
    # the parent commit's key of this job, written out: (B, tc, tu, steps, g, phi, control, streams, inpaint, tcd, (unet version,), epoch, sampler)
    from minsdtf_amd import engine

    assert plain == (1, 77, 77, 4, 7.5, 0.7, False, None, False, False, (1,), engine.GN_EPOCH, None)
    assert sd._engine_key(*args, t2i_units=None) == plain
    one = sd._engine_key(*args, t2i_units=2)
    assert one[:len(plain)] == plain and one[len(plain):] == (("t2i", 2),)
    assert sd._engine_key(*args, ip_tokens=4, t2i_units=1)[len(plain):] == (("ip", 4), ("t2i", 1))


def test_plan_digests_are_the_parent_commit_s():
    """tools/plan_digest.py on this tree against its output on the parent commit (tests/golden/plan_digests_before_t2i.txt): no
    existing job's plan moved a launch."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import plan_digest as PD
    finally:
        sys.path.pop(0)
    want = [ln.split() for ln in open(os.path.join(ROOT, "tests", "golden", "plan_digests_before_t2i.txt")).read().splitlines() if ln.strip()]
    kinds = PD.cpu_kinds() + PD.model_kinds()
    assert len(want) == len(kinds) == 27
    for (kind, build), line in zip(kinds, want):
        n, sha = PD.record(build)
        assert " ".join(line[:-2]) == kind and (str(n), sha) == (line[-2], line[-1]), kind


# ------------------------------------------------------------------------------------------------- generate_image, no device
def _adapter(cin=3, seed=0):
    """A models.T2IAdapter on the CPU whose `features` is the float64 statement, rounded: counts its runs like the real one."""
    from minsdtf_amd.models import T2IAdapter

    m = T2IAdapter.synthetic(seed, cin, device=CPU)
    m._build = lambda H, W: _HostPlan(m, H, W)
    return m


class _HostPlan:
    def __init__(self, m, H, W):
        self.m = m
        self.io = {"picture": torch.zeros(1, H, W, m.in_channels)}

    def run(self):
        from minsdtf_amd import t2iadapter as T

        for l, f in enumerate(T.forward_host(self.m.state, self.io["picture"].numpy())):
            self.io[f"feature.{l}"] = torch.from_numpy(f).to(torch.bfloat16)


def test_features_are_cached_by_pixels_size_and_weights():
    from minsdtf_amd import t2iadapter as T

    m = _adapter()
    a, b = np.full((1, 64, 64, 3), 0.25, dtype=np.float32), np.full((1, 64, 64, 3), 0.5, dtype=np.float32)
    fa = m.features(a)
    assert m.runs == 1 and [tuple(f.shape) for f in fa] == [(1, 8, 8, 320), (1, 4, 4, 640), (1, 2, 2, 1280), (1, 1, 1, 1280)]
    assert all(f.dtype == torch.bfloat16 for f in fa)
    assert all(torch.equal(x, y) for x, y in zip(m.features(a.copy()), fa)) and m.runs == 1      # the same pixels: not run again
    fa[0].zero_()                                                                                  # the caller owns what it got:
    assert float(m.features(a)[0].float().abs().max()) > 0 and m.runs == 1                         # the kept features are untouched
    fa = m.features(a)
    fb = m.features(b)
    assert m.runs == 2 and not torch.equal(fb[0], fa[0])
    m.features(np.full((1, 64, 128, 3), 0.5, dtype=np.float32))
    assert m.runs == 3                                                                             # another size
    m.features(a)
    m.set_state(T.synthetic_state(9, 3))
    fc = m.features(a)
    assert m.runs == 5 and m.weights_version == 2 and not torch.equal(fc[0], fa[0])                # other weights
    out = m.predict_on_batch(a[0])
    assert m.runs == 5 and [o.dtype for o in out] == [np.float32] * 4 and out[0].shape == (1, 8, 8, 320)
    ref = T.forward_host(m.state, a)
    for o, r in zip(out, ref):
        assert float(np.abs(o - r).max()) <= 2.0 ** -8 * float(np.abs(r).max())                    # one bf16 rounding
    with pytest.raises(ValueError, match="one picture per job"):
        m.features(np.zeros((2, 64, 64, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="multiples of 64"):
        m.features(np.zeros((1, 64, 72, 3), dtype=np.float32))


def test_generate_image_refusals_and_route():
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    ctx = np.zeros((77, 768), dtype=np.float32)
    sd = StableDiffusionBase(64, 64)   # (no models behind it: anything that reaches a model fails another way)
    sd.unconditional_context = ctx
    m = _adapter()
    spec = dict(image=PIC, model=m)
    kw = dict(batch_size=1, num_steps=3, seed=0)
    mask = np.ones((64, 64), dtype=np.float32)
    kinds = dict(pag=dict(scale=3.0), regions=dict(regions=[dict(prompt=ctx, mask=mask)]), tiled=dict(size=(64, 128)), hires=dict(scale=2.0),
                 sag=dict(scale=0.75), hypertile=dict(tile=64), reference_only=dict(latent=np.zeros((1, 8, 8, 4), dtype=np.float32)),
                 control_net_image=np.zeros((64, 64, 3), dtype=np.float32))
    for kind, val in kinds.items():
        for fn in (sd.generate_image, sd.text_to_image):
            with pytest.raises(ValueError, match=f"^t2i_adapter: .*cannot be combined with {kind}$"):
                fn(ctx, t2i_adapter=spec, **{kind: val}, **kw)
    with pytest.raises(ValueError, match="^t2i_adapter: .*cannot be combined with pag, sag$"):
        sd.generate_image(ctx, t2i_adapter=spec, sag=dict(scale=0.75), pag=dict(scale=3.0), **kw)
    sd.denoise_streams = 2
    with pytest.raises(ValueError, match="^t2i_adapter: .*cannot be combined with denoise_streams = 2$"):
        sd.generate_image(ctx, t2i_adapter=spec, **kw)
    sd.denoise_streams = None
    with pytest.raises(ValueError, match="^t2i_adapter: unit 0: weight"):
        sd.generate_image(ctx, t2i_adapter=dict(spec, weight=-1.0), **kw)
    with pytest.raises(ValueError, match=r"^t2i_adapter: a picture of shape \(64, 64, 1\) \(1 channel\(s\)\) for an adapter of 3 input"):
        sd.generate_image(ctx, t2i_adapter=dict(spec, image=np.zeros((64, 64))), **kw)
    with pytest.raises(ValueError, match="^t2i_adapter: model is int"):
        sd.generate_image(ctx, t2i_adapter=dict(image=PIC, model=3), **kw)
    with pytest.raises(ValueError, match="^t2i_adapter: a 72 x 64 job"):
        StableDiffusionBase(72, 64).generate_image(ctx, t2i_adapter=spec, **kw)
    assert not sd._engines and m.runs == 0
    # the route: the picture is resized to the job's size and the features reach the engine; the engine is asked for by its unit count
    seen = {}

    def denoise_pass(u, c, start, steps, g, phi, first, count, callback, engine_opts, extras):
        seen.update(opts=engine_opts, t2i=extras["t2i_adapter"])
        raise RuntimeError("reached the engine")

    sd._denoise_pass = denoise_pass
    sd.device = CPU
    units = [dict(image=np.full((32, 48, 3), 100, dtype=np.uint8), model=m, weight=[1, 0.5, 0.25, 0], end=0.75), dict(image=PIC, model=m, weight=2.0)]
    with pytest.raises(RuntimeError, match="reached the engine"):
        sd.generate_image(ctx, t2i_adapter=units, **kw)
    assert seen["opts"] == dict(t2i_units=2) and m.runs == 2
    feats, tab = seen["t2i"]
    assert len(feats) == 2 and [tuple(f.shape) for f in feats[0]] == [(1, 8, 8, 320), (1, 4, 4, 640), (1, 2, 2, 1280), (1, 1, 1, 1280)]
    np.testing.assert_array_equal(np.asarray(tab), __import__("minsdtf_amd.t2iadapter", fromlist=["table"]).table(units, 3))
    # weight 0 (an all-zero table) is the plain job on the plain engine: no adapter run, no t2i option
    seen.clear()
    sd._denoise_pass = lambda u, c, start, steps, g, phi, first, count, callback, engine_opts, extras: (_ for _ in ()).throw(
        RuntimeError(f"plain {engine_opts} {extras.get('t2i_adapter')}"))
    with pytest.raises(RuntimeError, match=r"plain \{\} None"):
        sd.generate_image(ctx, t2i_adapter=dict(spec, weight=0.0), **kw)
    with pytest.raises(RuntimeError, match=r"plain \{\} None"):
        sd.generate_image(ctx, t2i_adapter=dict(spec, start=1.0), **kw)
    assert m.runs == 2
    for fn in (sd.text_to_image, sd.image_to_image, sd.inpaint, sd.generate_image):
        assert "t2i_adapter" in fn.__doc__


def test_committed_fixtures_are_told_apart_from_the_plain_job():
    for size, units in ((128, 1), (256, 2)):
        path = os.path.join(ROOT, "tests", "golden", f"t2i_adapter_{size}.npz")
        assert os.path.exists(path) and os.path.getsize(path) <= 1 << 20, path
        z = np.load(path)
        assert z["latent"].shape == (1, size // 8, size // 8, 4) and float(z["plain_psnr"]) < 35.0
        assert (int(z["steps"]), int(z["units"]), float(z["guidance"])) == (4, units, 7.5)
        assert z["site_weights"].shape == (units, 4)
    z = np.load(os.path.join(ROOT, "tests", "golden", "t2i_adapter_128.npz"))
    assert float(z["end"][0]) == 0.75
    z = np.load(os.path.join(ROOT, "tests", "golden", "t2i_adapter_256.npz"))
    assert len(set(z["site_weights"][0].tolist())) == 4 and list(z["in_channels"]) == [3, 1]
