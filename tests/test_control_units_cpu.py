"""ControlNet units (minsdtf_amd/control.py, include/minsdtf_hip_control.h) without a device: the unit description and every
ValueError, the per-call table against rows written out by hand, the fourth library's ABI, its argument errors, what an engine
built on the stand-ins of tests/_layer_walk.py records for 0 .. 3 units, the engine key, and the refusals that stay what they are."""
import ctypes
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

import _extents_control as XC
import _layer_walk as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 16


# ------------------------------------------------------------------------------------------------------------ the description
def test_parse_defaults_and_forms():
    from minsdtf_amd import control as C

    assert C.MODES == ("balanced", "prompt", "control") and C.MAX_UNITS == 3
    assert C.parse(None) is None
    (u,) = C.parse({})
    assert u == C.Resolved((1.0,) * 13, 0.0, 1.0, "balanced")
    assert C.parse(C.ControlUnit()) == (u,) == C.parse([{}]) == C.parse((u,))
    w13 = [0.1 * k for k in range(13)]
    (v,) = C.parse(dict(weight=w13, start=0.25, end=0.75, mode="prompt"))
    assert v.weight == tuple(float(x) for x in w13) and (v.start, v.end, v.mode) == (0.25, 0.75, "prompt")
    img = np.zeros((8, 8, 3), dtype=np.float32)
    nets = (object(), object())
    a, b, c = C.parse([dict(weight=0), dict(image=img, path="x.h5"), C.ControlUnit(image=img, models=list(nets), mode="control")])
    assert a.weight == (0.0,) * 13 and b.path == "x.h5" and b.models is None and b.image is img
    assert c.models == nets and c.path is None and c.mode == "control"


@pytest.mark.parametrize("bad, word", [
    ([], "0 units"), ([{}] * 4, "4 units"), ("balanced", "unit 0 is str"), (dict(strength=1.0), "unknown field"),
    (dict(weight=-0.1), "weight"), (dict(weight=float("nan")), "weight"), (dict(weight=float("inf")), "weight"), (dict(weight=True), "weight"),
    (dict(weight="much"), "weight"), (dict(weight=[1.0] * 12), "12 entries"), (dict(weight=[1.0] * 12 + [-1.0]), r"weight\[12\]"),
    (dict(start=-0.1), "start"), (dict(end=1.5), "end"), (dict(start=0.6, end=0.5), "start = 0.6 > end = 0.5"), (dict(start=None), "start"),
    (dict(mode="guess"), "mode"), (dict(mode=None), "mode"), (dict(image=np.zeros((8, 8, 3))), "unit 0 is the pipeline's own"),
    (dict(path="x.h5"), "unit 0 is the pipeline's own"), (dict(models=(1, 2)), "unit 0 is the pipeline's own"),
    ([{}, {}], "unit 1 needs its own `image`"), ([{}, dict(image=1, path="p", models=(1, 2))], "should not both"),
    ([{}, dict(image=1, models=(1,))], r"must be \(ControlNet, HintNet\)"), ([{}, dict(image=1), dict(image=1, weight=-1)], "unit 2: weight"),
])
def test_parse_value_errors(bad, word):
    from minsdtf_amd import control as C

    with pytest.raises(ValueError, match="^control: .*" + word):
        C.parse(bad)


def test_table_against_rows_written_by_hand():
    from minsdtf_amd import control as C

    f32 = lambda x: float(np.float32(x))
    # one unit, 4 steps: end = 0.5 keeps rows 0 and 1 ((i + 1) / 4 <= 0.5), "prompt" scales tap k by 0.825 ** (12 - k) on both halves
    t = C.table(dict(weight=0.6, end=0.5, mode="prompt"), 4)
    assert t.shape == (4, 1, 13, 2) and t.dtype == np.float32
    row = [[f32(0.6 * 0.825 ** (12 - k))] * 2 for k in range(13)]
    assert t[0, 0].tolist() == row and t[1, 0].tolist() == row and not t[2:].any()
    assert t[0, 0, 12].tolist() == [f32(0.6)] * 2 and t[0, 0, 0, 0] == np.float32(0.6 * 0.825 ** 12)
    # an end that falls between two steps: 5 steps, end = 0.5 -> rows 0, 1 ((2 + 1) / 5 = 0.6 > 0.5); start = 0.3 -> rows from 2 (1 / 5 < 0.3)
    assert [C.keep(i, 5, 0.0, 0.5) for i in range(5)] == [1.0, 1.0, 0.0, 0.0, 0.0]
    assert [C.keep(i, 5, 0.3, 1.0) for i in range(5)] == [0.0, 0.0, 1.0, 1.0, 1.0]
    assert [C.keep(i, 5, 0.3, 0.5) for i in range(5)] == [0.0] * 5
    assert [C.keep(i, 4, 0.25, 0.75) for i in range(4)] == [0.0, 1.0, 1.0, 0.0]
    # two units: "control" mode's zero column, per-tap weights, "balanced" at a later start
    w13 = [0.25 * k for k in range(13)]
    t = C.table([dict(weight=w13, mode="control"), dict(weight=0.7, start=0.25, image=1)], 4)
    assert t.shape == (4, 2, 13, 2)
    for i in range(4):
        assert not t[i, 0, :, 0].any()
        assert t[i, 0, :, 1].tolist() == [f32(w13[k] * 0.825 ** (12 - k)) for k in range(13)]
        assert t[i, 1].tolist() == [[f32(0.7) if i >= 1 else 0.0] * 2] * 13
    ones = C.table({}, 3)
    assert ones.shape == (3, 1, 13, 2) and (ones == 1.0).all()
    with pytest.raises(ValueError, match="num_steps"):
        C.table({}, 0)


def test_scale_host_sums_in_unit_order_and_skips_zero_scales():
    from minsdtf_amd import control as C

    rng = np.random.default_rng(0)
    r0 = [rng.standard_normal((2, 3)).astype(np.float32) for _ in range(13)]
    r1 = [np.full((2, 3), np.nan, dtype=np.float32) for _ in range(13)]
    row = np.zeros((2, 13), dtype=np.float32)
    row[0] = np.linspace(0.5, 1.5, 13)
    out = C.scale_host([r0, r1], row)
    assert len(out) == 13 and all(np.array_equal(o, np.float32(s) * a) for o, s, a in zip(out, row[0], r0))
    row[1, 3] = 2.0
    out = C.scale_host([r0, r0], row)
    np.testing.assert_array_equal(out[3], np.float32(row[0, 3]) * r0[3] + np.float32(2.0) * r0[3])


# -------------------------------------------------------------------------------------------------------------- the C ABI
def test_library_exports_its_header_and_the_others_are_untouched():
    from minsdtf_amd import _lib, _lib_control, _lib_dynthresh, _lib_ext

    assert os.path.exists(_lib_control.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    header = open(os.path.join(ROOT, "include", "minsdtf_hip_control.h")).read()
    declared = set(re.findall(r"^MSDC_API\s+(?:int|const char\*)\s+(msdc_\w+)\s*\(", header, flags=re.M))
    assert declared == set(_lib_control.SYMBOLS) == {"msdc_abi_version", "msdc_last_error", "msdc_control_combine"}
    assert not re.search(r"^(?:int|const char\*)\s+msdc_\w+\s*\(", header, flags=re.M), "a declaration without MSDC_API"
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib_control.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert exported == declared, sorted(exported ^ declared)
    lib = _lib_control.load()
    assert lib.msdc_abi_version() == _lib_control.ABI_VERSION == int(re.search(r"#define MSDC_ABI_VERSION (\d+)", header).group(1))
    for name, value in (("MSDC_TAPS", _lib_control.TAPS), ("MSDC_MAX_UNITS", _lib_control.MAX_UNITS), ("MSDC_CHUNK", _lib_control.CHUNK)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value
    emap = open(os.path.join(ROOT, "minsdtf_amd", "csrc", "control", "exports_control.map")).read()
    assert set(re.findall(r"\b(msdc_\w+);", emap)) == declared and "*;" in emap and "msdc_*" not in emap
    for other in (_lib, _lib_ext, _lib_dynthresh):
        table = subprocess.check_output(["nm", "-D", "--defined-only", other.LIB_PATH], text=True)
        assert "msdc_" not in table and not any(n.startswith("msdc_") for n in other.SYMBOLS)


def test_struct_layout_matches_the_header():
    from minsdtf_amd import _lib_control

    cls, struct = _lib_control.MsdcControlCombine, "MsdcControlCombine"
    fields = [n for n, _t in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "minsdtf_hip_control.h"\nint main(){printf("%zu", sizeof(' + struct + '));' + \
        "".join(f'printf(" %zu", offsetof({struct}, {f}));' for f in fields) + \
        f'printf(" %zu %zu", sizeof((({struct}*)0)->resid[0]), sizeof((({struct}*)0)->chunk_prefix));' + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields] + [13 * 8, 14 * 4]


BASE = 1 << 24   # (addresses are only compared and checked for alignment: every bad call returns before a launch)
COUNTS = [8 * 8 * 320] * 3 + [4 * 4 * 320] + [4 * 4 * 640] * 2 + [2 * 2 * 640] + [2 * 2 * 1280] * 2 + [1280] * 4   # an 8 x 8 latent's taps


def _call(over):
    """The argument block of a good launch with `over` laid over it; a tuple key (field, index, ...) names one entry of an array."""
    from minsdtf_amd import _lib_control, ops

    over = dict(over)
    units, rows, counts, prefix = over.pop("units", 2), over.pop("rows", 2), over.pop("counts", COUNTS), over.pop("prefix", None)

    s = _lib_control.MsdcControlCombine()
    for k in range(13):
        s.skip[k] = BASE + k * (1 << 20)
        s.count[k] = counts[k]
        for n in range(3):
            s.resid[n][k] = 2 * BASE + (n * 13 + k) * (1 << 20)
    s.chunk_prefix[:] = ops.control_chunk_prefix(counts) if prefix is None else prefix
    s.scales, s.step_ptr = 8 * BASE, 9 * BASE
    s.rows, s.rows_u, s.units, s.num_steps = rows, 1, units, 4
    for k, v in over.items():
        if isinstance(k, tuple):
            arr = getattr(s, k[0])
            for i in k[1:-1]:
                arr = arr[i]
            arr[k[-1]] = v
        else:
            setattr(s, k, v)
    return s


def _counts(k, v):
    c = list(COUNTS)
    c[k] = v
    return c


BAD = [dict(units=0), dict(units=4), dict(units=-1), dict(rows=0), dict(rows=65536), dict(rows_u=3), dict(rows_u=-1), dict(num_steps=0),
       dict(scales=None), dict(scales=8 * BASE + 8), dict(step_ptr=9 * BASE + 2),
       {("skip", 0): None}, {("skip", 12): None}, {("skip", 5): BASE + 5 * (1 << 20) + 8}, {("resid", 0, 0): None}, {("resid", 1, 12): None},
       {("resid", 1, 3): 2 * BASE + 8}, {"units": 3, ("resid", 2, 7): None},
       dict(counts=_counts(4, 4 * 4 * 640 + 4)), dict(counts=_counts(12, 0)), dict(counts=_counts(0, -8)), dict(counts=_counts(9, 1284)),
       dict(prefix=[1] + [0] * 13), dict(prefix=[0] * 14), dict(prefix=list(range(14))),
       {("skip", 2): 8 * BASE}, {("skip", 2): 9 * BASE - 16}, {("skip", 1): 2 * BASE + (13 + 1) * (1 << 20)}]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}={v if not isinstance(v, list) else len(v)}" for k, v in b.items())[:60])
def test_argument_errors_without_a_device(bad):
    from minsdtf_amd import _lib_control

    lib = _lib_control.load()
    assert lib.msdc_control_combine(ctypes.byref(_call(bad)), None) == -1, bad   # MSD_E_ARG
    assert b"control_combine" in lib.msdc_last_error()


def test_null_struct_and_the_list_lengths():
    from minsdtf_amd import _lib_control, ops

    lib = _lib_control.load()
    assert lib.msdc_control_combine(None, None) == -1 and b"control_combine: null" in lib.msdc_last_error()
    # a unit behind `units` may hold anything: its pointers are not read
    assert ops.control_chunk_prefix(COUNTS) == [0, 10, 20, 30, 33, 38, 43, 45, 48, 51, 52, 53, 54, 55]
    good = dict(skips=[BASE] * 13, resid=[[BASE] * 13], counts=COUNTS, scales=BASE, rows=2, rows_u=1, num_steps=3)
    for bad in (dict(skips=[BASE] * 12), dict(counts=COUNTS[:12]), dict(resid=[]), dict(resid=[[BASE] * 13] * 4), dict(resid=[[BASE] * 12])):
        with pytest.raises(ValueError, match="control_combine"):
            ops.control_combine(**dict(good, **bad))


# ------------------------------------------------------------------------------------------------------------------ engines
class _Tensor(LW._Tensor):
    dtype = torch.bfloat16   # (emit_time_embedding reads it)


class _Weights(LW._AnyWeights):
    def __missing__(self, k):
        return _Tensor()


def _net(**kw):
    return types.SimpleNamespace(_require_weights=lambda: None, device=torch.device("cpu"), _W=_Weights(), **kw)


def _engine(monkeypatch, units, streams=None, overlap=False, t_uncond=77, further=None, **kw):
    """A DenoiseEngine with a ControlNet on the stand-ins, its Plan.rec calls as Rec records, per plan in recording order."""
    import minsdtf_amd.stable_diffusion as sdm
    from minsdtf_amd import engine

    monkeypatch.setattr(sdm, "CONTROLNET_OVERLAP", overlap)
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: object())   # (the side stream of a two-stream / overlapped engine)
    recs = []
    orig = engine.Plan.rec

    def flat(k):   # (the list operands of the combine as "skips.k" / "resid.n.k", in the state they have when the launch is recorded)
        for n, v in k.items():
            if n == "skips":
                yield from ((f"skips.{i}", b) for i, b in enumerate(v))
            elif n == "resid":
                yield from ((f"resid.{u}.{i}", b) for u, rs in enumerate(v) for i, b in enumerate(rs))
            else:
                yield n, v

    def rec(self, f, **k):
        recs.append(LW.Rec(f.__name__, k.get("name", ""), k, {n: LW._operand(v) for n, v in flat(k) if LW._operand(v) is not None}))
        return orig(self, f, **k)

    monkeypatch.setattr(engine.Plan, "rec", rec)
    if units:
        kw.update(control_units=units, control_nets=[(_net(), _net()) for _ in range(units - 1)] if further is None else further)
    eng = sdm.DenoiseEngine(_net(h=SIZE, w=SIZE), 2, 77, t_uncond, 3, 7.5, 0.7, control_net=_net(), hint_net=_net(), streams=streams, **kw)
    monkeypatch.setattr(engine.Plan, "rec", orig)
    return eng, recs


def _zero(recs):
    return [r for r in recs if r.op == "conv_gemm" and "zero_convs." in r.name]


@pytest.mark.parametrize("form", ["inline", "two_streams", "two_passes", "overlap"])
@pytest.mark.parametrize("units", [1, 2, 3])
def test_engine_records_the_fp32_zero_convs_and_one_combine_per_pass(monkeypatch, units, form):
    from minsdtf_amd import ops

    kw = dict(streams=2 if form == "two_streams" else None, overlap=form == "overlap", t_uncond=154 if form == "two_passes" else 77)
    base, base_recs = _engine(monkeypatch, 0, **kw)
    eng, recs = _engine(monkeypatch, units, **kw)
    passes = 1 if form in ("inline", "overlap") else 2
    assert len(eng.passes) == passes and eng.dual == (form == "two_streams") and (eng.cn_plan is not None) == (form == "overlap")
    # the job without units: 13 fused zero convs per pass, bf16 with the skip as residual and output, no combine
    z0 = _zero(base_recs)
    assert len(z0) == 13 * passes and not any(r.op == "control_combine" for r in base_recs)
    assert all(r.kw["residual"] is r.kw["out"] and r.kw["out_dtype"] == ops.OUT_BF16 for r in z0)
    # with units: 13 N per pass, fp32, no residual, each with the tile and split-K configuration of the fused one of its shape
    z = _zero(recs)
    combines = [r for r in recs if r.op == "control_combine"]
    assert len(z) == 13 * units * passes and len(combines) == passes
    assert all(r.kw["residual"] is None and r.kw["out_dtype"] == ops.OUT_F32 for r in z)
    cfg = lambda r: tuple(r.kw[k] for k in ("batch", "h_in", "w_in", "c0", "N", "ksize", "tile_m", "tile_n", "splitk", "stages", "w_layout"))
    per_pass = len(z) // passes
    for p in range(passes):
        for n in range(units):
            mine = z[p * per_pass + n * 13:p * per_pass + (n + 1) * 13]
            assert [cfg(r) for r in mine] == [cfg(r) for r in z0[p * 13:(p + 1) * 13]]
            assert [r.name for r in mine] == [(f"unit{n}." if n else "") + f"zero_convs.{k}" for k in range(13)]
    # the combine: behind the pass's last zero conv, in front of the up path; the rows, the u rows and the table of the engine
    B = 2
    rows = {"inline": [(2 * B, B)], "overlap": [(2 * B, B)], "two_streams": [(B, B), (B, 0)], "two_passes": [(B, B), (B, 0)]}[form]
    assert tuple(eng.cn_scales.shape) == (3, units, 13, 2) and eng.cn_scales.dtype == torch.float32 and base.cn_scales is None
    for c, (nb, nu) in zip(combines, rows):
        i = recs.index(c)
        assert recs[i - 1] in z and recs[i + 1].name.startswith("up_blocks.0.resnets.0")
        assert (c.kw["rows"], c.kw["rows_u"], c.kw["num_steps"]) == (nb, nu, 3) and c.kw["scales"] is eng.cn_scales
        assert c.kw["step_ptr"] is eng.step_ptr and len(c.kw["resid"]) == units
        levels = [(SIZE >> lv) ** 2 * ch for lv, ch in zip((0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3), (320,) * 4 + (640,) * 3 + (1280,) * 6)]
        assert c.kw["counts"] == levels
        # every operand inside its live buffer (tests/_extents_control.py), the residuals the outputs of this pass's zero convs
        ext = XC.control_combine(rows=nb, counts=c.kw["counts"], units=units, num_steps=3, step_ptr=True)
        mine = [r for r in z if recs.index(r) < i][-13 * units:]
        assert set(c.operands) == set(ext) - {"scales", "step_ptr"}   # (the table and the counter: the engine's tensors)
        for name, o in c.operands.items():
            assert not o.freed and ext[name][0] <= o.avail, name
        spans = sorted((o.offset, o.offset + ext[name][0]) for name, o in c.operands.items())
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "two operands of the combine overlap"
        for k in range(13):
            for n in range(units):
                assert c.kw["resid"][n][k] is mine[n * 13 + k].kw["out"]
        assert ext["scales"][0] == eng.cn_scales.numel() * 4
    # nothing else moves: without the combine(s), the launch names of one unit are the plain ControlNet job's
    if units == 1:
        assert [r.name for r in recs if r.op != "control_combine"] == [r.name for r in base_recs]
    assert len(eng.calls) == len([r for r in recs if r not in []]) - len(eng.prep.calls) - len(eng.prep_t.calls)


def test_units_on_one_controlnet_share_its_table_and_context(monkeypatch):
    """A further unit on the ControlNet of a unit in front of it (path=None: another picture, the same weights) records its own
    HintNet and encoder, and no second time-embedding table or context K/V."""
    own, _ = _engine(monkeypatch, 2)
    import minsdtf_amd.stable_diffusion as sdm

    cn, hn = _net(), _net()
    monkeypatch.setattr(sdm, "CONTROLNET_OVERLAP", False)
    shared = sdm.DenoiseEngine(_net(h=SIZE, w=SIZE), 2, 77, 77, 3, 7.5, 0.7, control_net=cn, hint_net=hn, control_units=2,
                               control_nets=[(cn, hn)])
    one, _ = _engine(monkeypatch, 1)
    assert len(shared.prep_t.calls) == len(one.prep_t.calls) < len(own.prep_t.calls)
    assert len(one.prep.calls) < len(shared.prep.calls) < len(own.prep.calls)
    assert len(shared.calls) == len(own.calls)


def test_engine_checks():
    import minsdtf_amd.stable_diffusion as sdm
    from minsdtf_amd.jobopts import REFUSED, EngineOptions

    assert EngineOptions.of(control_units=2).key() == (("control", 2),)
    assert EngineOptions.of(control_units=None) == EngineOptions.of(control_units=0) == EngineOptions() and EngineOptions().key() == ()
    assert EngineOptions.of(sag=True, control_units=1, sampler="euler_a").key() == (("sag",), ("control", 1))
    assert "control" not in REFUSED and "control_units" not in REFUSED
    unet = _net(h=SIZE, w=SIZE)
    for n in (4, -1):
        with pytest.raises(ValueError, match="^control: "):
            sdm.DenoiseEngine(unet, 2, 77, 77, 3, 7.5, 0.7, control_net=_net(), hint_net=_net(), control_units=n)
    with pytest.raises(ValueError, match="^control: "):
        sdm.DenoiseEngine(unet, 2, 77, 77, 3, 7.5, 0.7, control_units=1)   # (no ControlNet)
    with pytest.raises(ValueError, match="^control: .*1 further"):
        sdm.DenoiseEngine(unet, 2, 77, 77, 3, 7.5, 0.7, control_net=_net(), hint_net=_net(), control_units=2)
    with pytest.raises(ValueError, match="^control: .*0 further"):
        sdm.DenoiseEngine(unet, 2, 77, 77, 3, 7.5, 0.7, control_net=_net(), hint_net=_net(), control_nets=[(_net(), _net())])
    # whatever refuses a ControlNet refuses it with units too, under its own name
    for kind, opts in (("pag", dict(pag=("mid_block.attentions.0",))), ("sag", dict(sag=True)), ("dynamic_threshold", dict(dynthresh=True)),
                       ("regions", dict(regions=2)), ("hypertile", dict(hypertile=(2, 2, 0))), ("reference_only", dict(reference=("mid_block.attentions.0",)))):
        with pytest.raises(ValueError, match=f"^{kind}: .*ControlNet"):
            sdm.DenoiseEngine(unet, 2, 77, 77, 3, 7.5, 0.7, control_net=_net(), hint_net=_net(), control_units=1, **opts)


def test_prepare_carries_the_goes_with_check(monkeypatch):
    eng, _ = _engine(monkeypatch, 2)
    plain, _ = _engine(monkeypatch, 0)
    with pytest.raises(ValueError, match="`control` goes with an engine built with control_units=N"):
        eng.prepare({}, None, None, None)
    with pytest.raises(ValueError, match="`control` goes with an engine built with control_units=N"):
        plain.prepare({}, None, None, None, control=(np.ones((3, 1, 13, 2), dtype=np.float32), []))
    with pytest.raises(ValueError, match="control table of shape"):
        eng.prepare({}, None, None, None, control=(np.ones((3, 1, 13, 2), dtype=np.float32), [None]))
    with pytest.raises(ValueError, match="with 0 further hint"):
        eng.prepare({}, None, None, None, control=(np.ones((3, 2, 13, 2), dtype=np.float32), []))


def test_engine_key_holds_the_number_of_units_and_the_further_models():
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    class Net:
        weights_version = 1

    sd = StableDiffusionBase(64, 64)
    sd.diffusion_model, sd.control_net, sd.hint_net = Net(), Net(), Net()
    args = (1, 77, 77, 4, 7.5, 0.7, True)
    plain = sd._engine_key(*args)
    assert sd._engine_key(*args, control_units=None) == plain == sd._engine_key(*args, control_nets=())
    one = sd._engine_key(*args, control_units=1)
    assert one[:len(plain)] == plain and one[len(plain):] == (("control", 1),)
    cn, hn = Net(), Net()
    two = sd._engine_key(*args, control_units=2, control_nets=((cn, hn),))
    assert two[-1] == ("control", 2) and two != sd._engine_key(*args, control_units=2, control_nets=((Net(), hn),))
    cn.weights_version = 2
    assert two != sd._engine_key(*args, control_units=2, control_nets=((cn, hn),))


# ------------------------------------------------------------------------------------------------- generate_image, no device
def test_generate_image_refusals_keep_their_names():
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    ctx = np.zeros((77, 768), dtype=np.float32)
    img = np.zeros((64, 64, 3), dtype=np.float32)
    sd = StableDiffusionBase(64, 64)   # (no models behind it: anything that reaches a model fails another way)
    kw = dict(batch_size=1, num_steps=3, seed=0)
    with pytest.raises(ValueError, match="^control: .*control_net_image"):
        sd.generate_image(ctx, control=dict(weight=0.5), **kw)
    with pytest.raises(ValueError, match="^control: .*control_net_image"):
        sd.text_to_image(ctx, control=[{}], **kw)
    with pytest.raises(ValueError, match="^control: unit 0: mode"):
        sd.generate_image(ctx, control_net_image=img, control=dict(mode="guess"), **kw)
    mask = np.ones((64, 64), dtype=np.float32)
    kinds = dict(pag=dict(scale=3.0), regions=dict(regions=[dict(prompt=ctx, mask=mask)]), tiled=dict(size=(64, 128)),
                 hires=dict(scale=2.0), sag=dict(scale=0.75), hypertile=dict(tile=64), reference_only=dict(latent=np.zeros((1, 8, 8, 4), dtype=np.float32)),
                 dynamic_threshold=dict(mimic_scale=5.0))
    for kind, spec in kinds.items():
        with pytest.raises(ValueError, match=f"^{kind} is .*it cannot be combined with.*control_net_image"):
            sd.generate_image(ctx, control_net_image=img, control=dict(weight=0.5), **{kind: spec}, **kw)
    assert not sd._engines
    for fn in (sd.text_to_image, sd.image_to_image, sd.inpaint, sd.generate_image):
        assert "control" in fn.__doc__
