"""A job's engine options (minsdtf_amd/jobopts.py): every pair the refusal table excludes is refused by a directly constructed
DenoiseEngine, under the kind's own name; every pair it admits builds an engine that records launches; an option nobody knows
is a TypeError.  The engines are built on the CPU from the stand-ins of tests/_layer_walk.py: nothing is launched."""
import types

import pytest
import torch

import _layer_walk as LW

MID = "mid_block.attentions.0"
SIZE = 16   # latent rows and columns: the smallest HyperTile takes (2 x 2 windows of 8 x 8 tokens)


class _Tensor(LW._Tensor):
    dtype = torch.bfloat16   # (emit_time_embedding reads it)


class _Weights(LW._AnyWeights):
    def __missing__(self, k):
        return _Tensor()


def _net(**kw):
    return types.SimpleNamespace(_require_weights=lambda: None, device=torch.device("cpu"), _W=_Weights(), **kw)


def _geometry():
    from minsdtf_amd import tiled

    return tiled.parse(dict(size=(8 * SIZE, 16 * SIZE)), 8 * SIZE, 8 * SIZE)


# how an engine sees each job kind of the refusal table (hires has no engine form) ...
def _kind_options():
    return {"regions": dict(regions=2), "tiled": dict(tiled=_geometry()), "pag": dict(pag=(MID,)), "hypertile": dict(hypertile=(2, 2, 0)),
            "reference_only": dict(reference=(MID,)), "sag": dict(sag=True), "dynamic_threshold": dict(dynthresh=True)}


# ... and each argument or state a row may name (reference_image, hires and host_loop=True have none)
def _excluded_options():
    return dict(_kind_options(), control_net_image=dict(control_net=_net(), hint_net=_net()), inpaint_mask=dict(inpaint=True),
                **{"a TCD pipeline (active_tcd=True)": dict(tcd=True), "denoise_streams = 2": dict(streams=2)})


def _refused():
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    return StableDiffusionBase._REFUSED


def _pairs():
    """(kind, excluded argument or state) over the table, those with an engine form."""
    seen = _excluded_options()
    return [(kind, x) for kind in _kind_options() for x in _refused()[kind][1] + _refused()[kind][2] if x in seen]


def _construct(**kw):
    from minsdtf_amd.stable_diffusion import DenoiseEngine

    B = kw["tiled"].views if kw.get("tiled") is not None else 2
    return DenoiseEngine(_net(h=SIZE, w=SIZE), B, 77, 77, 3, 7.5, 0.7, **kw)


def test_the_table_has_forty_pairs_an_engine_can_see():
    assert len(_pairs()) == 40 and len(set(_pairs())) == 40
    assert set(_refused()) - set(_kind_options()) == {"hires"}


@pytest.mark.parametrize("kind, excluded", _pairs())
def test_engine_refuses_every_excluded_pair_under_the_kinds_name(kind, excluded):
    with pytest.raises(ValueError) as e:
        _construct(**_kind_options()[kind], **_excluded_options()[excluded])
    assert str(e.value).startswith(kind + ":"), str(e.value)


def _admitted():
    """Two kinds where neither row names the other, and a kind with the TCD or the inpaint state where its row does not name it."""
    kinds, rows = list(_kind_options()), _refused()
    out = [(a, b) for i, a in enumerate(kinds) for b in kinds[i + 1:] if b not in rows[a][1] and a not in rows[b][1]]
    for state in ("a TCD pipeline (active_tcd=True)", "inpaint_mask"):
        out += [(k, state) for k in kinds if state not in rows[k][1] + rows[k][2]]
    return out


def test_the_admitted_pairs_are_the_ones_the_table_leaves():
    dt, tcd = "dynamic_threshold", "a TCD pipeline (active_tcd=True)"
    assert set(_admitted()) == {(k, dt) for k in ("regions", "pag", "hypertile", "reference_only", "sag")} | {(k, tcd) for k in ("pag", "hypertile", "sag")}


@pytest.mark.parametrize("a, b", _admitted())
def test_engine_builds_every_admitted_pair(a, b):
    eng = _construct(**_kind_options()[a], **_excluded_options()[b])
    assert len(eng.calls) > 0


def test_defaults_key_and_unknown_names():
    from minsdtf_amd.jobopts import EngineOptions
    from minsdtf_amd.stable_diffusion import StableDiffusionBase

    assert EngineOptions.of() == EngineOptions() and EngineOptions.of().key() == ()
    assert EngineOptions.of(sampler=None, tiled=None, regions=None, region_mode=None, pag=None, reference=None, adain=None, hypertile=None,
                            sag=None, dynthresh=None) == EngineOptions()
    both = EngineOptions.of(regions=3, region_mode="attention", hypertile=[2, 2, 0], sag=True, dynthresh=True, sampler="euler_a")
    assert both.key() == (("regions", 3, "attention"), ("hypertile", 2, 2, 0), ("sag",), ("dynthresh",))
    ref = EngineOptions.of(adain=("mid_block.resnets.1",))
    assert ref.reference == frozenset() and ref.key() == (("reference", (), ("adain", "mid_block.resnets.1")),)
    assert EngineOptions.of(region_mode="attention").region_mode == "latent"
    with pytest.raises(TypeError):
        EngineOptions.of(bogus=1)
    with pytest.raises(ValueError, match=r"^hypertile: \[2, 2\] is not \(nh, nw, depth\)$"):   # (the value as the caller gave it)
        EngineOptions.of(hypertile=[2, 2]).check(SIZE, SIZE, 2, 7.5, False, False, False, None)

    class Net:
        weights_version = 1

    sd = StableDiffusionBase(128, 128)
    sd.diffusion_model = Net()
    with pytest.raises(TypeError):
        sd._engine_key(1, 77, 77, 4, 7.5, 0.0, False, bogus=1)
    with pytest.raises(TypeError):
        _construct(bogus=1)


def test_unet_variant_at_every_attention_block():
    """engine.UNetVariant.at over the 16 attention blocks, each with its input Act at its level: which blocks an option touches."""
    from minsdtf_amd import engine
    from minsdtf_amd import weights as wtab
    from minsdtf_amd.engine import AttnVariant, UNetVariant

    levels = engine.unet_levels(SIZE, SIZE)

    def level_of(block):
        part, idx = block.split(".")[:2]
        return 3 if part == "mid_block" else int(idx) if part == "down_blocks" else 3 - int(idx)

    acts = {b: engine.Act(None, 4, *levels[level_of(b)], wtab.UNET_CH[level_of(b)]) for b in engine.PAG_LAYERS}
    assert len(acts) == 16

    def touched(variant):
        return {b: variant.at(b, x) for b, x in acts.items() if variant.at(b, x) != AttnVariant()}

    assert touched(UNetVariant()) == {}
    some = {engine.PAG_LAYERS[1], MID}
    assert touched(UNetVariant(pag_layers=some, perturbed=2)) == {b: AttnVariant(perturbed=2) for b in some}
    assert touched(UNetVariant(pag_layers=some, perturbed=0)) == {}
    for depth in (0, 1, 2):
        got = touched(UNetVariant(window=[2, 2], window_depth=depth))
        assert set(got) == {b for b in acts if level_of(b) <= depth} and len(got) == 5 * (depth + 1)
        assert set(got.values()) == {AttnVariant(window=(2, 2))}
    sag = (object(), object(), 0, 2)
    assert touched(UNetVariant(sag=sag)) == {MID: AttnVariant(colsum=sag)}
    planes = {lv: object() for lv in levels}
    got = touched(UNetVariant(region_attn=(3, 2, planes)))
    assert got == {b: AttnVariant(regions=3, region_rows=2, region_w=planes[(x.H, x.W)]) for b, x in acts.items()}
    assert all(got[b].region_w is planes[levels[level_of(b)]] for b in acts)
    # a block in the window levels and in the reference layers takes the window; the reference layers elsewhere stay
    mix = object()
    both = touched(UNetVariant(window=(2, 2), window_depth=0, reference=(frozenset(engine.PAG_LAYERS), object(), mix)))
    assert all(both[b] == (AttnVariant(window=(2, 2)) if level_of(b) == 0 else AttnVariant(reference=1, mix=mix)) for b in acts)
    assert touched(UNetVariant(reference=({MID}, object(), mix))) == {MID: AttnVariant(reference=1, mix=mix)}
    for cls in (UNetVariant, AttnVariant):
        with pytest.raises(TypeError):
            cls(bogus=1)
