"""The packed weight image and the LoRA merge plan against the fixtures recorded before the layout table existed
(tools/make_pack_digests.py -> tests/golden/pack_digests.json.gz, lora_merge_plan.json.gz): launch plans hold raw addresses into the
image and the LoRA switch rewrites it in place, so the packing code may change only if every byte, every master and every merge
job stays where it was."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_pack_digests as mpd  # noqa: E402

# (the three UNet images follow one another: its weights are generated once)
NAMES = sorted(mpd.VARIANTS, key=lambda n: mpd.VARIANTS[n][0])


@pytest.fixture(scope="module")
def golden():
    return mpd.read_fixture("pack_digests")


@pytest.fixture(scope="module")
def arrays():
    last = {}

    def get(kind):
        if kind not in last:
            last.clear()   # one kind's fp32 weights alive at a time
            last[kind] = mpd.synth(kind)
        return last[kind]
    return get


def test_fixture_covers_every_kind_and_variant(golden):
    assert set(golden["images"]) == set(mpd.VARIANTS) and len(mpd.KINDS) == 7
    assert set(golden["masters"]) == set(mpd.SWITCHED)
    assert len(golden["commit"]) == 40 and golden["seed"] == mpd.SEED


@pytest.mark.parametrize("name", NAMES)
def test_packed_image_is_byte_identical(golden, arrays, name):
    """Per key: shape, dtype, chunk-major or not, sha256 of the bytes; with lora_switch also every master, ffproj top block and
    saved vector."""
    kind, chunk_major, mfma_temb_proj = mpd.VARIANTS[name]
    switched = name in mpd.SWITCHED
    m = mpd.packed_model(kind, arrays(kind), chunk_major, mfma_temb_proj, lora_switch=switched)
    bad = mpd.differences(golden["images"][name], mpd.image_digests(m))
    if switched:
        bad += mpd.differences(golden["masters"][name], mpd.master_digests(m))
    assert not bad, f"{name}: {len(bad)} packed keys differ: {bad[:20]}"


@pytest.mark.parametrize("name", NAMES)
def test_layout_describes_the_image(golden, name):
    """The layout table, from the weight table alone, names exactly the image's keys with their shapes, dtypes and chunk-major
    flags."""
    from minsdtf_amd import layout, weights

    kind, chunk_major, mfma_temb_proj = mpd.VARIANTS[name]
    table = layout.layout(weights.table(kind, **mpd.table_kw(kind)), layout.Flags(chunk_major, mfma_temb_proj))
    assert len({e.key for e in table}) == len(table)
    said = {e.key: [list(e.stored_shape), e.dtype, e.chunk_major] for e in table}
    bad = mpd.differences({k: v[:3] for k, v in golden["images"][name].items()}, said)
    assert not bad, f"{name}: {bad[:20]}"


@pytest.mark.parametrize("kind", mpd.SWITCHED)
def test_merge_plan_is_unchanged(kind):
    """Ordered targets, their .lncs / .lnb keys, ordered parts with offsets, scales and row maps, the ffproj.b map, the layers."""
    from minsdtf_amd import layout, lora, weights

    want = mpd.read_fixture("lora_merge_plan")["plans"][kind]
    specs = weights.table(kind, **mpd.table_kw(kind))
    got = mpd.merge_plan(lora.Plan(specs, layout.layout(specs)))
    assert [t["key"] for t in got["targets"]] == [t["key"] for t in want["targets"]]
    for g, w in zip(got["targets"], want["targets"]):
        assert g == w, w["key"]
    assert got["ffproj_b"] == want["ffproj_b"] and got["layers"] == want["layers"]
    assert list(got["layers"]) == list(lora.targetable(specs))


def test_layout_module_stands_alone():
    """layout.py is read by the packer and by the merge, so it imports neither (nor models / engine); lora.py no longer reads
    models.py, and only layout.py matches layer names."""
    import re

    def imports(module):
        src = open(os.path.join(ROOT, "minsdtf_amd", module + ".py")).read()
        return src, set(re.findall(r"^\s*(?:from \.(\w*) import ([\w, ]+)|import (\w+))", src, re.M))

    src, imp = imports("layout")
    names = {n for a, b, c in imp for n in ([a] if a else re.split(r",\s*", b)) + [c]}
    assert not names & {"models", "engine", "lora", "packing"}, names
    for module in ("lora", "models", "packing"):
        src, imp = imports(module)
        names = {n for a, b, c in imp for n in ([a] if a else re.split(r",\s*", b)) + [c]}
        assert module != "lora" or "models" not in names
        assert "_ffproj_stash" not in src
        assert not re.search(r"endswith\(\(?\"\.(attn|to_|ff\.|conv|proj|query|self_attn|transformer)", src), module
