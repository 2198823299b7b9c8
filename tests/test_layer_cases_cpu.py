"""CPU tests (no GPU) of the per-layer case list of tests/test_layer_shapes_gpu.py: the tensor-less walk of the emitters
(tests/_layer_walk.py) turned into test cases, the tuning table against what the engines really record, and the launch
configurations of the shapes the table has no row of."""
import json
import os

import pytest

import _layer_walk as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Rows of conv_tuning.json that no walk of tests/_layer_walk.ALL_WALKS records, each with the reason it stays.  All ten are the
# UNet's 64x64-level (96x96 at 768 x 768) conv_shortcut 1x1 as a launch of its own: engine.SHORTCUT_FOLD folds it into conv2 (the
# "+x640" / "+x960" rows), so the default product never looks them up.  They are kept, not deleted: MSD_SHORTCUT_FOLD=0 (and
# MSD_SHORTCUT_FOLD_MAX_PIXELS), the same-box A/B switches of engine.py, emit exactly these launches, and with the rows gone that
# baseline would run on tuning.shape_config's guess instead of the configuration that was measured for it
# (test_unreachable_rows_are_what_the_unfolded_shortcut_emits holds them to that reason).
UNREACHABLE_ROWS = {
    "1x64x64x640->320k1s1u0": "up_blocks.3 conv_shortcut, fused batch 1: only with MSD_SHORTCUT_FOLD=0",
    "1x64x64x960->320k1s1u0": "up_blocks.3.resnets.0 conv_shortcut, fused batch 1: only with MSD_SHORTCUT_FOLD=0",
    "2x64x64x640->320k1s1u0": "up_blocks.3 conv_shortcut, fused batch 2: only with MSD_SHORTCUT_FOLD=0",
    "2x64x64x960->320k1s1u0": "up_blocks.3.resnets.0 conv_shortcut, fused batch 2: only with MSD_SHORTCUT_FOLD=0",
    "2x96x96x640->320k1s1u0": "up_blocks.3 conv_shortcut at 768 x 768, fused batch 2: only with MSD_SHORTCUT_FOLD=0",
    "2x96x96x960->320k1s1u0": "up_blocks.3.resnets.0 conv_shortcut at 768 x 768, fused batch 2: only with MSD_SHORTCUT_FOLD=0",
    "4x64x64x640->320k1s1u0": "up_blocks.3 conv_shortcut, fused batch 4: only with MSD_SHORTCUT_FOLD=0",
    "4x64x64x960->320k1s1u0": "up_blocks.3.resnets.0 conv_shortcut, fused batch 4: only with MSD_SHORTCUT_FOLD=0",
    "8x64x64x640->320k1s1u0": "up_blocks.3 conv_shortcut, fused batch 8: only with MSD_SHORTCUT_FOLD=0",
    "8x64x64x960->320k1s1u0": "up_blocks.3.resnets.0 conv_shortcut, fused batch 8: only with MSD_SHORTCUT_FOLD=0",
}


def _table():
    return json.load(open(os.path.join(ROOT, "minsdtf_amd", "conv_tuning.json")))


def _launches():
    return [l for per in LW.cases().values() for ls in per.values() for l in ls]


def test_every_recorded_signature_becomes_a_case():
    """Every (layer signature, batch) the walks record is something the GPU test knows how to draw, launch and check; ids are
    unique and readable.  Prints the counts the GPU test runs."""
    from minsdtf_amd import ops, tuning

    cases = LW.cases()
    ids = [LW.sig_id(s) for s in cases]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    launches = _launches()
    for s, per in cases.items():
        what = LW.sig_id(s)
        assert s.act in (ops.ACT_NONE, ops.ACT_SILU, ops.ACT_GEGLU) and s.out_dtype in (ops.OUT_BF16, ops.OUT_F32), what
        assert s.c0 % 64 == 0 and s.c1 % 64 == 0 and s.c2 % 64 == 0 and s.c3 % 64 == 0, what
        if s.ln_in or s.ln_out or s.split or s.act == ops.ACT_GEGLU:   # the Dense epilogues: 1x1 over one tensor, no shortcut operand
            assert s.ksize == 1 and s.stride == 1 and not s.upsample and not s.c1 and not s.c2, what
        if s.ln_in:
            assert s.bias and not s.residual and not s.rowvec, what
        if s.split or s.act == ops.ACT_GEGLU:
            assert not s.residual and not s.rowvec and not s.ln_out and s.out_dtype == ops.OUT_BF16, what
        assert s.rowvec == s.step_ptr, what
        for b, ls in per.items():
            assert ls and all(l.batch == b for l in ls), what
            for l in ls:
                form = tuning.form_of(l.tile_m, l.tile_n, l.stages)   # (raises for a code that names no kernel form)
                assert l.w_layout == (2 if form.family == "wreg" else 1), (what, l)
                assert l.splitk >= 1 and (l.splitk == 1 or not (s.ln_in or s.ln_out or s.split or s.act == ops.ACT_GEGLU)), (what, l)
                assert (l.ln_in_slots > 0) == s.ln_in and (l.ln_out_slots > 0) == s.ln_out, (what, l)
    keys = {LW.shape_key(l) for l in launches}
    print(f"\nlayer cases: {len(cases)} signatures, {len(launches)} launches, {len(keys)} shape keys over {len(LW.ALL_WALKS)} walks")
    assert len(cases) == LW.EXPECTED_CASES, "the engines record another set of layer signatures: update _layer_walk.EXPECTED_CASES"
    assert len(keys) >= 343 and len(launches) >= 419


def test_every_table_row_is_recorded_or_listed():
    """A row of conv_tuning.json is either looked up by some walk or named, with its reason, in UNREACHABLE_ROWS; the list
    holds nothing that is reached or that is not a row."""
    table = _table()
    keys = {LW.shape_key(l) for l in _launches()}
    unreached = set(table) - keys
    assert unreached == set(UNREACHABLE_ROWS), sorted(unreached ^ set(UNREACHABLE_ROWS))
    assert len(UNREACHABLE_ROWS) == 10 and all(isinstance(r, str) and len(r) > 20 for r in UNREACHABLE_ROWS.values())


def test_unreachable_rows_are_what_the_unfolded_shortcut_emits(monkeypatch):
    """The reason UNREACHABLE_ROWS gives: with the shortcut fold switched off (MSD_SHORTCUT_FOLD=0) the UNet walks look up exactly
    these rows, and the row's configuration is one the library builds for the shape."""
    from minsdtf_amd import engine, tuning

    monkeypatch.setattr(engine, "SHORTCUT_FOLD", False)
    seen = {}
    for (nb, hw) in ((1, 64), (2, 64), (4, 64), (8, 64), (2, 96)):
        for sh in LW.walk_shapes(nb, hw, hw, "unet"):
            seen[tuning.shape_key(*sh[:8], sh[10], sh[11])] = sh
    assert set(UNREACHABLE_ROWS) <= set(seen), sorted(set(UNREACHABLE_ROWS) - set(seen))
    for key in UNREACHABLE_ROWS:
        assert LW.config_is_built(tuning.lookup(*seen[key]), seen[key]), key


def test_launches_without_a_table_row_name_built_kernels():
    """For every recorded launch whose key has no table row (nearest measured batch, tuning.shape_config) the configuration the
    engine chose is one the library builds and that takes the shape."""
    table = _table()
    n = 0
    for l in _launches():
        if LW.shape_key(l) in table:
            continue
        n += 1
        assert LW.config_is_built((l.tile_m, l.tile_n, l.splitk, l.stages), LW.lookup_args(l)), (LW.shape_key(l), l)
    assert n >= 47


@pytest.mark.parametrize("what,nb,hw", [("unet", 2, 64), ("vae", 1, 64)])
def test_walk_records_the_engines_own_lookup(what, nb, hw):
    """The walk leaves tuning.lookup in place: the configuration in a record is what lookup returns for the record's arguments
    (split-K forced to 1 by the LayerNorm fold, as Emitter.conv does)."""
    from minsdtf_amd import tuning

    for l in LW.walk(what, nb, hw, hw):
        bm, bn, sk, stg = tuning.lookup(*LW.lookup_args(l))
        assert (l.tile_m, l.tile_n, l.stages) == (bm, bn, stg) and l.splitk == (1 if (l.ln_in or l.ln_out) else sk), l
