"""CPU tests (no GPU) of the per-layer case list of tests/test_layer_shapes_gpu.py: the tensor-less walk of the emitters
(tests/_layer_walk.py) turned into test cases, the tuning table against what the engines really record, and the launch
configurations of the shapes the table has no row of.  Then the case lists of tests/test_layer_launches_gpu.py (GroupNorm,
attention, cross_attention_q, conv_direct, layer_norm), and CPU emulations of wrong kernels that its comparison must refuse."""
import json
import os

import pytest
import torch

import _layer_draw as D
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


# ---- the other launch families (tests/test_layer_launches_gpu.py): the lists, and that the comparison can fail ------------------------
def test_every_recorded_launch_of_the_other_families_becomes_a_case():
    """GroupNorm, attention, cross_attention_q, conv_direct and the text encoder's layer_norm: ids are unique, the signature counts
    are pinned, and every record is something the GPU module knows how to draw, launch and check.  Prints the counts."""
    from minsdtf_amd import ops

    fam = LW.family_cases()
    counts = {}
    for f, cases in fam.items():
        ids = [LW.family_id(f, s) for s in cases]
        assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
        counts[f] = (len(cases), sum(len(ls) for per in cases.values() for ls in per.values()))
        for s, per in cases.items():
            for b, ls in per.items():
                assert ls and all(l.batch == b for l in ls), (f, s)
    print("\n" + "\n".join(f"{f}: {n} signatures, {m} launches" for f, (n, m) in counts.items()) + f" over {len(LW.FAMILY_WALKS)} walks")
    assert {f: n for f, (n, _) in counts.items()} == LW.EXPECTED_FAMILY_CASES, "the engines record another set of launches: update _layer_walk.EXPECTED_FAMILY_CASES"
    for s, per in fam["group_norm"].items():
        what = LW.family_id("group_norm", s)
        assert s.c0 % 8 == 0 and s.c1 % 8 == 0 and (s.c0 + s.c1) % 32 == 0 and s.hw > 0, what
        assert s.sync, what + ": the engine lends its sync block to every GroupNorm"
    for s, per in fam["attention"].items():
        what = LW.family_id("attention", s)
        C = s.heads * s.head_dim
        assert s.head_dim in D.ATTN_HEAD_SIZES, what
        assert s.vt_ld >= s.t and s.vt_ld % 8 == 0, what
        assert s.q_ld == s.k_ld == s.o_ld == C, what
        assert not (s.causal and s.s != s.t), what
        for b, ls in per.items():
            for l in ls:
                if l.workspace_floats:
                    assert s.head_dim == 512 and l.workspace_floats == 4 * b * s.s * 514, (what, l)
        if s.head_dim == 512:
            assert s.heads == 1 and s.t % 32 == 0 and not s.causal and not s.q_prescaled, what
        else:
            assert not s.workspace_per_sample, what
    for s, per in fam["cross_attention_q"].items():
        what = LW.family_id("cross_attention_q", s)
        assert s.heads == 8 and s.head_dim in (40, 80, 160) and s.t <= 96 and s.vt_ld >= s.t and s.vt_ld % 8 == 0, what
        assert s.k_ld == s.o_ld == s.heads * s.head_dim, what
        for ls in per.values():
            assert all(1 <= l.ln_in_slots <= 20 and l.w_layout in (0, 1) for l in ls), what
    for s, per in fam["conv_direct"].items():
        what = LW.family_id("conv_direct", s)
        assert s.ksize in (1, 3) and s.stride == 1 and s.bias and not s.act_in and not s.shared_input, what
        assert s.in_dtype in (ops.OUT_BF16, ops.OUT_F32) and s.out_dtype in (ops.OUT_BF16, ops.OUT_F32, ops.OUT_U8) and s.act == ops.ACT_NONE, what
    for s in fam["layer_norm"]:
        assert s.c % 8 == 0, LW.family_id("layer_norm", s)


def _smallest_and_largest(cases, key, size):
    """The smallest and the largest signature (by `size`) of every value of `key`."""
    out = []
    for v in sorted({key(s) for s in cases}):
        group = sorted((s for s in cases if key(s) == v), key=size)
        out += [group[0]] + ([group[-1]] if len(group) > 1 else [])
    return out


ATTN_PICKS = _smallest_and_largest(LW.cases_attention(), lambda s: s.head_dim, lambda s: (s.s * s.t, s.s))
NORM_PICKS = _smallest_and_largest(LW.cases_group_norm(), lambda s: s.c0 + s.c1, lambda s: (s.hw, s.c1))


def _refused(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("sig", ATTN_PICKS, ids=[LW.family_id("attention", s) for s in ATTN_PICKS])
def test_attention_comparison_refuses_the_faults(sig):
    """A passing check means nothing unless a failing one is shown to fail: on the draw, the reference and the bound of the GPU
    module, the CPU emulation of the legitimate error (P rounded to bf16 before P V, the output rounded to bf16) passes, and each of
    a dropped last key, a dropped last 64-key tile, the last query row carrying its neighbour's result and two swapped interior rows
    is refused - on head 0 of sample 0, whose queries are all compared."""
    s, sid = sig, LW.family_id("attention", sig)
    q, k, v = D.attn_draw_sample(s, sid, 0)
    b, h, idx = D.attn_blocks(1, s.heads, s.s)[0]
    assert (b, h) == (0, 0) and idx.numel() == s.s
    ref = D.attn_reference(s, q, k, v, h, idx)
    D.attn_compare(D.attn_emulate(s, q, k, v, h), ref, f"{sid}: legitimate rounding")
    for fault in D.ATTN_FAULTS:
        got = D.attn_emulate(s, q, k, v, h, fault)
        assert _refused(lambda: D.attn_compare(got, ref, fault)), f"{sid}: '{fault}' passes the comparison unseen"


def test_attention_subset_covers_every_pair():
    """No (sample, head) pair goes unchecked; the first and the last pair are compared in full, the others on their first and last 256
    queries and every 37th between."""
    for (B, H, S) in ((1, 1, 64), (2, 8, 100), (10, 8, 4096), (2, 8, 9216)):
        blocks = D.attn_blocks(B, H, S)
        assert [(b, h) for b, h, _ in blocks] == [(b, h) for b in range(B) for h in range(H)]
        for b, h, idx in blocks:
            assert int(idx[0]) == 0 and int(idx[-1]) == S - 1 and idx.unique().numel() == idx.numel()
            if (b, h) in ((0, 0), (B - 1, H - 1)) or S <= 512:
                assert idx.numel() == S
            else:
                assert bool((idx[:256] == torch.arange(256)).all()) and bool((idx[-256:] == torch.arange(S - 256, S)).all())
                assert int((idx[1:] - idx[:-1]).max()) <= 37


@pytest.mark.parametrize("sig", NORM_PICKS, ids=[LW.family_id("group_norm", s) for s in NORM_PICKS])
def test_group_norm_comparison_refuses_the_faults(sig):
    """The same for GroupNorm: the output rounded to bf16 passes; the last pixel left out of the statistics (hw <= 1024), the last
    1 / 64 of the pixels left out, and the group that straddles x0 | x1 normalised by its x0 channels alone are refused."""
    s, sid = sig, LW.family_id("group_norm", sig)
    x = D.gn_draw_sample(s, sid, 0)
    gamma, beta = D.gn_affine(s, sid)
    ref, mean, rstd = D.gn_reference(s, x, gamma, beta)
    out, stats = D.gn_emulate(s, x, gamma, beta)
    D.gn_compare(out, stats, ref, mean, rstd, f"{sid}: legitimate rounding")
    applied = 0
    for fault in D.GN_FAULTS:
        got = D.gn_emulate(s, x, gamma, beta, fault)
        if got is None:
            assert (fault == "last pixel" and s.hw > D.GN_SPIKE_HW) or (fault == "x0 only" and D.gn_straddles(s) is None), (sid, fault)
            continue
        applied += 1
        assert _refused(lambda: D.gn_compare(got[0], got[1], ref, mean, rstd, fault)), f"{sid}: '{fault}' passes the comparison unseen"
    assert applied >= 1


def test_the_straddling_group_fault_is_exercised():
    """Some pick has a group across x0 | x1 (C = 960 and 1920), so the 'x0 only' emulation is not vacuous."""
    assert any(D.gn_straddles(s) is not None for s in NORM_PICKS)
