"""CPU tests (no GPU) of tests/test_lora_exact_gpu.py: the case lists of the exact and the rank-0 stage meet their conditions
(_exact_lora.conditions), the checker accepts a numpy model built the way the kernel is (_exact_lora.model) and refuses each of its
23 faults (_exact_lora.FAULTS: the issue's 22, "row_off or rowmap ignored in the fragment copy" as two) on at least one case, the
fragment index and the GEGLU row map of the statement equal packing's, and every form a job takes in the real merge plans of the
UNet and the text encoder has a case of the exact stage.

Two of the faults are stated more narrowly than a first reading suggests, because a lane's elements past K are zeros in a right
kernel and reach nothing: "K rounded up to 4" is the scalar-load path taken as if K were a multiple of 4 (it loads, stores and sums
up to three elements past K: the next row's values, a NaN gap or the NaN band), and "colsum of the padded lanes" sums all eight
elements of the tail lane after unguarded loads."""
import os
import sys

import numpy as np
import pytest

import _exact_lora as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_pack_digests as mpd  # noqa: E402

EXACT = E.launches("exact")
RANK0 = E.launches("rank0")
BOTH = EXACT + RANK0


def test_conditions_hold():
    """Every exact-stage job is exact (asserted per operation), every rank-0 job finite; over the lists: >= 32 bf16 ties in each
    direction, and elements whose bits depend on the order of the two scales."""
    even = odd = 0
    for c in EXACT:
        e, o, _ = E.conditions(c)
        even, odd = even + e, odd + o
    order = sum(E.conditions(c)[2] for c in RANK0)
    print(f"\nRECORD | exact stage: {sum(len(c.jobs) for c in EXACT)} jobs in {len(EXACT)} launches; bf16 ties rounding down to an even "
          f"mantissa {even}, up from an odd one {odd}; rank-0 elements that tell the scale orders apart: {order}")
    assert even >= 32 and odd >= 32 and order >= 32


def test_case_list_has_the_issues_shapes():
    jobs = [(c, j, c.dests[j.dest]) for c in EXACT for j in c.jobs]
    ks = {j.k for _, j, _ in jobs}
    assert {1, 8, 13, 100, 512, 520, 1032, 1088} <= ks and {1, 8, 9, 37} <= {j.n for _, j, _ in jobs}
    assert {0, 1, 7, 512} <= {j.rank for _, j, _ in jobs}
    ranks = [j.rank for j in next(c for c in EXACT if c.id.endswith("ranks")).jobs]
    assert ranks[:3] == [512, 1, 0]
    table = next(c for c in EXACT if c.id.endswith("job table"))
    assert [-(-j.n // 8) for j in table.jobs] == [1, 1, 5, 1, 2, 1, 1, 3, 1]
    assert {3, 4} <= {j.master_ld - j.k for _, j, _ in jobs}
    assert {"master", "down", "colscale"} <= set().union(*(j.mis for _, j, _ in jobs))
    assert {0, 8, 2} <= {j.col_off for _, j, d in jobs if d.layout == E.ROWS and d.dtype == E.BF16}
    assert any(d.layout == E.ROWS and d.ld == d.cols == 100 for _, _, d in jobs) and any(d.ld == 104 and d.cols == 100 for _, _, d in jobs)
    assert any(d.off and d.layout == lay and d.dtype == dt for _, _, d in jobs for lay, dt in ((E.ROWS, E.BF16),)) and any(d.off and d.layout == E.TRANS for _, _, d in jobs)
    assert any(d.layout == E.CHUNK and j.n < d.rows and j.row_off > 0 for _, j, d in jobs)
    assert any(d.layout == E.CHUNK and d.cols == 128 and j.k == 64 and j.col_off == 64 for _, j, d in jobs)
    assert any(d.layout == E.CHUNK and j.k == 60 and j.col_off == 2 for _, j, d in jobs)
    for scales in ((False, False), (True, False), (False, True), (True, True)):
        assert any((j.rs is not None, j.cs is not None) == scales for _, j, _ in jobs), scales
    for _, j, d in jobs:
        if j.rowmap is not None and ((j.rowmap + j.row_off < 0).sum(), (j.rowmap + j.row_off >= d.rows).sum()) == (2, 2):
            assert j.frag and j.colsum
            break
    else:
        raise AssertionError("no row map with two entries below 0 and two at or above out_rows")


@pytest.mark.parametrize("c", BOTH, ids=[c.id for c in BOTH])
def test_faultless_model_passes(c):
    E.check_model(c)


@pytest.mark.parametrize("fault", E.FAULTS)
def test_fault_is_caught(fault):
    caught = []
    for c in BOTH:
        try:
            E.check_model(c, fault)
        except AssertionError as e:
            caught.append((c.id, str(e)))
    print(f"\nRECORD | fault '{fault}' is refused on {len(caught)} of {len(BOTH)} launches: {', '.join(i for i, _ in caught)}")
    if caught:
        print(f"         e.g. {caught[0][1][:300]}")
    assert caught, f"no case sees the fault '{fault}'"


def test_statement_against_packing():
    """Two statements of the fragment-major index and of the GEGLU row map, written apart, agree."""
    import torch

    from minsdtf_amd import packing

    assert tuple(E.FRAG_ROW) == tuple(packing.FRAGMENT_ROW_ORDER) and np.array_equal(E.FRAG_ROW[E.FRAG_ROW], np.arange(16))
    for rows, cols in ((32, 128), (48, 192), (16, 64)):
        c = E.Case(f"fragment {rows} x {cols}", "exact")
        c.dest("w", E.ROWS, rows, cols, frag=True)
        j = c.job("w", rows, cols)
        _, _, oi, fi = E.place(j, c.dests["w"])
        w = torch.arange(rows * cols, dtype=torch.int32).reshape(rows, cols)
        assert np.array_equal(oi, w.numpy())
        got = np.zeros(rows * cols, dtype=np.int32)
        got[fi.ravel()] = w.numpy().ravel()
        assert np.array_equal(got, packing.fragment_major(w).reshape(-1).numpy())
        cm = np.zeros(rows * cols, dtype=np.int32)
        c.dests["w"].layout = E.CHUNK
        cm[E.place(j, c.dests["w"])[2].ravel()] = w.numpy().ravel()
        assert np.array_equal(cm, packing.chunk_major(w).reshape(-1).numpy())
    for n in (64, 128, 2560):
        assert np.array_equal(E.geglu_rowmap(n), np.argsort(packing.geglu_row_order(n // 2)).astype(np.int32))
    assert not np.array_equal(E.geglu_rowmap(64), np.arange(64))       # (at 32 rows the map is the identity)


def plan_signatures(kind, flags):
    """The signature of the job MergeBase.apply records for every part of every target of the plan, from the layout table alone."""
    from minsdtf_amd import layout, lora, weights

    specs = weights.table(kind, **mpd.table_kw(kind))
    plan = lora.Plan(specs, layout.layout(specs, flags))
    out = {}
    for t in plan.targets:
        if t.store == layout.KERAS:         # the fp32 time-embedding form (1, 1, K, N_total)
            lay, dt, rows, cols = E.TRANS, E.F32, t.shape[3], t.shape[2]
        else:
            rows, cols = (t.shape[0], t.pad_k) if t.pad_k else t.shape
            lay, dt = (E.CHUNK if t.chunk_major else E.ROWS), E.BF16
        for p in t.parts:
            if p.ffproj_top:                # the master is the [C][4C] product of ff.net.2 and proj_out
                n, k = plan.layers[t.parts[1].layer][0], plan.layers[p.layer][1]
            else:
                n, k = plan.layers[p.layer][:2]
            eligible = dt == E.BF16 and rows % 16 == 0 and cols % 64 == 0
            for frag in ((False, True) if eligible else (False,)):      # the copy exists once a launch has asked for it
                s = E.signature(layout=lay, dtype=dt, n=n, k=k, row_off=p.row_off, col_off=p.col_off, out_rows=rows, rowmap=p.rowmap,
                                rowscale=p.qscale is not None, colscale=p.colscale is not None, colsum=t.colsum is not None, frag=frag,
                                parts=len(t.parts))
                out.setdefault(s, f"{t.key} <- {p.layer}")
    return out


@pytest.mark.parametrize("name", sorted(n for n, (kind, _, _) in mpd.VARIANTS.items() if kind in mpd.SWITCHED))
def test_plan_signatures_are_covered(name):
    """Every form of job a real merge plan holds (per flag variant the pack fixtures cover) has a case in the exact stage."""
    from minsdtf_amd.layout import Flags

    kind, chunk_major, mfma_temb_proj = mpd.VARIANTS[name]
    real = plan_signatures(kind, Flags(chunk_major=chunk_major, mfma_temb_proj=mfma_temb_proj))
    have = E.case_signatures(EXACT)
    missing = {s: w for s, w in real.items() if s not in have}
    print(f"\nRECORD | {name}: {len(real)} job signatures, all among the exact stage's {len(have)}")
    assert not missing, "no exact-stage case for: " + "; ".join(f"{w}: {dict(zip(E.SIGNATURE, s))}" for s, w in missing.items())


def test_real_stage_bound_is_reachable():
    """The numpy float32 chain (two roundings per rank step: more than the kernel's FMA makes) stays inside the derived bound, and the
    bound is not loose: most bf16 intervals are one number."""
    c = E.real_launches()[2]
    got = {}
    for name, (n, dt) in c.buffers().items():
        got[name] = np.full(n, E.canary_bits(dt), dtype=E.np_dtype(dt))
    for j in c.jobs:
        d = c.dests[j.dest]
        v = j.master.copy()
        acc = np.zeros_like(v)
        for r in range(j.rank):
            acc = acc + j.up[:, r:r + 1] * j.down[r:r + 1, :]
        v = v + acc
        if j.rs is not None:
            v = v * j.rs[:, None]
        if j.cs is not None:
            v = v * j.cs[None, :]
        kept, row, oi, fi = E.place(j, d)
        bits = E.bf16_rne(v) if d.dtype == E.BF16 else E.f32_bits(v)
        got[d.name + ".out"][oi.ravel()] = bits.ravel()
        if j.frag:
            got[d.name + ".frag"][fi.ravel()] = bits.ravel()
        if j.colsum:
            got[d.name + ".colsum"][row] = E.f32_bits(E.bf16_value(bits).astype(np.float64).sum(axis=1).astype(np.float32))
    worst, single = E.check_real(c, got)
    print(f"\nRECORD | {c.id}: numpy float32 chain: |v - v64| / b at most {worst:.3f}; {single * 100:.2f} % of the bf16 intervals are one number")
    assert worst <= 1.0 and single > 0.9
    bad = dict(got)
    bad["rows.out"] = got["rows.out"].copy()
    j = c.jobs[0]
    i = E.place(j, c.dests["rows"])[2][5, 7]
    bad["rows.out"][i] += 2                        # two bf16 ulps
    with pytest.raises(AssertionError):
        E.check_real(c, bad)
