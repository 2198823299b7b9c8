"""CPU tests (no GPU) of the exact comparison of tests/test_norm_exact_gpu.py: every GPU case's draw keeps the conditions exactness
rests on, the checks refuse what they must, and the bounds the suite used until now let the same faults through.

Walked without a GPU: every case of test_group_norm_exact, test_recorded_group_norm_exact and test_layer_norm_exact.
  - every draw meets its conditions and caps (asserted inside gn_problem / ln_problem), and names the form the host rule gives it
  - fp32 sums of a draw, in shuffled and chunked orders, give S and Q bit for bit
  - a restatement of the kernel's formula passes check_stats with mean moved by +-1 ulp and rstd by +-4 ulp: the fp32
    values 4 ulp either side of the EXACT rstd (the whole budget the Q bound is derived from: where mean^2 > eps on a +-1 draw rstd
    lies just above 1, an ulp is 2^-23 of it and 4 ulp are the bound itself), and the formula evaluated in fp32 - whose three roundings
    of var + eps already spend up to 1.5 ulp of that budget - moved by +-2 (v_rsq_f32's one ulp and one of margin).  The fp32
    evaluation moved by a further +-4 ulp is up to 5.5 ulp from the exact value and does NOT pass everywhere (1.01 x the bound at
    rstd = 0.633, 1.1 x just above 1): the bound stays, the budget is not spent twice
  - three emulated faults are refused for every case (_exact_norm.gn_faulty: the statistics lose the last pixel of the last part; the
    statistics count one chunk twice; one part's pixels are normalised with the statistics of the other P - 1 parts), and for
    LayerNorm the last vector of a row left out of the mean
  - the same faulty results pass the bounds of test_group_norm and test_layer_norm where reasoning says they must (below): the gap
    is on record, as tests/test_exact_cpu.py records it for the GEMMs.  If one of those assertions fails, the old bounds have become
    able to see the fault - good; say so here.

Where the old bounds ({mean, rstd} within 1e-3, output within 2e-2 + 1 %) cannot see a fault, by the size of its effect and not by
trying.  "last pixel": a pixel of |x| <= 2 moves a group's mean by at most 2 / hw and its variance by at most 4 / hw of itself:
passes from hw = 4096 on (5e-4).  "chunk twice": the variance rises by one part in nchunks, rstd falls by half that: passes where
the statistics pass has at least 1024 chunks (5e-4); with P <= 64 parts it is seen - it is the ordered finalize's fault.  "part
statistics": the published statistics are the right ones; the last part's outputs move by the sampling error of the other parts'
moments, (|x| / sigma) / sqrt(cnt (P - 1) / P) <= 2 / sqrt(cnt / 2) at P = 2: under 1.1e-2 from cnt = 65536 on, and with P >= 8
(cnt 7 / 8) from cnt = 16384 on (1.7e-2), inside atol 2e-2."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _exact_norm as N
import test_norm_exact_gpu as T
from _checks import close


def _refused(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _form(c, **v):
    return N.gn_form(c["B"], c["hw"], c["c0"] + c["c1"], c["sync"], **dict(c["opt"], **v))


_problems = {}


def _problem(c):
    """One draw per operand shape for the module (the cluster list runs each shape in two forms)."""
    k = T.problem_id(c)
    if k not in _problems:
        if len(_problems) >= 3:
            _problems.pop(next(iter(_problems)))
        _problems[k] = T.case_problem(c)
    return _problems[k]


CASES = sorted(T.EXACT_CASES, key=T.problem_id)
IDS = [c["id"] for c in CASES]


def test_every_form_is_reached_and_named():
    names = {}
    for c in T.EXACT_CASES:
        for v in T.variants(c):
            names.setdefault(_form(c, **v).name, []).append(c["id"])
        assert _form(c).name == c["form"], (c["id"], _form(c).name)
    print()
    for n in sorted(names):
        print(f"{n:36s} {' '.join(names[n])}")
    ids = [c["id"] for c in T.EXACT_CASES]
    assert len(set(ids)) == len(ids) == len(T.GROUP_NORM_CASES) + 2 * len(T.GROUP_NORM_CLUSTER_CASES) + len(T.MORE_CASES)
    for kind, npts, vs in (("group", (2, 4, 8, 16), (1, 2, 4)), ("cluster", (2, 4, 8, 16), (1, 2, 4))):
        got = [n.split(">")[0].split("<")[1].split(",") for n in names if n.startswith(kind + "<")]
        assert {int(a) for a, _ in got} == set(npts) and {int(b) for _, b in got} == set(vs), (kind, got)
    assert {n.split()[1] for n in names if n.startswith("cluster<")} == {"P=2", "P=4", "P=8"}
    assert any(n.endswith(" xcd") for n in names) and any(n.startswith("cluster<") and not n.endswith(" xcd") for n in names)
    rows = [n.split() for n in names if n.startswith("rows<")]
    assert {r[0] for r in rows} == {"rows<2>", "rows<4>", "rows<6>"}
    assert {r[1] for r in rows} == {"P=4", "P=8", "P=16", "P=32", "P=64"} and {r[2] for r in rows} == {"Q=1", "Q=2", "Q=4"}
    three = [n for n in names if n.startswith("three")]
    assert any(n.startswith("three<1> fused") for n in three) and any(n.startswith("three<1> finalize") for n in three)
    assert any(n.startswith("three<2> finalize") for n in three) and any(n.startswith("three wide fused") for n in three)
    for n in three:      # the wide form's statistics chunks are four times coarser than its apply chunks
        if n.startswith("three wide"):
            s, a = (int(k) for k in n.split()[3].split("/"))
            assert s == -(-a // 4) or s * 4 >= a
    assert {(c // 8 + 63) // 64 for _, c in T.LN_CASES} == {1, 2, 3, 4}
    assert {c for _, c in T.LN_CASES} >= {8, 512, 520, 1024, 1032, 1536, 1544, 2048}, "each NV's full width and the first partial vector of the next"
    assert any(r % 4 for r, _ in T.LN_CASES)
    wrong = [_form(next(c for c in T.EXACT_CASES if c["id"] == cid)).name for cid in T.WRONG_PIXEL_CASES]      # one per form
    assert sorted(n.split("<")[0].split(" fused")[0] + (" finalize" if "finalize" in n else "") for n in wrong) == \
        ["cluster", "group", "rows", "three", "three finalize", "three wide"], wrong


def test_the_non_fused_wide_branch_cannot_be_reached():
    """msd_group_norm: wide <=> 2^20 <= hw C <= 2^22 (C <= 2048); gn_form asserts `fused` there.  Every C and the hw at both ends."""
    for C in range(32, 2049, 32):
        for hw in {-(-(1 << 20) // C), (4 << 20) // C, -(-(1 << 20) // C) + 1, (4 << 20) // C - 1, (3 << 20) // C}:
            f = N.gn_form(1, hw, C, False, impl=0)
            assert f.name.startswith("three wide fused"), (C, hw, f.name)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_group_norm_case_on_the_cpu(c):
    p = _problem(c)
    form = _form(c)
    what = c["id"]
    # any order and any chunking of fp32 additions gives the integers
    g = N.gen(what + "/order")
    cpg = p.C // 32
    b = p.B - 1
    for grp in (0, 31):
        v = p.x[b, :, grp * cpg:(grp + 1) * cpg].reshape(-1).float()
        for vals, want in ((v, int(p.S[b, grp])), (v * v, int(p.Q[b, grp]))):
            sh = vals[torch.randperm(vals.numel(), generator=g)].numpy()
            assert float(np.cumsum(sh, dtype=np.float32)[-1]) == want                                   # one long chain
            k = max(1, sh.size // 37)
            chunks = [np.cumsum(sh[i:i + k], dtype=np.float32)[-1] for i in range(0, sh.size, k)]
            assert float(np.cumsum(np.array(chunks, dtype=np.float32), dtype=np.float32)[-1]) == want   # 37 chunks, then their sums
    # the kernel's formula, moved by whole ulps, passes
    worst = 0.0
    for du, exact in ((-4, True), (4, True), (-2, False), (0, False), (2, False)):
        for dm in (-1, 0, 1):
            worst = max(worst, N.check_stats(N.gn_emulate_stats(p.S, p.Q, p.cnt, du, dm, exact=exact), p.S, p.Q, p.cnt,
                                             f"{what} {'exact' if exact else 'fp32'} rstd {du:+d} ulp, mean {dm:+d} ulp"))
    print(f"\n{what}: largest |Q_rec - Q| / Q of the moved restatements {worst:.2f} x 2^-24 (bound 16)")
    right = N.gn_emulate_stats(p.S, p.Q, p.cnt)
    N.check_out(N.gn_emulate_out(p, right), p.x, (p.y, p.tol), what + ": the right result")
    # the faults
    for fault in N.GN_FAULTS:
        st, out = N.gn_faulty(p, form, fault)
        if out is None:
            assert _refused(lambda: N.check_stats(st, p.S, p.Q, p.cnt, fault)), f"{what}: '{fault}' passes check_stats unseen"
        else:
            N.check_stats(st, p.S, p.Q, p.cnt, fault)
            assert _refused(lambda: N.check_out(out, p.x, (p.y, p.tol), fault)), f"{what}: '{fault}' passes check_out unseen"


def _old_bounds(p, st, out):
    """What test_group_norm asserts today, on the same operands."""
    x = p.x.float()
    ref = F.group_norm(x.permute(0, 2, 1), 32, p.gamma, p.beta, eps=1e-5).permute(0, 2, 1)
    if p.silu:
        ref = ref * torch.sigmoid(ref)
    close(out, ref, atol=2e-2, what="old bounds")
    xs = x.reshape(p.B, p.hw, 32, p.C // 32).permute(0, 2, 1, 3).reshape(p.B, 32, -1)
    np.testing.assert_allclose(st[..., 0].numpy(), xs.mean(-1).numpy(), rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(st[..., 1].numpy(), (xs.var(-1, unbiased=False) + 1e-5).rsqrt().numpy(), rtol=1e-3)


def _gap_applies(c, form, fault):
    cnt = c["hw"] * ((c["c0"] + c["c1"]) // 32)
    if fault == "last pixel":
        return c["hw"] >= 4096
    if fault == "chunk twice":
        return form.parts >= 1024
    return cnt >= (65536 if form.parts <= 2 else 16384)


GAP_CASES = [c for c in CASES if any(_gap_applies(c, _form(c), f) for f in N.GN_FAULTS)]


@pytest.mark.parametrize("c", GAP_CASES, ids=[c["id"] for c in GAP_CASES])
def test_the_old_bounds_let_the_faults_through(c):
    p = _problem(c)
    form = _form(c)
    seen = []
    for fault in N.GN_FAULTS:
        if not _gap_applies(c, form, fault):
            continue
        st, out = N.gn_faulty(p, form, fault)
        if out is None:
            out = N.gn_emulate_out(p, st)
        _old_bounds(p, st, out)
        seen.append(fault)
    print(f"\n{c['id']} [{form.name}]: passes the old bounds with {', '.join(seen)}")


def test_the_gap_is_on_record_for_every_fault():
    got = {f for c in GAP_CASES for f in N.GN_FAULTS if _gap_applies(c, _form(c), f)}
    assert got == set(N.GN_FAULTS), got


def test_recorded_cases_on_the_cpu():
    """Every recorded signature: conditions, the form at default options, the faults at the level of the moments (the outputs of the
    same shapes are walked above).  The LARGE ones are exactly those listed in the GPU module's docstring, each but one on the
    three-launch path with the separate finalize, where their faults are refused by check_partials' sums."""
    large = []
    for s in T.RECORDED:
        sid = T.LW.family_id("group_norm", s)
        cnt = s.hw * ((s.c0 + s.c1) // 32)
        form = N.gn_form(1, s.hw, s.c0 + s.c1, s.sync)
        if cnt >= N.Q_MAX:
            large.append(sid)
            assert (form.kind == "three" and "finalize" in form.name) or sid == "gn 65536x256 silu", (sid, form.name)
            if cnt > (1 << 20):        # (the draw of the very largest is left to the GPU run: 151 M values)
                continue
        p = T.recorded_problem(s)
        for fault in N.GN_FAULTS[:2]:
            P = max(2, form.parts)
            dS, dQ = N.gn_moments(p.x[:, -1:] if fault == "last pixel" else p.x[:, :-(-p.hw // P)])
            sign = -1 if fault == "last pixel" else 1
            assert bool((dQ > 0).all())
            if p.large:
                assert int(p.Q.max()) < (1 << 24) and bool(((p.Q + sign * dQ) != p.Q).all())      # check_partials compares exact sums
            else:
                st = N.gn_emulate_stats(p.S + sign * dS, p.Q + sign * dQ, p.cnt)
                assert _refused(lambda: N.check_stats(st, p.S, p.Q, p.cnt, fault)), f"{sid}: '{fault}' passes check_stats unseen"
        if not p.large:
            N.check_stats(N.gn_emulate_stats(p.S, p.Q, p.cnt, 4, 1, exact=True), p.S, p.Q, p.cnt, sid)
    doc = T.__doc__
    assert len(large) == 9 and all(sid in doc for sid in large), large


def test_check_partials():
    S = torch.tensor([[5] * 32, [-3] * 32])
    Q = torch.tensor([[9] * 32, [7] * 32])
    buf = torch.full((2 * 8, 64), float("nan"))
    N.check_partials(buf, 2, S, Q, "t", written=False)
    assert _refused(lambda: N.check_partials(buf, 2, S, Q, "t"))
    v = buf.view(-1)[:2 * 3 * 64].view(2, 3, 32, 2)
    v[:] = 0.0
    v[:, 0, :, 0], v[:, 2, :, 0] = 1.0, (S - 1).float()
    v[:, 1, :, 1], v[:, 2, :, 1] = 2.0, (Q - 2).float()
    assert N.check_partials(buf, 2, S, Q, "t") == 3
    assert _refused(lambda: N.check_partials(buf, 2, S, Q, "t", written=False))
    v[1, 1, 7, 1] += 1
    with pytest.raises(AssertionError, match="sample 1, group 7: the partial sums of squares"):
        N.check_partials(buf, 2, S, Q, "t")
    v[1, 1, 7, 1] -= 0.5
    assert _refused(lambda: N.check_partials(buf, 2, S, Q, "t")), "a partial that is no integer"
    v[1, 1, 7, 1] -= 0.5
    buf.view(-1)[2 * 3 * 64 + 5] = 0.0
    assert _refused(lambda: N.check_partials(buf, 2, S, Q, "t")), "a float behind the prefix"


def test_rne_bf16():
    y = torch.tensor([1.0, 1.00390625, 1.01171875, -1.00390625, 1.0039062500001, 3.0e-3, -255.5, 1.99609375 + 2.0 ** -9], dtype=N.F64)
    want = torch.tensor([1.0, 1.0, 1.015625, -1.0, 1.0078125, 0.0030059814453125, -256.0, 2.0], dtype=N.F64)
    assert torch.equal(N.rne_bf16(y), want), N.rne_bf16(y)
    r = torch.randn(100000, generator=N.gen("rne"), dtype=N.F64)
    assert torch.equal(N.rne_bf16(r.float().double()), r.float().to(torch.bfloat16).double())


@pytest.mark.parametrize("rows,c", T.LN_CASES + [(s.rows_per_sample, s.c) for s in T.RECORDED_LN])
def test_layer_norm_case_on_the_cpu(rows, c):
    p = N.ln_problem(rows, c, f"ln/{rows}x{c}")
    N.check_ln_out(N.ln_emulate(p), p, "the right result")
    bad = N.ln_emulate(p, skip_last_vector=True)
    assert _refused(lambda: N.check_ln_out(bad, p, "last vector")), f"ln {rows}x{c}: the last vector left out of the mean passes unseen"
    if c >= 2048:      # 8 values of |x| <= 2 move the mean by at most 16 / c sigma-units: 8e-3 of an output of order 1, under atol 2e-2
        close(bad, F.layer_norm(p.x.float(), (c,), p.gamma, p.beta, eps=1e-5), atol=2e-2, what="old bounds")
