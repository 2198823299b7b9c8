"""What tests/_select.py promises, checked without a GPU: every draw of tests/test_attention_exact_gpu.py meets `conditions`; the CPU
emulation of the pinned arithmetic returns the expected bits on every case of at most _select.EMULATION_CAP = 2^20 scores per
(sample, head) (S, T <= 1024: the CPU suite stays quick; the long walks, 4090 / 4096 / 9216 and head_dim 512 at 2048, are held by
`conditions` alone); every fault of an attention kernel that the issue lists, applied INSIDE that emulation, is refused by the exact
comparison; and `_checks.close`, on test_ops_gpu.test_attention's own Gaussian draw at S = T = 4096, lets the first of them through -
which is why tests/test_attention_exact_gpu.py exists."""
import math

import pytest
import torch

import _select as S
from _checks import bf, close

BF16 = torch.bfloat16


def _refused(fn):
    try:
        fn()
    except AssertionError as e:
        return str(e)
    return None


def _draws():
    """(case, presc, m) of every msd_attention run, once."""
    seen = {}
    for _rid, case, _qf, presc, _form, m in S.attention_runs():
        seen.setdefault((S.case_name(case), presc, m), (case, presc, m))
    return list(seen.values())


DRAW_IDS = [f"{S.case_name(c)}-presc{int(p)}-ties{m}" for c, p, m in _draws()]


# ---- conditions -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,presc,m", _draws(), ids=DRAW_IDS)
def test_conditions_hold_for_every_attention_case(case, presc, m):
    p = S.attention_problem(case, presc, m)
    S.conditions(p)
    assert float(p.q.abs().max()) <= 8 and float(p.k.abs().max()) <= 8     # (the S = T = 9216 entry among them: nothing is left out)


def test_conditions_hold_for_every_other_case():
    from test_hypertile_gpu import GEOMETRIES, HEAD_DIMS

    for s, t, _ws, m in S.D512_RUNS:
        S.conditions(S.d512_problem(s, t, m), tile=32)
    for run in S.JOINT_RUNS:
        S.joint_conditions(S.joint_problem(*run))
    for geo in GEOMETRIES:
        for d in HEAD_DIMS:
            S.conditions(S.window_problem(geo, d))
    for shape in S.REGION_SHAPES:
        for R in S.REGION_COUNTS:
            S.region_conditions(S.region_problem(*shape, R))
    for shape in S.DECOUPLED_SHAPES:
        x = S.decoupled_problem(*shape)
        S.conditions(x.text)
        S.conditions(x.ip)
        for sc in S.DECOUPLED_SCALES:
            S.decoupled_expect(x, sc)
    for run in S.COLSUM_RUNS:
        S.colsum_conditions(S.colsum_problem(*run))
    for case in S.XATTN_CASES:
        S.xattn_conditions(S.xattn_problem(case))


def test_conditions_refuse_a_draw_that_breaks_them():
    def draw():
        return S.select("refuse", B=1, H=2, d=40, S=100, T=130, m=2)

    S.conditions(draw())
    p = draw()
    p.k = p.k / 2                                    # the gap halves
    p.a = p.a / 2
    assert "gap" in (_refused(lambda: S.conditions(p)) or "")
    p = draw()
    p.v[0, 5, 3] = 0.5                               # no integer
    assert "bf16 integers" in (_refused(lambda: S.conditions(p)) or "")
    p = draw()
    p.k[0, 7] = p.k[0, 9]                            # a third key with the codeword of key 9, in every head
    assert _refused(lambda: S.conditions(p)) is not None
    p = draw()
    p.expect[0, 0, 0] += 1
    assert "mean of V" in (_refused(lambda: S.conditions(p)) or "")
    p = draw()
    p.q[0, 0] = p.q[0, 1]                            # query 0 now selects query 1's key: pi no longer covers min(S, T) keys
    p.pi[0, :, 0] = p.pi[0, :, 1]
    p.expect[0, 0] = p.expect[0, 1]
    assert "distinct keys" in (_refused(lambda: S.conditions(p)) or "")


# ---- the emulation returns the expected bits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,presc,m", [x for x in _draws() if x[0]["S"] * x[0]["T"] <= S.EMULATION_CAP],
                         ids=[i for i, x in zip(DRAW_IDS, _draws()) if x[0]["S"] * x[0]["T"] <= S.EMULATION_CAP])
def test_emulated_attention_gives_the_expected_bits(case, presc, m):
    """msd_attention's lazy walk, with the row sum adding the rounded P (the ones-row forms) and the fp32 P (the others)."""
    p = S.attention_problem(case, presc, m)
    for round_l in (True, False):
        S.exact_rows(S.emulate_attention(p, presc=presc, round_l=round_l).to(BF16), p.expect, f"{p.id} round_l={round_l}", H=p.H, v=p.v)


def test_emulated_side_kernels_give_the_expected_bits():
    from test_hypertile_gpu import GEOMETRIES, HEAD_DIMS

    for s, t, _ws, m in S.D512_RUNS:
        if s * t <= S.EMULATION_CAP:
            p = S.d512_problem(s, t, m)
            S.exact_rows(S.emulate_attention(p, presc=False, round_l=False, tile=32).to(BF16), p.expect, p.id, H=1, v=p.v)
    for run in S.JOINT_RUNS:
        j = S.joint_problem(*run)
        S.exact_rows(S.emulate_joint(S.with_q(j.own, j.q), j.ref, S.JOINT_MIX).to(BF16), j.expect, j.id, H=j.H)
    for geo in GEOMETRIES:
        for d in HEAD_DIMS:
            p = S.window_problem(geo, d)
            S.exact_rows(S.emulate_windowed(p).to(BF16), p.expect, p.id, H=p.H, v=p.v)
    for shape in S.REGION_SHAPES:
        for R in S.REGION_COUNTS:
            r = S.region_problem(*shape, R)
            S.exact_rows(S.emulate_region([S.with_q(pt, r.q) for pt in r.parts], r.w).to(BF16), r.expect, r.id, H=r.H)
    for shape in S.DECOUPLED_SHAPES:
        x = S.decoupled_problem(*shape)
        for sc in S.DECOUPLED_SCALES:
            S.exact_rows(S.emulate_decoupled(S.with_q(x.text, x.q), x.ip, sc).to(BF16), S.decoupled_expect(x, sc), f"{x.id} sc={sc}", H=x.H)
    for case in S.XATTN_CASES:
        x = S.xattn_problem(case)
        S.exact_rows(S.emulate_attention(x.p, presc=True).to(BF16), x.p.expect, x.id, H=x.p.H, v=x.p.v)


# ---- the mutants --------------------------------------------------------------------------------------------------------------------
RAGGED = dict(B=1, H=4, d=40, S=200, T=520, spike=True)         # test_ops_gpu.ATTENTION_CASES: nine tiles, the last one of 8 keys
CAUSAL = S.ATTENTION_EXTRA[1]
WINDOWS = (24, 16, 12, 8)


def _last_key_tied_and_selected(p):
    """Key T - 1, the ragged tile's last: counted twice it shows only where it shares its codeword with a key of another tile (alone,
    numerator and row sum double together) - so the m = 2 draw, where it does and a query of head 0 selects the pair."""
    mem, pi = p.members[0][0], set(p.pi[0, 0].tolist())
    assert any(p.T - 1 in row.tolist() and any(int(x) in pi for x in row) for row in mem), "key T - 1 has no selected partner: another seed (_select.SALT)"
    return p.T - 1


def _two_rows_with_different_keys(p):
    i = next(i for i in range(p.S - 1) if int(p.pi[0, 0, i]) != int(p.pi[0, 0, i + 1]))
    return i, i + 1


MUTANTS = {
    "key 0 dropped": (RAGGED, 1, lambda p: dict(drop=(0,))),
    "key T - 1 dropped": (RAGGED, 1, lambda p: dict(drop=(p.T - 1,))),
    "the ragged tile's last key included twice": (RAGGED, 2, lambda p: dict(twice=_last_key_tied_and_selected(p))),
    "one query row reads its neighbour": (RAGGED, 1, lambda p: dict(row=_two_rows_with_different_keys(p))),
    "one head reads another head's V^T": (RAGGED, 1, lambda p: dict(head_v=(2, 3))),
    "one channel shifted": (RAGGED, 1, lambda p: dict(channel=17)),
    "causal mask off by one": (CAUSAL, 1, lambda p: dict(vis=torch.arange(p.T)[None, :] <= torch.arange(p.S)[:, None] + 1)),
    "a rescale skipped at one tile": (RAGGED, 1, lambda p: dict(skip_rescale=5)),
}


@pytest.mark.parametrize("name,presc", [(n, p) for n in MUTANTS for p in (True, False) if p or MUTANTS[n][1] == 1],   # (tied keys: prescaled only)
                         ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else f"presc{int(v)}")
def test_exact_rows_refuses_the_mutants(name, presc):
    """Each fault inside the emulated walk: the clean walk passes, the mutant is refused."""
    case, m, make = MUTANTS[name]
    p = S.attention_problem(case, presc, m)
    S.exact_rows(S.emulate_attention(p, presc=presc).to(BF16), p.expect, p.id, H=p.H, v=p.v)
    msg = _refused(lambda: S.exact_rows(S.emulate_attention(p, presc=presc, mutant=make(p)).to(BF16), p.expect, name, H=p.H, v=p.v))
    assert msg is not None and "differ from the selected row" in msg, f"{name}: not refused"


def test_exact_rows_refuses_a_window_that_admits_a_foreign_key():
    p = S.window_problem(WINDOWS, 40)
    foreign = int(p.geo.tokens[1][0])                                # window 0 also walks the first key of window 1
    S.exact_rows(S.emulate_windowed(p).to(BF16), p.expect, p.id, H=p.H, v=p.v)
    msg = _refused(lambda: S.exact_rows(S.emulate_windowed(p, mutant=dict(admit=(0, foreign))).to(BF16), p.expect, "foreign key", H=p.H, v=p.v))
    assert msg is not None and "differ from the selected row" in msg


def test_exact_rows_names_the_place_and_the_key():
    p = S.attention_problem(RAGGED, True, 1)
    got = p.expect.to(BF16).clone()
    S.exact_rows(got, p.expect, "clean", H=p.H, v=p.v)
    d = p.d
    got[0, 7, 2 * d:3 * d] = p.v[0, 11, 2 * d:3 * d].to(BF16)         # query 7, head 2 holds key 11's row
    msg = _refused(lambda: S.exact_rows(got, p.expect, "swap", H=p.H, v=p.v))
    assert msg is not None and "sample 0, query 7, head 2" in msg and "V of (sample 0, key 11, head 2)" in msg, msg
    near = p.expect.to(BF16).clone()
    near.view(torch.int16)[0, 3, 5] += 1                             # one bf16 ulp: refused at ulp = 0, let through at ulp = 1
    assert _refused(lambda: S.exact_rows(near, p.expect, "ulp", H=p.H)) is not None
    S.exact_rows(near, p.expect, "ulp", H=p.H, ulp=1)


# ---- and what `close` sees of the first mutant ---------------------------------------------------------------------------------------
def test_close_lets_the_dropped_key_through():
    """test_ops_gpu.test_attention's Gaussian draw for B = 1, H = 2, d = 40, S = T = 4096, spike, and its bound: a result in which EVERY
    query drops key 0 (renormalised) passes."""
    torch.manual_seed(7)
    B, H, d, Sq, T = 1, 2, 40, 4096, 4096
    C = H * d
    q, k, v = bf(torch.randn(B, Sq, C)), bf(torch.randn(B, T, C)), bf(torch.randn(B, T, C))
    k[:, T // 2 + 3] *= 6.0
    k[:, T - 5] *= 12.0
    k = bf(k)
    qh, kh, vh = S.split_heads(q, H), S.split_heads(k, H), S.split_heads(v, H)
    scores = (qh @ kh.transpose(-1, -2)) * d ** -0.5
    ref = (torch.softmax(scores, -1) @ vh).permute(0, 2, 1, 3).reshape(B, Sq, C)
    scores[..., 0] = -math.inf
    mutant = (torch.softmax(scores, -1) @ vh).permute(0, 2, 1, 3).reshape(B, Sq, C)
    assert not torch.equal(bf(mutant), bf(ref))
    close(mutant.to(BF16), ref, rtol=2e-2, atol=1.5e-2 * max(1.0, float(ref.abs().max())), what="key 0 dropped")
