"""Every attention kernel on selector operands (tests/_select.py): the output row of query i must be V[pi(i)], bit for bit.

tests/_checks.close on Gaussian operands lets a dropped key through from T of a few thousand on (tests/test_attention_exact_cpu.py);
here one wrong key, query row, head, sample, channel, mask or rescale moves the stored bf16 by whole integers.  The operands lie
between guard bands (tests/_guard.py, sized by tests/_extents*.py) with NaN in every padding region, as in the kernels' own tests,
whose launch helpers these tests use.  `_select.conditions` is asserted for every draw of this module by the CPU module
(test_conditions_hold_for_every_attention_case, test_conditions_hold_for_every_other_case), so a bad draw fails without a GPU; no case is left out: the S = T = 9216 entry of
test_ops_gpu.ATTENTION_CASES meets the conditions with |q|, |k| <= 8 (prescaled (4, 2), not prescaled (8, 4)).

What "exact" means, per form (read from the kernels).  The comparison is exact_rows with ulp = 0 everywhere: no tolerance appears in
this file.

  msd_attention, q_prescaled, m = 1, 2, 4 - every form (16x16x32: attention_kernel; 32x32x16 plain and software-pipelined:
      attention32_kernel, with its bf16 reference in the padding channel at d = 40): the scores are integers, the reference maximum is
      an integer (the padded form's a bf16 integer), so every exp2 argument is an integer.  Bit equality rests on
      __builtin_amdgcn_exp2f (v_exp_f32) returning the exact power of two for an integer argument on gfx950 - which these tests are
      the first to measure: then every P, every rescale factor exp2(-delta) and, with m tied keys, every row sum m 2^e is exact,
      whether the row sum adds the bf16-rounded P (the ones row of V^T: d = 40 everywhere, d = 80 on the 32x32x16 forms) or the fp32 one
      (d = 80 on 16x16x32, d = 160, d = 64) - a power of two is its own bf16.
  msd_attention, not prescaled, m = 1 - all forms, head_dim 512 with and without the four-way key split among them: the exp2 argument
      is fma(score, sl2, -(m_ref sl2)).  The match's tile always moves the reference onto the match (the gap is far above ATTN_THR), so
      P_match = exp2(e) with |e| <= half an ulp of score sl2 (<= 2^-13 at |score sl2| < 4096): bf16(P_match) = 1 exactly in the
      numerator.  Forms whose row sum adds the rounded P (ones row) divide by 1 + (less than 2^-12); the others by P_match (1 +
      |e| ln 2) + (less than 2^-12): either way the quotient is V[pi(i)] (1 + r), |r| < 2^-11, well inside half a bf16 ulp (2^-9) of an
      integer below 128 - the issue's one-ulp allowance for these forms is not needed, bit equality is asserted.  head_dim 512, m = 4
      with the workspace: one tied key per quarter, the four parts' references are the same float, the merge weights exp2(0) = 1,
      and sum V / (4 (1 + r)) rounds to the integer mean by the same argument.
  msd_attention_joint, msd_attention_windowed (prescaled by contract; the header pins P = bf16(exp2(score - m)) as the row sum's
      addend, the true running maximum, a rescale at every tile): bit equality; at mix = 0.5 fma(0.5, plain, 0.5 joint) of even integers.
  msd_region_attention (one tile per region, true maximum, rounded P in the row sum; acc = w O_r, then fma): bit equality; weights
      from {0, 1/4, 1/2, 1} and V in multiples of 4 keep every partial sum an integer (+ less than 2^-12).
  msdi_attention_decoupled (each probability 2^(x - max) (factor / sum), rounded once): the match's is bf16(1 / (1 + tiny)) = 1, the
      image one bf16(sc / (1 + tiny)) = sc for sc in {0.5, 2}: bit equality of V[pi(i)] + sc V_ip[rho(i)], |out| <= 255.
  msdx_attention_colsum (fp32 probabilities, no bf16 anywhere): with a gap above 157 every other probability is exp2 of less than
      -149 = 0.0f and the row sum is m exactly: out[b][j] = (pairs that select j) / (8 m), fp32 bits, zeros included.
  msd_cross_attention_q (m = 1): x one-hot rows of amplitude b, wq's columns codewords, ln_in partials with sum 0 and sum of squares
      c: q = rsqrt(1 + eps) b c_pi(i), which bf16 rounds back to b c_pi(i); then the prescaled attention above: bit equality.

Observed on the MI355X (gfx950): every test of this module passes at ulp = 0 - v_exp_f32 returned the exact power of two for every
integer argument these draws produce (hundreds below the reference, up to ATTN_THR above it), so the fallback the issue allows (tied draws at one bf16 ulp) is not used, and
the forms whose row sum adds the fp32 P gave the integer's bits too.  No kernel needed a fix."""
import pytest
import torch

import _select as S
import test_hypertile_gpu as TW
import test_ip_adapter_gpu as TI
import test_ops_gpu as TO
import test_reference_only_gpu as TJ
import test_region_attention_gpu as TR
import test_sag_gpu as TS
from conftest import run_calls

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAN = float("nan")


def up8(n):
    return (n + 7) // 8 * 8


@pytest.mark.parametrize("rid,case,qf,presc,form,m", [pytest.param(*r, id=r[0]) for r in S.attention_runs()])
def test_attention(gpu, rid, case, qf, presc, form, m):
    """msd_attention: every (case, qf, form) of test_ops_gpu.test_attention, prescaled with m = 1, 2, 4 and not prescaled with m = 1,
    and the CLIP head size with and without the causal mask (decoys behind the mask: a leaking mask turns the row into a mean)."""
    from minsdtf_amd import _lib, ops

    p = S.attention_problem(case, presc, m)
    H, d, T = p.H, p.d, p.T
    _lib.load().msd_set_option(b"attn_qf", qf)
    _lib.load().msd_set_option(b"attn_form", form)
    try:   # q inside a 3C-wide buffer, V^T's padding keys [T, Tp): NaN, then zeros
        a, b = TO.attention_ab(gpu, lambda **o: ops.attention(scale=d ** -0.5, q_prescaled=presc, causal=bool(case.get("causal")), **o),
                               p.q, p.k, p.v, H=H, d=d, q_ld=3 * H * d, vt_ld=up8(T))
    finally:
        _lib.load().msd_set_option(b"attn_qf", 0)
        _lib.load().msd_set_option(b"attn_form", 2)
    S.exact_rows(a[2], p.expect, rid, H=H, v=p.v)
    TO.same_bits_whatever_the_padding(a, b, rid)


@pytest.mark.parametrize("s,t,ws,m", S.D512_RUNS, ids=lambda v: str(int(v)))
def test_attention_d512(gpu, s, t, ws, m):
    """head_dim 512: a single workgroup, a ragged query tile, and S = T = 2048 without the workspace (one walk) and with it (the
    four-way key split merged in part order; m = 4: one tied key per quarter)."""
    from minsdtf_amd import ops

    p = S.d512_problem(s, t, m)
    what = f"d512 S={s} T={t} workspace={ws} m={m}"
    a, b = TO.attention_ab(gpu, lambda **o: ops.attention(scale=512 ** -0.5, **o), p.q, p.k, p.v, H=1, d=512, q_ld=512 + 8, vt_ld=t + 8, workspace=ws)
    S.exact_rows(a[2], p.expect, what, H=1, v=p.v)
    TO.same_bits_whatever_the_padding(a, b, what)
    if ws:
        assert not bool(torch.isnan(a[1]["workspace"]).all()), "the key split did not run"


@pytest.mark.parametrize("d,t,tr", S.JOINT_RUNS, ids=lambda v: str(v))
def test_attention_joint(gpu, d, t, tr):
    """msd_attention_joint: ragged own and reference segments; the three samples run mix = 0 (joint = V_ref[rho(i)]), 1 (plain =
    V[pi(i)], the reference not read) and 0.5 (their mean)."""
    j = S.joint_problem(d, t, tr)
    got = TJ.launch(gpu, j.q, j.own.k, j.own.v, j.ref.k[0], j.ref.v[0], S.JOINT_MIX, H=j.H, d=d, wide=True)
    for b, f in enumerate(S.JOINT_MIX):
        rows = j.own.v if f == 1.0 else (torch.cat([j.ref.v] * j.B) if f == 0.0 else None)
        S.exact_rows(got[b:b + 1].to(BF16), j.expect[b:b + 1], f"{j.id} sample {b} mix {f}", H=j.H, v=rows)


@pytest.mark.parametrize("d", TW.HEAD_DIMS, ids=TW.ids)
@pytest.mark.parametrize("geo", TW.GEOMETRIES, ids=TW.ids)
def test_attention_windowed(gpu, geo, d):
    """msd_attention_windowed: pi stays inside the query's window and EVERY other window holds a copy of the matched codeword with
    another V row - a window that admits a foreign key gives a mean or a foreign row."""
    p = S.window_problem(geo, d)
    h, w, wh, ww = geo
    got = TW.launch(gpu, p.q, p.k, p.v, heads=p.H, d=d, h=h, w=w, wh=wh, ww=ww, wide=True)
    S.exact_rows(got.to(BF16), p.expect, p.id, H=p.H, v=p.v)


@pytest.mark.parametrize("R", S.REGION_COUNTS)
@pytest.mark.parametrize("d,s,t", S.REGION_SHAPES, ids=lambda v: str(v))
def test_region_attention(gpu, d, s, t, R):
    """msd_region_attention: sum_r w_r V_r[pi_r(i)] with a pi of its own per region, dyadic weights, zero weights among them."""
    r = S.region_problem(d, s, t, R)
    C = r.H * d
    got = TR.launch(gpu, r.q, r.k, r.v, r.w, H=r.H, d=d, q_ld=3 * C, vt_ld=up8(t) + 8, o_ld=C + 16)
    S.exact_rows(got.cpu().to(BF16), r.expect, r.id, H=r.H)


@pytest.mark.parametrize("sc", S.DECOUPLED_SCALES)
@pytest.mark.parametrize("d,s,t,n", S.DECOUPLED_SHAPES, ids=lambda v: str(v))
def test_attention_decoupled(gpu, d, s, t, n, sc):
    """msdi_attention_decoupled: V[pi(i)] + sc V_ip[rho(i)]; sc from row 1, column 3 of a table whose other entries are NaN."""
    x = S.decoupled_problem(d, s, t, n)
    table = torch.full((2, 16), NAN)
    table[1, 3] = sc
    got = TI.launch(gpu, x.q, x.text.k, x.text.v, x.ip.k, x.ip.v, table, H=x.H, d=d, step=1, layer=3)
    S.exact_rows(got.to(BF16), S.decoupled_expect(x, sc), f"{x.id} sc={sc}", H=x.H, v=x.text.v if sc == 0 else None)


@pytest.mark.parametrize("s,m", S.COLSUM_RUNS, ids=lambda v: str(v))
def test_attention_colsum(gpu, s, m):
    """msdx_attention_colsum: out[b][j] = (the (head, query) pairs that select key j) / (8 m), fp32 bits - keys nobody selects get 0.0."""
    p = S.colsum_problem(s, m)
    lead = torch.zeros(1, s, p.H * p.d)               # (row 0 is never launched on: test_sag_gpu.colsum_run takes offset pointers)
    q, k = torch.cat([lead, p.q]).to(BF16), torch.cat([lead, p.k]).to(BF16)
    got, _gd = TS.colsum_run(gpu, (p.B, p.H, p.d, s), q, k)
    S.exact_rows(torch.from_numpy(got)[..., None], p.colsum[..., None], p.id)


@pytest.mark.parametrize("layout,nw", [(1, 4), (0, 4), (1, 8)])   # both weight layouts, both workgroup sizes (test_ops_gpu.test_cross_attention_q)
@pytest.mark.parametrize("case", S.XATTN_CASES, ids=S.case_name)
def test_cross_attention_q(gpu, case, layout, nw):
    """msd_cross_attention_q: the projection restores b c_pi(i) after its bf16 store, then the selector attention."""
    import _extents as X
    import _guard as G
    from minsdtf_amd import _lib, ops, packing

    x = S.xattn_problem(case)
    p, B, Sq, T, d, C = x.p, case["B"], case["S"], case["T"], case["d"], 8 * case["d"]
    Tp = up8(T)
    wf, cs, cb = packing.fold_layer_norm(x.wq.contiguous(), None, torch.ones(C).numpy(), torch.zeros(C).numpy(), gpu)
    geo = dict(batch=B, heads=8, head_dim=d, s=Sq, t=T, k_ld=C, vt_ld=Tp, o_ld=C, ln_in_slots=case["slots"])
    g = G.Guard(gpu, X.cross_attention_q(x=1, ln_in=1, wq=1, ln_colsum=1, bias=1, k=1, vt=1, out=1, **geo))
    stats = g.inp(x.ln_in, "ln_in")
    xd, kd = g.inp(x.x.to(BF16), "x"), g.inp(p.k.to(BF16), "k")
    wdev, cs, cb = g.inp(packing.chunk_major(wf) if layout else wf, "wq"), g.inp(cs, "ln_colsum"), g.inp(cb, "bias")
    vtf = torch.zeros(B, C, Tp, dtype=BF16)
    vtf[:, :, :T] = p.v.permute(0, 2, 1).to(BF16)
    vt = g.inp(vtf, "vt")
    g.gaps(vt, T)                                          # (padding keys hold NaN)
    out = g.out((B * Sq, C), BF16, NAN, "out")
    _lib.load().msd_set_option(b"xattn_nw", nw)
    try:
        run_calls(ops.cross_attention_q(x=xd, ln_in=stats, wq=wdev, ln_colsum=cs, bias=cb, k=kd, vt=vt, out=out, w_layout=layout, **geo))
    finally:
        _lib.load().msd_set_option(b"xattn_nw", 0)
    S.exact_rows(out.reshape(B, Sq, C), p.expect, f"{x.id} layout={layout} nw={nw}", H=8, v=p.v)
    g.check()
