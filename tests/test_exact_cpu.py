"""CPU tests (no GPU) of the exact comparison of tests/test_conv_exact_gpu.py: the check refuses what it must, and every GPU case's
draw keeps the conditions exactness rests on.

A passing check means nothing unless a failing one is shown to fail.  Five wrong kernels are emulated on the CPU, at a small, a
middle and a large contraction (K = 576, 2,880, 11,520), on both draws of tests/_exact.py:
  last column        the centre tap's last channel never read, for the LAST output column only (a ragged last column block)
  rowvec block       a 16-column block gets 5 % of the other sample's rowvec row (one sample: of the other step's)
  every output       the centre tap's last channel never read at all (the last channel of a 64-channel chunk)
  corner tap         the top-left tap of the image's top-left pixel reads its neighbour instead of the zero padding
  concat channel     the first channel behind a concat boundary (the channels taken as two halves) read from the other tensor
`exact_equal` refuses every one.  The last test replays test_conv_gemm's own Gaussian draw and bounds: `close` lets the "last
column" fault through at K = 2,880 and K = 11,520 - the reason tests/test_conv_exact_gpu.py exists.  If `close` is ever tightened
enough to see it, that test fails and says so."""
import math

import pytest
import torch

import _exact as E
from _checks import bf, close
from test_ops_gpu import conv_ref

SHAPES = [dict(B=2, H=16, W=16, c0=64, N=128, ks=3), dict(B=2, H=16, W=16, c0=320, N=320, ks=3), dict(B=1, H=8, W=8, c0=1280, N=1280, ks=3)]
SHAPE_IDS = ["K576", "K2880", "K11520"]
FAULTS = ("last column", "rowvec block", "every output", "corner tap", "concat channel")


def _refused(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def faulty(fault, x, w, rowvec_rows, ref):
    """The result a kernel with `fault` would give for conv(x, w) + epilogue = ref (3x3, stride 1, pad 1; any float dtype):
    x [B][H][W][cin], w HWIO, rowvec_rows [B][N] = for each sample the rowvec row the fault adds."""
    cin, N = x.shape[-1], w.shape[-1]
    got = ref.clone()
    if fault == "last column":       # (the last column whose weight there is not zero: a dropped zero is no fault; the draws' coverage
        n = int(w[1, 1, cin - 1].nonzero()[-1])   # condition puts it inside the last 64-column block)
        assert n >= N - 64
        got[..., n] -= x[..., cin - 1] * w[1, 1, cin - 1, n]
    elif fault == "rowvec block":
        got[..., 16:32] += 0.05 * rowvec_rows[:, None, None, 16:32]
    elif fault == "every output":
        got -= x[..., cin - 1:cin] * w[1, 1, cin - 1, :]
    elif fault == "corner tap":      # output pixel (0, 0) of sample 0, tap (ky, kx) = (0, 0): input (-1, -1) is padding; (0, 0) is read
        got[0, 0, 0, :] += x[0, 0, 0, :] @ w[0, 0]
    elif fault == "concat channel":  # channel c0 = cin / 2 of a0 | a1 is a1's first: read from a0's last (an off-by-one at the boundary)
        c0 = cin // 2
        xf = torch.zeros_like(x)
        xf[..., c0] = x[..., c0 - 1] - x[..., c0]
        got += conv_ref(xf, w, None, pad=1)
    else:
        raise KeyError(fault)
    return got


def _other_rowvec(rowvec, step):
    """[B][N]: the other sample's row of this step; with one sample, its row of the step before."""
    B = rowvec.shape[1]
    return rowvec[step].roll(1, 0) if B > 1 else rowvec[step - 1]


def _store(ref64, draw):
    """What a right kernel stores: bf16 for the small draw, fp32 for the dense one."""
    return ref64.to(torch.float32) if draw == "dense" else ref64.to(torch.float32).to(torch.bfloat16)


@pytest.mark.parametrize("draw", E.DRAWS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_exact_equal_refuses_the_faults(shape, draw):
    what = f"exact_cpu/{shape['c0']}/{draw}"
    p = E.conv_gemm_problem(shape, draw, what)
    E.exact_equal(_store(p.ref, draw), p.ref, what + ": the right result")
    x, w = p.xin.to(E.F64), p.w.to(E.F64)
    for fault in FAULTS:
        got = faulty(fault, x, w, _other_rowvec(p.rowvec, E.RV_STEP).to(E.F64), p.ref)
        assert not torch.equal(got, p.ref), (what, fault)
        assert _refused(lambda: E.exact_equal(_store(got, draw), p.ref, fault)), f"{what}: '{fault}' passes the exact comparison unseen"


def test_exact_equal_names_the_first_difference():
    """The message carries the (pixel, column), the count and the integer difference that points at the dropped term."""
    ref = torch.arange(24, dtype=E.F64).reshape(2, 3, 4)
    got = ref.clone()
    got[1, 0, 2] -= 3
    got[1, 2, 3] += 1
    with pytest.raises(AssertionError, match=r"2/24 outputs differ.*first at pixel 3, column 2: got 11\.0, reference 14\.0, got - ref = -3\.0"):
        E.exact_equal(got.to(torch.float32), ref, "t")
    with pytest.raises(AssertionError, match=r"2/24 outputs"):
        E.exact_equal(got.to(torch.bfloat16), ref, "t")
    E.exact_equal(ref.to(torch.bfloat16), ref, "t")
    assert _refused(lambda: E.exact_equal(-torch.zeros(1, 1), torch.zeros(1, 1, dtype=E.F64), "t")), "bit identity: -0 is not +0"


def test_conditions_refuse_a_draw_that_breaks_them():
    w = torch.ones(128, 64)
    ref = torch.full((4, 128), 7.0, dtype=E.F64)
    E.conditions(ref, w, 1.0, "small", "t")
    assert _refused(lambda: E.conditions(ref + 0.5, w, 1.0, "small", "t")), "a reference that is no integer"
    assert _refused(lambda: E.conditions(ref * 40, w, 1.0, "small", "t")), "|ref| > 256 on the small draw"
    E.conditions(ref * 40, w * 2, 4.0, "dense", "t")
    hole = w.clone()
    hole[64:, 5] = 0
    assert _refused(lambda: E.conditions(ref, hole, 1.0, "small", "t")), "a K position without a weight in one 64-column block"
    assert _refused(lambda: E.conditions(ref, w * 2, float(1 << 18), "dense", "t")), "partial sums that can reach 2^24"


# ---- every parametrised GPU case: the draw keeps the conditions (asserted inside the *_problem functions) ------------------------------
def test_conditions_hold_for_every_conv_gemm_case():
    import test_conv_exact_gpu as T

    assert len(T.GEMM_PARAMS) == 2 * len(T.CONV_GEMM_CASES)
    worst = 0.0
    for i, draw in T.GEMM_PARAMS:
        p = E.conv_gemm_problem(T.CONV_GEMM_CASES[i], draw, T.gemm_id(i, draw))
        if draw == "small":
            worst = max(worst, float(p.ref.abs().max()))
    print(f"\nconv_gemm: {len(T.GEMM_PARAMS)} draws, worst max |ref| of a small draw {worst:.0f}")


def test_conditions_hold_for_every_other_case():
    import test_conv_exact_gpu as T

    for i in T.SHORTCUT_PARAMS:
        E.shortcut_problem(T.CONV_GEMM_SHORTCUT_CASES[i], "small", T.shortcut_id(i))
    ids = [T.qkv_id(q) for q in T.QKV_PARAMS]
    assert len(set(ids)) == len(ids) and len(ids) >= 2 + 6, ids
    assert {q["ctile"][0] // 1000 for q in T.QKV_PARAMS if "ctile" in q} >= {3, 4, 5}, "row-panel, wreg and big consumers"
    for q in T.QKV_PARAMS:
        T.qkv_problem(q)
    for i in T.LN_OUT_PARAMS:
        p = E.ln_out_problem(T.CONV_GEMM_LAYER_NORM_FOLD_CASES[i], T.ln_out_id(i))
        assert float(p.ref.abs().max()) <= E.LN_MAX_OUT and float(p.squares.max()) < E.TWO24
        assert torch.equal(p.sums.sum(1), p.ref.sum(1)) and p.sums.shape == (p.ref.shape[0], p.slots)
    outs = {c.get("out", "bf16") for c in T.CONV_DIRECT_CASES}
    assert outs == {"bf16", "f32", "u8"}
    assert len({i for i, _ in T.DIRECT_PARAMS}) == sum(c.get("out", "bf16") != "u8" for c in T.CONV_DIRECT_CASES)
    for i, draw in T.DIRECT_PARAMS:
        E.direct_problem(T.CONV_DIRECT_CASES[i], draw, T.direct_id(i, draw))


# ---- why the GPU module exists --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES[1:], ids=SHAPE_IDS[1:])
def test_close_lets_the_last_column_fault_through(shape):
    """test_conv_gemm's draw (its seed first, then four more), reference and bounds; the kernel's legitimate error emulated by the bf16
    round of the output.  One product of w ~ N(0, 1 / K) is about |x| / sqrt(K), under `close`'s floor of 1 % of max |ref|, and the
    relative RMS spreads it over every right output: the fault passes.  If this fails, `close` has become able to see one wrong
    element of a long contraction - good; say so here."""
    B, H, W, c0, N, ks = (shape[k] for k in ("B", "H", "W", "c0", "N", "ks"))
    for seed in (1, 2, 3, 4, 5):
        torch.manual_seed(seed)
        x0 = bf(torch.randn(B, H, W, c0))
        w = bf(torch.randn(ks, ks, c0, N) / math.sqrt(ks * ks * c0))
        bias = torch.randn(N)
        ref = conv_ref(x0, w, bias, pad=1)
        temb = torch.randn(3, B, N)
        resid = bf(torch.randn(B, H, W, N))
        ref = ref + temb[2][:, None, None, :] + resid
        got = faulty("last column", x0, w, None, ref)
        assert int((got != ref).sum()) > 0.9 * B * H * W
        close(bf(ref).to(torch.bfloat16), ref, what="the right result")
        close(bf(got).to(torch.bfloat16), ref, what=f"seed {seed}: the last column's dropped product")
