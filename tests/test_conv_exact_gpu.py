"""Every conv / GEMM kernel form on integer operands: the result equals a float64 reference BIT FOR BIT (tests/_exact.py).

tests/test_ops_gpu.py compares Gaussian operands through `close` and forms with each other bit by bit; one wrong element of a long
contraction - an off-by-one at a concat boundary, the last channel of a chunk, one lane's bias index, one tap at one image corner -
stays under that floor from K of a few thousand on, and two forms that share a loader or an epilogue share the fault
(tests/test_exact_cpu.py replays it).  Here the launches of its forced-form lists (the smallest shapes that reach each loader, ring
depth, ragged edge and slice split) run on draws whose every partial sum is an integer below 2^24: any order of sums, any tile and
any split-K must store the reference's bits, and a dropped or doubled term is off by at least 1.

  test_conv_gemm_exact                   every CONV_GEMM_CASES entry at its own tile_m / tile_n / stages / splitk / weight layout, with
                                         bias, rowvec (step 2 of 3), residual, no activation: small draw -> bf16, dense draw -> fp32
  test_conv_gemm_shortcut_operand_exact  every CONV_GEMM_SHORTCUT_CASES entry (K = taps of h, then the channels of x0 | x1), small draw
  test_conv_gemm_qkv_split_exact         the q | k | v^T epilogue: nq = 1, 0 and the qkv consumer tiles of the LayerNorm-fold list as
                                         plain launches; the padding columns of v^T keep their canary
  test_conv_gemm_ln_out_exact            the producer half of every CONV_GEMM_LAYER_NORM_FOLD_CASES entry: the stored row and EACH slot's
                                         (sum, sum of squares) over that slot's own columns
  test_conv_direct_exact                 every bf16- and fp32-output CONV_DIRECT_CASES entry, in_scale 1, no activation

Output types.  msd_conv_gemm's argument checks (csrc/conv_gemm.hip) take MSD_OUT_F32 for every form of a plain launch - tile, halo,
wreg, big and staged-halo big; a row-panel request with an fp32 output is not eligible and runs on the 128x64 tile - so the dense draw
runs on every CONV_GEMM_CASES entry.  The launches WITHOUT an fp32 output (the same checks refuse it), held to exactness through the
bf16 store of the small draw alone: the q | k | v^T split (split_mode) and the LayerNorm-fold producer (ln_out).  The shortcut-operand
list runs the small draw only as well: its epilogue is the plain one, whose fp32 store test_conv_gemm_exact covers on every form.
Not held to exactness at all, because their arithmetic is inexact on any operands: the SiLU, GEGLU and QuickGELU epilogues, the
LayerNorm-fold consumer (ln_in), conv_direct's uint8 store and an in_scale other than 1."""
import pytest
import torch

import _exact as E
import _extents as X
import _guard as G
from conftest import run_calls
from test_ops_gpu import CONV_DIRECT_CASES, CONV_GEMM_CASES, CONV_GEMM_LAYER_NORM_FOLD_CASES, CONV_GEMM_SHORTCUT_CASES

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAN = float("nan")

GEMM_PARAMS = [(i, draw) for i in range(len(CONV_GEMM_CASES)) for draw in E.DRAWS]
SHORTCUT_PARAMS = list(range(len(CONV_GEMM_SHORTCUT_CASES)))
# the existing test's two launches (rows inside wider buffers), then the qkv consumers of the LayerNorm-fold list with a tile of their own
QKV_PARAMS = [dict(nq=1), dict(nq=0)] + [dict(M=c["M"], C=c["C"], ctile=c["ctile"]) for c in CONV_GEMM_LAYER_NORM_FOLD_CASES
                                          if c["mode"] == "qkv" and c.get("ctile")]
LN_OUT_PARAMS = list(range(len(CONV_GEMM_LAYER_NORM_FOLD_CASES)))
DIRECT_PARAMS = [(i, draw) for i, c in enumerate(CONV_DIRECT_CASES) if c.get("out", "bf16") != "u8"
                 for draw in (E.DRAWS if c.get("out") == "f32" else E.DRAWS[:1])]


def gemm_id(i, draw):
    return f"conv_gemm/{i}/{draw}"


def shortcut_id(i):
    return f"shortcut/{i}"


def qkv_id(q):
    return "qkv/nq%d" % q["nq"] if "nq" in q else "qkv/%dx%d/%d-%d-%d" % (q["M"], q["C"], *q["ctile"])


def ln_out_id(i):
    return f"ln_out/{i}"


def direct_id(i, draw):
    return f"conv_direct/{i}/{draw}"


def qkv_problem(q):
    """(problem, B, S, Cin, C): the existing test's shapes for nq = 1 / 0, else one sample of M tokens, C -> 3 C."""
    if "nq" in q:
        B, S, Cin, C = 2, 77 if q["nq"] == 0 else 64, 128, 64
        return E.dense_problem(B * S, Cin, C * (2 + q["nq"]), "small", qkv_id(q), bias=True), B, S, Cin, C
    return E.dense_problem(q["M"], q["C"], 3 * q["C"], "small", qkv_id(q), bias=True), 1, q["M"], q["C"], q["C"]


@pytest.mark.parametrize("i,draw", GEMM_PARAMS, ids=[f"case{i}-{d}" for i, d in GEMM_PARAMS])
def test_conv_gemm_exact(gpu, i, draw):
    from minsdtf_amd import ops, packing

    case = CONV_GEMM_CASES[i]
    p = E.conv_gemm_problem(case, draw, gemm_id(i, draw))
    B, H, W, c0, N, ks = case["B"], case["H"], case["W"], case["c0"], case["N"], case["ks"]
    c1, stride, ups, splitk, asym = case.get("c1", 0), case.get("stride", 1), case.get("upsample", False), case.get("splitk", 1), case.get("asym", False)
    M = B * p.Ho * p.Wo
    f32out = draw == "dense"
    geo = dict(batch=B, h_in=H, w_in=W, c0=c0, c1=c1, N=N, ksize=ks, stride=stride, upsample=ups, rv_step_stride=B * N, rv_batch_stride=N,
               out_dtype=ops.OUT_F32 if f32out else ops.OUT_BF16, splitk=splitk, **(dict(pad=0, pad_end=1) if asym else {}))
    g = G.Guard(gpu, X.conv_gemm(a0=1, a1=p.x1, w=1, bias=1, rowvec=1, step_ptr=1, residual=1, out=1, workspace=1 if splitk > 1 else None,
                                 rv_steps=E.RV_STEPS, **geo))
    wp = packing.pack_conv(p.w.numpy(), gpu)
    wreg = 4000 <= case.get("tile_m", 0) < 5000
    wd = g.inp(packing.fragment_major(wp) if wreg else wp, "w")          # the wreg form reads the fragment-major image
    out = g.out((M, N), torch.float32 if f32out else BF16, NAN, "out")
    ws = g.out((splitk * M, N), torch.float32, NAN, "workspace") if splitk > 1 else None
    call = ops.conv_gemm(a0=g.inp(p.x0.to(BF16), "a0"), a1=g.inp(p.x1.to(BF16), "a1") if c1 else None, w=wd, w_layout=2 if wreg else 0,
                         bias=g.inp(p.bias, "bias"), rowvec=g.inp(p.rowvec, "rowvec"), step_ptr=g.inp(torch.tensor([E.RV_STEP], dtype=torch.int32), "step_ptr"),
                         residual=g.inp(p.resid.to(BF16), "residual"), act=ops.ACT_NONE, out=out, workspace=ws,
                         workspace_floats=0 if ws is None else ws.numel(), tile_n=case.get("tile_n", 0), tile_m=case.get("tile_m", 0),
                         stages=case.get("stages", 0), **geo)
    run_calls(call)
    E.exact_equal(out.reshape(B, p.Ho, p.Wo, N), p.ref, f"{gemm_id(i, draw)} {case}")
    g.check()


def test_one_wrong_weight_is_seen(gpu):
    """The comparison end to end, on the device: the K = 11,520 launch with ONE weight of the last column negated in the uploaded image
    (the centre tap's last channel) is refused, the message names that column and every difference is +-2 x, i.e. 0 or +-2."""
    from minsdtf_amd import ops, packing

    i = next(k for k, c in enumerate(CONV_GEMM_CASES) if c["c0"] == 1280 and not c.get("tile_m"))
    case = CONV_GEMM_CASES[i]
    p = E.conv_gemm_problem(case, "small", gemm_id(i, "small"))
    B, H, W, c0, N, splitk = case["B"], case["H"], case["W"], case["c0"], case["N"], case["splitk"]
    n = int(p.w[1, 1, c0 - 1].nonzero()[-1])
    assert n >= N - 64
    w = p.w.clone()
    w[1, 1, c0 - 1, n] *= -1
    M = B * H * W
    geo = dict(batch=B, h_in=H, w_in=W, c0=c0, N=N, ksize=3, splitk=splitk)
    g = G.Guard(gpu, X.conv_gemm(a0=1, w=1, bias=1, residual=1, out=1, workspace=1, **geo))
    out = g.out((M, N), BF16, NAN, "out")
    ws = g.out((splitk * M, N), torch.float32, NAN, "workspace")
    run_calls(ops.conv_gemm(a0=g.inp(p.x0.to(BF16), "a0"), w=g.inp(packing.pack_conv(w.numpy(), gpu), "w"),
                            bias=g.inp(p.bias + p.rowvec[E.RV_STEP, 0], "bias"), residual=g.inp(p.resid.to(BF16), "residual"), out=out, workspace=ws,
                            workspace_floats=ws.numel(), **geo))
    g.check()
    with pytest.raises(AssertionError, match=rf"column {n}: .*got - ref = -?2\.0"):
        E.exact_equal(out.reshape(B, H, W, N), p.ref, "one weight negated")
    diff = out.reshape(B, H, W, N).double().cpu() - p.ref
    assert bool((diff[..., :n] == 0).all()) and bool((diff[..., n + 1:] == 0).all())
    assert torch.equal(diff[..., n], -2 * p.w[1, 1, c0 - 1, n].double() * p.x0[..., c0 - 1].double())


@pytest.mark.parametrize("i", SHORTCUT_PARAMS, ids=[f"case{i}" for i in SHORTCUT_PARAMS])
def test_conv_gemm_shortcut_operand_exact(gpu, i):
    from minsdtf_amd import ops, packing

    case = CONV_GEMM_SHORTCUT_CASES[i]
    p = E.shortcut_problem(case, "small", shortcut_id(i))
    B, H, W, c, N, ks = case["B"], case["H"], case["W"], case["c"], case["N"], case["ks"]
    cx0, cx1, sk = case["cx0"], case["cx1"], case.get("splitk", 1)
    M = B * H * W
    geo = dict(batch=B, h_in=H, w_in=W, c0=c, N=N, ksize=ks, c2=cx0, c3=cx1, splitk=sk)
    g = G.Guard(gpu, X.conv_gemm(a0=1, w=1, out=1, bias=1, a2=1, a3=p.x1, workspace=1 if sk > 1 else None, **geo))
    wreg = 4000 <= case.get("tile_m", 0) < 5000
    wcat = p.w_nk.to(BF16)
    wd = g.inp(packing.fragment_major(wcat) if wreg else wcat, "w")
    ws = g.out((sk * M, N), torch.float32, NAN, "workspace") if sk > 1 else None
    out = g.out((M, N), BF16, NAN, "out")
    call = ops.conv_gemm(a0=g.inp(p.h.to(BF16), "a0"), a2=g.inp(p.x0.to(BF16), "a2"), a3=g.inp(p.x1.to(BF16), "a3") if cx1 else None,
                         bias=g.inp(p.bias, "bias"), w=wd, w_layout=2 if wreg else 0, out=out, workspace=ws,
                         workspace_floats=0 if ws is None else ws.numel(), tile_m=case.get("tile_m", 0), tile_n=case.get("tile_n", 0),
                         stages=case.get("stages", 0), **geo)
    run_calls(call)
    E.exact_equal(out.reshape(B, H, W, N), p.ref, f"{shortcut_id(i)} {case}")
    g.check()


@pytest.mark.parametrize("q", QKV_PARAMS, ids=[qkv_id(q).split("/", 1)[1].replace("/", "-") for q in QKV_PARAMS])
def test_conv_gemm_qkv_split_exact(gpu, q):
    """q | k | v^T (nq = 0: k | v^T, nothing written through `out`): each part exact, the padding columns [S, Sp) of v^T untouched."""
    from minsdtf_amd import ops, packing

    p, B, S, Cin, C = qkv_problem(q)
    nq = q.get("nq", 1)
    N = p.N
    Sp = (S + 7) // 8 * 8
    ld = C + 8 if "nq" in q else C      # (the existing test: q and k rows inside wider buffers, the gaps hold a canary)
    tm, tn, stg = q.get("ctile", (0, 0, 0))
    geo = dict(batch=B, h_in=S, w_in=1, c0=Cin, N=N, out_ld=ld)
    g = G.Guard(gpu, X.conv_gemm(a0=1, w=1, bias=1, out=1, split=(C * nq, C, 1, ld, 1, Sp), **geo))
    qd = g.out((B * S, C), BF16, NAN, "out" if nq else None, ld=ld if ld > C else None, label="q")
    kd = g.out((B * S, C), BF16, NAN, "out1", ld=ld if ld > C else None)
    vt = g.out((B, C, Sp), BF16, NAN, "out2")
    g.gaps(vt, S)
    wp = packing.pack_dense(p.w.numpy(), gpu)
    wreg = 4000 <= tm < 5000
    call = ops.conv_gemm(a0=g.inp(p.x.to(BF16), "a0"), w=g.inp(packing.fragment_major(wp) if wreg else wp, "w"), w_layout=2 if wreg else 0,
                         bias=g.inp(p.bias, "bias"), out=qd, split=(C * nq, C, kd, ld, vt, Sp), tile_m=tm, tile_n=tn, stages=stg, **geo)
    run_calls(call)
    what = f"{qkv_id(q)}"
    ref = p.ref.reshape(B, S, N)
    if nq:
        E.exact_equal(qd.reshape(B, S, C), ref[:, :, :C].contiguous(), what + " q")
    else:
        assert bool(torch.isnan(qd.float()).all()), "part 0 has no columns: nothing is written through `out`"
    E.exact_equal(kd.reshape(B, S, C), ref[:, :, C * nq:C * (nq + 1)].contiguous(), what + " k")
    E.exact_equal(vt[:, :, :S].permute(0, 2, 1).contiguous(), ref[:, :, C * (nq + 1):].contiguous(), what + " v^T")
    g.check()


@pytest.mark.parametrize("i", LN_OUT_PARAMS, ids=[f"case{i}" for i in LN_OUT_PARAMS])
def test_conv_gemm_ln_out_exact(gpu, i):
    """The LayerNorm-fold producer: the stored bf16 row, and per slot the integer (sum, sum of squares) of that slot's own columns."""
    from minsdtf_amd import ops, packing

    case = CONV_GEMM_LAYER_NORM_FOLD_CASES[i]
    p = E.ln_out_problem(case, ln_out_id(i))
    M, C = case["M"], case["C"]
    tm, tn, stg = case["tile"]
    slots = ops.conv_gemm_ln_slots(N=C, tile_n=tn, tile_m=tm)
    assert slots == p.slots
    nores = p.resid is None
    geo = dict(batch=1, h_in=M, w_in=1, c0=C, N=C, ln_out_slots=slots)
    g = G.Guard(gpu, X.conv_gemm(a0=1, w=1, bias=1, residual=None if nores else 1, out=1, ln_out=1, **geo))
    out = g.out((M, C), BF16, NAN, "out")
    stats = g.out((M, slots, 2), torch.float32, NAN, "ln_out")
    wp = packing.pack_dense(p.w.numpy(), gpu)
    wreg = 4000 <= tm < 5000
    call = ops.conv_gemm(a0=g.inp(p.x.to(BF16), "a0"), w=g.inp(packing.fragment_major(wp) if wreg else wp, "w"), w_layout=2 if wreg else 0,
                         bias=g.inp(p.bias, "bias"), residual=None if nores else g.inp(p.resid.to(BF16), "residual"), out=out, ln_out=stats,
                         tile_m=tm, tile_n=tn, stages=stg, **geo)
    run_calls(call)
    what = f"{ln_out_id(i)} {case}"
    E.exact_equal(out, p.ref, what)
    E.exact_equal(stats[:, :, 0], p.sums, what + f": per-slot sums ({p.slot_cols} columns a slot)")
    E.exact_equal(stats[:, :, 1], p.squares, what + f": per-slot sums of squares ({p.slot_cols} columns a slot)")
    g.check()


@pytest.mark.parametrize("i,draw", DIRECT_PARAMS, ids=[f"case{i}-{d}" for i, d in DIRECT_PARAMS])
def test_conv_direct_exact(gpu, i, draw):
    from minsdtf_amd import ops

    case = CONV_DIRECT_CASES[i]
    p = E.direct_problem(case, draw, direct_id(i, draw))
    B, mod, H, W, cin, cout = case["B"], case["mod"], case["H"], case["W"], case["cin"], case["cout"]
    f32out = case.get("out", "bf16") == "f32"
    geo = dict(batch=B, in_batch_mod=mod, h_in=H, w_in=W, c_in=cin, c_out=cout, ksize=case.get("ks", 3), stride=case.get("stride", 1),
               in_dtype=ops.OUT_F32 if case["in_f32"] else ops.OUT_BF16, out_dtype=ops.OUT_F32 if f32out else ops.OUT_BF16)
    g = G.Guard(gpu, X.conv_direct(x=1, w=1, bias=1, residual=p.resid, out=1, **geo))
    out = g.out((B, p.Ho, p.Wo, cout), torch.float32 if f32out else BF16, NAN, "out")
    call = ops.conv_direct(x=g.inp(p.x if case["in_f32"] else p.x.to(BF16), "x"), w=g.inp(p.w, "w"), bias=g.inp(p.bias, "bias"), out=out, act=ops.ACT_NONE,
                           in_scale=1.0, residual=None if p.resid is None else g.inp(p.resid.to(BF16), "residual"), **geo)
    run_calls(call)
    E.exact_equal(out, p.ref, f"{direct_id(i, draw)} {case}")
    g.check()
