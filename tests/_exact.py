"""Integer operands for the conv / GEMM kernels: draws on which every form must give the SAME bits as a float64 reference.

Small integers are exact in bf16 and so are their products; while every partial sum stays an integer below 2^24, fp32 addition
gives the same bits in any order, for any tile shape and any split-K.  One dropped, doubled or misplaced term changes an integer
sum by at least 1, so a comparison without a tolerance sees what `_checks.close` cannot: ONE wrong element of a long contraction
(tests/test_exact_cpu.py shows both halves of that sentence on CPU emulations).

Two draws, seeded per case id (`gen`):
  small   x in {-1, 0, 1}; w in {-1, +1} with density min(1, 2000 / K), zero elsewhere; bias, rowvec and residual integers in
          [-8, 8].  |result| <= 256, so the bf16 store is exact as well: for every form, bf16 or fp32 output.
  dense   x in [-4, 4], w in [-2, 2], the same epilogue operands: for fp32 outputs only.
`conditions` asserts, on the draw and the reference alone and before anything is compared, that the draw keeps these promises.  A
draw that breaks one is a bug of the test: give the case another seed (SALT), never a weaker condition.

The `*_problem` functions turn one entry of the forced-form lists of tests/test_ops_gpu.py into operands and reference; the GPU module
(tests/test_conv_exact_gpu.py) launches them and the CPU module walks them all, so a bad case fails without a GPU.

Plain torch on the CPU.  Not a conftest: imported by name."""
import types
import zlib

import torch

from test_ops_gpu import conv_ref

F64 = torch.float64
TWO24 = float(1 << 24)
BF16_EXACT = 256          # integers up to 2^8 are bf16 values (8 significand bits)
EPI = 8                   # bias, rowvec, residual: integers in [-EPI, EPI]
SMALL_NONZEROS = 2000     # expected non-zero weights per output column of the small draw
LN_MAX_OUT = 64           # test_conv_gemm_ln_out_exact: C * max|out|^2 < 2^24 for C <= 1280
DRAWS = ("small", "dense")

# case id -> added to its seed.  An entry is here because the case's first seed broke a condition (at K = 11,520 the small draw's
# weight density is 0.17: about one (K position, 64-column block) pair in 230,400 draws 64 zeros); found on the CPU by
# tests/test_exact_cpu.py, which fails for a case that needs one and has none.
SALT = {
    "conv_gemm/73/small": 1,   # K = 11,520: K position 272 had no non-zero weight in columns [64, 128)
    "conv_gemm/88/small": 2,   # K = 11,520: K position 10,883 had none in columns [448, 512)
}


def gen(case_id):
    """The case's own generator: crc32 of its id (+ SALT)."""
    return torch.Generator().manual_seed(zlib.crc32(case_id.encode()) + SALT.get(case_id, 0))


def ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(torch.float32)


def draw_x(g, shape, draw, density=None):
    """Activations.  density (small draw only): the share of non-zero entries, 2 / 3 by default (uniform over {-1, 0, 1})."""
    if draw == "dense":
        return ints(g, shape, -4, 4)
    if density is None:
        return ints(g, shape, -1, 1)
    return (ints(g, shape, 0, 1) * 2 - 1) * (torch.rand(tuple(shape), generator=g) < density)


def draw_w(g, shape, draw, K, density=None):
    """Weights of a contraction of length K (every operand of a launch's K counts: taps x channels + shortcut channels)."""
    if draw == "dense":
        return ints(g, shape, -2, 2)
    density = min(1.0, SMALL_NONZEROS / K) if density is None else density
    return (ints(g, shape, 0, 1) * 2 - 1) * (torch.rand(tuple(shape), generator=g) < density)


def epi(g, shape, bound=EPI):
    return ints(g, shape, -bound, bound)


def conditions(ref, w_nk, x_max, draw, what, *, n_epi=3, epi_bound=EPI, max_out=BF16_EXACT):
    """What exactness rests on.  ref: the float64 reference; w_nk: the weights [N][K]; x_max: max |x|; n_epi: epilogue operands."""
    N, K = w_nk.shape
    assert ref.dtype == F64 and ref.shape[-1] == N, what
    assert bool((ref == ref.round()).all()), f"{what}: the reference is not integer-valued"
    bound = K * x_max * float(w_nk.abs().max()) + n_epi * epi_bound            # >= sum |x| |w| + |epilogue| of every output
    assert bound < TWO24, f"{what}: partial sums up to {bound:.0f} >= 2^24"
    assert float(ref.abs().max()) <= bound, what
    if draw == "small":
        assert float(ref.abs().max()) <= max_out, f"{what}: max |ref| = {float(ref.abs().max()):.0f} > {max_out}: the bf16 store would round"
        nz = w_nk != 0
        for n0 in range(0, N, 64):
            cov = nz[n0:n0 + 64].any(0)
            assert bool(cov.all()), (f"{what}: K position {int((~cov).nonzero()[0])} has no non-zero weight in columns [{n0}, {min(n0 + 64, N)}) - "
                                     f"a wrong read there would go unseen (another seed: _exact.SALT)")
    else:
        assert draw == "dense", draw


def exact_equal(got, ref64, what):
    """got (fp32 or bf16, any device) against the float64 reference, bit for bit: the fp32 bits of ref, or the bits of its
    round-to-nearest-even bf16.  The last dimension is the column; everything in front of it the pixel."""
    got = got.detach().cpu()
    assert got.dtype in (torch.float32, torch.bfloat16), got.dtype
    assert ref64.dtype == F64 and tuple(got.shape) == tuple(ref64.shape), (what, tuple(got.shape), tuple(ref64.shape))
    want32 = ref64.to(torch.float32)
    assert torch.equal(want32.to(F64), ref64), f"{what}: the reference is no fp32 value"
    if got.dtype == torch.float32:
        same = got.contiguous().view(torch.int32) == want32.contiguous().view(torch.int32)
    else:
        same = got.contiguous().view(torch.int16) == want32.to(torch.bfloat16).contiguous().view(torch.int16)
    if bool(same.all()):
        return
    N = got.shape[-1]
    bad = (~same).reshape(-1, N)
    m, n = (int(v) for v in bad.nonzero()[0])
    g, r = float(got.reshape(-1, N)[m, n]), float(ref64.reshape(-1, N)[m, n])
    raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} outputs differ from the integer reference, first at pixel {m}, column {n}: "
                         f"got {g!r}, reference {r!r}, got - ref = {g - r!r}")


def w_rows(w_hwio):
    """HWIO -> the logical [N][K] matrix in pack order (packing.logical)."""
    return w_hwio.permute(3, 0, 1, 2).reshape(w_hwio.shape[3], -1)


# ---- the launches of tests/test_ops_gpu.py on these draws ---------------------------------------------------------------------------
RV_STEPS, RV_STEP = 3, 2      # rowvec: a table of 3 steps, *step_ptr = 2


def conv_reference(case, xin, w, bias=None):
    """test_conv_gemm's reference (upsample, stride, the VAE encoder's bottom / right padding) in float64."""
    import torch.nn.functional as F

    stride, ks = case.get("stride", 1), case["ks"]
    xin, w = xin.to(F64), w.to(F64)
    bias = None if bias is None else bias.to(F64)
    if case.get("asym"):
        return conv_ref(F.pad(xin, (0, 0, 0, 1, 0, 1)), w, bias, stride=stride, pad=0)
    return conv_ref(xin, w, bias, stride=stride, pad=1 if ks == 3 else 0, upsample=case.get("upsample", False))


def conv_gemm_problem(case, draw, case_id):
    """An entry of test_ops_gpu.CONV_GEMM_CASES: a0 | a1 -> conv + bias + rowvec[step 2] + residual, no activation."""
    g = gen(case_id)
    B, H, W, c0, N, ks = case["B"], case["H"], case["W"], case["c0"], case["N"], case["ks"]
    c1 = case.get("c1", 0)
    K = ks * ks * (c0 + c1)
    p = types.SimpleNamespace(draw=draw, K=K, N=N)
    p.x0 = draw_x(g, (B, H, W, c0), draw)
    p.x1 = draw_x(g, (B, H, W, c1), draw) if c1 else None
    p.w = draw_w(g, (ks, ks, c0 + c1, N), draw, K)
    p.bias, p.rowvec = epi(g, (N,)), epi(g, (RV_STEPS, B, N))
    p.xin = torch.cat([p.x0, p.x1], dim=-1) if c1 else p.x0
    conv = conv_reference(case, p.xin, p.w)
    p.Ho, p.Wo = conv.shape[1], conv.shape[2]
    p.resid = epi(g, (B, p.Ho, p.Wo, N))
    p.ref = conv + p.bias.to(F64) + p.rowvec[RV_STEP].to(F64)[:, None, None, :] + p.resid.to(F64)
    conditions(p.ref, w_rows(p.w), float(p.xin.abs().max()), draw, case_id)
    return p


def shortcut_problem(case, draw, case_id):
    """An entry of CONV_GEMM_SHORTCUT_CASES: conv(h) + conv1x1(x0 | x1) as one contraction, K = taps of h, then the channels of x0 | x1."""
    g = gen(case_id)
    B, H, W, c, N, ks = case["B"], case["H"], case["W"], case["c"], case["N"], case["ks"]
    cx0, cx1 = case["cx0"], case["cx1"]
    K = ks * ks * c + cx0 + cx1
    p = types.SimpleNamespace(draw=draw, K=K, N=N)
    p.h = draw_x(g, (B, H, W, c), draw)
    p.x0 = draw_x(g, (B, H, W, cx0), draw)
    p.x1 = draw_x(g, (B, H, W, cx1), draw) if cx1 else None
    p.w2 = draw_w(g, (ks, ks, c, N), draw, K)
    p.wsc = draw_w(g, (1, 1, cx0 + cx1, N), draw, K)
    p.bias = epi(g, (N,))
    xin = torch.cat([p.x0, p.x1], dim=-1) if cx1 else p.x0
    p.w_nk = torch.cat([w_rows(p.w2), w_rows(p.wsc)], dim=1).contiguous()
    p.ref = conv_reference(case, p.h, p.w2) + conv_ref(xin.to(F64), p.wsc.to(F64), None, pad=0) + p.bias.to(F64)
    conditions(p.ref, p.w_nk, max(float(p.h.abs().max()), float(xin.abs().max())), draw, case_id, n_epi=1)
    return p


def dense_problem(M, K, N, draw, case_id, *, bias=False, resid=False, x_density=None, epi_bound=EPI, max_out=BF16_EXACT):
    """x [M][K] @ w [K][N] (+ bias) (+ residual): the Dense launches (q | k | v^T split, the LayerNorm-fold producer)."""
    g = gen(case_id)
    p = types.SimpleNamespace(draw=draw, K=K, N=N)
    p.x = draw_x(g, (M, K), draw, density=x_density)
    p.w = draw_w(g, (K, N), draw, K)                      # Keras Dense layout (in, out)
    p.bias = epi(g, (N,), epi_bound) if bias else None
    p.resid = epi(g, (M, N), epi_bound) if resid else None
    p.ref = p.x.to(F64) @ p.w.to(F64)
    for t in (p.bias, p.resid):
        if t is not None:
            p.ref = p.ref + t.to(F64)
    conditions(p.ref, p.w.t(), float(p.x.abs().max()), draw, case_id, n_epi=int(bias) + int(resid), epi_bound=epi_bound, max_out=max_out)
    return p


def ln_out_problem(case, case_id):
    """The producer half of an entry of CONV_GEMM_LAYER_NORM_FOLD_CASES: Dense C -> C + bias (+ residual), bf16 out, and per slot (column
    tile) the (sum, sum of squares) of the stored row.  Squares: |out| <= 256 would reach 1280 * 2^16 > 2^24, so this draw is scaled to
    |out| <= 64 (x with about 96 non-zeros per row, epilogue operands in [-4, 4]) and C * 64^2 < 2^24 is asserted.  Returns the problem
    with .slot_cols (the header: slot j = column tile j of the launch; the row-panel form counts 64-column tiles)."""
    M, C = case["M"], case["C"]
    tm, tn, _ = case["tile"]
    p = dense_problem(M, C, C, "small", case_id, bias=True, resid=not case.get("nores"), x_density=min(2 / 3, 96 / C), epi_bound=4,
                      max_out=LN_MAX_OUT)
    assert C * LN_MAX_OUT ** 2 < TWO24, case_id
    p.slot_cols = 64 if 3000 <= tm < 4000 else tn
    p.slots = -(-C // p.slot_cols)
    parts = p.ref.split(p.slot_cols, dim=1)
    assert len(parts) == p.slots
    p.sums = torch.stack([t.sum(1) for t in parts], dim=1)                # [M][slots]
    p.squares = torch.stack([(t * t).sum(1) for t in parts], dim=1)
    return p


def direct_problem(case, draw, case_id):
    """An entry of CONV_DIRECT_CASES with in_scale = 1 and no activation: fp32 weights, input of sample b % mod, (+ residual).
    Fewer than 64 output channels (conv_out, 320 -> 4 at K = 2,880): every weight is non-zero, or no seed would cover every K position
    in a block of 4 columns; the few outputs keep max |ref| under 256 all the same (asserted)."""
    g = gen(case_id)
    B, mod, H, W, cin, cout = case["B"], case["mod"], case["H"], case["W"], case["cin"], case["cout"]
    ks, stride = case.get("ks", 3), case.get("stride", 1)
    K = ks * ks * cin
    p = types.SimpleNamespace(draw=draw, K=K, N=cout)
    p.x = draw_x(g, (mod, H, W, cin), draw)
    p.w = draw_w(g, (ks, ks, cin, cout), draw, K, density=1.0 if cout < 64 else None)
    p.bias = epi(g, (cout,))
    xb = p.x[torch.arange(B) % mod]
    p.ref = conv_ref(xb.to(F64), p.w.to(F64), p.bias.to(F64), stride=stride, pad=1 if ks == 3 else 0)
    p.Ho, p.Wo = p.ref.shape[1], p.ref.shape[2]
    p.resid = None
    if case.get("resid"):
        p.resid = epi(g, (B, p.Ho, p.Wo, cout))
        p.ref = p.ref + p.resid.to(F64)
    conditions(p.ref, w_rows(p.w), float(p.x.abs().max()), draw, case_id, n_epi=2)
    return p
