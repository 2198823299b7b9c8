"""tests/_guard.py on CPU tensors: a passing check() means nothing unless a failing one is shown to fail.  Each violation a kernel
could commit is simulated with plain torch on the guarded views, and check() - or the finite-value check of close() - must fail
with the operand and the side named; an untouched run must pass; the payloads are the sizes tests/_extents.py gives."""
import pytest
import torch

import _extents as X
import _guard as G
from _checks import close

M, N, LD = 6, 8, 12


def _operands():
    ext = X.conv_gemm(a0=1, w=1, out=1, bias=1, batch=1, h_in=M, w_in=1, c0=64, N=N, out_ld=LD)
    g = G.Guard("cpu", ext)
    a0 = g.inp(torch.randn(M, 64).to(torch.bfloat16), "a0")
    bias = g.inp(torch.randn(N), "bias")
    out = g.out((M, N), torch.bfloat16, float("nan"), "out", ld=LD)
    return g, a0, bias, out


def _past(view, k):
    """The payload of `view` seen k elements further on each side: what a kernel's address arithmetic can reach."""
    flat_n = view.numel() if view.is_contiguous() else (view.shape[0] - 1) * view.stride(0) + view.shape[1]
    return torch.as_strided(view, (flat_n + 2 * k,), (1,), view.storage_offset() - k)


def test_untouched_run_passes():
    g, a0, bias, out = _operands()
    out.copy_((a0.float()[:, :N] + bias).to(torch.bfloat16))     # a well-behaved "kernel": writes its N columns only
    g.check()
    close(out, a0.float()[:, :N] + bias, what="well-behaved")


def test_write_behind_the_payload_is_caught():
    g, a0, bias, out = _operands()
    _past(out, 1)[-1] = 1.0
    with pytest.raises(AssertionError, match=r"'out' \(out\): tail band damaged, first byte at offset " + str(((M - 1) * LD + N) * 2)):
        g.check()


def test_write_in_front_of_the_payload_is_caught():
    g, a0, bias, out = _operands()
    _past(out, 1)[0] = 1.0
    with pytest.raises(AssertionError, match=r"'out' \(out\): front band damaged, first byte at offset -2 "):
        g.check()


def test_write_into_an_input_band_is_caught():
    g, a0, bias, out = _operands()
    _past(bias, 1)[-1] = 1.1
    with pytest.raises(AssertionError, match=r"'bias' \(in\): tail band damaged, first byte at offset " + str(N * 4)):
        g.check()


def test_write_into_a_row_gap_is_caught():
    g, a0, bias, out = _operands()
    torch.as_strided(out, (M, LD), (LD, 1))[2, N] = 0.25          # the 16-byte store past a ragged N edge
    with pytest.raises(AssertionError, match=r"'out' \(out\): row gap damaged, first byte at offset " + str((2 * LD + N) * 2) + r" .*row 2, column 8"):
        g.check()


def test_gaps_of_a_whole_row_operand_are_poisoned_and_checked():
    """vt-like operand: whole rows of ld elements, `used` of them carried (the last row's padding belongs to the operand too)."""
    g = G.Guard("cpu")
    t, ld = 5, 8
    vt = g.inp(torch.ones(3, ld, dtype=torch.bfloat16), label="vt")
    g.gaps(vt, t)
    assert bool(torch.isnan(vt[:, t:].float()).all()) and bool((vt[:, :t] == 1).all())
    g.check()
    vt[2, ld - 1] = 0.0
    with pytest.raises(AssertionError, match=r"'vt' \(in\): row gap damaged, first byte at offset " + str((2 * ld + ld - 1) * 2)):
        g.check()


def test_read_past_an_input_times_zero_reaches_the_result():
    """A "kernel" that reads one element past `bias` and multiplies it by a zero weight: 0 * NaN is NaN, close() refuses it; no band
    was written, so check() alone would pass - the NaN bands are what makes stray READS visible."""
    g, a0, bias, out = _operands()
    wide = _past(bias, 1)[1:]                                       # N + 1 elements: the last one is the band's
    weight = torch.cat([torch.ones(N), torch.zeros(1)])
    out.copy_((a0.float()[:, :N] + bias + (wide * weight)[-1]).to(torch.bfloat16))
    g.check()
    with pytest.raises(AssertionError, match="non-finite outputs"):
        close(out, a0.float()[:, :N] + bias, what="read past bias")


def test_integer_operands_carry_the_pattern():
    g = G.Guard("cpu")
    step = g.inp(torch.zeros(2, dtype=torch.int32), label="step_ptr")
    op = g.operands[0]
    assert bool((op.tail.view(torch.int32) == G.INT_PATTERN).all()) and bool((op.front.view(torch.int32) == G.INT_PATTERN).all())
    step += 1
    g.check()
    _past(step, 1)[-1] = 0
    with pytest.raises(AssertionError, match=r"'step_ptr' \(in\): tail band damaged, first byte at offset 8 "):
        g.check()


@pytest.mark.parametrize("op,kw,views", [
    ("conv_gemm", dict(a0=1, a1=1, w=1, out=1, out1=1, workspace=1, batch=2, h_in=12, w_in=20, c0=64, c1=128, N=192, ksize=3, splitk=3),
     dict(a0=((2, 12, 20, 64), torch.bfloat16, None), a1=((2, 12, 20, 128), torch.bfloat16, None), w=((192, 9 * 192), torch.bfloat16, None),
          out=((480, 192), torch.bfloat16, None), workspace=((3 * 480 * 192,), torch.float32, None))),
    ("attention", dict(q=1, k=1, vt=1, out=1, batch=2, heads=8, head_dim=40, s=72, t=77, q_ld=960, k_ld=320, vt_ld=80, o_ld=320),
     dict(q=((144, 320), torch.bfloat16, 960), k=((154, 320), torch.bfloat16, None), vt=((2, 320, 80), torch.bfloat16, None),
          out=((144, 320), torch.bfloat16, None))),
    ("group_norm", dict(x0=1, gamma=1, beta=1, stats=1, partials=1, out=1, sync=1, batch=3, hw=100, c0=512),
     dict(x0=((3, 100, 512), torch.bfloat16, None), stats=((3 * 64,), torch.float32, None), sync=((3 * 16384,), torch.int32, None))),
])
def test_payloads_and_bands_agree_with_the_extents(op, kw, views):
    ext = X.extents(op, **kw)
    g = G.Guard("cpu", ext)
    for name, (shape, dtype, ld) in views.items():
        v = g.out(shape, dtype, 0, name, ld=ld)          # (asserts payload == the header's bytes)
        o = g.operands[-1]
        esz = v.element_size()
        assert o.nbytes == ext[name][0]
        assert v.data_ptr() % G.ALIGN == 0, "the payload starts on the arena's alignment"
        assert o.tail.data_ptr() == v.data_ptr() + o.nbytes, "the tail band starts on the byte behind the payload"
        band = max(64 * 1024, 256 * (ld or shape[-1]) * esz)
        assert o.tail.numel() == band and o.front.numel() >= band
    g.check()
    with pytest.raises(AssertionError, match="bytes allocated, the header gives operand"):
        g.out((7,), torch.float32, 0, next(iter(views)))
