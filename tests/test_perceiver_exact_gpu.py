"""msdr_perceiver_attention on selector operands (tests/_select.py, tests/_select_perceiver.py): the output row of query i must be
V[pi(i)], bit for bit, whichever of the two key segments key pi(i) lies in.

On Gaussian operands a bound of a few bf16 ulps cannot see one wrong key among 273; here a key read from the wrong segment, head or
sample, a key dropped at the segment boundary or at a tile's edge, or a latent V row shifted by one moves the stored bf16 by whole
integers (tests/test_perceiver_exact_cpu.py shows it on an emulation of the pinned arithmetic, and asserts `conditions` for every draw
of this module, so a bad draw fails without a GPU).  The operands lie between guard bands with NaN in every padding column, every ld
larger than its width (test_ip_resampler_gpu.guarded).

What "exact" rests on: the matched key's score is the row maximum (with scale != 1 the product score * scale is the same float for
the maximum and for the key), so its probability is exp2(0) = 1; every other key's is at most 2^-G with (t_x + n) 127 2^-G <= 2^-12;
the row sum is 1 + (less than 2^-12), bf16(1 / sum) = 1, and V[pi(i)] + (less than 2^-12) rounds to the integer V[pi(i)] <= 127.  The
comparison is exact_rows with ulp = 0.

Observed on the MI355X (gfx950): every case passes at ulp = 0."""
import pytest
import torch

import _select as S
import _select_perceiver as SP
import test_ip_resampler_gpu as TR

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.mark.parametrize("run", SP.RUNS, ids=[SP.run_id(*r) for r in SP.RUNS])
def test_perceiver_attention(gpu, run):
    p = SP.problem(*run)
    SP.conditions(p)                                   # asserted on the operands before anything is compared
    kx, vx, kl, vl = SP.segments(p)
    got = TR.launch(gpu, p.q, kx, vx, kl, vl, H=p.H, scale=p.sl2)
    S.exact_rows(got.to(BF16), p.expect, p.id, H=p.H, v=p.v)
