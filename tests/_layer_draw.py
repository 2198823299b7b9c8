"""What tests/test_layer_launches_gpu.py draws, what it compares with and how: plain torch on the CPU, no device needed, so that
tests/test_layer_cases_cpu.py can show the comparison refusing a wrong result (and passing the legitimate rounding) at the very
shapes the GPU module launches.  Signatures and ids are those of tests/_layer_walk.py.  Not a conftest: imported by name.

Sample i of a case is drawn from a generator seeded by (signature id, i) alone: the same tensor at every batch."""
import hashlib
import math

import numpy as np
import torch
import torch.nn.functional as F

from _checks import bf, close

LOG2E = 1.4426950408889634
GROUPS = 32
EPS = 1e-5


def gen(sid, *what):
    g = torch.Generator()
    g.manual_seed(int.from_bytes(hashlib.sha256(repr((sid,) + what).encode()).digest()[:7], "little"))
    return g


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------------------
GN_SPIKE_HW = 1024   # samples of at most this many pixels get their last pixel scaled by 8: one pixel then moves the statistics


def gn_draw_sample(s, sid, i):
    """One sample [hw][C], bf16-rounded fp32: per-channel offsets N(0.3, 1) and scales U(0.5, 1.5) (a group's channels do not share a
    mean), a ramp 2 p / hw along the pixel index (a range of pixels left out moves the mean), and - hw <= 1024 - the last pixel x 8."""
    g = gen(sid, "sample", i)
    C = s.c0 + s.c1
    off = 0.3 + torch.randn(1, C, generator=g)
    std = 0.5 + torch.rand(1, C, generator=g)
    x = torch.randn(s.hw, C, generator=g)
    x.mul_(std).add_(off).add_((2.0 / s.hw) * torch.arange(s.hw, dtype=torch.float32)[:, None])
    if s.hw <= GN_SPIKE_HW:
        x[-1] *= 8.0
    return bf(x)


def gn_affine(s, sid):
    g = gen(sid, "affine")
    C = s.c0 + s.c1
    return torch.randn(C, generator=g) * 0.2 + 1, torch.randn(C, generator=g) * 0.2


def _gn_moments(x, rows=1 << 16):
    """float64 (mean, biased variance) per channel GROUP of x [n][C], in row chunks (the largest sample is 151 M values).  One pass,
    E[x^2] - mean^2: in float64 the cancellation costs 2^-53 mean^2 / var per term - nothing next to the fp32 bounds, since the draws
    keep mean^2 within a small multiple of the variance."""
    n, C = x.shape
    cpg = C // GROUPS
    tot = torch.zeros(GROUPS, dtype=torch.float64)
    sq = torch.zeros(GROUPS, dtype=torch.float64)
    for a in range(0, n, rows):
        xd = x[a:a + rows].double().view(-1, GROUPS, cpg)
        tot += xd.sum((0, 2))
        sq += (xd * xd).sum((0, 2))
    mean = tot / (n * cpg)
    return mean, sq / (n * cpg) - mean * mean


def gn_apply(s, x, mean, rstd, gamma, beta):
    """The affine step and SiLU in fp32 from given per-group {mean, rstd}: [hw][C] fp32."""
    cpg = x.shape[1] // GROUPS
    m = mean.float().repeat_interleave(cpg)
    a = rstd.float().repeat_interleave(cpg) * gamma
    y = (x - m).mul_(a).add_(beta)
    return y.mul_(torch.sigmoid(y)) if s.silu else y


def gn_reference(s, x, gamma, beta):
    """(out [hw][C] fp32, mean [32], rstd [32] float64) of one sample: statistics in float64, the rest in fp32."""
    mean, var = _gn_moments(x)
    rstd = (var + EPS).rsqrt()
    return gn_apply(s, x, mean, rstd, gamma, beta), mean, rstd


def gn_straddles(s):
    """The group that holds channels of both x0 and x1, or None."""
    cpg = (s.c0 + s.c1) // GROUPS
    return s.c0 // cpg if (s.c1 and s.c0 % cpg) else None


GN_FAULTS = ("last pixel", "last 64th", "x0 only")


def gn_emulate(s, x, gamma, beta, fault=None):
    """(out bf16 [hw][C], stats fp32 [32][2]) as a kernel would leave them.  fault None: the legitimate error, the output rounded to
    bf16.  "last pixel" / "last 64th": the last pixel / the last hw / 64 pixels are left out of the statistics; "x0 only": the group
    that straddles x0 | x1 takes its statistics from its x0 channels alone.  Returns None where the fault does not apply."""
    hw = s.hw
    if fault == "last pixel":
        if hw > GN_SPIKE_HW:
            return None
        mean, var = _gn_moments(x[:hw - 1])
    elif fault == "last 64th":
        mean, var = _gn_moments(x[:hw - max(1, hw // 64)])
    elif fault == "x0 only":
        gs = gn_straddles(s)
        if gs is None:
            return None
        mean, var = _gn_moments(x)
        cpg = (s.c0 + s.c1) // GROUPS
        part = x[:, gs * cpg:s.c0].double()
        mean[gs], var[gs] = part.mean(), part.var(unbiased=False)
    else:
        assert fault is None, fault
        mean, var = _gn_moments(x)
    rstd = (var + EPS).rsqrt()
    out = gn_apply(s, x, mean, rstd, gamma, beta).to(torch.bfloat16)
    return out, torch.stack([mean, rstd], -1).float()


def gn_compare(out, stats, ref, mean, rstd, what):
    """The bounds of test_group_norm as it stands: close() with atol 2e-2 (rtol 1e-2, relative RMS 2^-7) on the output, {mean, rstd}
    within rtol 1e-3 (mean: + atol 1e-3).  out [..][hw][C], stats [..][32][2] against ref / mean / rstd of the same leading shape."""
    close(out, ref, atol=2e-2, what=what)
    st = stats.detach().float().cpu()
    np.testing.assert_allclose(st[..., 0].numpy(), mean.float().numpy(), rtol=1e-3, atol=1e-3, err_msg=f"{what}: group means")
    np.testing.assert_allclose(st[..., 1].numpy(), rstd.float().numpy(), rtol=1e-3, err_msg=f"{what}: group rstd")


# ---- attention -----------------------------------------------------------------------------------------------------------------------
ATTN_HEAD_SIZES = (40, 64, 80, 160, 512)
ATTN_FULL_EDGE = 256     # every other (sample, head): the first and the last 256 queries ...
ATTN_STRIDE = 37         # ... and every 37th between


def attn_draw_sample(s, sid, i):
    """(q [S][C], k [T][C], v [T][C]) of one sample, bf16-rounded fp32.  q ~ 2 N(0, 1): the scores q k^T / sqrt(d) have standard
    deviation 2, so neighbouring rows of the result differ by far more than the tolerance even where 9216 keys are averaged; the last
    key and the first key of the last 64-key tile are scaled by 2 (scores of standard deviation 4: for some queries each of them
    carries a share of the softmax no tolerance hides).  q is what the engine hands the kernel: bf16(q scale log2 e) where the
    record says prescaled."""
    g = gen(sid, "sample", i)
    C = s.heads * s.head_dim
    q = 2.0 * torch.randn(s.s, C, generator=g)
    k = torch.randn(s.t, C, generator=g)
    v = torch.randn(s.t, C, generator=g)
    k[s.t - 1] *= 2.0
    first = (s.t - 1) // 64 * 64
    if first != s.t - 1:
        k[first] *= 2.0
    if s.causal:   # only the last query sees the last key: that key lies along it, a score of about 6 in every head
        ql = q[s.s - 1].view(s.heads, s.head_dim)
        k[s.t - 1] = 0.125 * k[s.t - 1] + (ql * (6.0 / (s.scale * (ql * ql).sum(-1, keepdim=True)))).reshape(C)
    if s.q_prescaled:
        q = q * (s.scale * LOG2E)
    return bf(q), bf(k), bf(v)


def attn_score_scale(s):
    return math.log(2.0) if s.q_prescaled else s.scale


def attn_queries(S, full):
    """The query rows of a (sample, head) pair that are compared: all of them (`full`), or the first 256, the last 256 and every 37th
    between."""
    if full or S <= 2 * ATTN_FULL_EDGE:
        return torch.arange(S)
    return torch.cat([torch.arange(ATTN_FULL_EDGE), torch.arange(ATTN_FULL_EDGE, S - ATTN_FULL_EDGE, ATTN_STRIDE), torch.arange(S - ATTN_FULL_EDGE, S)])


def attn_blocks(B, H, S):
    """[(sample, head, query rows)]: every pair, (0, 0) and (B - 1, H - 1) with all their queries."""
    return [(b, h, attn_queries(S, (b, h) in ((0, 0), (B - 1, H - 1)))) for b in range(B) for h in range(H)]


def _attn_probs(s, q, k, h, idx):
    d = s.head_dim
    sc = (q[idx, h * d:(h + 1) * d] @ k[:, h * d:(h + 1) * d].t()) * attn_score_scale(s)
    if s.causal:
        sc.masked_fill_(torch.arange(s.t)[None, :] > idx[:, None], float("-inf"))
    sc -= sc.max(-1, keepdim=True).values
    return sc.exp_()


def attn_reference(s, q, k, v, h, idx):
    """fp32 softmax(q k^T) v of head h of one sample on the bf16-rounded inputs, query rows idx: [len(idx)][d]."""
    p = _attn_probs(s, q, k, h, idx)
    d = s.head_dim
    return (p @ v[:, h * d:(h + 1) * d]) / p.sum(-1, keepdim=True)


ATTN_FAULTS = ("last key", "last tile", "last row", "interior row")


def attn_emulate(s, q, k, v, h, fault=None):
    """Head h of one sample, all queries, as a kernel would leave it: P rounded to bf16 before P V, the output rounded to bf16 (fault
    None: the legitimate error).  "last key" / "last tile": the last key / the last 64-key tile is dropped from both sums; "last row":
    the last query row receives its neighbour's result; "interior row": row S / 2 is swapped with the one behind it."""
    d = s.head_dim
    p = bf(_attn_probs(s, q, k, h, torch.arange(s.s)))
    vh = v[:, h * d:(h + 1) * d]
    t0 = {None: s.t, "last key": s.t - 1, "last tile": (s.t - 1) // 64 * 64}.get(fault, s.t)
    den = p[:, :t0].sum(-1, keepdim=True)
    out = (p[:, :t0] @ vh[:t0]) / den.clamp_min(1e-30)
    out = out.to(torch.bfloat16)
    if fault == "last row":
        out[s.s - 1] = out[s.s - 2]
    elif fault == "interior row":
        i = s.s // 2
        out[[i, i + 1]] = out[[i + 1, i]]
    return out


def attn_compare(got, ref, what):
    """The bounds of test_attention / test_attention_d512 as they stand (rtol 2e-2, atol 1.5e-2 max(1, max|ref|), relative RMS 2^-7),
    on one (sample, head) block: max|ref| of a block is at most that of the whole tensor, so never a wider floor."""
    close(got, ref, rtol=2e-2, atol=1.5e-2 * max(1.0, float(ref.abs().max())), what=what)


# ---- cross_attention_q ---------------------------------------------------------------------------------------------------------------
def xattn_draw_sample(s, sid, i):
    """(x [S][C] rows in front of norm2, k [T][C], v [T][C]) of one sample, as test_cross_attention_q draws them."""
    g = gen(sid, "sample", i)
    C = s.heads * s.head_dim
    return bf(torch.randn(s.s, C, generator=g) * 1.5 + 0.3), bf(torch.randn(s.t, C, generator=g)), bf(torch.randn(s.t, C, generator=g))


def xattn_weights(s, sid):
    """(gamma, beta, wq (in, out) with scale log2 e folded in, fp32)."""
    g = gen(sid, "weights")
    C = s.heads * s.head_dim
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    wq = bf(torch.randn(C, C, generator=g) / math.sqrt(C))
    return gamma, beta, wq * ((s.head_dim ** -0.5) * LOG2E)


def xattn_reference(s, x, k, v, gamma, beta, wq):
    """LayerNorm -> Dense (q stored as bf16) -> softmax(q k^T) v of one sample in fp32: [S][C]."""
    H, d = s.heads, s.head_dim
    q = bf(F.layer_norm(x, (H * d,), gamma, beta, eps=EPS) @ wq)
    qh, kh, vh = (t.view(-1, H, d).permute(1, 0, 2) for t in (q, k, v))
    return (torch.softmax((qh @ kh.transpose(-1, -2)) * math.log(2.0), -1) @ vh).permute(1, 0, 2).reshape(s.s, H * d)


def xattn_compare(got, ref, what):
    """test_cross_attention_q's bound."""
    close(got, ref, rtol=2e-2, atol=1.5e-2 * max(1.0, float(ref.abs().max())), what=what)
