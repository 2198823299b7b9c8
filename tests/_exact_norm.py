"""Integer operands for the GroupNorm / LayerNorm kernels: draws on which every form's two moments are exact integers.

Activations are non-zero small integers.  A group's S = sum x and Q = sum x^2 are then integers far below 2^24, so fp32 addition
gives them exactly in any order, for any part count, chunking or placement; a dropped, doubled or misplaced term changes Q by at
least 1 and almost always S as well.  Both integers are read back from what the kernel publishes (cnt = hw * C / 32):
    S_rec = mean * cnt          Q_rec = (1 / rstd^2 - eps + mean^2) * cnt
and, where the three-launch path ran, directly from `partials`.  `_checks.close` with test_group_norm's bounds cannot see one wrong
term of these sums (tests/test_norm_exact_cpu.py shows both halves of that sentence on CPU emulations).

The draw (`gn_problem`, `ln_problem`; seeded per case id, `gen`): x iid uniform over {-2, -1, 1, 2} if 4 cnt < 2^19, else over
{-1, 1} (which needs cnt < 2^19; `large=True` lifts that for the VAE's largest stages, whose Q is then out of check_stats' reach); a
concat case draws one tensor and splits it at c0; gamma = 1 + 0.2 N(0, 1), beta = 0.2 N(0, 1) as test_group_norm draws them; eps =
1e-5 (the fp32 value the kernel is handed).  `conditions` asserts, on the draw and the float64 reference alone and before anything is
compared: no zero in x; Q < 2^19 and |S| < 2^21 for every (sample, group); mean^2 <= var in every group, so the kernel's formula
sq / cnt - mean * mean amplifies no rounding error; at most 3 % of a case's (sample, channel, x value) triples within `tol` of a bf16
rounding boundary.  A draw that breaks one is a bug of the test: give the case another seed (SALT), never a weaker condition.

check_stats bounds.
  |S_rec - S| <= |S| 2^-22, exactly 0 where S = 0: one fp32 division (half an ulp: 2^-24 relative) plus one ulp of margin.
  |Q_rec - Q| <= Q 2^-20: v_rsq_f32 is 1 ulp; the three roundings of var + eps (the quotient, the difference, the sum; mean^2 <= var
  keeps each at an ulp of var), halved by the square root, add at most 1.5 ulp; the total is taken as at most 4 ulp of rstd, which is
  8 ulp of 1 / rstd^2 - an ulp being at most 2^-23 of the value, 2^-20 of Q.  The fp32 values 4 ulp either side of the exact rstd
  give |Q_rec - Q| up to 15.98 x 2^-24 Q where rstd lies just above 1 (tests/test_norm_exact_cpu.py): the bound IS that budget, no
  more.  With Q < 2^19 the bound is below 0.5: a change of 1 in Q cannot pass.

check_out: (a) pixel independence, without a tolerance - for every (sample, channel) all pixels that hold the same x value carry the
same output bits (the map is ONE affine function per channel; every workgroup of a cluster, every part and every apply chunk
re-derives the statistics for itself, so a stale granule, another summation order in one part or a pixel normalised with its
neighbour group's statistics breaks this).  (b) the common value of each triple is the round-to-nearest-even bf16 of the float64
reference built from the exact S and Q, unless the reference lies within tol = 2^-16 (|x a| + |mean a| + |beta|), a = rstd gamma, of
a rounding boundary (x 1.1 with SiLU, the bound of its slope), where either neighbour passes: 1 / 256 of a bf16 ulp, 16 times a
16-ulp estimate of the fp32 chain.  check_ln_out: rule (b) per element with tol = 2^-16 (|(x - mean) rstd gamma| + |beta|).

Measured on an MI355X (tests/test_norm_exact_gpu.py, its first run, 156 launches, none refused; per kernel form the largest
|Q_rec - Q| / Q in units of 2^-24 - the bound is 16 - and how many of the near-tie triples took the reference's other neighbour):
  gn_group_kernel     <2,1> 3.11  <2,2> 2.32  <2,4> 3.38  <4,2> 3.02  <4,4> 2.85  <8,2> 2.82  <8,4> 3.07  <16,1> 2.65  <16,2> 3.02;  3 of 4072
  gn_cluster_kernel   <2,1> 3.14  <2,2> 3.32  <2,4> 3.00  <4,1> 3.25  <4,2> 2.54  <4,4> 3.49  <8,1> 2.95  <8,2> 3.19  <16,1> 3.27;  3 of 4438
  gn_rows_kernel      <2> 2.30  <4> 2.85  <6> 3.03;  4 of 2610
  three launches      <1> fused 3.25  <1> finalize 3.46  <2> finalize 3.58  wide fused 3.03;  0 of 896
  layer_norm_kernel   (publishes no statistics)  3 of 912 near-tie elements
The largest is 3.58: about one ulp of rstd (1.58 x 2^-24 of it at rstd = 0.633, doubled by the square), under a quarter of the
bound.  Among the triples NOT near a tie every stored value is the reference's bf16, so their error is the store's own rounding (the
largest seen 0.498 of a bf16 ulp); the fp32 chain's error shows only in the 13 of 12,928 near-tie triples that landed on the other
side of their boundary.

`gn_form` restates the host rule of msd_group_norm (csrc/norm.hip) - which kernel form a launch takes, with which template
arguments, parts and chunks - so that every GPU case can NAME the form it expects and the test can hold the signs the launch leaves
(tickets, partials) against it.

Plain torch / numpy on the CPU.  Not a conftest: imported by name."""
import collections
import types
import zlib

import numpy as np
import torch

F64 = torch.float64
EPS = float(np.float32(1e-5))
GROUPS = 32
Q_MAX = 1 << 19
S_MAX = 1 << 21
S_REL = 2.0 ** -22
Q_REL = 2.0 ** -20
TOL_REL = 2.0 ** -16
SILU_SLOPE = 1.1
TIE_CAP = 0.03

# case id -> added to its seed.  An entry is here because the case's first seed broke a condition; found on the CPU by
# tests/test_norm_exact_cpu.py, which fails for a case that needs one and has none.
SALT = {
    "gn/1x1031x8|312/silu": 1,   # 3.05 % of the triples near a rounding boundary (SiLU cases sit at 2 - 2.9 %)
}


def gen(case_id):
    """The case's own generator: crc32 of its id (+ SALT)."""
    return torch.Generator().manual_seed(zlib.crc32(case_id.encode()) + SALT.get(case_id, 0))


def draw_values(n):
    """The value set for sums of n terms."""
    return (-2, -1, 1, 2) if 4 * n < Q_MAX else (-1, 1)


def draw_x(g, shape, n, large=False):
    """int8, iid uniform over draw_values(n)."""
    assert large or n < Q_MAX, f"{n} terms: even x in {{-1, 1}} gives Q >= 2^19"
    if len(draw_values(n)) == 4:
        r = torch.randint(0, 4, tuple(shape), generator=g, dtype=torch.int8)      # 0 1 2 3 -> -2 -1 1 2
        return r - 2 + (r >= 2).to(torch.int8)
    return torch.randint(0, 2, tuple(shape), generator=g, dtype=torch.int8) * 2 - 1


# ---- round-to-nearest-even bf16 of a float64, and the test of a bf16 against a float64 +- tol ------------------------------------------
def rne_bf16(y):
    """float64 -> the nearest bf16 (ties to even) as float64, in ONE rounding (through fp32 there would be two).  Normal range only."""
    assert y.dtype == F64
    bits = y.contiguous().view(torch.int64)
    drop = 52 - 7
    bits = (bits + ((1 << (drop - 1)) - 1) + ((bits >> drop) & 1)) & ~((1 << drop) - 1)
    return bits.view(F64)


def _value_check(got, y, tol, what, names):
    """got (float64 values of the stored bf16) against y +- tol: got must lie in [rne(y - tol), rne(y + tol)] - where both ends are
    the same bf16 that is equality with rne(y), else y is near a rounding boundary and either neighbour passes.  Returns (near-tie
    mask, mask of those that took the other neighbour, |got - y| in bf16 ulps of y)."""
    lo, hi = rne_bf16(y - tol), rne_bf16(y + tol)
    near = lo != hi
    bad = (got < lo) | (got > hi) | ~torch.isfinite(got)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} values are not the bf16 of the float64 reference, first at "
                             f"{names(i)}: got {float(got[i])!r}, reference {float(y[i])!r} (bf16 {float(rne_bf16(y)[i])!r}), tol {float(tol[i]):.3g}")
    ulp = torch.exp2(torch.frexp(y.abs().clamp_min(1e-300))[1].to(F64) - 8)
    return near, near & (got != rne_bf16(y)), (got - y).abs() / ulp


# ---- GroupNorm -----------------------------------------------------------------------------------------------------------------------
def gn_moments(x):
    """(S, Q) int64 [B][32] of x int8 [B][hw][C]."""
    B, hw, C = x.shape
    S = torch.zeros(B, GROUPS, dtype=torch.int64)
    Q = torch.zeros(B, GROUPS, dtype=torch.int64)
    step = max(1, (1 << 24) // C)
    for a in range(0, hw, step):
        xs = x[:, a:a + step].view(B, -1, GROUPS, C // GROUPS)
        S += xs.sum((1, 3), dtype=torch.int64)
        Q += (xs * xs).sum((1, 3), dtype=torch.int64)      # int8: |x| <= 2
    return S, Q


def gn_reference(S, Q, cnt, gamma, beta):
    """float64 (mean [B][32], var, rstd, a [B][C], shift [B][C]) from the exact integers: out = x a + shift before SiLU."""
    cpg = gamma.numel() // GROUPS
    mean = S.to(F64) / cnt
    var = Q.to(F64) / cnt - mean * mean
    rstd = (var + EPS).rsqrt()
    a = rstd.repeat_interleave(cpg, 1) * gamma.to(F64)
    shift = beta.to(F64) - mean.repeat_interleave(cpg, 1) * a
    return mean, var, rstd, a, shift


def gn_ref_terms(p):
    """Per (sample, channel, value index): the float64 reference y [B][C][nv] and its tolerance."""
    vals = torch.tensor(p.values, dtype=F64)
    t1 = p.a[:, :, None] * vals                                          # x a
    pre = t1 + p.shift[:, :, None]
    mean_a = (p.beta.to(F64) - p.shift).abs()                            # |mean a|
    tol = TOL_REL * (t1.abs() + mean_a[:, :, None] + p.beta.to(F64).abs()[None, :, None])
    if p.silu:
        return pre * torch.sigmoid(pre), tol * SILU_SLOPE
    return pre, tol


def gn_problem(B, hw, c0, c1, silu, case_id, large=False):
    """One GroupNorm launch: x int8 [B][hw][C] (x0 = x[..., :c0], x1 the rest), gamma, beta fp32, the exact (S, Q) and the float64
    reference terms; the conditions asserted."""
    g = gen(case_id)
    C = c0 + c1
    p = types.SimpleNamespace(B=B, hw=hw, c0=c0, c1=c1, C=C, silu=bool(silu), cnt=hw * (C // GROUPS), large=large, id=case_id)
    p.values = draw_values(p.cnt)
    p.x = draw_x(g, (B, hw, C), p.cnt, large)
    p.gamma = torch.randn(C, generator=g) * 0.2 + 1
    p.beta = torch.randn(C, generator=g) * 0.2
    p.S, p.Q = gn_moments(p.x)
    p.mean, p.var, p.rstd, p.a, p.shift = gn_reference(p.S, p.Q, p.cnt, p.gamma, p.beta)
    p.y, p.tol = gn_ref_terms(p)
    conditions(p, case_id)
    return p


def x_parts(p):
    """(x0, x1) bf16, as the launch reads them."""
    x = p.x.to(torch.bfloat16)
    return x[..., :p.c0].contiguous(), (x[..., p.c0:].contiguous() if p.c1 else None)


def near_ties(y, tol):
    return rne_bf16(y - tol) != rne_bf16(y + tol)


def conditions(p, what):
    """What exactness rests on: asserted on the draw and the float64 reference alone."""
    assert p.x.dtype == torch.int8 and not bool((p.x == 0).any()), f"{what}: a zero in x"
    assert int(p.x.abs().max()) <= max(p.values)
    assert p.S.dtype == torch.int64 and p.Q.dtype == torch.int64
    assert int(p.S.abs().max()) < S_MAX, f"{what}: |S| = {int(p.S.abs().max())} >= 2^21"
    if not p.large:
        assert int(p.Q.max()) < Q_MAX, f"{what}: Q = {int(p.Q.max())} >= 2^19"
    else:
        assert p.values == (-1, 1) and bool((p.Q == p.cnt).all()) and p.cnt < (1 << 24), what
    assert bool((p.mean * p.mean <= p.var).all()), f"{what}: mean^2 > var in a group (another seed: _exact_norm.SALT)"
    share = float(near_ties(p.y, p.tol).double().mean())
    assert share <= TIE_CAP, f"{what}: {100 * share:.2f} % of the triples lie near a bf16 rounding boundary (another seed: _exact_norm.SALT)"
    p.tie_share = share


def recover(stats, cnt):
    """(S_rec, Q_rec) float64 [B][32] from the published {mean, rstd}."""
    st = stats.detach().cpu().reshape(-1, GROUPS, 2).to(F64)
    mean, rstd = st[..., 0], st[..., 1]
    return mean * cnt, (1.0 / (rstd * rstd) - EPS + mean * mean) * cnt


def check_stats(stats, S, Q, cnt, what, q_half=True):
    """The published {mean, rstd} [B][32][2] carry the exact integers (bounds: the module docstring).  q_half=False: the S half alone
    (cnt >= 2^19).  Returns the largest |Q_rec - Q| / Q in units of 2^-24."""
    assert bool(torch.isfinite(stats.detach().cpu()).all()), f"{what}: non-finite statistics"
    S_rec, Q_rec = recover(stats, cnt)
    assert S_rec.shape == S.shape, (what, S_rec.shape, S.shape)
    dS = (S_rec - S.to(F64)).abs()
    bad = dS > S.to(F64).abs() * S_REL
    if bool(bad.any()):
        b, g = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: sample {b}, group {g}: mean * cnt = {float(S_rec[b, g])!r}, the sum of the group is {int(S[b, g])} "
                             f"(recovered - exact = {float(S_rec[b, g]) - int(S[b, g]):.4f}; {int(bad.sum())}/{bad.numel()} groups)")
    if not q_half:
        return 0.0
    dQ = (Q_rec - Q.to(F64)).abs()
    bad = dQ > Q.to(F64) * Q_REL
    if bool(bad.any()):
        b, g = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: sample {b}, group {g}: (1 / rstd^2 - eps + mean^2) cnt = {float(Q_rec[b, g])!r}, the sum of squares of the "
                             f"group is {int(Q[b, g])} (recovered - exact = {float(Q_rec[b, g]) - int(Q[b, g]):.4f}, bound "
                             f"{int(Q[b, g]) * Q_REL:.4f}; {int(bad.sum())}/{bad.numel()} groups)")
    return float((dQ / Q.to(F64)).max()) * 2.0 ** 24


def check_partials(partials, B, S, Q, what, written=True):
    """The statistics pass writes [B][nchunks][32][2] floats compactly from the start of the NaN-prefilled buffer: the floats that are
    not NaN form a prefix whose length is a multiple of B * 64, each is an integer, and their float64 sum over the chunk axis is
    (S, Q) exactly.  written=False (a single-launch form): the whole buffer is still NaN.  Returns nchunks."""
    flat = partials.detach().reshape(-1)
    there = ~torch.isnan(flat)
    n = int(there.sum())
    if not written:
        assert n == 0, f"{what}: a single-launch form wrote {n} floats of `partials`"
        return 0
    assert n > 0, f"{what}: the statistics pass wrote nothing to `partials`"
    assert bool(there[:n].all()), f"{what}: the floats written to `partials` are no prefix of the buffer"
    assert n % (B * 64) == 0, f"{what}: {n} floats written to `partials`, no multiple of batch * 64"
    nchunks = n // (B * 64)
    v = flat[:n].cpu().to(F64).view(B, nchunks, GROUPS, 2)
    assert bool((v == v.round()).all()), f"{what}: a partial moment that is no integer"
    tot = v.sum(1)
    for m, want, name in ((0, S, "sums"), (1, Q, "sums of squares")):
        bad = tot[..., m] != want.to(F64)
        if bool(bad.any()):
            b, g = (int(i) for i in bad.nonzero()[0])
            raise AssertionError(f"{what}: sample {b}, group {g}: the partial {name} of {nchunks} chunks add up to {float(tot[b, g, m])!r}, "
                                 f"the group's is {int(want[b, g])} ({int(bad.sum())}/{bad.numel()} groups)")
    return nchunks


def check_out(out, x, ref_terms, what, values=None):
    """out bf16 [B][hw][C] against x int8 [B][hw][C] and ref_terms = (y, tol) [B][C][nv] (gn_ref_terms): pixel independence, then the
    representative values.  Runs where `out` lives.  Returns (near-tie triples that took the other neighbour / near-tie triples, the
    largest |got - y| in bf16 ulps among the triples not near a tie)."""
    y, tol = ref_terms
    B, hw, C = out.shape
    nv = y.shape[-1]
    values = values if values is not None else ((-2, -1, 1, 2) if nv == 4 else (-1, 1))
    assert out.dtype == torch.bfloat16 and tuple(x.shape) == (B, hw, C) and tuple(y.shape) == (B, C, nv)
    cpg = C // GROUPS
    dev = out.device
    bits = out.contiguous().view(torch.int16).to(torch.int32)
    xd = x.to(dev)
    rep = torch.zeros(B, C, nv, dtype=torch.int32, device=dev)
    have = torch.zeros(B, C, nv, dtype=torch.bool, device=dev)
    big = 1 << 20
    for k, v in enumerate(values):
        m = xd == v
        hi = torch.where(m, bits, -big).amax(1)
        lo = torch.where(m, bits, big).amin(1)
        have[..., k] = m.any(1)
        bad = have[..., k] & (hi != lo)
        if bool(bad.any()):
            b, c = (int(i) for i in bad.nonzero()[0])
            px = (m[b, :, c] & (bits[b, :, c] != bits[b, int(m[b, :, c].nonzero()[0]), c])).nonzero()
            raise AssertionError(f"{what}: sample {b}, channel {c} (group {c // cpg}): pixels that hold x = {v} carry different output bits, "
                                 f"first at pixel {int(px[0])} ({int(px.numel())} of {int(m[b, :, c].sum())} differ from the first; "
                                 f"{int(bad.sum())} (sample, channel) pairs) - the map is not one affine function per channel")
        rep[..., k] = hi
    rep, have = rep.cpu(), have.cpu()
    got = (rep.to(torch.int16).view(torch.bfloat16)).to(F64)
    got = torch.where(have, got, rne_bf16(y))                 # (a value no pixel of the channel holds: nothing to compare)
    near, other, err = _value_check(got, y, tol, what, lambda i: f"sample {i[0]}, channel {i[1]} (group {i[1] // cpg}), x = {values[i[2]]}")
    near, other = near & have, other & have
    clear = have & ~near
    return (int(other.sum()), int(near.sum())), float(err[clear].max()) if bool(clear.any()) else 0.0


# ---- which form msd_group_norm takes (csrc/norm.hip, restated) --------------------------------------------------------------------------
Form = collections.namedtuple("Form", ["kind", "name", "parts", "ppart", "nchunks", "xsh"])
# kind "group" | "cluster" | "rows" | "three"; parts: workgroups that share a (sample, group) / a sample by pixel range (three: the
# chunks of the statistics pass); ppart: their pixels; nchunks: chunks the statistics pass writes to `partials` (0: none)
GN_DEFAULTS = dict(impl=1, cluster=256, rows=9216, rows_q=-1, xmap=1, wide=1)


def _ceil(a, b):
    return -(-a // b)


def gn_form(B, hw, C, sync, **opt):
    o = dict(GN_DEFAULTS, **opt)
    cv, cpg = C // 8, C // GROUPS
    if o["rows"] > 0 and o["cluster"] and sync and hw >= o["rows"] and cv <= 512:
        r = 1024 // cv
        ps = 2
        while ps <= 6 and _ceil(_ceil(hw, 1 << ps), r) > 6:
            ps += 1
        if ps <= 6:
            ppart = _ceil(hw, 1 << ps)
            npt = _ceil(ppart, r)
            qs = 0
            if o["rows_q"] < 0:
                while qs < 2 and (B << (ps + qs)) < 256 and cv % (2 << qs) == 0 and ps + qs < 8:
                    qs += 1
            else:
                while qs < o["rows_q"] and qs < 2 and cv % (2 << qs) == 0 and ps + qs < 8:
                    qs += 1
            N = 2 if npt <= 2 else 4 if npt <= 4 else 6
            return Form("rows", f"rows<{N}> P={1 << ps} Q={1 << qs}", 1 << ps, ppart, 0, 0)
    if o["impl"] == 1 and cpg % 2 == 0 and cpg <= 160:
        dpp = cpg // 2
        V = 4 if dpp % 4 == 0 else 2 if dpp % 2 == 0 else 1
        ppp = 1024 // (dpp // V)
        lim = 8 if V == 4 else 16

        def N_(n):
            return 2 if n <= 2 else 4 if n <= 4 else 8 if n <= 8 else 16
        ps = 0
        if o["cluster"] and sync:
            P = min(hw // o["cluster"], 8)
            while (2 << ps) <= P:
                ps += 1
        if ps > 0:
            ppart = _ceil(hw, 1 << ps)
            nptc = _ceil(ppart, ppp)
            if nptc <= lim:
                bp = B << ps
                xsh = int(bool(o["xmap"]) and 8 <= bp <= 128 and bp & (bp - 1) == 0)
                return Form("cluster", f"cluster<{N_(nptc)},{V}> P={1 << ps}" + (" xcd" if xsh else ""), 1 << ps, ppart, 0, xsh)
        npt = _ceil(hw, ppp)
        if npt <= lim:
            return Form("group", f"group<{N_(npt)},{V}>", 1, hw, 0, 0)
    wide = bool(o["wide"]) and (1 << 20) <= hw * C <= (4 << 20) and C <= 2048
    NT = 1024 if wide else 256
    pl = NT // min(cv, 256)
    vpt = _ceil(cv, 256)
    small = hw * C <= (4 << 20)
    target = (128 if wide else 64) if small else 1024
    ppb = min(max(_ceil(hw, target), pl if wide else pl * 4), hw)
    nchunks = _ceil(hw, ppb)
    fused = nchunks <= (128 if wide else 64)
    assert fused or not wide, "the non-fused wide branch is unreachable: wide => hw C <= 4 Mi => at most 128 chunks"
    if wide:
        ppb_s = min(ppb * 4, hw)
        return Form("three", f"three wide fused {_ceil(hw, ppb_s)}/{nchunks} chunks", _ceil(hw, ppb_s), ppb_s, _ceil(hw, ppb_s), 0)
    return Form("three", f"three<{vpt}> {'fused' if fused else 'finalize'} {nchunks} chunks", nchunks, ppb, nchunks, 0)


# ---- what a kernel would leave: the formula restated in fp32, right or with a fault ------------------------------------------------------
def gn_emulate_stats(S, Q, cnt, rstd_ulps=0, mean_ulps=0, exact=False):
    """{mean, rstd} fp32 [B][32][2] from (possibly wrong) sums that are fp32 values, moved by whole ulps on request (a mean of 0 stays).
    exact=False: the kernel's formula evaluated in fp32, then moved.  exact=True: the fp32 value that lies AT MOST |rstd_ulps| ulp from
    the exact rstd on that side (the exact value moved, then rounded towards it)."""
    if exact:
        s, q, n = (np.asarray(t, dtype=np.float64) for t in (S, Q, cnt))
        mean = (s / n).astype(np.float32)
        r64 = 1.0 / np.sqrt(q / n - (s / n) ** 2 + EPS)
        moved = r64 + rstd_ulps * np.spacing(r64.astype(np.float32)).astype(np.float64)
        rstd = moved.astype(np.float32)
        beyond = (rstd.astype(np.float64) - moved) * np.sign(rstd_ulps) > 0
        rstd = np.where(beyond, np.nextafter(rstd, r64.astype(np.float32)), rstd).astype(np.float32)
    else:
        s, q, n = (np.asarray(t, dtype=np.float64).astype(np.float32) for t in (S, Q, cnt))
        mean = (s / n).astype(np.float32)
        var = np.maximum((q / n).astype(np.float32) - (mean * mean).astype(np.float32), np.float32(0)).astype(np.float32)
        rstd = (np.float32(1) / np.sqrt((var + np.float32(EPS)).astype(np.float32))).astype(np.float32)
        for _ in range(abs(rstd_ulps)):
            rstd = np.nextafter(rstd, np.float32(np.inf if rstd_ulps > 0 else 0))
    for _ in range(abs(mean_ulps)):
        mean = np.where(mean == 0, mean, np.nextafter(mean, np.float32(np.inf if mean_ulps > 0 else -np.inf))).astype(np.float32)
    return torch.from_numpy(np.stack([mean, rstd], -1))


def gn_emulate_out(p, stats, pixels=None, stats_there=None):
    """out bf16 [B][hw][C] in fp32 arithmetic from stats [B][32][2]; pixels [a, b) from stats_there instead."""
    cpg = p.C // GROUPS

    def apply(x, st):
        a = st[..., 1].repeat_interleave(cpg, 1) * p.gamma
        sh = p.beta - st[..., 0].repeat_interleave(cpg, 1) * a
        y = x.float() * a[:, None, :] + sh[:, None, :]
        return (y * torch.sigmoid(y) if p.silu else y).to(torch.bfloat16)
    out = apply(p.x, stats)
    if pixels is not None:
        a, b = pixels
        out[:, a:b] = apply(p.x[:, a:b], stats_there)
    return out


GN_FAULTS = ("last pixel", "chunk twice", "part statistics")


def gn_faulty(p, form, fault):
    """(stats, out or None) as a kernel with `fault` would leave them; `form` gives the parts (at least two are taken).
      last pixel       the statistics lose the last pixel of the last part
      chunk twice      the statistics count the first part / chunk twice
      part statistics  the published statistics are right, but the LAST part's pixels are normalised with the statistics of the other
                       parts alone (their own count: what a stale granule of an average part amounts to)"""
    P = max(2, form.parts)
    ppart = _ceil(p.hw, P)
    cnt = p.cnt
    if fault == "last pixel":
        dS, dQ = gn_moments(p.x[:, -1:])
        return gn_emulate_stats(p.S - dS, p.Q - dQ, cnt), None
    if fault == "chunk twice":
        dS, dQ = gn_moments(p.x[:, :ppart])
        return gn_emulate_stats(p.S + dS, p.Q + dQ, cnt), None
    if fault == "part statistics":
        first = (P - 1) * ppart
        while first >= p.hw:         # (ragged: the last part that holds a pixel)
            first -= ppart
        dS, dQ = gn_moments(p.x[:, first:])
        there = gn_emulate_stats(p.S - dS, p.Q - dQ, first * (p.C // GROUPS))
        st = gn_emulate_stats(p.S, p.Q, cnt)
        return st, gn_emulate_out(p, st, (first, p.hw), there)
    raise KeyError(fault)


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------
def ln_problem(rows, c, case_id):
    """x int8 [rows][c], gamma, beta, the exact row sums and the float64 reference y [rows][c] with its tolerance."""
    g = gen(case_id)
    p = types.SimpleNamespace(rows=rows, c=c, cnt=c, large=False, id=case_id)
    p.values = draw_values(c)
    p.x = draw_x(g, (rows, c), c)
    p.gamma = torch.randn(c, generator=g) * 0.2 + 1
    p.beta = torch.randn(c, generator=g) * 0.2
    xi = p.x.to(torch.int64)
    p.S, p.Q = xi.sum(1), (xi * xi).sum(1)
    p.mean = p.S.to(F64) / c
    p.var = p.Q.to(F64) / c - p.mean * p.mean
    p.rstd = (p.var + EPS).rsqrt()
    t1 = (p.x.to(F64) - p.mean[:, None]) * p.rstd[:, None] * p.gamma.to(F64)
    p.y = t1 + p.beta.to(F64)
    p.tol = TOL_REL * (t1.abs() + p.beta.to(F64).abs())
    conditions(p, case_id)
    return p


def check_ln_out(out, p, what):
    """out bf16 [rows][c]: every element is the bf16 of the float64 reference (either neighbour within tol of a rounding boundary).
    Returns as check_out."""
    got = out.detach().cpu().to(F64)
    assert tuple(got.shape) == tuple(p.y.shape), what
    near, other, err = _value_check(got, p.y, p.tol, what, lambda i: f"row {i[0]}, column {i[1]}")
    return (int(other.sum()), int(near.sum())), float(err[~near].max())


def ln_emulate(p, skip_last_vector=False):
    """The kernel's two passes in fp32; skip_last_vector: the row's last 8 channels are left out of the MEAN's sum."""
    x = p.x.float()
    s = (x[:, :-8] if skip_last_vector else x).sum(1)
    mean = s / p.c
    d = x - mean[:, None]
    rstd = ((d * d).sum(1) / p.c + EPS).rsqrt()
    return (d * rstd[:, None] * p.gamma + p.beta).to(torch.bfloat16)
