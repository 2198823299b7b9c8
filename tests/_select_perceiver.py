"""Selector operands (tests/_select.py, imported, not edited) for msdr_perceiver_attention: one softmax over two key segments - the
t_x keys of the x segment first, then the n latent keys - and n <= 16 queries.

A draw is ONE code book over the t_x + n keys of a (sample, head), in the concatenated order the header gives the softmax; the
launch gets keys [0, t_x) as k_x / vt_x and keys [t_x, t_x + n) as k_l / vt_l.  pi is a prefix of a permutation of the keys with n
distinct keys that holds, per (sample, head): key 0, the last x key, the first and the last latent key and - the kernel tiles the key
rows by MSDR_KEY_TILE = 16 - the first key of the x segment's ragged tile (`forced`).  So n must be at least the number of those
keys that differ: every case below is.  `conditions` = _select.conditions (with need_gap(t_x + n), the bf16-integer operands, the
distinct keys, the expectation = V[pi(i)]) plus the forced keys, asserted on the operands before anything is compared.  A draw that
breaks one gets another seed here (SALT), never a weaker condition.

`emulate` restates the arithmetic the header pins (fp32 scores times `scale` in one multiplication, the true maximum over both
segments, exp2, an fp32 row sum, each probability times 1 / sum rounded once to bf16, fp32 products with V, one rounding) with a
`mutant` hook for tests/test_perceiver_exact_cpu.py.

Plain torch on the CPU.  Not a conftest: imported by name."""
import types

import torch

import _select as S

F64 = torch.float64
D = 64                      # MSDR_HEAD_DIM
KEY_TILE = 16               # MSDR_KEY_TILE
MAX_TX = 272                # MSDR_MAX_TX
SL2_SCORES = D ** -0.5 * S.LOG2E   # the scale the resampler's plan passes (engine.emit_ip_resampler); 1.0: q carries it

# case id -> added to its seed (an entry is here because the case's first seed broke a condition; tests/test_perceiver_exact_cpu.py
# fails for a case that needs one and has none)
SALT = {}

# (batch, heads, n, t_x): the resampler's shape; a ragged x tile and a ragged latent chunk; whole tiles; the largest x segment; the
# smallest one (t_x = 1: key 0 IS the last x key)
SHAPES = [(2, 12, 16, 257), (2, 2, 5, 77), (1, 3, 16, 64), (2, 1, 8, MAX_TX), (2, 2, 3, 1), (1, 2, 9, 40)]
RUNS = [(B, H, n, t, sl2) for (B, H, n, t) in SHAPES for sl2 in (1.0, SL2_SCORES)]

_DRAWS = {}


def run_id(B, H, n, t, sl2):
    return f"B{B}-H{H}-n{n}-tx{t}-{'presc' if sl2 == 1.0 else 'scores'}"


def forced(t_x, n):
    """The keys (concatenated index) every pi must hold."""
    keys = {0, t_x - 1, t_x, t_x + n - 1}
    if t_x % KEY_TILE:
        keys.add(t_x // KEY_TILE * KEY_TILE)
    return sorted(keys)


def _gen(case_id):
    import zlib

    return torch.Generator().manual_seed(zlib.crc32(case_id.encode()) + SALT.get(case_id, 0))


def problem(B, H, n, t_x, sl2):
    """The draw of one launch: q [B][n][H 64], k / v [B][t_x + n][H 64] (x keys first), pi [B][H][n], expect [B][n][H 64] float64."""
    key = "perceiver/" + run_id(B, H, n, t_x, sl2)
    if key in _DRAWS:
        return _DRAWS[key]
    g = _gen(key)
    T = t_x + n
    heads = []
    for _b in range(B):
        row = []
        for _h in range(H):
            hd = types.SimpleNamespace(vis=None)
            hd.ck = S._signs(g, T, D)
            hd.pi = S._pi(g, n, T, forced(t_x, n))
            hd.v = S._values(g, T, D, torch.arange(T)[:, None], 1, S.VMAX)
            hd.want = hd.v[hd.pi].to(F64)
            row.append(hd)
        heads.append(row)
    p = types.SimpleNamespace(id=key, B=B, H=H, d=D, S=n, T=T, m=1, sl2=float(sl2), kind="plain", geo=None, step=1, vmax=S.VMAX, cover=None,
                              min_gap=S.need_gap(T), t_x=t_x, n=n, vis=None, ch=(0, D))
    unit = min(float(S.scan(hd.ck[hd.pi], hd.ck, hd.v, hd.pi).gap.min()) for row in heads for hd in row)
    p.a, p.b = next(((a, b) for a, b in S.AMPS if a * b * unit * p.sl2 >= p.min_gap), S.AMPS[-1])
    cat = lambda f: torch.stack([torch.cat([f(hd) for hd in row], -1) for row in heads])   # noqa: E731
    p.q, p.k, p.v = cat(lambda hd: p.b * hd.ck[hd.pi]), cat(lambda hd: p.a * hd.ck), cat(lambda hd: hd.v)
    p.expect = cat(lambda hd: hd.want)
    p.pi = torch.stack([torch.stack([hd.pi for hd in row]) for row in heads])
    p.members = [[torch.arange(T)[:, None] for _ in row] for row in heads]
    p.cid = [[torch.arange(T) for _ in row] for row in heads]
    _DRAWS[key] = p
    return p


def conditions(p):
    """_select.conditions (the gap need_gap(t_x + n) among them) and the forced keys of both segments; returns the smallest gap."""
    assert p.min_gap == S.need_gap(p.t_x + p.n) and 1 <= p.n <= 16 and 1 <= p.t_x <= MAX_TX, p.id
    G = S.conditions(p, tile=p.T)      # (tile = T: _select's own forced keys are then key 0 and key T - 1; ours follow)
    want = set(forced(p.t_x, p.n))
    assert len(want) <= p.n, f"{p.id}: {len(want)} forced keys and {p.n} queries"
    for b in range(p.B):
        for h in range(p.H):
            keys = set(p.pi[b, h].tolist())
            assert keys >= want, f"{p.id} [{b}][{h}]: pi misses {sorted(want - keys)} of the forced keys {sorted(want)}"
            assert any(k < p.t_x for k in keys) and any(k >= p.t_x for k in keys), f"{p.id} [{b}][{h}]: pi leaves a segment out"
    return G


def segments(p):
    """(k_x, v_x, k_l, v_l) of the draw: [B][t_x][C] and [B][n][C]."""
    return p.k[:, :p.t_x], p.v[:, :p.t_x], p.k[:, p.t_x:], p.v[:, p.t_x:]


def emulate(p, mutant=None):
    """msdr_perceiver_attention on the draw p in the pinned arithmetic.  mutant (a dict):
    v_segment      the latent keys' V rows are read from the head of the x segment (vt_l = vt_x)
    k_segment      the latent keys' K rows are read from the head of the x segment
    head_v=(h, h2) head h reads the V of head h2
    sample_k=(b, b2) sample b reads the keys of sample b2
    drop=(keys)    those keys (concatenated index) are treated as padding
    shift_l        latent key j reads the V row of latent key j + 1 (the last one: the first)"""
    mutant = mutant or {}
    qs, ks, vs = S.split_heads(p.q, p.H), S.split_heads(p.k, p.H), S.split_heads(p.v, p.H)
    scale = torch.tensor(p.sl2, dtype=torch.float32)
    t, n = p.t_x, p.n
    out = torch.zeros(p.B, p.H, n, D)
    for b in range(p.B):
        for h in range(p.H):
            qh, kh, vh = qs[b, h], ks[b, h].clone(), vs[b, h].clone()
            if "sample_k" in mutant and b == mutant["sample_k"][0]:
                kh = ks[mutant["sample_k"][1], h].clone()
            if "head_v" in mutant and h == mutant["head_v"][0]:
                vh = vs[b, mutant["head_v"][1]].clone()
            if mutant.get("v_segment"):
                vh[t:] = vh[:n] if t >= n else vh[torch.arange(n) % t]
            if mutant.get("k_segment"):
                kh[t:] = kh[:n] if t >= n else kh[torch.arange(n) % t]
            if mutant.get("shift_l"):
                vh[t:] = vh[t:].roll(-1, 0)
            s = (qh @ kh.t()) * scale                                   # fp32: integers below 2^24, then ONE multiplication
            for j in mutant.get("drop", ()):
                s[:, j] = S.NEG
            m = s.max(1, keepdim=True).values
            e = S.exp2(s - m)
            if mutant.get("drop"):
                e[:, list(mutant["drop"])] = 0.0
            c = 1.0 / e.sum(1, keepdim=True)
            out[b, h] = S.rbf(S.rbf(e * c) @ vh)
    return out.permute(0, 2, 1, 3).reshape(p.B, n, -1)
