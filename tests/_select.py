"""Selector operands for the attention kernels: draws on which every form must store the bits of V[pi(i)].

Every key j of a (sample, head) carries a codeword c_j in {-1, +1}^d; k_j = a c_j and q_i = b c_pi(i) with small integers a, b, so
q_i . k_j = a b (d - 2 hamming(pi(i), j)): key pi(i) beats every other key by 2 a b h_min at least.  With that gap G (in exp2 units)
at T 127 2^-G <= 2^-12 the other keys add less than 2^-12 to a row whose entries are integers in [1, 127]: the bf16 store gives
V[pi(i)] itself, and a wrong key, query row, head, sample or channel moves the stored bits by whole integers - which
tests/_checks.close cannot see on Gaussian operands (tests/test_attention_exact_cpu.py shows both halves of that sentence).

Draws, seeded per case id (`gen`; SALT as in tests/_exact.py):
  m = 1      one matching key per query.
  m = 2, 4   the match's codeword on m keys in different 64-key tiles (different m-ths of the walk: for the four-way key split of
             head_dim 512 its quarters), their V rows chosen so that the mean is an integer: in the q_prescaled form the scores are
             integers, so every P, every rescale factor and every row sum (m 2^e) is a power of two and the mean is exact.
  a different code book and a different pi per (sample, head); pi a prefix of a permutation of the keys (min(S, T) distinct keys)
  that holds key 0, key T - 1 and, where T % 64 != 0, the first key of the ragged tile.
  causal     pi(i) <= i, and for some queries a second copy of the matched codeword at a key > i with another V row (a decoy),
             for some of them at key i + 1.
  windows    one code book per window-local position: EVERY other window holds a decoy copy of the matched codeword.
`conditions` asserts, on the operands alone and before anything is compared, what exactness rests on.  A draw that breaks one is a
bug of the test: give the case another seed (SALT), never a weaker condition.

`emulate*` walk the keys on the CPU in the arithmetic the headers pin (64-key tiles; msd_attention's lazy reference, ATTN_THR = 8;
msd_attention_joint's always-rescale walk with its segment boundary; msd_region_attention's per-region fma; the once-rounded
probabilities of msdi_attention_decoupled), with a `mutant` hook for tests/test_attention_exact_cpu.py.

Plain torch on the CPU.  Not a conftest: imported by name."""
import math
import types
import zlib

import torch

F64 = torch.float64
LOG2E = 1.4426950408889634
TWO24 = float(1 << 24)
ATTN_THR = 8.0            # attention.hip: the lazy reference moves when a tile's maximum exceeds it by more than this (exp2 units)
TILE = 64
VMAX = 127
AMPS = [(1, 1), (2, 1), (2, 2), (4, 2), (4, 4), (8, 4), (8, 8)]   # (a, b): |k| = a, |q| = b; the smallest pair that opens the gap
NEG = -1e30               # what the kernels write over a masked score

# case id -> added to its seed.  An entry is here because the case's first seed broke a condition; found on the CPU by
# tests/test_attention_exact_cpu.py, which fails for a case that needs one and has none.
SALT = {}


def gen(case_id):
    """The case's own generator: crc32 of its id (+ SALT)."""
    return torch.Generator().manual_seed(zlib.crc32(case_id.encode()) + SALT.get(case_id, 0))


def need_gap(T):
    """The smallest G (exp2 units) with T 127 2^-G <= 2^-12."""
    return math.log2(T * VMAX) + 12.0


def forced_keys(T, tile=TILE):
    """Keys every pi must hold: the first, the last and the first of a ragged last tile."""
    return sorted({0, T - 1} | ({T // tile * tile} if T % tile else set()))


def _signs(g, n, d, hmin=None):
    """n codewords in {-1, +1}^d, any two at Hamming distance hmin at least (rows that come closer to an earlier row are drawn again):
    2 by default, 1 (distinct) where d < 16 leaves no room for more."""
    hmin = (2 if d >= 16 else 1) if hmin is None else hmin
    c = (torch.randint(0, 2, (n, d), generator=g) * 2 - 1).to(torch.float32)
    for _ in range(200):
        near = torch.zeros(n, dtype=torch.bool)
        for i0 in range(0, n, 2048):
            ham = (d - c[i0:i0 + 2048] @ c.t()) / 2
            earlier = torch.arange(n)[None, :] < torch.arange(i0, min(n, i0 + 2048))[:, None]
            near[i0:i0 + 2048] = ((ham < hmin) & earlier).any(1)
        if not bool(near.any()):
            return c
        c[near] = (torch.randint(0, 2, (int(near.sum()), d), generator=g) * 2 - 1).to(torch.float32)
    raise AssertionError(f"no {n} codewords of {d} bits at distance {hmin}")


def _edges(T, m):
    """The walk in m parts: whole 64-key tiles where it has m of them (T = 2048, m = 4: the quarters of the four-way key split)."""
    nt = -(-T // TILE)
    return [TILE * (nt * r // m) for r in range(m)] + [T] if nt >= m else [T * r // m for r in range(m + 1)]


def _groups(g, T, m):
    """(code id per key, members [n][m]): the keys of a group share a codeword, one member per m-th of the walk (whole 64-key tiles
    where the walk has m of them).  Keys left over stay alone under their own id."""
    cid = torch.arange(T)
    if m == 1:
        return cid, cid[:, None]
    edges = _edges(T, m)
    stripes = [edges[r] + torch.randperm(edges[r + 1] - edges[r], generator=g) for r in range(m)]
    n = min(len(s) for s in stripes)
    members = torch.stack([s[:n] for s in stripes], 1)
    for r in range(1, m):
        cid[members[:, r]] = members[:, 0]
    return cid, members


def _pi(g, S, T, forced, cover=None):
    """A prefix of a permutation of the keys that holds `forced`, in random query order; queries past its end start over.  The prefix
    has min(S, T) keys, or `cover` of them (msdx_attention_colsum: keys that no query selects, keys that several do)."""
    n = min(S, T) if cover is None else cover
    perm = torch.randperm(T, generator=g).tolist()
    keys = (list(forced) + [j for j in perm if j not in set(forced)])[:n]
    order = torch.randperm(n, generator=g)
    prefix = torch.tensor(keys)[order]
    return prefix[torch.arange(S) % n]


def _values(g, T, d, members, step, vmax):
    """V rows: multiples of `step` in [1, vmax] (2: for the joint blend at mix = 0.5 and the image term at sc = 0.5; 4: for region weights
    of 1/4); the last member of every group is moved by less than m steps so that the group's mean is such a multiple too."""
    v = (torch.randint(1, vmax // step + 1, (T, d), generator=g) * step).to(torch.float32)
    m = members.shape[1]
    if m > 1:
        r = v[members].sum(1) % (m * step)                    # [n][d]
        last = v[members[:, -1]] - r
        v[members[:, -1]] = torch.where(last < 1, last + m * step, last)
    return v


def _head(g, S, T, d, dv, m, kind, geo, step, vmax, cover):
    """One (sample, head): unit codewords (d bits) of the queries and keys, V (dv channels), pi, and the visibility of key j to query i
    (None: all)."""
    hd = types.SimpleNamespace(vis=None)
    if kind == "windows":
        tokens, L = geo.tokens, geo.tokens.shape[1]
        book = _signs(g, L, d)
        ck, pi = torch.zeros(T, d), torch.zeros(S, dtype=torch.long)
        for row in tokens:
            ck[row] = book
            pi[row] = row[_pi(g, L, L, forced_keys(L))]
        hd.ck, hd.pi, hd.v = ck, pi, _values(g, T, dv, torch.arange(T)[:, None], step, vmax)
        hd.vis = geo.win_of[:, None] == geo.win_of[None, :]
        hd.want = hd.v[pi].to(F64)
        return hd
    if kind == "causal":
        assert S == T and m == 1
        ck = _signs(g, T, d)
        i = torch.arange(S)
        below = (torch.rand(S, generator=g) * (i + 1)).long()                 # uniform in [0, i]
        pi = torch.where(torch.rand(S, generator=g) < 0.3, i, below)
        r0 = T // TILE * TILE
        pi[0], pi[T - 1] = 0, T - 1
        if T % TILE:
            pi[r0 + (T - r0) // 2] = r0
        used = set(pi.tolist())
        last_user = {}
        for qi, p in enumerate(pi.tolist()):
            last_user[p] = qi
        hd.decoys = 0
        for j in range(1, T):
            if j in used:
                continue
            cands = [p for p, qi in last_user.items() if qi < j]              # every query that matches p comes before key j
            tight = [p for p in cands if last_user[p] == j - 1]               # ... the last of them directly: a mask off by one shows it
            cands = tight or cands
            if cands:
                ck[j] = ck[cands[int(torch.randint(0, len(cands), (1,), generator=g))]]
                hd.decoys += 1
        hd.ck, hd.pi, hd.v = ck, pi, _values(g, T, dv, torch.arange(T)[:, None], step, vmax)
        hd.vis = torch.arange(T)[None, :] <= i[:, None]
        hd.want = hd.v[pi].to(F64)
        return hd
    assert kind == "plain", kind
    cid, members = _groups(g, T, m)
    hd.ck = _signs(g, T, d)[cid]
    hd.pi = _pi(g, S, T, forced_keys(T), cover)
    hd.v = _values(g, T, dv, members, step, vmax)
    gsum = torch.zeros(T, dv, dtype=F64).index_add_(0, cid, hd.v.to(F64))
    cnt = torch.bincount(cid, minlength=T).to(F64)
    hd.want = gsum[cid[hd.pi]] / cnt[cid[hd.pi]][:, None]
    hd.cid, hd.members = cid, members
    return hd


def scan(qh, kh, vh, pi, vis=None, chunk=1024):
    """From the operands of one (sample, head) alone, per query: how many visible keys score as high as key pi(i) (ties), the mean of
    their V rows, the distance to the best other visible key (raw score units), how many HIDDEN keys score as high (decoys), and the
    largest |score|.  The only place that forms the S x T score matrix: fp32, exact (integers below 2^24)."""
    S, T = qh.shape[0], kh.shape[0]
    ties, gap, hidden = torch.zeros(S, dtype=torch.long), torch.zeros(S), torch.zeros(S, dtype=torch.long)
    mean = torch.zeros(S, vh.shape[1], dtype=F64)
    top = 0.0
    for i0 in range(0, S, chunk):
        i1 = min(S, i0 + chunk)
        s = qh[i0:i1] @ kh.t()
        top = max(top, float(s.abs().max()))
        match = s.gather(1, pi[i0:i1, None])
        high = s >= match
        seen = torch.ones_like(high) if vis is None else vis[i0:i1]
        tied = high & seen
        assert bool(tied.gather(1, pi[i0:i1, None]).all()), "a query's own match is hidden from it"
        ties[i0:i1] = tied.sum(1)
        hidden[i0:i1] = (high & ~seen).sum(1)
        mean[i0:i1] = (tied.to(F64) @ vh.to(F64)) / tied.sum(1, keepdim=True)
        other = torch.where(seen & ~tied, s, torch.full_like(s, -float("inf")))
        gap[i0:i1] = match[:, 0] - other.max(1).values            # inf where a query sees nothing but its ties
    return types.SimpleNamespace(ties=ties, mean=mean, gap=gap, hidden=hidden, top=top)


def split_heads(x, H):
    """[B][N][H d] -> [B][H][N][d]"""
    B, N, C = x.shape
    return x.view(B, N, H, C // H).permute(0, 2, 1, 3)


def select(case_id, *, B, H, d, S, T, m=1, sl2=1.0, kind="plain", geo=None, step=1, vmax=VMAX, min_gap=None, ch=None, amp=None,
           cover=None):
    """The draw of one launch: q [B][S][H d] = b c_pi(i), k [B][T][H d] = a c_j, v [B][T][H d], pi [B][H][S] and the expected output
    [B][S][H d] (float64).  sl2: exp2 units per unit of q.k (1 in the q_prescaled form, scale log2(e) otherwise); min_gap: the gap
    to open (default: need_gap(T)).  The smallest (a, b) of AMPS that opens it is taken (or amp); `conditions` decides whether it
    did.  ch = (c0, c1): the codewords live in channels [c0, c1) of a head and q, k are zero in its other channels, so the draws of
    several key segments (own / reference keys, regions, text / image tokens) add up to ONE q with a pi of its own per segment."""
    g = gen(case_id)
    c0, c1 = ch or (0, d)
    full, d = d, c1 - c0
    p = types.SimpleNamespace(id=case_id, B=B, H=H, d=d, S=S, T=T, m=m, sl2=float(sl2), kind=kind, geo=geo, step=step, vmax=vmax, cover=cover,
                              min_gap=need_gap(T) if min_gap is None else float(min_gap))
    heads = [[_head(g, S, T, d, full, m, kind, geo, step, vmax, cover) for _ in range(H)] for _ in range(B)]
    unit = min(float(scan(hd.ck[hd.pi], hd.ck, hd.v, hd.pi, hd.vis).gap.min()) for row in heads for hd in row)
    p.a, p.b = amp or next(((a, b) for a, b in AMPS if a * b * unit * p.sl2 >= p.min_gap), AMPS[-1])
    p.d, p.ch = full, (c0, c1)
    cat = lambda f: torch.stack([torch.cat([f(hd) for hd in row], -1) for row in heads])   # noqa: E731
    wide = lambda x: torch.nn.functional.pad(x, (c0, full - c1))                           # noqa: E731
    p.q, p.k, p.v = cat(lambda hd: wide(p.b * hd.ck[hd.pi])), cat(lambda hd: wide(p.a * hd.ck)), cat(lambda hd: hd.v)
    p.expect = cat(lambda hd: hd.want)
    p.pi = torch.stack([torch.stack([hd.pi for hd in row]) for row in heads])
    p.vis = heads[0][0].vis                                    # (causal, windows: the same for every sample and head)
    p.members = [[getattr(hd, "members", None) for hd in row] for row in heads]
    p.cid = [[getattr(hd, "cid", None) for hd in row] for row in heads]
    p.decoys = sum(getattr(hd, "decoys", 0) for row in heads for hd in row)
    return p


def is_bf16(x):
    return bool((x.to(torch.bfloat16).to(x.dtype) == x).all())


def conditions(p, *, ties=None, tile=TILE):
    """What exactness rests on, asserted on the operands and the expected output alone.  ties: the tie counts a query may have
    (default {1, m}: a key outside every group stands alone).  Returns the smallest gap (exp2 units) for the record."""
    what = p.id
    for name in ("q", "k", "v"):
        x = getattr(p, name)
        assert is_bf16(x) and bool((x == x.round()).all()), f"{what}: {name} holds values that are no bf16 integers"
    assert float(p.q.abs().max()) <= 8 and float(p.k.abs().max()) <= 8, f"{what}: |q| or |k| > 8"
    assert float(p.v.min()) >= 1 and float(p.v.max()) <= p.vmax, f"{what}: V outside [1, {p.vmax}]"
    assert p.expect.dtype == F64 and is_bf16(p.expect) and bool((p.expect != 0).all()), f"{what}: the expected output is not a non-zero bf16 value everywhere"
    ties = {1, p.m} if ties is None else set(ties)
    qs, ks, vs, es = split_heads(p.q, p.H), split_heads(p.k, p.H), split_heads(p.v, p.H), split_heads(p.expect, p.H)
    G, seen_m, hidden, tight = float("inf"), 0, 0, 0
    for b in range(p.B):
        for h in range(p.H):
            pi = p.pi[b, h]
            sc = scan(qs[b, h], ks[b, h], vs[b, h], pi, p.vis)
            assert sc.top < TWO24, f"{what}: |score| up to {sc.top:.0f} >= 2^24"
            got = set(sc.ties.tolist())
            assert got <= ties, f"{what} [{b}][{h}]: queries with {sorted(got - ties)} tied keys (allowed: {sorted(ties)}) - another seed: _select.SALT"
            assert torch.equal(sc.mean, es[b, h]), f"{what} [{b}][{h}]: the expected output is not the mean of V over the matched keys"
            G = min(G, float(sc.gap.min()) * p.sl2)
            seen_m += int((sc.ties == p.m).sum())
            if p.m > 1:                                      # the queries whose match is a member of a group, and at least m of them
                in_group = torch.isin(pi, p.members[b][h].flatten())
                assert torch.equal(sc.ties == p.m, in_group) and int(in_group.sum()) >= p.m, f"{what} [{b}][{h}]: {int(in_group.sum())} queries with {p.m} tied keys"
            hidden += int((sc.hidden > 0).sum())
            # coverage
            keys = set(pi.tolist())
            if p.kind == "plain":
                want_n = min(p.S, p.T) if p.cover is None else p.cover
                assert len(keys) == want_n, f"{what} [{b}][{h}]: pi holds {len(keys)} distinct keys of {want_n}"
                assert keys >= set(forced_keys(p.T, tile)), f"{what} [{b}][{h}]: pi misses one of the keys {forced_keys(p.T, tile)}"
                mem = p.members[b][h]
                if p.m > 1:
                    part = torch.bucketize(mem, torch.tensor(_edges(p.T, p.m)[1:]), right=True)
                    assert torch.equal(part, torch.arange(p.m).expand_as(part)), f"{what}: tied keys not one per part of the walk"
                    if -(-p.T // TILE) >= p.m:
                        assert bool((mem[:, 1:] // TILE > mem[:, :-1] // TILE).all()), f"{what}: two tied keys share a 64-key tile"
                    if getattr(p, "quarters", False):
                        assert torch.equal(mem * 4 // p.T, torch.arange(4).expand_as(mem)), f"{what}: tied keys not one per quarter of the walk"
            elif p.kind == "causal":
                assert bool((pi <= torch.arange(p.S)).all()) and keys >= set(forced_keys(p.T, tile)), what
                s = qs[b, h] @ ks[b, h].t()
                tight += int((s.diagonal(1) >= s.gather(1, pi[:, None])[:-1, 0]).sum())      # key i + 1 scores as high as query i's match
            else:
                for row in p.geo.tokens:
                    L = len(row)
                    local = {int((row == j).nonzero()) for j in pi[row].tolist()}        # pi stays inside the query's window
                    assert local == set(range(L)), f"{what}: pi leaves a window or misses one of its keys"
    assert math.isfinite(G) and p.T * VMAX * 2.0 ** -G <= 2.0 ** -12 and G >= p.min_gap, \
        f"{what}: smallest gap {G:.1f} exp2 units, {max(need_gap(p.T), p.min_gap):.1f} needed (a, b = {p.a}, {p.b})"
    if p.kind == "causal":
        assert hidden > 0 and tight > 0, f"{what}: {hidden} queries with a decoy behind the mask, {tight} with one at the very next key"
    if p.kind == "windows" and len(p.geo.tokens) > 1:
        assert hidden == p.B * p.H * p.S, f"{what}: a query without a decoy in another window"
    return G


def window_geo(h, w, wh, ww):
    from minsdtf_amd import hypertile as HT

    tokens = torch.from_numpy(HT.window_tokens(h, w, wh, ww)).long()
    win_of = torch.zeros(h * w, dtype=torch.long)
    for i, row in enumerate(tokens):
        win_of[row] = i
    return types.SimpleNamespace(h=h, w=w, wh=wh, ww=ww, tokens=tokens, win_of=win_of)


# ---- the comparison -------------------------------------------------------------------------------------------------------------
def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32).to(torch.int64)


def exact_rows(got, expect, what, *, H=1, v=None, ulp=0):
    """got (bf16 or fp32, any device) [B][S][H d] against the float64 expectation: the bits of its round-to-nearest bf16 (its fp32
    bits), or at most `ulp` steps of that format away.  Names the first wrong (sample, query, head, channel) and, with v [B][T][H d],
    the (sample, key, head) whose V row the output row actually holds, if any."""
    got = got.detach().cpu()
    assert got.dtype in (torch.float32, torch.bfloat16), got.dtype
    assert expect.dtype == F64 and tuple(got.shape) == tuple(expect.shape), (what, tuple(got.shape), tuple(expect.shape))
    want = expect.to(got.dtype)
    assert torch.equal(want.to(F64), expect), f"{what}: the expectation is no {got.dtype} value"
    assert bool(torch.isfinite(got.float()).all()), f"{what}: {int((~torch.isfinite(got.float())).sum())}/{got.numel()} non-finite outputs"
    bad = (_bits(got) - _bits(want)).abs() > ulp
    if not bool(bad.any()):
        return
    B, S, C = got.shape
    d = C // H
    b, i, c = (int(x) for x in bad.nonzero()[0])
    h = c // d
    row = got[b, i, h * d:(h + 1) * d].float()
    holds = "no key's V row"
    if v is not None:
        vh = v.reshape(v.shape[0], v.shape[1], -1, d)
        hit = (vh == row).all(-1).nonzero()
        if len(hit):
            holds = "V of (sample {}, key {}, head {})".format(*(int(x) for x in hit[0]))
    raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} outputs differ from the selected row, first at sample {b}, query {i}, head {h}, "
                         f"channel {c - h * d}: got {float(got[b, i, c])!r}, expected {float(expect[b, i, c])!r}; the output row holds {holds}")


# ---- CPU emulation of the pinned arithmetic -------------------------------------------------------------------------------------
def rbf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def exp2(x):
    """exp2 in fp32: an exact power of two for integer arguments (ldexp), the rounded float64 value otherwise."""
    x = x.clamp(-200.0, 200.0)
    if bool((x == x.round()).all()):
        return torch.ldexp(torch.ones_like(x), x.to(torch.int32)).to(torch.float32)
    return torch.exp2(x.to(F64)).to(torch.float32)


def _walk(qh, kh, vh, *, lazy, presc=True, sl2=1.0, vis=None, tile=TILE, round_l=True, mutant=None, boundary=None, state=None):
    """One (sample, head): queries [S][d] against keys [T][d], V [T][dv], in ascending tiles.  lazy: msd_attention (reference moved
    when a tile's maximum passes it by more than ATTN_THR; presc or scores times sl2 by one fma), else msd_attention_joint's walk
    (true running maximum, rescale at every tile).  P rounded to bf16 for the second product; the row sum adds the rounded P
    (round_l) or the fp32 one.  Returns (O, l) - the caller divides."""
    S, T = qh.shape[0], kh.shape[0]
    mutant = mutant or {}
    if state is None:
        mref = torch.zeros(S) if lazy else torch.full((S,), NEG)
        l, O = torch.zeros(S), torch.zeros(S, vh.shape[1])
    else:
        mref, l, O = state
    for ti, t0 in enumerate(range(0, T, tile)):
        t1 = min(T, t0 + tile)
        s = qh @ kh[t0:t1].t()
        vt = vh[t0:t1]
        if vis is not None:
            s = torch.where(vis[:, t0:t1], s, torch.full_like(s, NEG))
        for j in mutant.get("drop", ()):
            if t0 <= j < t1:
                s[:, j - t0] = NEG
        if mutant.get("twice") is not None and t0 <= mutant["twice"] < t1:        # a key of this tile counted twice
            j = mutant["twice"] - t0
            s, vt = torch.cat([s, s[:, j:j + 1]], 1), torch.cat([vt, vt[j:j + 1]], 0)
        first = ti == 0 and state is None
        mx = s.max(1).values
        if lazy and presc:
            s = s - mref[:, None]
            need = (mx - mref > ATTN_THR) | first
            delta = torch.where(need, mx - mref, torch.zeros(S))
            alpha = exp2(-delta)
            mref = mref + delta
            P = exp2(s - delta[:, None])
        elif lazy:
            need = ((mx - mref) * sl2 > ATTN_THR) | first
            mnew = torch.where(need, mx, mref)
            alpha = exp2((mref - mnew) * sl2)
            mref = mnew
            nm = (-mref * sl2).to(torch.float32)
            P = exp2((s.to(F64) * float(torch.tensor(sl2, dtype=torch.float32)) + nm.to(F64)[:, None]).to(torch.float32))   # one fma
        else:
            mnew = torch.maximum(mref, mx)
            alpha = exp2(mref - mnew)
            mref = mnew
            P = exp2(s - mref[:, None])
        if not first and mutant.get("skip_rescale") != ti:
            l, O = l * alpha, O * alpha[:, None]
        Pb = rbf(P)
        l = l + (Pb if round_l else P).sum(1)
        O = O + Pb @ vt
    return O, l, (mref, l, O)


def _store(O, l):
    return rbf(O * (1.0 / l)[:, None])


def _per_head(p, fn):
    qs, ks, vs = split_heads(p.q, p.H), split_heads(p.k, p.H), split_heads(p.v, p.H)
    out = torch.stack([torch.stack([fn(qs[b, h], ks[b, h], vs[b, h], b, h) for h in range(p.H)]) for b in range(p.B)])   # [B][H][S][d]
    return out.permute(0, 2, 1, 3).reshape(p.B, p.S, -1)


def emulate_attention(p, *, presc, round_l=True, tile=TILE, mutant=None):
    """msd_attention on the draw p.  mutant (a dict, tests/test_attention_exact_cpu.py): drop=(keys), twice=key, skip_rescale=tile,
    row=(i, i2) query i reads q row i2, head_v=(h, h2) head h reads the V of head h2, channel=(c) V channel c reads c + 1,
    vis=another visibility."""
    mutant = mutant or {}
    vis = mutant.get("vis", p.vis)
    vs = split_heads(p.v, p.H)

    def one(qh, kh, vh, b, h):
        if "row" in mutant:
            qh = qh.clone()
            qh[mutant["row"][0]] = qh[mutant["row"][1]]
        if "head_v" in mutant and h == mutant["head_v"][0]:
            vh = vs[b, mutant["head_v"][1]]
        if "channel" in mutant:
            c = mutant["channel"]
            vh = vh.clone()
            vh[:, c] = vh[:, (c + 1) % vh.shape[1]]
        O, l, _ = _walk(qh, kh, vh, lazy=True, presc=presc, sl2=p.sl2, vis=vis, tile=tile, round_l=round_l, mutant=mutant)
        return _store(O, l)

    return _per_head(p, one)


def emulate_windowed(p, *, mutant=None):
    """msd_attention_windowed: per window, its keys in window-linear tiles of 64, msd_attention_joint's walk with one segment."""
    mutant = mutant or {}
    admit = mutant.get("admit")                               # (window, token): the window's walk also takes this foreign key

    def one(qh, kh, vh, b, h):
        out = torch.zeros(p.S, vh.shape[1])
        for wi, row in enumerate(p.geo.tokens):
            keys = torch.cat([row, torch.tensor([admit[1]])]) if admit is not None and admit[0] == wi else row
            O, l, _ = _walk(qh[row], kh[keys], vh[keys], lazy=False)
            out[row] = _store(O, l)
        return out

    return _per_head(p, one)


def emulate_joint(p, pr, mix):
    """msd_attention_joint: p the own segment's draw, pr the reference row's (B = 1), mix [B] or None."""
    krs, vrs = split_heads(pr.k, p.H)[0], split_heads(pr.v, p.H)[0]

    def one(qh, kh, vh, b, h):
        f = 0.0 if mix is None else float(mix[b])
        O, l, st = _walk(qh, kh, vh, lazy=False)
        plain = O * (1.0 / l)[:, None]
        if f == 1.0:
            return rbf(plain)
        O, l, _ = _walk(qh, krs[h], vrs[h], lazy=False, state=st)
        joint = O * (1.0 / l)[:, None]
        if f == 0.0:
            return rbf(joint)
        f32 = torch.tensor(f, dtype=torch.float32)
        return rbf((f32.to(F64) * plain.to(F64) + ((1.0 - f32) * joint).to(F64)).to(torch.float32))     # fma(f, plain, (1 - f) joint)

    return _per_head(p, one)


def emulate_region(ps, w):
    """msd_region_attention: ps the regions' draws over the SAME queries, w [R][S]: one tile per region (t <= 96), true maximum,
    O_r = (sum P v) (1 / l), acc = w O_r at the first positive region, fma(w, O_r, acc) at each later one."""
    p = ps[0]

    def one(qh, kh, vh, b, h):
        acc, started = torch.zeros(p.S, vh.shape[1]), torch.zeros(p.S, dtype=torch.bool)
        for r, pr in enumerate(ps):
            kr, vr = split_heads(pr.k, p.H)[b, h], split_heads(pr.v, p.H)[b, h]
            O, l, _ = _walk(qh, kr, vr, lazy=False, tile=kr.shape[0])
            Or = O * (1.0 / l)[:, None]
            wr = w[r].to(torch.float32)[:, None]
            nxt = torch.where(started[:, None], (wr.to(F64) * Or.to(F64) + acc.to(F64)).to(torch.float32), wr * Or)
            acc = torch.where(wr > 0, nxt, acc)
            started = started | (w[r] > 0)
        return rbf(acc)

    return _per_head(p, one)


def emulate_decoupled(p, pip, sc):
    """msdi_attention_decoupled: p the text draw, pip the image tokens' (the same queries); each softmax its own true maximum and fp32
    row sum, a text probability 2^(x - max) (1 / sum), an image probability 2^(x - max_ip) (sc / sum_ip), each rounded once."""
    def probs(qh, kh, factor):
        s = qh @ kh.t()
        e = exp2(s - s.max(1, keepdim=True).values)
        return rbf(e * (torch.tensor(factor, dtype=torch.float32) / e.sum(1))[:, None])

    def one(qh, kh, vh, b, h):
        out = probs(qh, kh, 1.0) @ vh
        if sc != 0:
            out = out + probs(qh, split_heads(pip.k, p.H)[b, h], sc) @ split_heads(pip.v, p.H)[b, h]
        return rbf(out)

    return _per_head(p, one)


# ---- the launches of tests/test_attention_exact_gpu.py on these draws ---------------------------------------------------------------
# (the CPU module walks every one of them through `conditions`, so a bad case fails without a GPU)
EMULATION_CAP = 1 << 20      # the emulation runs where S x T of a (sample, head) is at most this (1024 x 1024): the CPU suite stays quick
_DRAWS = {}


def _cached(key, make):
    if key not in _DRAWS:
        _DRAWS[key] = make()
    return _DRAWS[key]


def case_name(case):
    return "-".join(f"{k}{int(v)}" for k, v in case.items())


# msd_attention beside test_ops_gpu.ATTENTION_CASES: the CLIP text encoder's head size, with and without its causal mask
ATTENTION_EXTRA = [dict(B=2, H=2, d=64, S=77, T=77), dict(B=2, H=2, d=64, S=77, T=77, causal=True)]


def attention_runs():
    """[(id, case, qf, presc, form, m)]: every (case, qf, presc, form) of test_ops_gpu._attention_params(), the prescaled ones with
    m = 1, 2 and 4 tied keys, the others with m = 1; then ATTENTION_EXTRA (64- and 128-query workgroups; causal: m = 1)."""
    from test_ops_gpu import _attention_params

    runs = []
    for prm in _attention_params():
        case, qf, presc, form = prm.values
        runs += [(f"{prm.id}-ties{m}", case, qf, presc, form, m) for m in ((1, 2, 4) if presc else (1,))]
    for case in ATTENTION_EXTRA:
        for presc in (False, True):
            for qf in (2, 1):
                ms = (1, 2, 4) if presc and not case.get("causal") else (1,)
                runs += [(f"form1-presc{int(presc)}-qf{qf}-{case_name(case)}-ties{m}", case, qf, presc, 1, m) for m in ms]
    return runs


def attention_problem(case, presc, m):
    """The draw of an msd_attention case: it depends on (case, presc, m) alone, so the forms and workgroup sizes share it."""
    key = f"attention/{case_name(case)}/presc{int(presc)}/m{m}"
    sl2 = 1.0 if presc else case["d"] ** -0.5 * LOG2E
    return _cached(key, lambda: select(key, B=case["B"], H=case["H"], d=case["d"], S=case["S"], T=case["T"], m=m, sl2=sl2,
                                       kind="causal" if case.get("causal") else "plain"))


# head_dim 512 (the VAE's single head; not prescaled, t % 32 == 0): (S, T, workspace, m).  With the workspace and t >= 2048 the key
# walk is split four ways and merged in part order: m = 4 puts one tied key in every quarter.
D512_RUNS = [(64, 64, False, 1), (200, 224, False, 1), (2048, 2048, False, 1), (2048, 2048, False, 4), (2048, 2048, True, 1), (2048, 2048, True, 4)]
D512_SL2 = 512 ** -0.5 * LOG2E


def d512_problem(S, T, m):
    key = f"d512/S{S}/T{T}/m{m}"

    def make():
        p = select(key, B=2 if S < 2048 else 1, H=1, d=512, S=S, T=T, m=m, sl2=D512_SL2)
        p.quarters = m == 4
        return p

    return _cached(key, make)


def with_q(p, q):
    """The draw p with the launch's whole q (the sum over the key segments' draws)."""
    out = types.SimpleNamespace(**vars(p))
    out.q = q
    return out


# msd_attention_joint: (d, t, t_ref); s = t, three samples with mix = 0, 1 and 0.5 in one launch
JOINT_RUNS = [(d, t, tr) for d in (40, 80, 160) for t, tr in ((200, 130), (64, 64))]
JOINT_MIX = [0.0, 1.0, 0.5]
JOINT_H = 2


def joint_problem(d, t, tr):
    """Own keys in the lower half of a head's channels at amplitude (4, 2), reference keys in the upper half at (8, 4): the query's own
    match scores 4 d, its reference key 16 d, so plain = V[pi(i)] and joint = V_ref[rho(i)] - a pi per sample and head and a rho per
    sample and head over the ONE reference row (its draw takes the three samples' queries as 3 t queries of one sample).  Even V:
    fma(0.5, plain, 0.5 joint) is an integer."""
    key = f"joint/d{d}/t{t}/tr{tr}"

    def make():
        B, gap = len(JOINT_MIX), need_gap(t + tr)
        own = select(key + "/own", B=B, H=JOINT_H, d=d, S=t, T=t, ch=(0, d // 2), amp=(4, 2), step=2, vmax=126, min_gap=gap)
        ref = select(key + "/ref", B=1, H=JOINT_H, d=d, S=B * t, T=tr, ch=(d // 2, d), amp=(8, 4), step=2, vmax=126, min_gap=gap)
        j = types.SimpleNamespace(id=key, own=own, ref=ref, H=JOINT_H, d=d, B=B, S=t)
        j.q = own.q + ref.q.view(B, t, -1)
        plain, joint = own.expect, ref.expect.view(B, t, -1)
        f = torch.tensor(JOINT_MIX, dtype=F64)[:, None, None]
        j.expect = f * plain + (1 - f) * joint
        return j

    return _cached(key, make)


def joint_conditions(j):
    conditions(j.own)
    conditions(j.ref)
    own_top = float((split_heads(j.own.q, j.H) @ split_heads(j.own.k, j.H).transpose(-1, -2)).max())
    rq, rk = split_heads(j.ref.q, j.H)[0], split_heads(j.ref.k, j.H)[0]
    ref_match = float((rq * rk.gather(1, j.ref.pi[0][..., None].expand(-1, -1, rq.shape[-1]))).sum(-1).min())
    assert ref_match - own_top >= need_gap(j.own.T + j.ref.T), f"{j.id}: the reference key beats the own keys by {ref_match - own_top:.0f} only"
    assert is_bf16(j.expect) and bool((j.expect != 0).all()), j.id


# msd_attention_windowed: every geometry of test_hypertile_gpu.GEOMETRIES (all of them small) x head size
WINDOW_B, WINDOW_H = 2, 2


def window_problem(geo, d):
    key = "windows/" + "x".join(map(str, geo)) + f"/d{d}"
    h, w = geo[0], geo[1]
    return _cached(key, lambda: select(key, B=WINDOW_B, H=WINDOW_H, d=d, S=h * w, T=h * w, kind="windows", geo=window_geo(*geo),
                                       min_gap=need_gap(geo[2] * geo[3])))


# msd_region_attention: (d, S, T) x regions; H = 2, B = 2
REGION_SHAPES = [(40, 200, 77), (80, 128, 96), (160, 64, 13)]
REGION_COUNTS = (1, 2, 5)
REGION_B, REGION_H = 2, 2
REGION_PATTERNS = [(1.0,), (0.5, 0.5), (0.5, 0.25, 0.25), (0.25, 0.25, 0.25, 0.25)]


def region_problem(d, S, T, R):
    """Region r's codewords live in the r-th of R channel ranges of a head: one q selects a key of its own in every region.  Weights
    from {0, 1/4, 1/2, 1} that sum to 1 per query, V in multiples of 4: sum_r w_r V_r[pi_r(i)] is an integer at every step of the fma
    chain."""
    key = f"region/d{d}/S{S}/T{T}/R{R}"

    def make():
        r = types.SimpleNamespace(id=key, H=REGION_H, d=d, B=REGION_B, S=S, T=T, R=R)
        r.parts = [select(f"{key}/r{i}", B=REGION_B, H=REGION_H, d=d, S=S, T=T, ch=(i * d // R, (i + 1) * d // R), step=4, vmax=124)
                   for i in range(R)]
        g = gen(key + "/w")
        w = torch.zeros(R, S)
        for i in range(S):
            pats = [pt for pt in REGION_PATTERNS if len(pt) <= R]
            pt = pats[int(torch.randint(0, len(pats), (1,), generator=g))]
            w[torch.randperm(R, generator=g)[:len(pt)], i] = torch.tensor(pt)
        r.w = w
        r.q = sum(pt.q for pt in r.parts)
        r.k = torch.cat([pt.k for pt in r.parts])                 # region-major: row r B + b
        r.v = torch.cat([pt.v for pt in r.parts])
        r.expect = sum(w[i].to(F64)[None, :, None] * pt.expect for i, pt in enumerate(r.parts))
        return r

    return _cached(key, make)


def region_conditions(r):
    for pt in r.parts:
        conditions(pt)
    assert bool((r.w.sum(0) == 1).all()) and set(r.w.unique().tolist()) <= {0.0, 0.25, 0.5, 1.0}, r.id
    assert bool((r.w > 0).any(1).all()), f"{r.id}: a region without a query"
    assert is_bf16(r.expect) and bool((r.expect != 0).all()) and bool((r.expect == r.expect.round()).all()), r.id


# msdi_attention_decoupled: (d, S, T, N) x sc; H = 2, B = 2
DECOUPLED_SHAPES = [(40, 200, 77, 4), (80, 128, 80, 16), (160, 64, 13, 16)]
DECOUPLED_SCALES = (0.0, 0.5, 2.0)
DECOUPLED_B, DECOUPLED_H = 2, 2
IP_BITS = 16               # the image tokens' codewords: the last 16 channels of a head


def decoupled_problem(d, S, T, N):
    """Text codewords in channels [0, d - 16) of a head, the image tokens' in the last 16: V[pi(i)] + sc V_ip[rho(i)] with V <= 127 and
    even V_ip <= 64, so |out| <= 255 is an integer for sc in {0, 0.5, 2}."""
    key = f"decoupled/d{d}/S{S}/T{T}/N{N}"

    def make():
        x = types.SimpleNamespace(id=key, H=DECOUPLED_H, d=d, B=DECOUPLED_B, S=S)
        x.text = select(key + "/text", B=x.B, H=x.H, d=d, S=S, T=T, ch=(0, d - IP_BITS))
        x.ip = select(key + "/ip", B=x.B, H=x.H, d=d, S=S, T=N, ch=(d - IP_BITS, d), step=2, vmax=64)
        x.q = x.text.q + x.ip.q
        return x

    return _cached(key, make)


def decoupled_expect(x, sc):
    e = x.text.expect + sc * x.ip.expect
    assert float(e.abs().max()) <= 256 and is_bf16(e) and bool((e != 0).all()), x.id
    return e


# msdx_attention_colsum (head_dim 160, 8 heads): S x m
COLSUM_RUNS = [(S, m) for S in (64, 200) for m in (1, 2)]
COLSUM_B, COLSUM_H = 2, 8
COLSUM_GAP = 192.0          # every other probability is exp2 of less than -149: 0.0f, so a key that nobody selects receives exactly 0


def colsum_problem(S, m):
    """pi covers an eighth of a head's keys: keys that no query of any head selects (0), keys that several do.  out[b][j] = (the number of (head, query)
    pairs that select j) / (8 m): sums of at most a few hundred terms 1 / m, exact in fp32 in any order."""
    key = f"colsum/S{S}/m{m}"

    def make():
        p = select(key, B=COLSUM_B, H=COLSUM_H, d=160, S=S, T=S, m=m, min_gap=COLSUM_GAP, cover=S // 8)
        out = torch.zeros(p.B, S, dtype=F64)
        for b in range(p.B):
            for h in range(p.H):
                cid = p.cid[b][h]
                size = torch.bincount(cid, minlength=S).to(F64)
                picks = torch.bincount(cid[p.pi[b, h]], minlength=S).to(F64)          # per group: the queries that select it
                out[b] += (picks / size.clamp(min=1))[cid]
        p.colsum = out / p.H
        return p

    return _cached(key, make)


def colsum_conditions(p):
    G = conditions(p)
    assert G >= COLSUM_GAP and G > 149 + 8, p.id
    assert bool((p.colsum == 0).any()) and bool((p.colsum > 1.0 / p.H).any()), f"{p.id}: no key without a query, or none with several"
    assert torch.equal(p.colsum.to(torch.float32).to(F64), p.colsum) and float(p.colsum.sum(1).min()) == float(p.colsum.sum(1).max()) == p.S, p.id


# msd_cross_attention_q (8 heads, t <= 96, m = 1): the smallest entries of test_ops_gpu.test_cross_attention_q's list per head size
XATTN_CASES = [dict(B=1, S=64, d=40, T=13, slots=3), dict(B=1, S=200, d=40, T=77, slots=4), dict(B=1, S=64, d=80, T=96, slots=5),
               dict(B=3, S=64, d=160, T=13, slots=3), dict(B=1, S=100, d=160, T=96, slots=5)]
XATTN_H = 8
LN_EPS = 1e-5


def xattn_problem(case):
    """Column n of wq holds, for every head, codeword n of that head's book (c of them); x row i is b at ONE column u(i) of a set U of
    T columns spread over [0, c) and 0 elsewhere, so x wq^T = b c_u(i) in every head, exactly; key j of (sample, head) carries the
    codeword of U[perm(j)] with a permutation of its own, so pi = perm^-1(u) differs per sample and head.  ln_in: per slot (sum 0, sum
    of squares c / slots): mean 0, variance 1, rstd = rsqrt(1 + eps), and bf16(rstd b c) = b c."""
    key = "xattn/" + case_name(case)

    def make():
        g = gen(key)
        B, Sq, d, T, H = case["B"], case["S"], case["d"], case["T"], XATTN_H
        C = H * d
        books = [_signs(g, C, d) for _ in range(H)]                               # [C][d] per head
        U = torch.randperm(C, generator=g)[:T].sort().values
        perms = [[torch.randperm(T, generator=g) for _ in range(H)] for _ in range(B)]
        inv = [[torch.argsort(pm) for pm in row] for row in perms]
        x = types.SimpleNamespace(id=key)
        p = types.SimpleNamespace(id=key, B=B, H=H, d=d, S=Sq, T=T, m=1, sl2=1.0, kind="plain", vis=None, vmax=VMAX, cover=None,
                                  min_gap=need_gap(T), geo=None)
        us = []
        for b in range(B):
            forced = sorted({int(perms[b][h][j]) for h in range(H) for j in forced_keys(T)})
            us.append(_pi(g, Sq, T, forced))
        unit = min(float(scan(books[h][U[us[b]]], books[h][U[perms[b][h]]], torch.ones(T, 1), inv[b][h][us[b]]).gap.min())
                   for b in range(B) for h in range(H))
        p.a, p.b = next(((a, b_) for a, b_ in AMPS if a * b_ * unit >= p.min_gap), AMPS[-1])
        p.pi = torch.stack([torch.stack([inv[b][h][us[b]] for h in range(H)]) for b in range(B)])
        p.q = torch.stack([torch.cat([p.b * books[h][U[us[b]]] for h in range(H)], -1) for b in range(B)])
        p.k = torch.stack([torch.cat([p.a * books[h][U[perms[b][h]]] for h in range(H)], -1) for b in range(B)])
        p.v = torch.randint(1, VMAX + 1, (B, T, C), generator=g).to(torch.float32)
        vh = split_heads(p.v, H)
        p.expect = torch.stack([torch.cat([vh[b, h][p.pi[b, h]] for h in range(H)], -1) for b in range(B)]).to(F64)
        p.members = [[torch.arange(T)[:, None]] * H] * B
        x.p = p
        x.wq = torch.cat([bk.t() for bk in books])                                # [N = C][K = C]: row h d + e, column n
        x.x = torch.zeros(B * Sq, C)
        x.x[torch.arange(B * Sq), U[torch.cat(us)]] = float(p.b)
        x.ln_in = torch.tensor([0.0, C / case["slots"]]).repeat(B * Sq, case["slots"], 1)
        return x

    return _cached(key, make)


def xattn_conditions(x):
    p = x.p
    conditions(p)
    C = p.H * p.d
    assert is_bf16(x.x) and is_bf16(x.wq) and bool(((x.x != 0).sum(1) == 1).all()), x.id
    assert torch.equal((x.x @ x.wq.t()).view(p.B, p.S, C), p.q), f"{x.id}: x wq^T is not b c_pi(i)"
    st = x.ln_in.sum(1)
    mean, var = st[:, 0] / C, st[:, 1] / C - (st[:, 0] / C) ** 2
    rstd = torch.rsqrt(var + LN_EPS)
    assert bool((mean == 0).all()) and torch.equal(rbf(rstd.view(p.B, p.S, 1) * p.q), p.q), f"{x.id}: the bf16 store of q does not restore b c_pi(i)"
