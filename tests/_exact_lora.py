"""msd_lora_merge (csrc/lora.hip) held to bits: a float64 statement of one job written from the text of include/minsdtf_hip.h, the
case lists of tests/test_lora_exact_gpu.py, their conditions, the checkers, and a numpy model of the kernel's addressing that can
be made wrong on purpose (tests/test_lora_exact_cpu.py shows every such fault refused).

The statement (`reference`), per logical element (n, k) of an N x K job:
  v   = master[n][k] + sum_j up[n][j] down[j][k]
  v   = (v * rowscale[n]) * colscale[k]                     each factor optional, in this order
  row = (rowmap ? rowmap[n] : n) + row_off, skipped outside [0, out_rows);   col = col_off + k
  rows         out[row * ld + col]
  chunk-major  out[((col / 64) * out_rows + row) * 64 + col % 64]
  transposed   out[col * out_rows + row]
  fragment     frag[(((((col / 64) * (out_rows / 16) + row / 16) * 2 + (col / 32) % 2) * 4 + (col / 8) % 4) * 16 + P[row % 16]) * 8 + col % 8]
               with P = (0 1 2 3 8 9 10 11 4 5 6 7 12 13 14 15), its own inverse
  colsum[row]  = fp32 of the float64 sum of the row's ROUNDED values
  bf16         = round to nearest even, done here on the integer bits of the fp32 value
It returns, per destination buffer, the expected bits and the mask of the elements the job may write; `expected` lays the jobs of a
launch over buffers filled with CANARY, so every element no job may write must come back as the canary.

Three stages:
1. exact: master integers in [-64, 64], up / down integers in [-3, 3], rank <= 512, rowscale in {1/4, 1/2, 1, 3/2, 2, 3}, colscale
   in {k / 4: k = 1..7}.  |v| < 2^13 and every value is a multiple of 1/16 below 2^24 sixteenths, so every intermediate is its own
   fp32 whatever the summation order or contraction, and the float64 statement's bits are demanded.  `conditions` asserts this per
   case and counts the bf16 ties (both directions must occur >= 32 times over the list).
2. rank 0: randn master and scales; v = master, (v * rs) * cs in numpy float32 in that order, round to nearest even: each operation
   is correctly rounded and the header fixes the order, so again bits.  This stage sees a swapped scale order.
3. rank > 0, real operands (`real_bounds`, `check_real`): S = sum_j |up down|, u = 2^-24, gamma_R = R u / (1 - R u); the fp32 v lies
   within b = |rs cs| (gamma_R S + 3 u (|master| + S)) (1 + 3 u) of the float64 v64; rounding is monotone, so a bf16 result lies in
   [bf16(v64 - b), bf16(v64 + b)], an fp32 one within b; colsum is, to the bit, the fp32 of the float64 sum of the kernel's own row.
   Assumed and not tested: __fadd_rn / __fmul_rn / fma are correctly rounded, no operand comes near overflow or the subnormals.

Plain numpy on the CPU.  Not a conftest: imported by name."""
import types
import zlib

import numpy as np

U = 2.0 ** -24
LIMIT = 1 << 24
CANARY = -2.0 ** 100            # finite, a bf16 and an fp32 number, far above any result: what a destination holds before the launch
ROWS, CHUNK, TRANS = 0, 1, 2
BF16, F32 = "bf16", "f32"
FRAG_ROW = np.array([0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15])
RS_SET = np.array([.25, .5, 1, 1.5, 2, 3], dtype=np.float32)
CS_SET = np.arange(1, 8, dtype=np.float32) / 4
SLACK = 64                      # elements of canary the model keeps on both sides of every destination (the guard band's stand-in)
BLOCK_ROWS, LANE_COLS, PASS_COLS = 8, 8, 512

FAULTS = (
    "tail lane drops its columns", "tail lane stores eight columns", "no second pass", "K rounded up to 4", "master row stride K",
    "up stride of the largest rank", "first block to the previous job", "row scale of the block's row", "column scale by destination column",
    "chunk stride n", "fragment: col_off dropped", "fragment: identity row order", "fragment: half dropped", "fragment: row_off ignored",
    "fragment: rowmap ignored", "skipped row clamped and written", "colsum of a skipped row written", "colsum of the unrounded values",
    "colsum of the padded lanes", "colsum in fp32", "bf16 truncated", "bf16 round half up", "scale order swapped")


# ---- bits -------------------------------------------------------------------------------------------------------------------------------
def f32_bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def bf16_rne(x):
    """fp32 -> bf16 bits, round to nearest even on the integer bits (NaN: the quiet NaN)."""
    b = f32_bits(x).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(np.asarray(x, dtype=np.float32)), np.uint16(0x7FC0), r)


def bf16_value(h):
    return (np.asarray(h, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_key(h):
    """Ordered integer of bf16 bits (monotone in the value)."""
    i = np.asarray(h, dtype=np.uint16).astype(np.int32)
    return np.where(i >= 0x8000, -(i & 0x7FFF), i)


def canary_bits(dtype):
    return (bf16_rne(np.float32(CANARY)) if dtype == BF16 else f32_bits(np.float32(CANARY))).reshape(-1)[0]


def np_dtype(dtype):
    return np.uint16 if dtype == BF16 else np.uint32


def geglu_rowmap(n):
    """Logical row of the (2 * half)-row GEGLU projection -> packed row: packed rows [32 i, 32 i + 16) are the value rows [16 i, 16 i + 16),
    packed rows [32 i + 16, 32 i + 32) the gate rows half + [16 i, 16 i + 16)."""
    half = n // 2
    assert half % 16 == 0
    r = np.arange(n)
    value = r < half
    w = np.where(value, r, r - half)
    return (32 * (w // 16) + w % 16 + np.where(value, 0, 16)).astype(np.int32)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def out_numel(d):
    return (d.rows - 1) * d.ld + d.cols if d.layout == ROWS else d.rows * d.cols


class Case:
    """One launch: destinations and the jobs that write them, in launch order.  stage: "exact", "rank0" or "real"."""
    def __init__(self, name, stage):
        self.id, self.stage, self.dests, self.jobs = f"{stage}/{name}", stage, {}, []

    def dest(self, name, layout, rows, cols, dtype=BF16, ld=None, frag=False, colsum=False, off=0):
        """off = 1: `out` starts one element past a 16-byte boundary."""
        assert name not in self.dests
        d = types.SimpleNamespace(name=name, layout=layout, rows=rows, cols=cols, dtype=dtype, ld=(ld or cols) if layout == ROWS else cols,
                                  frag=frag, colsum=colsum, off=off)
        assert (layout != CHUNK or (dtype == BF16 and cols % 64 == 0)) and (layout != TRANS or dtype == F32) and d.ld >= cols
        assert not frag or (dtype == BF16 and rows % 16 == 0 and cols % 64 == 0)
        self.dests[name] = d
        return d

    def job(self, dest, n, k, rank=0, row_off=0, col_off=0, rs=False, cs=False, rowmap=None, master_pad=0, mis=(), ranks=None):
        """One job into `dest` (with its fragment copy and colsum where the destination has them).  rs / cs: with a row / column scale;
        master_pad: master_ld = k + master_pad; mis: the operands among master / down / colscale that start one float past a 16-byte
        boundary; ranks (real stage): the ranks of several LoRAs concatenated as MergeBase._factors does."""
        d = self.dests[dest]
        j = types.SimpleNamespace(i=len(self.jobs), dest=dest, n=n, k=k, rank=0 if self.stage == "rank0" else rank, row_off=row_off,
                                  col_off=col_off, master_ld=k + master_pad, mis=frozenset(mis), frag=d.frag, colsum=d.colsum,
                                  up=None, down=None, rs=None, cs=None, rowmap=None if rowmap is None else np.asarray(rowmap, dtype=np.int32))
        j.id = f"{self.id}[{j.i}] -> {dest}: {n} x {k}, rank {j.rank}"
        assert col_off >= 0 and col_off + k <= d.cols and (j.rowmap is not None or (row_off >= 0 and row_off + n <= d.rows))
        assert not j.colsum or (col_off == 0 and k == d.cols)
        g = np.random.default_rng(zlib.crc32(j.id.encode()))
        if self.stage == "exact":
            j.master = g.integers(-64, 65, size=(n, k)).astype(np.float32)
            if j.rank:
                j.up = g.integers(-3, 4, size=(n, j.rank)).astype(np.float32)
                j.down = g.integers(-3, 4, size=(j.rank, k)).astype(np.float32)
            # neighbouring rows / columns never share a scale
            j.rs = RS_SET[(np.arange(n) * 5 + int(g.integers(6))) % 6] if rs else None
            j.cs = CS_SET[(np.arange(k) * 3 + int(g.integers(7))) % 7] if cs else None
        else:
            j.master = g.standard_normal((n, k)).astype(np.float32)
            if ranks:
                ups = [g.standard_normal((n, r)).astype(np.float32) * np.float32(0.1) for r in ranks]
                downs = [g.standard_normal((r, k)).astype(np.float32) * np.float32(0.1) for r in ranks]
                scales = (0.7, -0.4, 0.3)[:len(ranks)]
                j.up = np.ascontiguousarray(np.concatenate([u * np.float32(s) for u, s in zip(ups, scales)], axis=1))
                j.down = np.ascontiguousarray(np.concatenate(downs, axis=0))
                j.rank = j.up.shape[1]
            elif j.rank:
                j.up = g.standard_normal((n, j.rank)).astype(np.float32) * np.float32(0.1)
                j.down = g.standard_normal((j.rank, k)).astype(np.float32) * np.float32(0.1)
            j.rs = (np.abs(g.standard_normal(n)) + 0.5).astype(np.float32) if rs else None
            j.cs = (np.abs(g.standard_normal(k)) + 0.5).astype(np.float32) if cs else None
        self.jobs.append(j)
        return j

    def buffers(self):
        """{buffer name: (elements, "bf16" | "f32")} of every destination buffer of the launch."""
        out = {}
        for d in self.dests.values():
            out[d.name + ".out"] = (out_numel(d), d.dtype)
            if d.frag:
                out[d.name + ".frag"] = (d.rows * d.cols, BF16)
            if d.colsum:
                out[d.name + ".colsum"] = (d.rows, F32)
        return out


def _perm(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.int32)


def _plan_like(stage, layout, k):
    """The forms the merge plans of the UNet and the text encoder hold (tests/test_lora_exact_cpu.py::test_plan_signatures_are_covered),
    at 16-row parts: a plain matrix, two column-stacked parts (ffproj, conv2sc), q | k | v and k | v row stacks with and without the
    LayerNorm fold (column scale + colsum) and the query prescale (a row scale), the GEGLU row map with and without the fold; each
    with and without the fragment-major copy."""
    lname = {ROWS: "rows", CHUNK: "chunk"}[layout]
    c = Case(f"plan {lname} k{k}", stage)
    for frag in (False, True):
        f = "f" if frag else ""
        c.dest("plain" + f, layout, 16, k, frag=frag)
        c.job("plain" + f, 16, k, rank=4)
        c.dest("cols" + f, layout, 16, 2 * k, frag=frag)
        c.job("cols" + f, 16, k, rank=4)
        c.job("cols" + f, 16, k, rank=2, col_off=k)
        for fold in (False, True):
            n = f + ("n" if fold else "")
            c.dest("qkv" + n, layout, 48, k, frag=frag, colsum=fold)
            for i in range(3):
                c.job("qkv" + n, 16, k, rank=4, row_off=16 * i, rs=i == 0, cs=fold)
            c.dest("toq" + n, layout, 16, k, frag=frag, colsum=fold)
            c.job("toq" + n, 16, k, rank=4, rs=True, cs=fold)
            c.dest("geglu" + n, layout, 64, k, frag=frag, colsum=fold)
            c.job("geglu" + n, 64, k, rank=4, rowmap=geglu_rowmap(64), cs=fold)
        c.dest("kv" + f, layout, 32, k, frag=frag)
        c.job("kv" + f, 16, k, rank=4)
        c.job("kv" + f, 16, k, rank=4, row_off=16)
    return c


def launches(stage):
    """The launches of the exact stage, or (stage = "rank0") the same geometry with randn masters and scales at rank 0."""
    L = []
    c = Case("column passes", stage)         # K % 4 != 0: scalar loads of down; K % 8 = 4; one pass; a one-lane second pass; a ragged third
    for i, k in enumerate((1, 8, 13, 100, 512, 520, 1032)):
        c.dest(f"k{k}", ROWS, 9, k)
        c.job(f"k{k}", 9, k, rank=7, rs=bool(i & 1), cs=bool(i & 2))
    L.append(c)
    c = Case("rows", stage)                  # the last block has rows past N
    for i, n in enumerate((1, 8, 9, 37)):
        c.dest(f"n{n}", ROWS, n, 100)
        c.job(f"n{n}", n, 100, rank=1, rs=bool(i & 2), cs=bool(i & 1))
    L.append(c)
    c = Case("ranks", stage)                 # LDS is sized by the launch's largest rank: 512, then 1, then 0 with up = down = NULL
    c.dest("r512", ROWS, 16, 1032)
    c.job("r512", 16, 1032, rank=512, rs=True, cs=True)
    c.dest("r1", ROWS, 9, 100)
    c.job("r1", 9, 100, rank=1, rs=True)
    c.dest("r0", ROWS, 9, 100)
    c.job("r0", 9, 100, rank=0, cs=True)
    c.dest("r7", CHUNK, 9, 64)
    c.job("r7", 9, 64, rank=7)
    L.append(c)
    c = Case("job table", stage)             # block counts 1, 1, 5, 1, 2, 1, 1, 3, 1; every job its own master
    for i, n in enumerate((8, 1, 37, 8, 9, 5, 8, 17, 3)):
        c.dest(f"t{i}", ROWS, n, 13)
        c.job(f"t{i}", n, 13, rank=1, rs=bool(i & 1))
    L.append(c)
    c = Case("sources", stage)               # master_ld = K + 3 (vector loads off) and K + 4 (on), NaN in the padding; 4-byte-off operands
    for name, k, kw in (("ld3", 100, dict(master_pad=3)), ("ld4", 100, dict(master_pad=4)), ("ld4k", 104, dict(master_pad=4)),
                        ("master", 104, dict(mis=("master",))), ("down", 104, dict(mis=("down",))),
                        ("colscale", 104, dict(mis=("colscale",), cs=True)), ("all", 104, dict(mis=("master", "down", "colscale"), cs=True, rs=True))):
        c.dest(name, ROWS, 9, k)
        c.job(name, 9, k, rank=7, **kw)
    L.append(c)
    c = Case("rows layout", stage)           # idx & 7 differs between rows; gap columns; col_off 0 / 8 / 2; row_off; a 2-byte-off out
    c.dest("ld100", ROWS, 9, 100)
    c.job("ld100", 9, 100, rank=7, rs=True)
    c.dest("ld104", ROWS, 9, 100, ld=104)
    c.job("ld104", 9, 92, rank=7, col_off=8, cs=True)
    c.dest("co2", ROWS, 12, 100, ld=104)
    c.job("co2", 9, 96, rank=7, col_off=2, row_off=3, rs=True, cs=True)
    c.dest("off", ROWS, 9, 104, off=1)
    c.job("off", 9, 104, rank=7)
    c.dest("aligned", ROWS, 9, 104)
    c.job("aligned", 9, 104, rank=7)
    L.append(c)
    c = Case("chunk-major", stage)           # the second chunk only; a col_off that is no multiple of 8; n < out_rows with a row_off
    c.dest("second", CHUNK, 16, 128)
    c.job("second", 16, 64, rank=7, col_off=64, rs=True)
    c.dest("co2", CHUNK, 9, 128)
    c.job("co2", 9, 60, rank=7, col_off=2, cs=True)
    c.dest("stride", CHUNK, 24, 128)
    c.job("stride", 8, 128, rank=7, row_off=8, rs=True, cs=True)
    c.dest("off", CHUNK, 9, 64, off=1)
    c.job("off", 9, 64, rank=7)
    L.append(c)
    c = Case("fragment copy", stage)         # two 16-row blocks, both halves of a 64-column chunk, two chunks
    c.dest("plain", CHUNK, 32, 128, frag=True)
    c.job("plain", 32, 128, rank=7, rs=True)
    c.dest("perm", CHUNK, 32, 128, frag=True)
    c.job("perm", 32, 128, rank=7, rowmap=_perm(32, 5), cs=True)
    c.dest("stack", CHUNK, 32, 128, frag=True)
    c.job("stack", 16, 128, rank=7, rs=True, cs=True)
    c.job("stack", 16, 128, rank=1, row_off=16)
    c.dest("rows", ROWS, 32, 128, frag=True)
    c.job("rows", 32, 128, rank=7)
    c.dest("cols", ROWS, 32, 128, frag=True)
    c.job("cols", 32, 64, rank=7)
    c.job("cols", 32, 64, rank=1, col_off=64, rs=True)
    c.dest("part", CHUNK, 32, 128, frag=True)     # one part of a 2 x 2 stacking: the other three quarters keep the canary
    c.job("part", 16, 64, rank=7, row_off=16, col_off=64)
    L.append(c)
    c = Case("row map", stage)
    c.dest("perm", ROWS, 16, 100)
    c.job("perm", 16, 100, rank=7, rowmap=_perm(16, 6), rs=True)
    # destination rows -1, 3, 16, 1, 7, -5, 14, 20, 9, 4, 11, 2: two below 0, two at or above out_rows; rows 0 and 15 keep the canary
    c.dest("skip", CHUNK, 16, 64, frag=True, colsum=True)
    c.job("skip", 12, 64, rank=7, row_off=1, rowmap=[-2, 2, 15, 0, 6, -6, 13, 19, 8, 3, 10, 1], rs=True, cs=True)
    c.dest("skiprows", ROWS, 16, 64, frag=True, colsum=True)
    c.job("skiprows", 12, 64, rank=7, row_off=-1, rowmap=[0, 4, 17, 2, 8, -4, 15, 21, 10, 5, 12, 3])
    c.dest("geglu", CHUNK, 64, 64, frag=True, colsum=True)
    c.job("geglu", 64, 64, rank=7, rowmap=geglu_rowmap(64), cs=True)
    L.append(c)
    c = Case("column sum", stage)            # a ragged tail; several passes with every lane busy; a row-stacked pair; a row map
    c.dest("k100", ROWS, 9, 100, colsum=True)
    c.job("k100", 9, 100, rank=7, rs=True)
    c.dest("k1088", CHUNK, 9, 1088, colsum=True)
    c.job("k1088", 9, 1088, rank=7, rs=True, cs=True)
    c.dest("stack", ROWS, 17, 100, colsum=True)
    c.job("stack", 9, 100, rank=7, cs=True)
    c.job("stack", 8, 100, rank=1, row_off=9, cs=True)
    c.dest("map", ROWS, 16, 72, colsum=True)
    c.job("map", 16, 72, rank=7, rowmap=_perm(16, 7), cs=True)
    L.append(c)
    c = Case("fp32", stage)                  # rows at ld 101 (scalar stores) and 104 (vector); transposed with offsets, out 4 bytes off
    c.dest("ld101", ROWS, 9, 100, dtype=F32, ld=101)
    c.job("ld101", 9, 100, rank=7, cs=True)
    c.dest("ld104", ROWS, 9, 104, dtype=F32, ld=104)
    c.job("ld104", 9, 104, rank=7, rs=True, cs=True)
    c.dest("t", TRANS, 12, 16, dtype=F32, off=1)
    c.job("t", 9, 13, rank=7, row_off=3, col_off=2, rs=True)
    c.dest("temb", TRANS, 32, 1088, dtype=F32)     # the time-embedding form: row blocks of one transposed matrix
    c.job("temb", 16, 1088, rank=4)
    c.job("temb", 16, 1088, rank=4, row_off=16)
    L.append(c)
    for layout in (ROWS, CHUNK):
        for k in (64, 576, 1088):            # one, two, three passes
            L.append(_plan_like(stage, layout, k))
    return L


REAL_RANKS = (1, 7, 32, 128, (8, 4))


def real_launches():
    """N = 37, K = 1032 on randn operands: rows with the fragment copy, chunk-major, rows with colsum, fp32 rows."""
    L = []
    for r in REAL_RANKS:
        kw = dict(ranks=r) if isinstance(r, tuple) else dict(rank=r)
        c = Case(f"rank {'+'.join(map(str, r)) if isinstance(r, tuple) else r}", "real")
        c.dest("rows", ROWS, 48, 1088, frag=True)
        c.job("rows", 37, 1032, rs=True, cs=True, **kw)
        c.dest("chunk", CHUNK, 37, 1088)
        c.job("chunk", 37, 1032, col_off=8, rs=True, cs=True, **kw)
        c.dest("sum", ROWS, 37, 1032, colsum=True)
        c.job("sum", 37, 1032, cs=True, **kw)
        c.dest("f32", ROWS, 37, 1032, dtype=F32)
        c.job("f32", 37, 1032, rs=True, **kw)
        L.append(c)
    return L


# ---- the statement ----------------------------------------------------------------------------------------------------------------------
def place(j, d):
    """Where the header puts the job's elements: (kept [n] bool, destination rows [n], out index [n][k], fragment index [n][k] or None)."""
    row = (np.arange(j.n) if j.rowmap is None else j.rowmap.astype(np.int64)) + j.row_off
    kept = (row >= 0) & (row < d.rows)
    r = row[:, None]
    col = (j.col_off + np.arange(j.k))[None, :]
    if d.layout == ROWS:
        out = r * d.ld + col
    elif d.layout == CHUNK:
        out = ((col // 64) * d.rows + r) * 64 + col % 64
    else:
        out = col * d.rows + r
    frag = None
    if j.frag:
        p = FRAG_ROW[np.mod(r, 16)]
        frag = (((((col // 64) * (d.rows // 16) + r // 16) * 2 + (col // 32) % 2) * 4 + (col // 8) % 4) * 16 + p) * 8 + col % 8
    return kept, row, out, frag


def value64(j):
    """The job's values in float64 (the exact stage: asserted to be fp32 numbers by `conditions`)."""
    v = j.master.astype(np.float64)
    if j.rank:
        v = v + j.up.astype(np.float64) @ j.down.astype(np.float64)
    if j.rs is not None:
        v = v * j.rs.astype(np.float64)[:, None]
    if j.cs is not None:
        v = v * j.cs.astype(np.float64)[None, :]
    return v


def value32_rank0(j, order="rows first"):
    """v = master, (v * rs) * cs in numpy float32, each product rounded once.  order: "cols first" / "scales first" are the two other
    ways to write it, which the header rules out (used by `conditions` to show that the case list can tell them apart)."""
    assert j.rank == 0
    v = j.master
    rs = None if j.rs is None else j.rs[:, None]
    cs = None if j.cs is None else j.cs[None, :]
    if order == "scales first" and rs is not None and cs is not None:
        return v * (rs * cs)
    for s in ((rs, cs) if order == "rows first" else (cs, rs)):
        if s is not None:
            v = v * s
    return v


def job_value32(case, j):
    return value32_rank0(j) if case.stage == "rank0" else value64(j).astype(np.float32)


def reference(case, j):
    """{buffer name: (bits, mask)} of one job: the bits the header demands and the elements the job may write."""
    d = case.dests[j.dest]
    v = job_value32(case, j)
    kept, row, oi, fi = place(j, d)
    bits = bf16_rne(v) if d.dtype == BF16 else f32_bits(v)
    res = {}

    def put(name, numel, dtype, idx, vals):
        b, m = np.zeros(numel, dtype=np_dtype(dtype)), np.zeros(numel, dtype=bool)
        assert idx.min(initial=0) >= 0 and idx.max(initial=0) < numel and len(np.unique(idx)) == idx.size, j.id
        b[idx.ravel()] = vals.ravel()
        m[idx.ravel()] = True
        res[name] = (b, m)

    put(d.name + ".out", out_numel(d), d.dtype, oi[kept], bits[kept])
    if j.frag:
        put(d.name + ".frag", d.rows * d.cols, BF16, fi[kept], bits[kept])
    if j.colsum:
        s = bf16_value(bits).astype(np.float64).sum(axis=1).astype(np.float32)
        put(d.name + ".colsum", d.rows, F32, row[kept], f32_bits(s)[kept])
    return res


def expected(case):
    """{buffer name: (bits, written)}: the jobs of the launch laid in order over canary-filled buffers."""
    if getattr(case, "_expected", None) is not None:      # (computed once per case, shared, never written to)
        return case._expected
    out = {name: (np.full(n, canary_bits(dt), dtype=np_dtype(dt)), np.zeros(n, dtype=bool)) for name, (n, dt) in case.buffers().items()}
    case._expected = out
    for j in case.jobs:
        for name, (b, m) in reference(case, j).items():
            out[name][0][m] = b[m]
            out[name][1][m] = True
    return out


# ---- conditions -------------------------------------------------------------------------------------------------------------------------
def _is_f32(x, what):
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x), f"{what}: not an fp32 number: the case is not exact"


def _sum_exact(vals, what):
    """The float64 sum of every row of `vals` (bf16 numbers) is exact in any order: all are multiples of q, and sum |x| < 2^53 q."""
    nz = vals[vals != 0]
    if nz.size == 0:
        return
    q = 2.0 ** (np.frexp(np.abs(nz))[1].min() - 8)
    assert np.array_equal(np.round(vals / q) * q, vals), what
    assert np.abs(vals).sum(axis=-1).max() / q < 2.0 ** 53, f"{what}: a row sum that float64 may round"


def conditions(case):
    """Asserts that `case` is exact in its stage's sense; returns (ties rounding down to an even mantissa, ties rounding up from an odd
    one, elements whose bits depend on the order of the two scales) over its bf16 / all destinations."""
    even = odd = order = 0
    for j in case.jobs:
        d = case.dests[j.dest]
        if case.stage == "exact":
            assert j.rank <= 512 and np.abs(j.master).max() <= 64 and np.array_equal(j.master, np.round(j.master)), j.id
            v = j.master.astype(np.float64)
            if j.rank:
                assert np.abs(j.up).max() <= 3 and np.abs(j.down).max() <= 3, j.id
                assert np.array_equal(j.up, np.round(j.up)) and np.array_equal(j.down, np.round(j.down)), j.id
                s = np.abs(j.master).astype(np.float64) + np.abs(j.up).astype(np.float64) @ np.abs(j.down).astype(np.float64)
                assert s.max() < LIMIT, f"{j.id}: sum |up down| + |master| = {s.max():.0f}: not below 2^24"
                v = v + j.up.astype(np.float64) @ j.down.astype(np.float64)
            _is_f32(v, j.id + ": master + up down")
            assert np.abs(v).max() < 2 ** 13, j.id
            if j.rs is not None:
                assert np.isin(j.rs, RS_SET).all() and (j.n == 1 or (j.rs[1:] != j.rs[:-1]).all()), j.id
                v = v * j.rs.astype(np.float64)[:, None]
                _is_f32(v, j.id + ": v * rowscale")
            if j.cs is not None:
                assert np.isin(j.cs, CS_SET).all() and (j.k == 1 or (j.cs[1:] != j.cs[:-1]).all()), j.id
                v = v * j.cs.astype(np.float64)[None, :]
                _is_f32(v, j.id + ": (v * rowscale) * colscale")
            assert np.array_equal(np.round(v * 16), v * 16) and np.abs(v * 16).max() < LIMIT, f"{j.id}: not sixteenths below 2^24"
            v32 = v.astype(np.float32)
        else:
            assert j.rank == 0 and j.up is None and j.down is None, j.id
            v32 = value32_rank0(j)
            assert np.isfinite(v32).all() and (np.abs(v32[v32 != 0]) > 2.0 ** -100).all(), j.id
            other = [value32_rank0(j, o) for o in ("cols first", "scales first")]
            out_bits = (lambda x: bf16_rne(x)) if d.dtype == BF16 else f32_bits
            order += int(min((out_bits(o) != out_bits(v32)).sum() for o in other))
        if d.dtype == BF16:
            b = f32_bits(v32)
            tie = (b & 0xFFFF) == 0x8000
            even += int((tie & ((b >> 16) & 1 == 0)).sum())
            odd += int((tie & ((b >> 16) & 1 == 1)).sum())
            if j.colsum:
                _sum_exact(bf16_value(bf16_rne(v32)).astype(np.float64), j.id + ": colsum")
    return even, odd, order


# ---- the checkers -----------------------------------------------------------------------------------------------------------------------
def check(case, got):
    """got {buffer name: bits} against `expected`: the statement's bits where a job may write, the canary everywhere else."""
    want = expected(case)
    assert set(got) == set(want), (case.id, sorted(got), sorted(want))
    for name in sorted(want):
        w, written = want[name]
        g = np.asarray(got[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (case.id, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = g != w
        if bad.any():
            i = int(np.argwhere(bad)[0, 0])
            where = "an element a job writes" if written[i] else "an element no job may write (it held the canary)"
            raise AssertionError(f"{case.id}: {name}: {int(bad.sum())} of {bad.size} elements differ in their bits, "
                                 f"{int((bad & ~written).sum())} of them outside every job's mask; first at {i}, {where}: "
                                 f"got 0x{int(g[i]):x}, the statement gives 0x{int(w[i]):x}")


def real_bounds(j):
    """(v64, b): the float64 value of every element and the bound on the distance of the kernel's fp32 v from it."""
    a = np.abs(j.master).astype(np.float64)
    S = np.abs(j.up).astype(np.float64) @ np.abs(j.down).astype(np.float64)
    R = j.rank
    gamma = R * U / (1 - R * U)
    scale = np.ones_like(a)
    if j.rs is not None:
        scale = scale * np.abs(j.rs).astype(np.float64)[:, None]
    if j.cs is not None:
        scale = scale * np.abs(j.cs).astype(np.float64)[None, :]
    return value64(j), scale * (gamma * S + 3 * U * (a + S)) * (1 + 3 * U)


def check_real(case, got):
    """The rank > 0 stage on real operands.  Returns the largest |got - v64| / b over the launch's fp32 elements and the share of bf16
    elements whose interval is a single number."""
    bufs = case.buffers()
    written = {name: np.zeros(n, dtype=bool) for name, (n, _) in bufs.items()}
    worst, single, total = 0.0, 0, 0
    for j in case.jobs:
        d = case.dests[j.dest]
        v64, b = real_bounds(j)
        kept, row, oi, fi = place(j, d)
        assert kept.all()
        g = np.asarray(got[d.name + ".out"])[oi]
        written[d.name + ".out"][oi.ravel()] = True
        if d.dtype == BF16:
            lo, hi = bf16_key(bf16_rne((v64 - b).astype(np.float32))), bf16_key(bf16_rne((v64 + b).astype(np.float32)))
            k = bf16_key(g)
            bad = (k < lo) | (k > hi)
            if bad.any():
                i = tuple(int(x) for x in np.argwhere(bad)[0])
                raise AssertionError(f"{j.id}: {int(bad.sum())} of {bad.size} bf16 elements outside [bf16(v64 - b), bf16(v64 + b)], first at {i}: "
                                     f"got {float(bf16_value(g[i]))!r}, v64 {float(v64[i])!r}, b {float(b[i]):.3g}")
            single += int((lo == hi).sum())
            total += lo.size
            if j.frag:
                assert np.array_equal(np.asarray(got[d.name + ".frag"])[fi], g), f"{j.id}: the fragment copy differs from the matrix"
                written[d.name + ".frag"][fi.ravel()] = True
            if j.colsum:
                own = bf16_value(g).astype(np.float64)
                _sum_exact(own, j.id + ": colsum of the kernel's own row")
                want = f32_bits(own.sum(axis=1).astype(np.float32))
                assert np.array_equal(np.asarray(got[d.name + ".colsum"])[row], want), f"{j.id}: colsum is not the fp32 of the fp64 sum of the stored row"
                written[d.name + ".colsum"][row] = True
        else:
            err = np.abs(g.view(np.float32).astype(np.float64) - v64)
            bad = ~(err <= b)
            if bad.any():
                i = tuple(int(x) for x in np.argwhere(bad)[0])
                raise AssertionError(f"{j.id}: {int(bad.sum())} of {bad.size} fp32 elements further than b from v64, first at {i}: "
                                     f"got {float(g.view(np.float32)[i])!r}, v64 {float(v64[i])!r}, b {float(b[i]):.3g}")
            worst = max(worst, float((err / b).max()))
    for name, (n, dt) in bufs.items():
        g = np.asarray(got[name])
        assert (g[~written[name]] == canary_bits(dt)).all(), f"{case.id}: {name}: an element no job may write lost its canary"
    return worst, single / max(total, 1)


# ---- a model of the kernel's addressing, with faults ------------------------------------------------------------------------------------
def _flat(a, ld=None):
    """The operand as it lies in memory: rows `ld` apart, NaN between them."""
    if a.ndim == 1 or ld is None or ld == a.shape[1]:
        return np.ascontiguousarray(a).reshape(-1)
    n, k = a.shape
    f = np.full((n - 1) * ld + k, np.nan, dtype=a.dtype)
    for r in range(n):
        f[r * ld:r * ld + k] = a[r]
    return f


def _gather(flat, idx):
    """flat[idx]; outside the operand lies its NaN guard band."""
    out = np.full(idx.shape, np.nan, dtype=np.float32)
    ok = (idx >= 0) & (idx < flat.size)
    out[ok] = flat[idx[ok]]
    return out


def _store(buf, idx, val):
    """buf holds SLACK elements on both sides of the destination; what lands further out lands on the slack's edge."""
    i = np.clip(np.asarray(idx) + SLACK, 0, buf.size - 1)
    buf[i.ravel()] = np.asarray(val).ravel()


def model(case, fault=None):
    """{buffer name: bits with SLACK canaries on both sides} after the launch, computed the way the kernel is built: a workgroup per 8 rows
    of a job, a lane per 8 columns, passes of 512 columns, the up factors staged [rank][8] with the job's own rank as the stride, the
    destination index of each layout, the fragment index, colsum over the lanes' valid elements.  fault: one of FAULTS."""
    assert fault is None or fault in FAULTS
    bufs = {name: np.full(n + 2 * SLACK, canary_bits(dt), dtype=np_dtype(dt)) for name, (n, dt) in case.buffers().items()}
    max_rank = max(j.rank for j in case.jobs)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in case.jobs:
            _model_job(case, j, bufs, max_rank, fault)
    return bufs


def _model_job(case, j, bufs, max_rank, fault):
    d = case.dests[j.dest]
    N, K, R = j.n, j.k, j.rank
    blocks = -(-N // BLOCK_ROWS)
    n = np.arange(blocks * BLOCK_ROWS)                     # the rows of the job's workgroups
    k = np.arange(-(-K // LANE_COLS) * LANE_COLS)          # the columns of the lanes that have any
    Kl = -(-K // 4) * 4 if fault == "K rounded up to 4" else K
    in_job = n < N
    if fault == "first block to the previous job" and j.i > 0:
        in_job &= n >= BLOCK_ROWS                           # (the previous job has no such rows: its workgroup writes nothing)
    loaded = (k < k.size) if fault == "colsum of the padded lanes" else (k < Kl)    # load8: a lane's elements past K are zeros
    # the low-rank product
    v = np.where(in_job[:, None] & loaded[None, :], _gather(_flat(j.master, j.master_ld), n[:, None] * (K if fault == "master row stride K" else j.master_ld) + k[None, :]), np.float32(0))
    if R:
        stride = max_rank if fault == "up stride of the largest rank" else R
        jj = np.arange(R)
        up = np.where(in_job[:, None], _gather(_flat(j.up), n[:, None] * stride + jj[None, :]), np.float32(0))
        down = np.where(loaded[None, :], _gather(_flat(j.down), jj[:, None] * K + k[None, :]), np.float32(0))
        acc = (up.astype(np.float64) @ down.astype(np.float64)).astype(np.float32)      # (exact on the exact stage's operands)
        v = v + acc
    rs = cs = None
    if j.rs is not None:
        rs = np.where(in_job, _gather(j.rs, n % BLOCK_ROWS if fault == "row scale of the block's row" else n), np.float32(1))[:, None]
    if j.cs is not None:
        cs = np.where(loaded, _gather(j.cs, k + j.col_off if fault == "column scale by destination column" else k), np.float32(0))[None, :]
    for s in ((cs, rs) if fault == "scale order swapped" else (rs, cs)):
        if s is not None:
            v = (v * s).astype(np.float32)
    # destination rows
    row = np.where(in_job, (n if j.rowmap is None else _gather_int(j.rowmap, n)) + j.row_off, -1)
    outside = (row < 0) | (row >= d.rows)
    if fault == "skipped row clamped and written":
        row, outside = np.clip(row, 0, d.rows - 1), np.zeros_like(outside)
    kept = in_job & ~outside
    stored = k < Kl
    if fault == "tail lane drops its columns":
        stored = k < K // LANE_COLS * LANE_COLS
    if fault == "tail lane stores eight columns":
        stored = k < k.size
    summed = k < (k.size if fault == "colsum of the padded lanes" else Kl)
    if fault == "no second pass":
        stored, summed = stored & (k < PASS_COLS), summed & (k < PASS_COLS)
    col = j.col_off + k
    if d.dtype == BF16:
        b = f32_bits(v)
        if fault == "bf16 truncated":
            bits = (b >> 16).astype(np.uint16)
        elif fault == "bf16 round half up":
            bits = ((b.astype(np.uint64) + 0x8000) >> 16).astype(np.uint16)
        else:
            bits = bf16_rne(v)
    else:
        bits = f32_bits(v)
    r, c = row[kept][:, None], col[stored][None, :]
    sel = bits[kept][:, stored]
    if d.layout == ROWS:
        idx = r * d.ld + c
    elif d.layout == CHUNK:
        idx = ((c >> 6) * (N if fault == "chunk stride n" else d.rows) + r) * 64 + (c & 63)
    else:
        idx = c * d.rows + r
    _store(bufs[d.name + ".out"], idx, sel)
    if j.frag:
        fr = r
        if fault == "fragment: row_off ignored":
            fr = r - j.row_off
        if fault == "fragment: rowmap ignored":
            fr = n[kept][:, None] + j.row_off
        fc = k[stored][None, :] if fault == "fragment: col_off dropped" else c
        rp = (fr & 15) if fault == "fragment: identity row order" else FRAG_ROW[fr & 15]
        half = 0 if fault == "fragment: half dropped" else (fc >> 5) & 1
        idx = (((((fc >> 6) * (d.rows >> 4) + (fr >> 4)) * 2 + half) * 4 + ((fc >> 3) & 3)) * 16 + rp) * 8 + (fc & 7)
        _store(bufs[d.name + ".frag"], idx, sel)
    if j.colsum:
        if fault == "colsum of the unrounded values":
            s = v[:, summed].astype(np.float64).sum(axis=1)
        elif fault == "colsum in fp32":
            t = bf16_value(bits)[:, summed]
            s = np.cumsum(t, axis=1, dtype=np.float32)[:, -1] if t.shape[1] else np.zeros(n.size, dtype=np.float32)
        else:
            s = bf16_value(bits)[:, summed].astype(np.float64).sum(axis=1)
        who = in_job if fault == "colsum of a skipped row written" else kept
        _store(bufs[d.name + ".colsum"], np.clip(row[who], 0, d.rows - 1) if fault == "colsum of a skipped row written" else row[who],
               f32_bits(s.astype(np.float32))[who])


def _gather_int(a, idx):
    out = np.full(idx.shape, -(1 << 20), dtype=np.int64)      # (rows past N are never looked up)
    ok = idx < a.size
    out[ok] = a[idx[ok]]
    return out


def check_model(case, fault=None):
    """The model's launch through the same checks as the device's: the guard bands (here: the slack) keep their canary, then `check`."""
    bufs = model(case, fault)
    core = {}
    for name, (n, dt) in case.buffers().items():
        b = bufs[name]
        assert (b[:SLACK] == canary_bits(dt)).all() and (b[SLACK + n:] == canary_bits(dt)).all(), f"{case.id}: {name}: a guard band was damaged"
        core[name] = b[SLACK:SLACK + n]
    check(case, core)


# ---- what the kernel sees of a job ------------------------------------------------------------------------------------------------------
SIGNATURE = ("layout", "out dtype", "passes", "K % 8", "K % 4", "col_off % 8", "row_off != 0", "n % 8", "n < out_rows", "rowmap", "rowscale",
             "colscale", "colsum", "fragment copy", "parts")


def signature(*, layout, dtype, n, k, row_off, col_off, out_rows, rowmap, rowscale, colscale, colsum, frag, parts):
    """The branches of the kernel a job takes, as far as its descriptor decides them."""
    return (int(layout), dtype, min(3, -(-k // PASS_COLS)), k % 8, k % 4, col_off % 8, row_off != 0, n % 8, n < out_rows, bool(rowmap),
            bool(rowscale), bool(colscale), bool(colsum), bool(frag), min(2, parts))


def case_signatures(cases):
    out = set()
    for c in cases:
        parts = {}
        for j in c.jobs:
            parts[j.dest] = parts.get(j.dest, 0) + 1
        for j in c.jobs:
            d = c.dests[j.dest]
            out.add(signature(layout=d.layout, dtype=d.dtype, n=j.n, k=j.k, row_off=j.row_off, col_off=j.col_off, out_rows=d.rows,
                              rowmap=j.rowmap is not None, rowscale=j.rs is not None, colscale=j.cs is not None, colsum=j.colsum,
                              frag=j.frag, parts=parts[j.dest]))
    return out
