"""msd_lora_merge held to bits (tests/_exact_lora.py; the case lists are proven on the CPU by tests/test_lora_exact_cpu.py).

test_merge_kernel_matches_float64 (tests/test_lora_switch_gpu.py) runs one geometry on randn operands and allows one bf16 ulp.  Here:

  test_exact    integer operands: every launch of _exact_lora.launches("exact") - column passes K = 1 .. 1088, rows N = 1 .. 37, rank 0
                (up = down = NULL) .. 512 with a rank-512 job ahead of a rank-1 and a rank-0 job, a nine-job table with block counts
                1 1 5 1 2 1 1 3 1, master_ld = K + 3 / K + 4 over NaN padding, operands 4 bytes off a 16-byte boundary, every layout
                with column / row offsets, row gaps and a misaligned `out`, the fragment copy plain / mapped / row- and column-stacked,
                row maps with entries outside the destination, colsum over a ragged tail / several passes / stacked parts, fp32 rows
                and transposed, and every form a job takes in the real merge plans.  `out`, `out_frag` and `colsum` must hold the
                float64 statement's bits, and the canary wherever no job may write.  No tolerance.
  test_rank0    the same geometry at rank 0 on randn masters and scales: v = master, (v * rs) * cs in numpy float32, round to nearest
                even - the kernel-level form of "a rank-0 job reproduces the load-time packing bit for bit".  Sees a swapped scale order.
  test_real     rank 1, 7, 32, 128 and 8 + 4 concatenated (MergeBase._factors) at N = 37, K = 1032 on randn operands, rows with the
                fragment copy, chunk-major, rows with colsum, fp32 rows: every bf16 element in [bf16(v64 - b), bf16(v64 + b)], every
                fp32 element within b of v64, with b derived beside the reference (_exact_lora.real_bounds: no number chosen by hand);
                colsum = fp32 of the float64 sum of the kernel's own stored row, to the bit; the fragment copy = the matrix.
                Assumed, not tested: __fadd_rn / __fmul_rn / fma correctly rounded; no operand near overflow or the subnormals.

Every operand and destination lies between guard bands (tests/_guard.py) sized to the byte by tests/_extents_lora.py; a misaligned
operand is the view [1:] of a guarded buffer one element longer whose first element must keep its NaN / canary.

Measured on an MI355X (this module's first run: 40 tests in 3.2 s, the slowest 0.3 s; none refused, the kernel needed no change):
  exact, rank 0   every launch bit-equal, every canary and guard band intact
  real operands   fp32 |v - v64| / b at its largest: rank 1  0.618   7  0.538   32  0.310   128  0.042   8 + 4  0.565
                  (master ~ N(0, 1) and factors ~ 0.1 N(0, 1): the three final roundings dominate, so the ratio falls as gamma_R grows);
                  98.66 % (rank 128) to 99.99 % (rank 1) of the bf16 intervals are a single number, so the interval check is a bit
                  check for all but about 1 element in 100 .. 10,000
The RECORD lines print the same figures again."""
import numpy as np
import pytest
import torch

import _exact_lora as E
import _extents_lora as XL
import _guard as G
from conftest import run_calls

pytestmark = pytest.mark.gpu

NAN = float("nan")
EXACT = E.launches("exact")
RANK0 = E.launches("rank0")
REAL = E.real_launches()
TORCH = {E.BF16: torch.bfloat16, E.F32: torch.float32}


def _bits(t):
    """A bf16 / fp32 device tensor -> its bits as a flat uint16 / uint32 numpy array."""
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1)
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1)


class Launch:
    """The operands of one case on the device, every one between guard bands; run() launches once and returns {buffer name: bits}."""
    def __init__(self, gpu, case):
        from minsdtf_amd import ops

        self.case, self.g, self.off, self.flat = case, G.Guard(gpu), [], {}
        g = self.g
        jobs = []
        named = {}                                    # destination buffer -> the extent name it was allocated under
        for j in case.jobs:
            d = case.dests[j.dest]
            pre = f"j{j.i}."
            geo = dict(n=j.n, k=j.k, rank=j.rank, out_rows=d.rows, out_cols=d.cols, layout=d.layout, out_dtype=d.dtype,
                       master_ld=j.master_ld, ld=d.ld)
            ext = XL.lora_job(**geo, rowscale=j.rs, colscale=j.cs, rowmap=j.rowmap, out_frag=j.frag or None, colsum=j.colsum or None)
            g.bind(pre, ext)
            kw = dict(master=self._source(j, "master", j.master, pre, ext, ld=j.master_ld))
            if j.rank:
                kw["up"] = g.inp(torch.from_numpy(j.up), pre + "up")
                kw["down"] = self._source(j, "down", j.down, pre, ext)
            if j.rs is not None:
                kw["rowscale"] = g.inp(torch.from_numpy(j.rs), pre + "rowscale")
            if j.cs is not None:
                kw["colscale"] = self._source(j, "colscale", j.cs, pre, ext)
            if j.rowmap is not None:
                kw["rowmap"] = g.inp(torch.from_numpy(j.rowmap), pre + "rowmap")
            for part in ("out",) + (("out_frag",) if j.frag else ()) + (("colsum",) if j.colsum else ()):
                buf = d.name + {"out": ".out", "out_frag": ".frag", "colsum": ".colsum"}[part]
                if buf not in self.flat:
                    kw[part] = self._destination(d, part, buf, pre + part, ext[part][0])
                    named[buf] = kw[part]
                else:
                    kw[part] = named[buf]
                    if not (part == "out" and d.off):
                        g.same(kw[part], pre + part)    # a later part of the same matrix: the header gives it the same bytes
            jobs.append(ops.lora_job(**kw, n=j.n, k=j.k, rank=j.rank, master_ld=j.master_ld, out_rows=d.rows, out_cols=d.cols,
                                     layout=d.layout, out_dtype=ops.OUT_BF16 if d.dtype == E.BF16 else ops.OUT_F32, ld=d.ld,
                                     row_off=j.row_off, col_off=j.col_off))
            self.keep = getattr(self, "keep", []) + [kw]
        self.call = ops.lora_merge(jobs, gpu)

    def _source(self, j, name, array, pre, ext, ld=None):
        """An fp32 input; 4 bytes off a 16-byte boundary where the job asks for it; rows `ld` apart over NaN."""
        if name not in j.mis:
            wide = ld is not None and array.ndim == 2 and ld > array.shape[1]
            return self.g.inp(torch.from_numpy(np.ascontiguousarray(array)), pre + name, ld=ld if wide else None)
        flat = torch.from_numpy(E._flat(array, ld))
        assert flat.numel() * 4 == ext[name][0]
        buf = self.g.out((flat.numel() + 1,), torch.float32, NAN, label=f"{pre}{name}, 4 bytes off")
        view = buf[1:]
        assert view.data_ptr() % 16 == 4
        view.copy_(flat)
        self.off.append((buf, None))
        return view

    def _destination(self, d, part, buf, name, nbytes):
        g = self.g
        if part == "colsum":
            t = g.out((d.rows,), torch.float32, E.CANARY, name)
        elif part == "out_frag":
            t = g.out((d.rows * d.cols,), torch.bfloat16, E.CANARY, name)
        else:
            dt, numel = TORCH[d.dtype], E.out_numel(d)
            assert numel * (2 if d.dtype == E.BF16 else 4) == nbytes
            if d.off:
                whole = g.out((numel + 1,), dt, E.CANARY, label=f"{name}, one element off")
                t = whole[1:]
                assert t.data_ptr() % 16 == (2 if d.dtype == E.BF16 else 4)
                self.off.append((whole, E.canary_bits(d.dtype)))
            elif d.layout == E.ROWS and d.ld > d.cols:
                rows = g.out((d.rows, d.cols), dt, E.CANARY, name, ld=d.ld, gap=E.CANARY)
                self.flat[buf] = torch.as_strided(rows, (numel,), (1,))
                return rows
            else:
                t = g.out((numel,), dt, E.CANARY, name)
        self.flat[buf] = t
        return t

    def run(self):
        run_calls(self.call)
        return {name: _bits(t) for name, t in self.flat.items()}

    def check(self):
        self.g.check()
        for buf, canary in self.off:
            if canary is None:
                assert bool(torch.isnan(buf[0])), "the float in front of a misaligned operand was written"
            else:
                assert int(_bits(buf[:1])[0]) == int(canary), "the element in front of a misaligned destination was written"


@pytest.mark.parametrize("c", EXACT, ids=[c.id for c in EXACT])
def test_exact(gpu, c):
    E.conditions(c)
    run = Launch(gpu, c)
    E.check(c, run.run())
    run.check()


@pytest.mark.parametrize("c", RANK0, ids=[c.id for c in RANK0])
def test_rank0(gpu, c):
    E.conditions(c)
    run = Launch(gpu, c)
    E.check(c, run.run())
    run.check()


@pytest.mark.parametrize("c", REAL, ids=[c.id for c in REAL])
def test_real(gpu, c):
    run = Launch(gpu, c)
    worst, single = E.check_real(c, run.run())
    run.check()
    print(f"\nRECORD | {c.id} | fp32 |v - v64| / b at most {worst:.3f} | {single * 100:.2f} % of the bf16 intervals are one number")


def test_a_second_launch_gives_the_same_bits(gpu):
    """Deterministic: every element and every row sum has one evaluation order."""
    c = REAL[3]
    run = Launch(gpu, c)
    first = run.run()
    second = run.run()
    assert all(np.array_equal(first[k], second[k]) for k in first)
    run.check()
