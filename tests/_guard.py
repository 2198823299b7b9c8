"""Guard bands for the kernel tests: every operand of a launch lives between two poisoned bands, and after the launch every band
(and every unused column of a wide leading dimension) must carry the bits it was given.

The engines pack buffers back to back in one arena (engine.Arena: 256-byte granularity, ranges recycled), so a store one vector
past a ragged edge, a read of a padding column that reaches the result, or a write into an input damages a live neighbour in
production; behind an exactly-sized torch allocation nothing notices.  Here each operand is one uint8 storage

    [ band | payload | band ]

whose payload is EXACTLY the bytes tests/_extents.py gives the operand, starts on a 256-byte boundary (the arena's alignment)
and is followed by the tail band on the very next byte.  A band is max(64 KiB, 256 x the operand's innermost row bytes): 256 rows
is the most any tile form owns, so one tile's overrun cannot jump it.  Floating operands get NaN bands (a value read from outside
and used - even times a zero weight - reaches the result as NaN, which close() refuses); integer operands get a small non-zero
pattern (write detection only; harmless if it were read as an index).

Plain torch: works on "cpu" as on the GPU.  Not a conftest: imported by name."""
import torch

ALIGN = 256
MIN_BAND = 64 * 1024
ROWS = 256
INT_PATTERN = 3      # every integer band / canary element; small, non-zero, no wild index if read
CANARY = -1.5        # floating output gaps: finite, so a kernel that reads AND keeps it is still caught by the bit check

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _esz(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _fill(t, value):
    if t.numel():
        t.fill_(value)


class _Operand:
    def __init__(self, label, storage, lead, nbytes, dtype, role):
        self.label, self.storage, self.lead, self.nbytes, self.dtype, self.role = label, storage, lead, nbytes, dtype, role
        self.front = storage[:lead]
        self.tail = storage[lead + nbytes:]
        self.front_want = self.tail_want = None
        self.gaps = []     # (flat index tensor into the payload's elements, expected integer bits)

    def payload(self):
        """The way engine.Buf.tensor builds its views: a slice of the uint8 storage, re-typed."""
        return self.storage[self.lead:self.lead + self.nbytes].view(self.dtype)


class Guard:
    def __init__(self, device, ext=None):
        self.device = torch.device(device)
        self.ext = dict(ext or {})        # {operand name: (bytes, role)} of tests/_extents.py
        self.operands = []
        self._by_ptr = {}

    def bind(self, prefix, ext):
        """More extents under prefixed operand names ("prod.out", "cons.a0": a test with two kinds of launch)."""
        self.ext.update({prefix + k: v for k, v in ext.items()})

    def same(self, view, name):
        """`view` also serves as operand `name` (one launch's output is the next one's input): its payload is that operand's size too."""
        op = self._by_ptr[view.data_ptr()]
        assert op.nbytes == self.ext[name][0], f"{op.label}: {op.nbytes} bytes, the header gives operand '{name}' {self.ext[name][0]}"
        return view

    # ---- allocation
    def band_bytes(self, row_bytes):
        return max(MIN_BAND, ROWS * int(row_bytes))

    def _alloc(self, label, nbytes, dtype, row_bytes, role, name):
        if name is not None and name in self.ext:
            need = self.ext[name][0]
            assert nbytes == need, f"{label}: {nbytes} bytes allocated, the header gives operand '{name}' {need}"
            role = self.ext[name][1] if self.ext[name][1] == "inout" else role
        esz = _esz(dtype)
        assert nbytes % esz == 0
        band = self.band_bytes(row_bytes)
        storage = torch.empty(band + ALIGN + nbytes + band, dtype=torch.uint8, device=self.device)
        lead = band + (-(storage.data_ptr() + band)) % ALIGN
        storage = storage[:lead + nbytes + band]
        op = _Operand(label, storage, lead, nbytes, dtype, role)
        poison = float("nan") if dtype.is_floating_point else INT_PATTERN
        assert lead % esz == 0 and band % esz == 0
        _fill(op.front.view(dtype), poison)
        _fill(op.tail.view(dtype), poison)
        op.front_want, op.tail_want = op.front.clone(), op.tail.clone()
        self.operands.append(op)
        self._by_ptr[storage.data_ptr() + lead] = op
        return op

    @staticmethod
    def _view(op, shape, ld):
        flat = op.payload()
        if ld is None:
            return flat.view(*shape)
        strides, s = [], 1
        for i, n in enumerate(reversed(shape)):
            strides.append(s)
            s = ld if i == 0 else s * n
        return flat.as_strided(tuple(shape), tuple(reversed(strides)))

    def inp(self, tensor, name=None, ld=None, label=None, gap=None):
        """Upload `tensor` (CPU or device) as an input: a view of exactly its bytes between two bands.  ld: the rows of the last
        dimension lie `ld` elements apart (q inside a 3C-wide buffer); the payload is then (rows - 1) * ld + cols elements and the
        columns in between are NaN gaps (integers: the pattern), registered for the bit check."""
        return self._make(tuple(tensor.shape), tensor.dtype, None, name, ld, label, "in", tensor, gap)

    def out(self, shape, dtype, fill, name=None, ld=None, label=None, gap=None):
        """An output (or scratch) of `shape` filled with `fill`; ld as for inp(), its gaps hold a canary."""
        return self._make(tuple(shape), dtype, fill, name, ld, label, "out", None, gap)

    def _poison(self, op, gap):
        if gap is not None:
            return gap
        return (float("nan") if op.role == "in" else CANARY) if op.dtype.is_floating_point else INT_PATTERN

    def _make(self, shape, dtype, fill, name, ld, label, role, src, gap):
        esz = _esz(dtype)
        cols = shape[-1] if shape else 1
        rows = 1
        for n in shape[:-1]:
            rows *= n
        numel = rows * cols if ld is None else ((rows - 1) * ld + cols if rows else 0)
        op = self._alloc(label or name or f"operand{len(self.operands)}", numel * esz, dtype, (ld or cols) * esz, role, name)
        view = self._view(op, shape, ld)
        if ld is not None and ld > cols:
            _fill(op.payload(), self._poison(op, gap))
        if src is not None:
            view.copy_(src)
        elif fill is not None:
            view.fill_(fill)
        self._by_ptr[view.data_ptr()] = op
        if ld is not None and ld > cols:
            self._register_gap(op, ld, cols, None)
        return view

    def gaps(self, view, used_cols, ld=None, gap=None):
        """`view` (from inp / out) has a leading dimension wider than the `used_cols` it carries (vt_ld > t, out_ld > N, ld_in / ld_out >
        cols): fill columns [used_cols, ld) of every row of the payload with NaN (inputs) or a canary (outputs) and register them for
        check().  ld defaults to the view's row stride; gap overrides the fill (the zeros of an A / B launch)."""
        op = self._by_ptr[view.data_ptr()]
        ld = int(view.stride(-2)) if ld is None else ld
        assert 0 < used_cols <= ld
        if used_cols < ld:
            self._register_gap(op, ld, used_cols, self._poison(op, gap))
        return view

    def _register_gap(self, op, ld, cols, value):
        """Columns [cols, ld) of every row of the flat payload: filled with `value` (None: as they are), kept for check()."""
        flat = op.payload()
        idx = torch.arange(flat.numel(), device=self.device)
        idx = idx[(idx % ld) >= cols]
        if value is not None:
            flat[idx] = value
        op.gaps.append((idx, flat.view(_INT_VIEW[_esz(op.dtype)])[idx].clone(), ld))

    # ---- the check
    def check(self):
        """Every band and every registered gap of every operand is bit-identical to what was written (compared on the device)."""
        for op in self.operands:
            for side, got, want in (("front band", op.front, op.front_want), ("tail band", op.tail, op.tail_want)):
                if not torch.equal(got, want):
                    first = int(torch.nonzero(got != want)[0])
                    off = first - op.lead if side == "front band" else op.nbytes + first
                    raise AssertionError(f"guard: operand '{op.label}' ({op.role}): {side} damaged, first byte at offset {off} "
                                         f"relative to the payload ({op.nbytes} bytes)")
            for idx, want, ld in op.gaps:
                got = op.payload().view(_INT_VIEW[_esz(op.dtype)])[idx]
                if not torch.equal(got, want):
                    e = int(idx[torch.nonzero(got != want)[0]])
                    raise AssertionError(f"guard: operand '{op.label}' ({op.role}): row gap damaged, first byte at offset "
                                         f"{e * _esz(op.dtype)} relative to the payload (row {e // ld}, column {e % ld})")
