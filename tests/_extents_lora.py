"""The bytes one job of a msd_lora_merge launch may touch, restated from the comment of MsdLoraJob in include/minsdtf_hip.h (not
from the kernel), in the form of tests/_extents.py: {operand name: (bytes needed from the operand's base address, role)} from the
job's DIMENSIONS and from which optional operands are present.  Not a conftest: plain helpers, imported by name."""

LAYOUT_ROWS, LAYOUT_CHUNK, LAYOUT_T = 0, 1, 2
OUT_BYTES = {"bf16": 2, "f32": 4}


def out_elements(layout, out_rows, out_cols, ld=None):
    """rows: out[r * ld + c], the last row ends at its last column; chunk-major [out_cols / 64][out_rows][64] and the transposed
    rows out[c * out_rows + r] are dense."""
    if layout == LAYOUT_ROWS:
        return (out_rows - 1) * (out_cols if ld is None else ld) + out_cols
    return out_rows * out_cols


def lora_job(*, n, k, rank, out_rows, out_cols, layout=LAYOUT_ROWS, out_dtype="bf16", master_ld=None, ld=None, rowscale=None,
             colscale=None, rowmap=None, out_frag=None, colsum=None, **_):
    """master fp32 [n][master_ld] (the last row ends at column k), up fp32 [n][rank], down fp32 [rank][k], rowscale fp32 [n],
    colscale fp32 [k], rowmap int32 [n]; out in its layout, out_frag bf16 [out_cols / 64][out_rows / 16][2][4][16][8], colsum fp32
    [out_rows]."""
    master_ld = k if master_ld is None else master_ld
    d = {"master": (((n - 1) * master_ld + k) * 4, "in"),
         "out": (out_elements(layout, out_rows, out_cols, ld) * OUT_BYTES[out_dtype], "out")}
    if rank > 0:
        d["up"] = (n * rank * 4, "in")
        d["down"] = (rank * k * 4, "in")
    if rowscale is not None:
        d["rowscale"] = (n * 4, "in")
    if colscale is not None:
        d["colscale"] = (k * 4, "in")
    if rowmap is not None:
        d["rowmap"] = (n * 4, "in")
    if out_frag is not None:
        d["out_frag"] = (out_rows * out_cols * 2, "out")
    if colsum is not None:
        d["colsum"] = (out_rows * 4, "out")
    return d


EXTENTS = {"lora_job": lora_job}
