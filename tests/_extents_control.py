"""The bytes the launch of the ControlNet units' combine may touch, restated from the struct comment of
include/minsdtf_hip_control.h (not from the kernel), in the form of tests/_extents.py: {operand name: (bytes needed from the operand's
base address, role)} from the keyword arguments of ops.control_combine with DIMENSIONS only.  The list operands are named
"skips.k" and "resid.n.k".  Not a conftest: plain helpers, imported by name."""


def control_combine(**kw):
    """MsdcControlCombine: skip[k] bf16 [rows][count[k]], in place; resid[n][k] fp32 [rows][count[k]], read only; scales fp32
    [num_steps][units][13][2]; step_ptr one int32, read only."""
    rows, counts, units = kw["rows"], kw["counts"], kw["units"]
    d = {}
    for k, n in enumerate(counts):
        d[f"skips.{k}"] = (rows * n * 2, "inout")
        for u in range(units):
            d[f"resid.{u}.{k}"] = (rows * n * 4, "in")
    d["scales"] = (kw["num_steps"] * units * 13 * 2 * 4, "in")
    if kw.get("step_ptr") is not None:
        d["step_ptr"] = (4, "in")
    return d


EXTENTS = {"control_combine": control_combine}
