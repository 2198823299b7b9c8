"""The bytes an msd_reference_adain launch may touch, restated from the struct comment of include/minsdtf_hip.h (not from the
kernel), in the form of tests/_extents.py: {operand name: (bytes needed from the operand's base address, role)} from the keyword
arguments of ops.reference_adain with DIMENSIONS only.  Not a conftest: plain helpers, imported by name."""


def reference_adain(**kw):
    """MsdReferenceAdain: x bf16 [rows][hw][c] rewritten in place, ref bf16 [hw][c] read only, mix one float per row."""
    rows, hw, c = kw["rows"], kw["hw"], kw["c"]
    d = {}
    for name, nbytes, role in (("x", rows * hw * c * 2, "inout"), ("ref", hw * c * 2, "in"), ("mix", rows * 4, "in")):
        if kw.get(name) is not None:
            d[name] = (int(nbytes), role)
    return d


EXTENTS = {"reference_adain": reference_adain}
