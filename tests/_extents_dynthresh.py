"""The bytes the launch of a dynamic-thresholding step may touch, restated from the struct comment of
include/minsdtf_hip_dynthresh.h (not from the kernel), in the form of tests/_extents.py: {operand name: (bytes needed from the
operand's base address, role)} from the keyword arguments of ops.dynamic_threshold with DIMENSIONS only.  Not a conftest: plain
helpers, imported by name."""


def dynamic_threshold(**kw):
    """MsdtDynamicThreshold: eps fp32 [2 * batch][h * w * 4]; out fp32 [batch][h * w * 4] (eps itself, or apart from it); scales fp32
    [num_steps][2]; params 32 bytes; step_ptr one int32, read only."""
    batch, h, w = kw["batch"], kw["h"], kw["w"]
    n = h * w * 4
    d = {}
    for name, nbytes, role in (
            ("eps", 2 * batch * n * 4, "in"),
            ("out", batch * n * 4, "out"),
            ("scales", kw["num_steps"] * 2 * 4, "in"),
            ("params", 32, "in"),
            ("step_ptr", 4, "in")):
        if kw.get(name) is not None:
            d[name] = (int(nbytes), role)
    return d


EXTENTS = {"dynamic_threshold": dynamic_threshold}
# "out is eps itself (the u rows are overwritten in place) or lies apart from all of eps"
IN_PLACE = {"dynamic_threshold": {("eps", "out")}}
