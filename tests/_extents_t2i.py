"""The bytes a launch of the T2I-Adapter library may touch, restated from the comments of include/minsdtf_hip_t2i.h (not from the
kernels), in the form of tests/_extents.py: {operand name: (bytes needed from the operand's base address, role)} from the keyword
arguments of ops.feature_add / unshuffle / relu / avgpool2 with DIMENSIONS only.  Not a conftest: plain helpers, imported by name."""

SITES = 4


def feature_add(**kw):
    """MsdaFeatureAdd: x bf16 [rows][n] in place, feats bf16 [n] each, scales fp32 [num_steps][units][4], step_ptr one int32."""
    units = len(kw["feats"])
    d = {"x": (kw["rows"] * kw["n"] * 2, "inout"), "scales": (kw["num_steps"] * units * SITES * 4, "in")}
    for u in range(units):
        d[f"feats.{u}"] = (kw["n"] * 2, "in")
    if kw.get("step_ptr") is not None:
        d["step_ptr"] = (4, "in")
    return d


def unshuffle(**kw):
    n = kw["batch"] * kw["h"] * kw["w"] * kw["cin"]
    return {"x": (n * 4, "in"), "out": (n * 2, "out")}


def relu(**kw):
    return {"x": (kw["n"] * 2, "inout")}


def avgpool2(**kw):
    n = kw["batch"] * kw["h"] * kw["w"] * kw["c"]
    return {"x": (n * 2, "in"), "out": (n // 4 * 2, "out")}


EXTENTS = {"feature_add": feature_add, "unshuffle": unshuffle, "relu": relu, "avgpool2": avgpool2}
