"""The bytes a launch of the resampler library may touch, restated from the comments of include/minsdtf_hip_resampler.h (not from the
kernel), in the form of tests/_extents.py: {operand name: (bytes needed from the operand's base address, role)} from the keyword
arguments of ops.perceiver_attention with DIMENSIONS only.  Not a conftest: plain helpers, imported by name."""

HEAD_DIM = 64


def _rows(rows, ld, cols, esz):
    return ((rows - 1) * ld + cols) * esz


def perceiver_attention(**kw):
    """MsdrPerceiverAttention: q / k_x / k_l / out are rows of a wider buffer (heads * 64 columns of each), vt_x / vt_l whole rows
    of vtx_ld / vtl_ld keys (the header gives them as [batch][heads * 64][ld]: the padding columns belong to the operand)."""
    batch, n, t_x = kw["batch"], kw["n"], kw["t_x"]
    c = kw["heads"] * HEAD_DIM
    d = {}
    for name, nbytes, role in (
            ("q", _rows(batch * n, kw["q_ld"], c, 2), "in"),
            ("k_x", _rows(batch * t_x, kw["kx_ld"], c, 2), "in"),
            ("vt_x", batch * c * kw["vtx_ld"] * 2, "in"),
            ("k_l", _rows(batch * n, kw["kl_ld"], c, 2), "in"),
            ("vt_l", batch * c * kw["vtl_ld"] * 2, "in"),
            ("out", _rows(batch * n, kw["o_ld"], c, 2), "out")):
        if kw.get(name) is not None:
            d[name] = (int(nbytes), role)
    return d


EXTENTS = {"perceiver_attention": perceiver_attention}
