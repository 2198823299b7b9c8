"""The bytes an msd_region_attention launch may touch, restated from the struct comment of include/minsdtf_hip.h (not from the
kernel), in the form of tests/_extents.py: {operand name: (bytes needed from the operand's base address, role)} from the keyword
arguments of ops.region_attention with DIMENSIONS only.  Not a conftest: plain helpers, imported by name."""


def _rows(rows, ld, cols, esz):
    return ((rows - 1) * ld + cols) * esz


def region_attention(**kw):
    """MsdRegionAttention: q / k / out are rows of a wider buffer (head block only), vt whole rows of vt_ld keys, w rows of w_ld
    weights carrying s each."""
    batch, heads, d_, s, t, regions = kw["batch"], kw["heads"], kw["head_dim"], kw["s"], kw["t"], kw["regions"]
    c = heads * d_
    d = {}
    for name, nbytes, role in (
            ("q", _rows(batch * s, kw["q_ld"], c, 2), "in"),                 # bf16 [batch][s][q_ld]
            ("k", _rows(regions * batch * t, kw["k_ld"], c, 2), "in"),       # bf16 [regions * batch][t][k_ld]
            ("vt", regions * batch * c * kw["vt_ld"] * 2, "in"),             # bf16 [regions * batch][heads * d][vt_ld]
            ("w", _rows(regions, kw["w_ld"], s, 4), "in"),                   # fp32 [regions][w_ld]
            ("out", _rows(batch * s, kw["o_ld"], c, 2), "out")):             # bf16 [batch][s][o_ld]
        if kw.get(name) is not None:
            d[name] = (int(nbytes), role)
    return d


EXTENTS = {"region_attention": region_attention}
