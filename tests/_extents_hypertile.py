"""The bytes an msd_attention_windowed launch may touch, restated from the struct comment of include/minsdtf_hip.h (not from the
kernel), in the form of tests/_extents.py: {operand name: (bytes needed from the operand's base address, role)} from the keyword
arguments of ops.attention_windowed with DIMENSIONS only.  Not a conftest: plain helpers, imported by name."""


def _rows(rows, ld, cols, esz):
    return ((rows - 1) * ld + cols) * esz


def attention_windowed(**kw):
    """MsdAttentionWindowed: q / k / out are the s = h * w rows per sample of a wider buffer (head block only), vt whole rows of
    vt_ld keys.  The windows change which rows meet, never which rows exist."""
    batch, heads, d_, s = kw["batch"], kw["heads"], kw["head_dim"], kw["h"] * kw["w"]
    c = heads * d_
    d = {}
    for name, nbytes, role in (
            ("q", _rows(batch * s, kw["q_ld"], c, 2), "in"),          # bf16 [batch][s][q_ld]
            ("k", _rows(batch * s, kw["k_ld"], c, 2), "in"),          # bf16 [batch][s][k_ld]
            ("vt", batch * c * kw["vt_ld"] * 2, "in"),                # bf16 [batch][heads * d][vt_ld]
            ("out", _rows(batch * s, kw["o_ld"], c, 2), "out")):      # bf16 [batch][s][o_ld]
        if kw.get(name) is not None:
            d[name] = (int(nbytes), role)
    return d


EXTENTS = {"attention_windowed": attention_windowed}
