"""The bytes an msdi_attention_decoupled launch may touch, restated from the struct comment of include/minsdtf_hip_ipadapter.h (not
from the kernel), in the form of tests/_extents.py: {operand name: (bytes needed from the operand's base address, role)} from the
keyword arguments of ops.ip_attention with DIMENSIONS only.  Not a conftest: plain helpers, imported by name."""


def _rows(rows, ld, cols, esz):
    return ((rows - 1) * ld + cols) * esz


def ip_attention(**kw):
    """MsdiAttentionDecoupled: q / k / k_ip / out are rows of a wider buffer (head block only), vt / vt_ip whole rows of vt_ld /
    vtip_ld keys, scales the whole table, step_ptr one int32."""
    batch, heads, d_, s, t, n = kw["batch"], kw["heads"], kw["head_dim"], kw["s"], kw["t"], kw["n"]
    c = heads * d_
    d = {}
    for name, nbytes, role in (
            ("q", _rows(batch * s, kw["q_ld"], c, 2), "in"),               # bf16 [batch][s][q_ld]
            ("k", _rows(batch * t, kw["k_ld"], c, 2), "in"),               # bf16 [batch][t][k_ld]
            ("vt", batch * c * kw["vt_ld"] * 2, "in"),                     # bf16 [batch][heads * d][vt_ld]
            ("k_ip", _rows(batch * n, kw["kip_ld"], c, 2), "in"),          # bf16 [batch][n][kip_ld]
            ("vt_ip", batch * c * kw["vtip_ld"] * 2, "in"),                # bf16 [batch][heads * d][vtip_ld]
            ("scales", kw["num_steps"] * 16 * 4, "in"),                    # fp32 [num_steps][16]
            ("step_ptr", 4, "in"),                                         # one int32
            ("out", _rows(batch * s, kw["o_ld"], c, 2), "out")):           # bf16 [batch][s][o_ld]
        if kw.get(name) is not None:
            d[name] = (int(nbytes), role)
    return d


EXTENTS = {"ip_attention": ip_attention}
