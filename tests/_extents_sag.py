"""The bytes the launches of a self-attention-guidance step may touch, restated from the struct comments of
include/minsdtf_hip_ext.h (not from the kernels), in the form of tests/_extents.py: {operand name: (bytes needed from the operand's
base address, role)} from the keyword arguments of ops.attention_colsum / ops.sag_degrade with DIMENSIONS only.  Not a conftest:
plain helpers, imported by name."""


def _rows(rows, ld, cols, esz):
    return ((rows - 1) * ld + cols) * esz


def attention_colsum(**kw):
    """MsdxAttentionColsum: q / k are the s rows per sample of a wider buffer (head block only); out fp32 [batch][s]; workspace
    fp32 [batch][heads][s][2]."""
    batch, heads, d_, s = kw["batch"], kw["heads"], kw["head_dim"], kw["s"]
    c = heads * d_
    d = {}
    for name, nbytes, role in (
            ("q", _rows(batch * s, kw["q_ld"], c, 2), "in"),          # bf16 [batch][s][q_ld]
            ("k", _rows(batch * s, kw["k_ld"], c, 2), "in"),          # bf16 [batch][s][k_ld]
            ("out", batch * s * 4, "out"),                            # fp32 [batch][s]
            ("workspace", batch * heads * s * 2 * 4, "out")):         # fp32 [batch][heads][s][2]
        if kw.get(name) is not None:
            d[name] = (int(nbytes), role)
    return d


def sag_degrade(**kw):
    """MsdxSagDegrade: latent / eps / out fp32 [batch][h][w][4]; coef fp32 [num_steps][coef_stride] of which columns 0, 1 are read;
    colsum fp32 [batch][mh * mw]; params fp32 [10]; step_ptr one int32."""
    batch, h, w = kw["batch"], kw["h"], kw["w"]
    n = batch * h * w * 4 * 4
    d = {}
    for name, nbytes, role in (
            ("latent", n, "in"), ("eps", n, "in"), ("out", n, "out"),
            ("coef", ((kw["num_steps"] - 1) * kw["coef_stride"] + 2) * 4, "in"),
            ("colsum", batch * kw["mh"] * kw["mw"] * 4, "in"),
            ("params", 10 * 4, "in"),
            ("step_ptr", 4, "in")):
        if kw.get(name) is not None:
            d[name] = (int(nbytes), role)
    return d


EXTENTS = {"attention_colsum": attention_colsum, "sag_degrade": sag_degrade}
