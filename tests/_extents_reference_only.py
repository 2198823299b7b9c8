"""The bytes an msd_attention_joint / msd_reference_latent launch may touch, restated from the struct comments of
include/minsdtf_hip.h (not from the kernels), in the form of tests/_extents.py: {operand name: (bytes needed from the operand's
base address, role)} from the keyword arguments of ops.attention_joint / ops.reference_latent with DIMENSIONS only.  Not a
conftest: plain helpers, imported by name."""


def _rows(rows, ld, cols, esz):
    return ((rows - 1) * ld + cols) * esz


def attention_joint(**kw):
    """MsdAttentionJoint: q / k / k_ref / out are rows of a wider buffer (head block only), vt / vt_ref whole rows of vt_ld keys,
    mix one float per sample."""
    batch, heads, d_, s, t, t_ref = kw["batch"], kw["heads"], kw["head_dim"], kw["s"], kw["t"], kw["t_ref"]
    c = heads * d_
    d = {}
    for name, nbytes, role in (
            ("q", _rows(batch * s, kw["q_ld"], c, 2), "in"),          # bf16 [batch][s][q_ld]
            ("k", _rows(batch * t, kw["k_ld"], c, 2), "in"),          # bf16 [batch][t][k_ld]
            ("vt", batch * c * kw["vt_ld"] * 2, "in"),                # bf16 [batch][heads * d][vt_ld]
            ("k_ref", _rows(t_ref, kw["k_ld"], c, 2), "in"),          # bf16 [t_ref][k_ld]
            ("vt_ref", c * kw["vt_ld"] * 2, "in"),                    # bf16 [heads * d][vt_ld]
            ("mix", batch * 4, "in"),                                 # fp32 [batch]
            ("out", _rows(batch * s, kw["o_ld"], c, 2), "out")):      # bf16 [batch][s][o_ld]
        if kw.get(name) is not None:
            d[name] = (int(nbytes), role)
    return d


def reference_latent(**kw):
    """MsdReferenceLatent: z / noise / out fp32 [n], coef fp32 [num_steps][2], step_ptr one int32."""
    n, steps = kw["n"], kw["num_steps"]
    d = {}
    for name, nbytes, role in (("z", n * 4, "in"), ("noise", n * 4, "in"), ("coef", steps * 2 * 4, "in"), ("step_ptr", 4, "in"),
                               ("out", n * 4, "out")):
        if kw.get(name) is not None:
            d[name] = (int(nbytes), role)
    return d


EXTENTS = {"attention_joint": attention_joint, "reference_latent": reference_latent}
