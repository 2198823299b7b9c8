"""The bytes a launch of the vision library may touch, restated from the comments of include/minsdtf_hip_vision.h (not from the
kernels), in the form of tests/_extents.py: {operand name: (bytes needed from the operand's base address, role)} from the keyword
arguments of ops.patch_embed / ops.gelu / ops.pool_project with DIMENSIONS only.  Not a conftest: plain helpers, imported by name."""

IMAGE, TOKENS, WIDTH, PATCH_K, PROJ = 224, 257, 1280, 588, 1024


def _rows(rows, ld, cols, esz):
    return ((rows - 1) * ld + cols) * esz


def patch_embed(**kw):
    """MsdvPatchEmbed: whole pictures, w rows of w_ld of which 588 columns count, out rows of o_ld of which 1280 are written."""
    batch = kw["batch"]
    d = {}
    for name, nbytes, role in (
            ("pixels", batch * IMAGE * IMAGE * 3 * 4, "in"),                      # fp32 [batch][224][224][3]
            ("w", _rows(WIDTH, kw["w_ld"], PATCH_K, 2), "in"),                    # bf16 [1280][w_ld]
            ("cls", WIDTH * 4, "in"), ("pos", TOKENS * WIDTH * 4, "in"),          # fp32 [1280], [257][1280]
            ("gamma", WIDTH * 4, "in"), ("beta", WIDTH * 4, "in"),
            ("out", _rows(batch * TOKENS, kw.get("o_ld", WIDTH), WIDTH, 2), "out")):   # bf16 [batch][257][o_ld]
        if kw.get(name) is not None:
            d[name] = (int(nbytes), role)
    return d


def gelu(**kw):
    """msdv_gelu: x fp32 [rows][ld_in], out bf16 [rows][ld_out], cols of each row."""
    rows, cols = kw["rows"], kw["cols"]
    ld_in = cols if kw.get("ld_in") is None else kw["ld_in"]
    ld_out = cols if kw.get("ld_out") is None else kw["ld_out"]
    return {"x": (_rows(rows, ld_in, cols, 4), "in"), "out": (_rows(rows, ld_out, cols, 2), "out")}


def pool_project(**kw):
    """MsdvPoolProject: one row of 1280 per sample, x_stride elements apart; the whole matrix in either layout."""
    batch = kw["batch"]
    d = {}
    for name, nbytes, role in (
            ("x", _rows(batch, kw["x_stride"], WIDTH, 2), "in"),
            ("gamma", WIDTH * 4, "in"), ("beta", WIDTH * 4, "in"),
            ("w", PROJ * WIDTH * 2, "in"),
            ("out", batch * PROJ * 4, "out")):
        if kw.get(name) is not None:
            d[name] = (int(nbytes), role)
    return d


EXTENTS = {"patch_embed": patch_embed, "gelu": gelu, "pool_project": pool_project}
