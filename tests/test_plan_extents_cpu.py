"""The operand extents of include/minsdtf_hip.h (tests/_extents.py) over every launch the emitters record.

tests/_guard.py holds each kernel to its extents on operands the test allocates; this module holds the ENGINE to them: for every
Plan.rec call of the tensor-less walks (tests/_layer_walk.py walk_all: UNet, ControlNet, VAE decoder / encoder at the tuned sizes and
batches, untuned batches and an untuned size, the CLIP text transformer, a UNet with perturbed-attention rows, the HintNet, the UNet
fed by ControlNet taps) the launch must fit the Buf it was handed, the Buf must be live, operands may share bytes only where the
header allows a launch in place, and the plan's scratch (split-K workspace, GroupNorm statistics / partials / sync block) must
cover every launch that uses it.  Nothing is launched and finalize() is not called.

What the walk cannot see (not skipped silently - these have no size to compare with):
  - operands handed in from outside the plan, which the walk replaces by a size-less stand-in: every weight, bias and folded
    LayerNorm vector; the fp32 latent and eps buffers, the time-embedding table (conv_gemm's rowvec), the step counter, the
    image going into the VAE encoder / HintNet and coming out of the decoder;
  - launches recorded by the model classes around the emitters, which need real weights and a device to be constructed
    (minsdtf_amd/models.py: the fp32 <-> bf16 casts at the model boundary, msd_embedding_sum; minsdtf_amd/stable_diffusion.py:
    msd_cfg_step, msd_sampler_step, msd_region_combine, msd_tile_consensus, the context cast): tests/_extents.py has their
    formulas; the kernel tests hold the step kernels, casts and embedding_sum to them, nothing holds these plans;
  - the three-launch VAE attention (scores materialised: conv_gemm, softmax_rows, conv_gemm) and the add_f32_bf16 route of the
    ControlNet residuals are recorded only for geometries / model-boundary calls no walk here has."""
import numbers

import pytest

import _extents as X
import _layer_walk as LW
from minsdtf_amd import ops

# distinct ops over EXTENT_WALKS: an op the emitters start to record cannot stay unchecked unnoticed
EXPECTED_OPS = ("attention", "attention_identity", "conv_direct", "conv_gemm", "cross_attention_q", "group_norm", "layer_norm", "replicate")

_walks = {}


def _walk(w):
    if w not in _walks:
        _walks[w] = LW.walk_all(*w)
    return _walks[w]


def _dims(kw):
    """The keyword arguments of a recorded launch with every tensor / buffer replaced by True: dimensions only."""
    def one(v):
        if v is None or isinstance(v, (numbers.Number, str)):
            return v
        if isinstance(v, tuple):
            return tuple(one(x) for x in v)
        return True

    return {k: one(v) for k, v in kw.items() if k != "name"}


IDS = ["-".join(str(x) for x in w) for w in LW.EXTENT_WALKS]


@pytest.mark.parametrize("w", LW.EXTENT_WALKS, ids=IDS)
def test_every_recorded_launch_fits_its_buffers(w):
    recs, plan = _walk(w)
    assert recs
    ws_need = 0
    gn_launches = 0
    for r in recs:
        what = f"{'-'.join(map(str, w))} {r.op} '{r.name}'"
        assert r.op in X.EXTENTS, f"{what}: no extents for this op"
        ext = X.extents(r.op, **_dims(r.kw))
        seen = []
        for name, o in r.operands.items():
            assert name in ext, f"{what}: operand '{name}' has no extent"
            need, role = ext[name]
            if o.kind == "outside":      # a size-less stand-in (module docstring): nothing to compare with
                continue
            # (kinds "ws" / "gn_stats" / "gn_partials" / "gn_sync": plan scratch that finalize() sizes; no Buf exists yet, the
            #  "Scratch" assertions below hold them to ws_floats / gn_batch instead)
            if o.kind == "buf":
                # Fits / Live
                assert need <= o.avail, f"{what}: operand '{name}' needs {need} bytes, its buffer has {o.avail} from the operand's address"
                assert not o.freed, f"{what}: operand '{name}' lies in a buffer that was freed before the launch was recorded"
                seen.append((name, role, o.offset, o.offset + need))
        # Disjoint: byte ranges in the arena, in-place pairs as the header declares them
        for i, (na, ra, lo_a, hi_a) in enumerate(seen):
            for nb_, rb, lo_b, hi_b in seen[i + 1:]:
                if lo_a < hi_b and lo_b < hi_a:
                    assert X.may_share(r.op, na, nb_), f"{what}: operands '{na}' [{lo_a}, {hi_a}) and '{nb_}' [{lo_b}, {hi_b}) share bytes"
                    assert lo_a == lo_b, f"{what}: in-place operands '{na}' and '{nb_}' must be the same address"
        # Scratch
        if r.op == "conv_gemm" and r.kw.get("splitk", 1) > 1:
            assert r.operands["workspace"].kind == "ws"
            need = ext["workspace"][0]
            assert r.kw["workspace_floats"] * 4 == need, f"{what}: announces {r.kw['workspace_floats']} floats, the header asks for {need // 4}"
            ws_need = max(ws_need, need)
        if r.op == "conv_gemm" and r.kw.get("splitk", 1) <= 1:
            assert r.kw.get("workspace") is None and not r.kw.get("workspace_floats")
        if r.op == "group_norm":
            gn_launches += 1
            assert r.operands["stats"].kind == "gn_stats" and r.operands["partials"].kind == "gn_partials" and r.operands["sync"].kind == "gn_sync"
            assert r.kw["batch"] <= plan.gn_batch, f"{what}: batch {r.kw['batch']} > the {plan.gn_batch} samples the GroupNorm scratch is sized for"
            # finalize(): slots of gn_batch * 64 floats, gn_batch * MSD_GN_MAX_CHUNKS * 64 floats, gn_batch * MSD_GN_SYNC_WORDS_PER_SAMPLE words
            assert ext["stats"][0] <= plan.gn_batch * 64 * 4
            # the emitters leave partials_floats / sync_words to ops.group_norm, which announces batch * MSD_GN_MAX_CHUNKS * 64 floats and
            # batch * MSD_GN_SYNC_WORDS_PER_SAMPLE words for the LAUNCH's batch: what the library may use must fit the plan's buffer
            assert r.kw.get("partials_floats") is None and r.kw.get("sync_words") is None
            assert r.kw["batch"] * ops.GN_MAX_CHUNKS * 64 * 4 == ext["partials"][0]
            assert ext["partials"][0] <= plan.gn_batch * X.GN_MAX_CHUNKS * 64 * 4
            assert ext["sync"][0] <= plan.gn_batch * X.GN_SYNC_WORDS_PER_SAMPLE * 4
        if r.op == "attention" and r.kw["head_dim"] == 512 and r.kw.get("workspace") is not None:
            floats = X.attention_workspace_floats(r.kw["batch"], r.kw["heads"], r.kw["s"])
            assert r.kw["workspace_floats"] == floats, f"{what}: announces {r.kw['workspace_floats']} floats, the header asks for {floats}"
            assert -(-floats * 4 // 256) * 256 == r.operands["workspace"].avail, f"{what}: the workspace Buf is not the header's size (rounded to the arena's 256 bytes)"
    assert plan.ws_floats * 4 == ws_need, f"ws_floats {plan.ws_floats} against the largest split-K launch's {ws_need // 4}"
    assert plan.gn_slots == gn_launches


def test_every_recorded_op_has_extents():
    seen = set()
    for w in LW.EXTENT_WALKS:
        seen |= {r.op for r in _walk(w)[0]}
    assert seen <= set(X.EXTENTS), sorted(seen - set(X.EXTENTS))
    assert tuple(sorted(seen)) == EXPECTED_OPS


def test_the_walks_reach_the_special_launches():
    """What the extra walks are there for is really recorded: the d = 512 key-split workspace, the identity attention on a view
    behind msd_attention's rows, replicate in place, a zero conv with residual == out."""
    vae = _walk(("vae", 1, 64, 64))[0]
    assert any(r.op == "attention" and r.kw["head_dim"] == 512 and r.kw.get("workspace") is not None for r in vae)
    pag = _walk(("unet_pag", 3, 64, 64))[0]
    ident = [r for r in pag if r.op == "attention_identity"]
    assert len(ident) == 3 and all(r.kw["batch"] == 1 for r in ident)
    taps = _walk(("unet_taps", 2, 64, 64))[0]   # (the latent shared by the cond / uncond halves: the shared prefix is replicated)
    assert any(r.op == "replicate" and r.operands["src"].offset == r.operands["dst"].offset for r in taps)
    assert sum(1 for r in taps if r.op == "conv_gemm" and "residual" in r.operands and r.operands["residual"].offset == r.operands["out"].offset) == 13
