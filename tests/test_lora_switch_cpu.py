"""LoRA switch at run time (minsdtf_amd/lora.py, csrc/lora.hip) without a GPU: the factors against the load-time dense deltas, the
merge plan against what packing.pack actually changes, the ffproj / lnb correction algebra, and the C ABI of msd_lora_merge."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def lora_file(tmp_path_factory):
    from make_goldens import lora_fixture
    from safetensors.torch import save_file

    p = str(tmp_path_factory.mktemp("lora") / "lora.safetensors")
    save_file(lora_fixture(), p)
    return p


def _pack_order(delta: np.ndarray) -> np.ndarray:
    """Checkpoint layout (out, in[, kh, kw]) -> [out][(ky, kx, c)]."""
    if delta.ndim == 4:
        return delta.transpose(0, 2, 3, 1).reshape(delta.shape[0], -1)
    return delta


def test_factors_reproduce_load_time_deltas(lora_file):
    from minsdtf_amd import lora
    from minsdtf_amd import weights as Wt

    te, un = Wt.load_weights_from_lora(lora_file)
    f = lora.read_factors(lora_file, "cpu")
    want = {k[: -len(".weight")]: v for k, v in list(un.items()) + list(te.items())}
    assert set(f) == set(want)
    assert len(un) == 278 and len(te) == 12
    kinds = set()
    for name, (up, down) in f.items():
        ref = _pack_order(np.asarray(want[name], np.float64))
        kinds.add(want[name].ndim if want[name].ndim == 2 else want[name].shape[2])
        got = up.double().numpy() @ down.double().numpy()
        np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max())
    assert kinds == {2, 1, 3}   # Linear, 1x1 and 3x3 entries all covered


def test_factors_from_state_dict_and_missing_file(tmp_path):
    from minsdtf_amd import lora

    with pytest.raises(FileNotFoundError):
        lora.read_factors(str(tmp_path / "nope.safetensors"), "cpu")
    sd = {"lora_unet_down_blocks_0_attentions_0_proj_in.lora_up.weight": torch.ones(320, 2, 1, 1),
          "lora_unet_down_blocks_0_attentions_0_proj_in.lora_down.weight": torch.ones(2, 320, 1, 1),
          "lora_unet_down_blocks_0_attentions_0_proj_in.alpha": torch.tensor(1.0),
          "lora_unet_no_alpha_here.lora_up.weight": torch.ones(4, 2)}
    f = lora.read_factors(sd, "cpu")
    assert list(f) == ["down_blocks.0.attentions.0.proj_in"]
    up, down = f["down_blocks.0.attentions.0.proj_in"]
    assert up.shape == (320, 2) and down.shape == (2, 320) and float(up[0, 0]) == 0.5


def _packed_cpu(model_cls, arrays):
    """packing.pack on the host (device = cpu): the packed image without a GPU, and the layout table it was packed by."""
    from minsdtf_amd import layout, packing
    from minsdtf_amd import weights as Wt

    specs = Wt.table(model_cls.kind, **({"clip_skip": -1} if model_cls.kind == "text_encoder" else {}))
    table = layout.layout(specs)
    named = {(s.name, s.kind): a for s, a in zip(specs, arrays)}
    return specs, table, packing.pack(table, named, torch.device("cpu"))[0]


def _plan_vs_pack(model_cls, seed):
    from minsdtf_amd import lora
    from minsdtf_amd import weights as Wt

    kw = {"clip_skip": -1} if model_cls.kind == "text_encoder" else {}
    base = Wt.synth_keras_weights(model_cls.kind, seed=seed, bias_scale=0.05, **kw)
    specs, table, W0 = _packed_cpu(model_cls, base)
    layers = lora.targetable(specs)
    rng = np.random.default_rng(seed)
    bumped = [a + (rng.standard_normal(a.shape).astype(np.float32) * 0.05 if s.name in layers and s.kind.endswith("_w") else 0)
              for s, a in zip(specs, base)]
    _, _, W1 = _packed_cpu(model_cls, bumped)
    changed = {k for k in W0 if not torch.equal(W0[k], W1[k])}
    plan = lora.Plan(specs, table)
    return changed, plan, layers


def test_plan_covers_exactly_what_pack_changes_text_encoder():
    from minsdtf_amd.models import TextEncoder

    changed, plan, layers = _plan_vs_pack(TextEncoder, 1)
    assert len(layers) == 72
    assert changed == plan.keys()
    assert {p.layer for t in plan.targets for p in t.parts} == set(layers)


def test_plan_covers_exactly_what_pack_changes_unet():
    from minsdtf_amd.models import DiffusionModel

    changed, plan, layers = _plan_vs_pack(DiffusionModel, 2)
    assert len(layers) == 278
    assert changed == plan.keys()
    srcs = set()
    for t in plan.targets:
        srcs |= t.sources
    assert srcs == set(layers)
    forms = {k.rsplit(".", 1)[-1] for k in plan.keys()} | {k.split(".")[-2] for k in plan.keys()}
    for f in ("qkv", "lnw", "lncs", "lnb", "kv", "ffproj", "conv2sc"):
        assert f in forms, f
    assert "time_emb_proj_cat.w" in plan.keys()


def test_ffproj_and_lnb_correction_algebra():
    """[N][K] form: Ap' A2' = Ap A2 + [Ap' U2 | Up] [D2 ; Dp A2]; b' = b + Up (Dp b2); lnb' = lnb + s U (D beta)."""
    from minsdtf_amd import lora

    rng = np.random.default_rng(5)
    C, r2, rp = 24, 3, 5
    A2, Ap = rng.standard_normal((C, 4 * C)), rng.standard_normal((C, C))
    U2, D2 = rng.standard_normal((C, r2)), rng.standard_normal((r2, 4 * C))
    Up, Dp = rng.standard_normal((C, rp)), rng.standard_normal((rp, C))
    b2, bp = rng.standard_normal(C), rng.standard_normal(C)
    mb = lora.MergeBase.__new__(lora.MergeBase)
    l2, lp = "x.transformer_blocks.0.ff.net.2", "x.proj_out"
    mb.master = {l2: torch.from_numpy(A2), lp: torch.from_numpy(Ap)}
    t = lambda a: torch.from_numpy(a)  # noqa: E731
    for fac in ({l2: (t(U2), t(D2)), lp: (t(Up), t(Dp))}, {l2: (t(U2), t(D2))}, {lp: (t(Up), t(Dp))}):
        U, D = mb._ffproj_factors(l2, lp, fac)
        A2n = A2 + (U2 @ D2 if l2 in fac else 0)
        Apn = Ap + (Up @ Dp if lp in fac else 0)
        np.testing.assert_allclose(Ap @ A2 + U.numpy() @ D.numpy(), Apn @ A2n, rtol=1e-10, atol=1e-10)
    # the fused bias: proj_out(ff W2 + b2) = ... + (Ap' b2 + bp)
    np.testing.assert_allclose((Ap @ b2 + bp) + Up @ (Dp @ b2), (Ap + Up @ Dp) @ b2 + bp, rtol=1e-12)
    # the LayerNorm fold's constant: ((W + U D) * s) beta = W s beta + s U (D beta)
    W, beta, s = rng.standard_normal((C, C)), rng.standard_normal(C), 0.37
    np.testing.assert_allclose((W * s) @ beta + s * (Up[:, :3] @ (Dp[:3] @ beta)), ((W + Up[:, :3] @ Dp[:3]) * s) @ beta, rtol=1e-12)


def test_lora_merge_struct_matches_header():
    from minsdtf_amd import _lib

    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "minsdtf_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
           'sizeof(MsdLoraJob), offsetof(MsdLoraJob, colsum), offsetof(MsdLoraJob, n), offsetof(MsdLoraJob, layout), '
           'offsetof(MsdLoraJob, first_block), sizeof(MsdLoraMerge), offsetof(MsdLoraMerge, num_jobs));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    J, M = _lib.MsdLoraJob, _lib.MsdLoraMerge
    assert got == [ctypes.sizeof(J), J.colsum.offset, J.n.offset, J.layout.offset, J.first_block.offset, ctypes.sizeof(M),
                   M.num_jobs.offset]
    assert _lib.ABI_VERSION == 12 and "msd_lora_merge" in _lib.SYMBOLS


def test_lora_merge_rejects_bad_arguments_without_a_gpu():
    from minsdtf_amd import _lib, ops

    lib = _lib.load()
    assert lib.msd_lora_merge(None, None) == -1

    def run(**kw):
        args = dict(master=256, out=256, n=16, k=64, out_rows=16, out_cols=64)
        args.update(kw)
        j = ops.lora_job(**args)
        arr = (_lib.MsdLoraJob * 1)(j)
        s = _lib.MsdLoraMerge()
        s.jobs, s.jobs_dev, s.num_jobs = ctypes.addressof(arr), 256, 1
        return lib.msd_lora_merge(ctypes.byref(s), None)

    assert run(rank=4) == -1                                  # rank without factors
    assert run(row_off=8) == -1                               # rows outside the destination
    assert run(col_off=8) == -1                               # columns outside the destination
    assert run(layout=ops.LORA_LAYOUT_CHUNK, out_cols=96, k=96) == -1
    assert run(out_frag=256, out_rows=24, n=24) == -1         # fragment-major needs N % 16 == 0
    assert run(colsum=256, k=32) == -1                        # colsum over part of a row
    assert run(rank=1000, up=256, down=256) == -1
    assert b"lora_merge" in lib.msd_last_error()
    s = _lib.MsdLoraMerge()
    s.num_jobs = 0
    assert lib.msd_lora_merge(ctypes.byref(s), None) == 0     # nothing to do


def test_set_loras_needs_the_switch():
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sd = StableDiffusion(64, 64, device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="lora_switch"):
        sd.set_loras([])
    assert sd.active_loras == ()
