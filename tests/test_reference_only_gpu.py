"""msd_attention_joint and msd_reference_latent on the GPU: the kernels against the float64 reference between guard bands, the
bit-for-bit promises of the header (mix = NULL / 0 / 1, the reference segment not read at mix = 1, batch independence), and the
reference-only job through the pipeline (device loop against host loop, graph forms, residency, oracle fixtures, sharding)."""
import numpy as np
import pytest
import torch

import _extents_reference_only as XR
import _guard as G
from _checks import bf, close
from conftest import run_calls

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAN = float("nan")
LOG2E = 1.4426950408889634


def up8(n):
    return (n + 7) // 8 * 8


def guarded(dev, q, k, v, kr, vr, mix, *, H, d, wide=False, poison=True):
    """The operands of one launch between guard bands, sized by the header's extents: q [B, S, C] as rows of a q_ld-wide buffer,
    k / v [B, T, C] (v stored transposed, vt_ld >= max(T, T_ref) columns), kr / vr [T_ref, C] the one reference row with the SAME
    leading dimensions, mix [B] or None, out [B, S, C] as rows of o_ld.  The padding - V^T's columns past the segment, the wide
    buffers outside the head block - holds NaN (poison) or zeros; out's unused columns hold a canary.  Returns (guard, keyword
    arguments of ops.attention_joint, out)."""
    B, S, C = q.shape
    T, Tr = k.shape[1], kr.shape[0]
    assert C == H * d and kr.shape[1] == C
    q_ld, k_ld, o_ld = (3 * C, C + 24, C + 16) if wide else (C, C, C)
    vt_ld = up8(max(T, Tr)) + (8 if wide else 0)
    geo = dict(batch=B, heads=H, head_dim=d, s=S, t=T, t_ref=Tr, q_ld=q_ld, k_ld=k_ld, vt_ld=vt_ld, o_ld=o_ld)
    g = G.Guard(dev, XR.attention_joint(q=1, k=1, vt=1, k_ref=1, vt_ref=1, mix=1, out=1, **geo))
    pad = None if poison else 0.0
    qd = g.inp(q.to(BF16).reshape(B * S, C), "q", ld=q_ld if wide else None, gap=pad)
    kd = g.inp(k.to(BF16).reshape(B * T, C), "k", ld=k_ld if wide else None, gap=pad)
    vt = g.out((B, C, vt_ld), BF16, 0.0, "vt")
    vt[:, :, :T] = v.permute(0, 2, 1).to(BF16).to(dev)
    g.operands[-1].role = "in"
    g.gaps(vt, T, gap=pad)
    krd = g.inp(kr.to(BF16), "k_ref", ld=k_ld if wide else None, gap=pad)
    vtr = g.out((C, vt_ld), BF16, 0.0, "vt_ref")
    vtr[:, :Tr] = vr.t().to(BF16).to(dev)
    g.operands[-1].role = "in"
    g.gaps(vtr, Tr, gap=pad)
    md = None if mix is None else g.inp(torch.as_tensor(mix, dtype=torch.float32), "mix")
    out = g.out((B * S, C), BF16, NAN, "out", ld=o_ld if wide else None)
    return g, dict(q=qd, k=kd, vt=vt, k_ref=krd, vt_ref=vtr, mix=md, out=out, **geo), out


def launch(dev, q, k, v, kr, vr, mix, **kw):
    from minsdtf_amd import ops

    g, args, out = guarded(dev, q, k, v, kr, vr, mix, **kw)
    run_calls(ops.attention_joint(**args))
    g.check()
    B, S, C = q.shape
    return out.reshape(B, S, C).clone().cpu()


def operands(seed, B, H, d, S, T, Tr, ref_scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    C = H * d
    q = bf(torch.randn(B, S, C, generator=gen) * (d ** -0.5 * LOG2E))
    k, v = bf(torch.randn(B, T, C, generator=gen)), bf(torch.randn(B, T, C, generator=gen))
    kr, vr = bf(torch.randn(Tr, C, generator=gen) * ref_scale), bf(torch.randn(Tr, C, generator=gen))
    return q, k, v, kr, vr


def reference(q, k, v, kr, vr, mix, H):
    from minsdtf_amd import reference as R

    return torch.from_numpy(R.joint_attention_reference(q.numpy(), k.numpy(), v.numpy(), kr.numpy(), vr.numpy(), mix, H))


def bound(ref):
    """The project's attention bound (P rounded to bf16 before the PV product): rtol 2e-2, atol 1.5e-2 max(1, max|ref|)."""
    return dict(rtol=2e-2, atol=1.5e-2 * max(1.0, float(ref.abs().max())))


def bits(x):
    return x.view(torch.int16)


# (d, s, t, t_ref), heads
KERNEL_CASES = [
    ((40, 200, 200, 200), 2),    # partial tile in the middle of the walk
    ((80, 128, 128, 64), 2),
    ((160, 64, 64, 64), 2),
    ((160, 9, 9, 9), 3),
    ((40, 70, 70, 130), 3),
    ((40, 576, 576, 576), 2),    # nine tiles per segment
    ((40, 1, 1, 1), 2),          # the 64 px job's innermost level
]
MIXES = [[0.0, 0.5], [1.0, 0.25]]


@pytest.mark.parametrize("mix", MIXES, ids=["mix0-.5", "mix1-.25"])
@pytest.mark.parametrize("case,H", KERNEL_CASES, ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else f"H{c}")
def test_kernel_against_reference(gpu, case, H, mix):
    """Every leading dimension wider than its payload; the padding holds NaN, then zeros: the same bits."""
    d, S, T, Tr = case
    q, k, v, kr, vr = operands(11, 2, H, d, S, T, Tr)
    ref = reference(q, k, v, kr, vr, mix, H)
    a = launch(gpu, q, k, v, kr, vr, mix, H=H, d=d, wide=True, poison=True)
    b = launch(gpu, q, k, v, kr, vr, mix, H=H, d=d, wide=True, poison=False)
    close(a, ref.float(), what=f"{case} mix {mix}", **bound(ref))
    assert torch.equal(bits(a), bits(b)), f"{case}: the content of a padding region reached the result"


@pytest.mark.parametrize("scale", [4.0, 0.25])
@pytest.mark.parametrize("case,H", [((40, 200, 200, 200), 2), ((160, 64, 64, 64), 2)], ids=["d40", "d160"])
def test_plain_share_does_not_move_with_the_reference_keys(gpu, case, H, scale):
    """Reference keys scaled x4: the running maximum rises after the segment boundary and the joint result leaves the plain one
    far behind; x0.25: it never rises.  The blend still carries the own segment's plain attention: the reference at mix 0.5 / 0.75
    within the bound, and the mix = 1 sample's bits are those of a launch with unscaled reference keys."""
    d, S, T, Tr = case
    q, k, v, kr, vr = operands(12, 2, H, d, S, T, Tr, ref_scale=scale)
    for mix in ([0.5, 0.75], [1.0, 0.5]):
        ref = reference(q, k, v, kr, vr, mix, H)
        got = launch(gpu, q, k, v, kr, vr, mix, H=H, d=d)
        close(got, ref.float(), what=f"{case} x{scale} mix {mix}", **bound(ref))
    base = launch(gpu, q, k, v, bf(kr / scale), vr, [1.0, 0.5], H=H, d=d)
    assert torch.equal(bits(got[0]), bits(base[0]))
    assert not torch.equal(bits(got[1]), bits(base[1]))


def test_null_mix_is_mix_zero(gpu):
    d, S, T, Tr, H = 80, 100, 100, 70, 2
    q, k, v, kr, vr = operands(3, 2, H, d, S, T, Tr)
    a = launch(gpu, q, k, v, kr, vr, None, H=H, d=d)
    b = launch(gpu, q, k, v, kr, vr, [0.0, 0.0], H=H, d=d)
    assert torch.equal(bits(a), bits(b))


def test_mix_one_does_not_read_the_reference(gpu):
    d, S, T, Tr, H = 40, 150, 150, 150, 2
    q, k, v, kr, vr = operands(4, 2, H, d, S, T, Tr)
    a = launch(gpu, q, k, v, kr, vr, [1.0, 1.0], H=H, d=d)
    nan_k, nan_v = torch.full_like(kr, NAN), torch.full_like(vr, NAN)
    b = launch(gpu, q, k, v, nan_k, nan_v, [1.0, 1.0], H=H, d=d)
    assert bool(torch.isfinite(b.float()).all())
    assert torch.equal(bits(a), bits(b))


def _msd_attention(gpu, q, k, v, H, d):
    from minsdtf_amd import ops

    B, S, C = q.shape
    T = k.shape[1]
    Tp = up8(T)
    qd, kd = q.to(BF16).to(gpu), k.to(BF16).to(gpu)
    vt = torch.zeros(B, C, Tp, dtype=BF16, device=gpu)
    vt[:, :, :T] = v.permute(0, 2, 1).to(BF16).to(gpu)
    out = torch.empty(B, S, C, dtype=BF16, device=gpu)
    run_calls(ops.attention(q=qd, k=kd, vt=vt, out=out, batch=B, heads=H, head_dim=d, s=S, t=T, q_ld=C, k_ld=C, vt_ld=Tp, o_ld=C,
                            scale=1.0, q_prescaled=True))
    return out.float().cpu()


@pytest.mark.parametrize("d,S", [(40, 200), (80, 128), (160, 64)])
def test_duplicated_keys_against_msd_attention(gpu, d, S):
    """k_ref = k, vt_ref = vt (batch 1, mix 0): duplicated keys leave the softmax average unchanged, so this is the row's plain
    self-attention - within the attention bound of msd_attention on the own keys."""
    H = 2
    q, k, v, _, _ = operands(8, 1, H, d, S, S, S)
    got = launch(gpu, q, k, v, k[0], v[0], [0.0], H=H, d=d)
    ref = _msd_attention(gpu, q, k, v, H, d)
    close(got, ref, what=f"d={d}", **bound(ref))


@pytest.mark.parametrize("d,S,Tr", [(40, 200, 130), (160, 64, 64)])
def test_mix_zero_against_msd_attention_on_concatenated_keys(gpu, d, S, Tr):
    H, B = 2, 2
    q, k, v, kr, vr = operands(9, B, H, d, S, S, Tr)
    got = launch(gpu, q, k, v, kr, vr, None, H=H, d=d)
    kc = torch.cat([k, kr[None].expand(B, -1, -1)], 1)
    vc = torch.cat([v, vr[None].expand(B, -1, -1)], 1)
    ref = _msd_attention(gpu, q, kc, vc, H, d)
    close(got, ref, what=f"d={d}", **bound(ref))


def test_sample_bits_do_not_depend_on_the_batch_and_runs_repeat(gpu):
    B, H, d, S, T, Tr = 3, 2, 160, 100, 100, 50
    q, k, v, kr, vr = operands(6, B, H, d, S, T, Tr)
    mix = [0.0, 0.5, 1.0]
    full = launch(gpu, q, k, v, kr, vr, mix, H=H, d=d)
    again = launch(gpu, q, k, v, kr, vr, mix, H=H, d=d)
    assert torch.equal(bits(full), bits(again))
    for b in range(B):
        alone = launch(gpu, q[b:b + 1], k[b:b + 1], v[b:b + 1], kr, vr, mix[b:b + 1], H=H, d=d)
        assert torch.equal(bits(alone[0]), bits(full[b])), f"sample {b}"


def test_reference_latent_against_numpy(gpu):
    """out = fma(b, noise, a * z) in fp32, bit for bit, at two step indices (and a step past the table is clamped to its last row)."""
    from minsdtf_amd import ops
    from minsdtf_amd import reference as R

    rng = np.random.default_rng(5)
    n, steps = 9 * 7 * 4, 5
    z, noise = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    coef = rng.random((steps, 2)).astype(np.float32)
    for step, row in ((0, 0), (3, 3), (9, steps - 1)):
        g = G.Guard(gpu, XR.reference_latent(z=1, noise=1, coef=1, step_ptr=1, out=1, n=n, num_steps=steps))
        zd, nd = g.inp(torch.from_numpy(z), "z"), g.inp(torch.from_numpy(noise), "noise")
        cd = g.inp(torch.from_numpy(coef), "coef")
        sp = g.inp(torch.tensor([step], dtype=torch.int32), "step_ptr")
        out = g.out((n,), torch.float32, NAN, "out")
        run_calls(ops.reference_latent(z=zd, noise=nd, coef=cd, step_ptr=sp, out=out, n=n, num_steps=steps))
        g.check()
        want = R.reference_latent_host(z, noise, coef[row])
        assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32)), f"step {step}"


# ---------------------------------------------------------------------------------------------------------------- pipelines
PSNR_MIN = 40.0        # the project's bar for every job
SAMPLER_PSNR_MIN = 45.0   # ... for a samplers.py sampler's txt2img job against another route (test_samplers_gpu.py)
MID_UP1 = ["mid", "up_blocks.1.attentions.0", "up_blocks.1.attentions.1", "up_blocks.1.attentions.2"]


@pytest.fixture(scope="module")
def nets(gpu):
    from minsdtf_amd.models import DiffusionModel, ImageDecoder

    unet = DiffusionModel(64, 64, device=gpu)
    unet.load_synthetic(seed=0, bias_scale=0.05)
    dec = ImageDecoder(device=gpu)
    dec.load_synthetic(seed=0, bias_scale=0.05)
    return {"unet": unet, "dec": dec}


def _pipe(gpu, nets, jit=True):
    """(pipeline, two contexts P, Q)"""
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sd = StableDiffusion(64, 64, jit_compile=jit, device=gpu)
    sd._diffusion_model = nets["unet"]
    sd._image_decoder = nets["dec"]
    rng = np.random.default_rng(41)
    sd.unconditional_context = rng.standard_normal((77, 768)).astype(np.float32)
    return sd, [rng.standard_normal((77, 768)).astype(np.float32) for _ in range(2)]


def _z(seed=77, scale=1.0, hw=8):
    return (scale * np.random.default_rng(seed).standard_normal((1, hw, hw, 4))).astype(np.float32)


def _names(eng):
    return [c.name for c in eng.calls]


@pytest.mark.parametrize("fidelity, sampler", [(0.0, None), (0.5, None), (1.0, None), (0.5, "dpmpp_2m")])
def test_device_loop_vs_host_loop(gpu, nets, fidelity, sampler):
    """The device loop against host_loop=True (DiffusionModel.predict_reference through _guided_eps: one forward for the u rows
    with mix = fidelity, one for the c rows with mix = 0): 40 dB, or 45 dB with a samplers.py sampler."""
    from oracle import sd_oracle as O

    sd, (P, _Q) = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=4, seed=11, return_latent=True, sampler=sampler, guidance_rescale=0.7,
              reference_only=dict(latent=_z(), fidelity=fidelity, layers=MID_UP1 + ["down_blocks.0.attentions.1"]))
    calls_d, calls_h = [], []
    dev = sd.generate_image(P, callback=calls_d.append, **kw)
    eng = next(iter(sd._engines.values()))
    assert eng.passes == [(0, 5, 77, "both")] and eng.eps.shape[0] == 5 and eng.ctx_in["both"].shape[0] == 5
    names = _names(eng)
    assert names[0] == "reference_latent" and names[1:3] == ["conv_in", "conv_in.reference"]
    assert sum(n.endswith(".attn1.joint") for n in names) == 5 and not any(n.endswith(".replicate") for n in names)
    host = sd.generate_image(P, host_loop=True, callback=calls_h.append, **kw)
    assert calls_d == calls_h == [1, 2, 3, 4]
    p = O.psnr(dev, host)
    bar = SAMPLER_PSNR_MIN if sampler else PSNR_MIN
    print(f"reference-only job, fidelity {fidelity} ({sampler or 'default sampler'}): device loop vs host loop {p:.1f} dB (bar {bar:.0f})")
    assert p >= bar
    assert not np.array_equal(dev, sd.generate_image(P, **{k: v for k, v in kw.items() if k != "reference_only"}))


def test_predict_reference_with_mix_one_is_predict_on_batch(gpu, nets):
    """mix = 1 everywhere: every generated row takes its plain self-attention (on msd_attention_joint's own segment), whatever
    the reference row holds: 40 dB on the prediction against predict_on_batch."""
    from minsdtf_amd import engine
    from oracle import sd_oracle as O

    unet = nets["unet"]
    rng = np.random.default_rng(2)
    lat = rng.standard_normal((2, 8, 8, 4)).astype(np.float32)
    temb = O.timestep_embedding(500, 2)
    ctx = rng.standard_normal((2, 77, 768)).astype(np.float32)
    ref = unet.predict_on_batch([lat, temb, ctx])
    got = unet.predict_reference([lat, temb, ctx], 3.0 * _z(5), engine.PAG_LAYERS, 1.0)
    assert got.shape == ref.shape
    p = O.psnr(got, ref)
    print(f"predict_reference, mix 1, all layers vs predict_on_batch: {p:.1f} dB")
    assert p >= PSNR_MIN
    moved = unet.predict_reference([lat, temb, ctx], 3.0 * _z(5), engine.PAG_LAYERS, [0.0, 1.0])
    assert O.psnr(moved[1], ref[1]) >= PSNR_MIN and not np.array_equal(moved[0], got[0])
    with pytest.raises(ValueError):
        unet.predict_reference([lat, temb, ctx], _z(5), ["mid"], 1.0)
    with pytest.raises(ValueError):
        unet.predict_reference([lat, temb, ctx], _z(5)[0], engine.PAG_LAYERS, 1.0)
    with pytest.raises(ValueError):
        unet.predict_reference([lat, temb, ctx], _z(5), engine.PAG_LAYERS, 1.5)


def test_image_and_its_encoded_latent_give_the_same_bits(gpu, nets):
    from minsdtf_amd.models import ImageEncoder

    enc = ImageEncoder(device=gpu)
    enc.load_synthetic(seed=0, bias_scale=0.05)
    sd, (P, _Q) = _pipe(gpu, nets)
    sd._image_encoder = enc
    image = np.random.default_rng(9).integers(0, 256, (64, 64, 3)).astype(np.uint8)
    z = enc.predict_on_batch(sd.preprocessed_image(image)[1])
    assert z.shape == (1, 8, 8, 4)
    kw = dict(batch_size=1, num_steps=3, seed=4, return_latent=True, guidance_rescale=0.7)
    a = sd.generate_image(P, reference_only=dict(image=image, layers="mid"), **kw)
    b = sd.generate_image(P, reference_only=dict(latent=z, layers="mid"), **kw)
    np.testing.assert_array_equal(a, b)
    assert np.all(np.isfinite(a)) and len(sd._engines) == 1


def test_graph_forms_agree(gpu, nets):
    """The whole-loop graph == per-step graphs (a callback is installed) == eager launches (jit_compile=False), bit for bit."""
    sd, (P, _Q) = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=3, seed=8, return_latent=True, sampler="dpmpp_2m", guidance_rescale=0.7,
              reference_only=dict(latent=_z(), fidelity=0.5))
    whole = sd.generate_image(P, **kw)
    calls = []
    stepped = sd.generate_image(P, callback=calls.append, **kw)
    assert calls == [1, 2, 3]
    eng = next(iter(sd._engines.values()))
    assert eng._loop_graph is not None and eng._step_graph is not None and len(eng.reference) == 16
    eager_sd, _ = _pipe(gpu, nets, jit=False)
    np.testing.assert_array_equal(stepped, whole)
    np.testing.assert_array_equal(eager_sd.generate_image(P, **kw), whole)
    assert np.all(np.isfinite(whole))


def test_residency(gpu, nets, monkeypatch):
    """Another latent, draw and fidelity with the same layers build no engine and capture no graph."""
    import minsdtf_amd.stable_diffusion as sdm

    built = []
    init = sdm.DenoiseEngine.__init__

    def counting(self, *a, **k):
        built.append((a[1], k.get("reference")))
        init(self, *a, **k)

    monkeypatch.setattr(sdm.DenoiseEngine, "__init__", counting)
    sd, (P, _Q) = _pipe(gpu, nets)
    kw = dict(batch_size=1, num_steps=3, seed=5, guidance_rescale=0.7, return_latent=True)
    first = sd.generate_image(P, reference_only=dict(latent=_z(1), layers="mid", fidelity=0.5), **kw)
    assert built == [(1, ("mid_block.attentions.0",))]
    eng = next(iter(sd._engines.values()))
    graph = eng._loop_graph
    other = dict(latent=_z(2, 2.0), layers="mid", fidelity=0.9, noise=_z(3))
    second = sd.generate_image(P, reference_only=other, **kw)
    assert len(built) == 1 and next(iter(sd._engines.values())) is eng and eng._loop_graph is graph
    assert not np.array_equal(first, second)
    # the default draw is default_rng([seed, 3])
    drawn = dict(other, noise=np.random.default_rng([5, 3]).standard_normal((1, 8, 8, 4)).astype(np.float32))
    np.testing.assert_array_equal(sd.generate_image(P, reference_only=dict(other, noise=None), **kw), sd.generate_image(P, reference_only=drawn, **kw))
    assert len(built) == 1 and eng._loop_graph is graph
    # a pipeline that never saw the first job gives the second job's bits (it builds its own engine)
    fresh, _ = _pipe(gpu, nets)
    np.testing.assert_array_equal(second, fresh.generate_image(P, reference_only=other, **kw))
    assert len(built) == 2
    # other layers are another engine
    sd.generate_image(P, reference_only=dict(other, layers=MID_UP1), **kw)
    assert len(built) == 3 and len(built[-1][1]) == 4


def test_guidance_zero_job_runs(gpu, nets):
    sd, (P, _Q) = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=3, seed=2, unconditional_guidance_scale=0.0, return_latent=True)
    got = sd.generate_image(P, reference_only=dict(latent=_z()), **kw)
    eng = next(iter(sd._engines.values()))
    assert eng.passes == [(0, 3, 77, "cond")] and eng.eps.shape[0] == 3 and eng.ref_mix.shape[0] == 2
    assert np.all(np.isfinite(got)) and not np.array_equal(got, sd.generate_image(P, **kw))
    with pytest.raises(ValueError, match="token length"):
        sd.generate_image(P, negative_prompt=np.zeros((154, 768), np.float32), batch_size=1, num_steps=2, seed=0,
                          reference_only=dict(latent=_z()))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_against_the_oracle_fixture(gpu, nets, tag):
    """tests/golden/oracle_reference_only_{a,b}.npz (tools/make_reference_only_fixtures.py): final latent PSNR >= 40 dB on the
    whole batch and on each sample; the fixture's plain job is below 30 dB, so the bar tells the feature from its absence."""
    import os

    from minsdtf_amd.models import DiffusionModel
    from minsdtf_amd.stable_diffusion import StableDiffusion
    from oracle import sd_oracle as O

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"oracle_reference_only_{tag}.npz"))
    assert (int(g["weight_seed"]), float(g["bias_scale"])) == (0, 0.05) and float(g["plain_psnr"]) < 30.0
    size, B = int(g["size"]), int(g["batch"])
    if size == 64:
        unet = nets["unet"]
    else:
        unet = DiffusionModel(size, size, device=gpu)
        unet.load_synthetic(seed=0, bias_scale=0.05)
    sd = StableDiffusion(size, size, jit_compile=True, device=gpu)
    sd._diffusion_model, sd._image_decoder = unet, nets["dec"]
    rng = np.random.default_rng(int(g["context_seed"]))
    base = rng.standard_normal((1, 77, 768)).astype(np.float32)[0]
    sd.unconditional_context = rng.standard_normal((1, 77, 768)).astype(np.float32)[0]
    hw = size // 8
    z_ref = (float(g["reference_scale"]) * np.random.default_rng(int(g["reference_seed"])).standard_normal((1, hw, hw, 4))).astype(np.float32)
    n_ref = np.random.default_rng(int(g["reference_noise_seed"])).standard_normal((1, hw, hw, 4)).astype(np.float32)
    job = dict(latent=z_ref, noise=n_ref, fidelity=float(g["fidelity"]), layers=[str(n) for n in g["layers"]])
    got = sd.generate_image(base, batch_size=B, num_steps=int(g["steps"]), unconditional_guidance_scale=float(g["guidance"]),
                            seed=int(g["noise_seed"]), guidance_rescale=float(g["guidance_rescale"]), return_latent=True,
                            sampler=str(g["sampler"]) or None, reference_only=job)
    eng = next(iter(sd._engines.values()))
    assert eng.reference == frozenset(job["layers"]) and eng.eps.shape[0] == 2 * B + 1
    p = O.psnr(got, g["latent"])
    per = [round(O.psnr(got[b], g["latent"][b]), 1) for b in range(B)]
    print(f"reference-only job {tag}: final latent PSNR {p:.1f} dB (per sample {per}); the plain job is at {float(g['plain_psnr']):.1f} dB")
    assert p >= PSNR_MIN and min(per) >= PSNR_MIN


def test_sharded_job_equals_unsharded(gpu):
    """A one-rank process group with forced collectives (as tests/test_regions_gpu.py): the sharded reference-only job == the
    unsharded one.  (A child process is what the test is about: the group must exist before anything touches the GPU.)"""
    import os
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(here, "_reference_only_world1_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=570)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert any(line.startswith("OK ") for line in p.stdout.splitlines()), p.stdout[-2000:]
    print(p.stdout.strip().splitlines()[-1])
