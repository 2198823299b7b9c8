"""The IP-Adapter "plus" Resampler on the device: msdr_perceiver_attention between guard bands against float64, synthetic resamplers
against resampler.forward_host, and an ip_adapter job that starts from a picture and a plus adapter."""
import math

import numpy as np
import pytest
import torch

import _extents_resampler as XR
import _guard as G
from conftest import run_calls

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAN = float("nan")
LOG2E = 1.4426950408889634
SCALE = 64 ** -0.5 * LOG2E     # what engine.emit_ip_resampler passes
PSNR_MIN = 40.0                # the project's bar for every bf16 stack against its fp32 / float64 reference (test_text_encoder_gpu.py)
MAX_TX = 272                   # MSDR_MAX_TX


def bf(x):
    return x.to(BF16).to(torch.float32)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32).cpu().numpy()


def up8(n):
    return (n + 7) // 8 * 8


def psnr(test, ref):
    ref, test = np.asarray(ref, dtype=np.float64), np.asarray(test, dtype=np.float64)
    mse = float(np.mean((ref - test) ** 2))
    return float("inf") if mse == 0 else 10.0 * np.log10(float(ref.max() - ref.min()) ** 2 / mse)


# -------------------------------------------------------------------------------------------------------- msdr_perceiver_attention
def guarded(dev, q, kx, vx, kl, vl, *, H, scale, wide=True, **over):
    """The launch's operands between guard bands: q [B][n][C], kx / vx [B][t][C], kl / vl [B][n][C] (V NOT transposed) on the CPU.
    wide: every ld larger than its width, NaN in the padding columns of both vt operands (and in every row gap)."""
    B, n, C = q.shape
    t = kx.shape[1]
    pad = 8 if wide else 0
    geo = dict(batch=B, heads=H, n=n, t_x=t, q_ld=C + pad, kx_ld=C + 2 * pad, vtx_ld=up8(t) + pad, kl_ld=C + 3 * pad, vtl_ld=up8(n) + pad,
               o_ld=C + pad)
    geo.update(over)
    g = G.Guard(dev, XR.perceiver_attention(q=1, k_x=1, vt_x=1, k_l=1, vt_l=1, out=1, **geo))

    def rows(x, name, ld):
        return g.inp(x.reshape(-1, C).to(BF16), name, ld=ld if ld > C else None)

    def vt(v, name, ld, used):
        full = torch.zeros(B, C, ld, dtype=BF16)
        full[:, :, :used] = v.permute(0, 2, 1).to(BF16)
        view = g.inp(full.reshape(B * C, ld), name)
        g.gaps(view, used, ld=ld)                          # (padding keys hold NaN)
        return view

    args = dict(q=rows(q, "q", geo["q_ld"]), k_x=rows(kx, "k_x", geo["kx_ld"]), vt_x=vt(vx, "vt_x", geo["vtx_ld"], t),
                k_l=rows(kl, "k_l", geo["kl_ld"]), vt_l=vt(vl, "vt_l", geo["vtl_ld"], n))
    out = g.out((B * n, C), BF16, NAN, "out", ld=geo["o_ld"] if geo["o_ld"] > C else None)
    return g, dict(out=out, scale=scale, **args, **geo), out


def launch(dev, q, kx, vx, kl, vl, *, H, scale, wide=True):
    from minsdtf_amd import ops

    g, args, out = guarded(dev, q, kx, vx, kl, vl, H=H, scale=scale, wide=wide)
    run_calls(ops.perceiver_attention(**args))
    g.check()
    B, n, C = q.shape
    return out.reshape(B, n, C).clone().cpu()


_OPERANDS = {}


def operands(H, n, t, B):
    """bf16-rounded Gaussian operands, a spike on one x key and on one latent key (a peaked row beside flat ones); made once per
    (H, n, t) for 3 samples and sliced, so sample 0 of every batch is the same."""
    key = (H, n, t)
    if key not in _OPERANDS:
        gen = torch.Generator().manual_seed(1000 * H + 10 * n + t)
        C = H * 64
        q, kl, vl = (bf(torch.randn(3, n, C, generator=gen)) for _ in range(3))
        kx, vx = (bf(torch.randn(3, t, C, generator=gen)) for _ in range(2))
        kx[:, t // 2] *= 3.0
        kl[:, n - 1] *= 3.0
        _OPERANDS[key] = (q, bf(kx), vx, bf(kl), vl)
    return tuple(x[:B] for x in _OPERANDS[key])


def reference(q, kx, vx, kl, vl, H, scale):
    """(resampler.attention_reference - softmax2(scale q [kx ; kl]^T) [vx ; vl] in float64 on the bf16 operands -, the same with |v| =
    sum_j p_j |v_j|, max_ij sum_c |q_ic k_jc|)."""
    from minsdtf_amd import resampler

    s32 = float(np.float32(scale))
    ref, A = (torch.from_numpy(resampler.attention_reference(q.numpy(), kx.numpy(), v1.numpy(), kl.numpy(), v2.numpy(), s32, H))
              for v1, v2 in ((vx, vl), (vx.abs(), vl.abs())))
    B, n, _C = q.shape
    qh = q.double().view(B, n, H, 64).permute(0, 2, 1, 3)
    kh = torch.cat([kx, kl], 1).double().view(B, -1, H, 64).permute(0, 2, 1, 3)
    return ref, A, float((qh.abs() @ kh.abs().transpose(-1, -2)).max())


KERNEL_SHAPES = [(1, 12, 16, 257), (2, 12, 16, 257), (1, 1, 1, 1), (3, 2, 5, 77), (1, 3, 16, 64), (2, 1, 8, MAX_TX)]
_RUNS = {}


@pytest.mark.parametrize("B,H,n,t", KERNEL_SHAPES, ids=lambda v: str(v))
def test_perceiver_attention_against_float64(gpu, B, H, n, t):
    """Every ld larger than its width, NaN in the padding columns of both vt operands, out pre-filled with NaN, guard bands around
    every operand.  The bound, from the roundings include/minsdtf_hip_resampler.h pins (not fitted), per output element with
    A = sum_j p_j |v_j|:

        |got - ref| <= 2^-8 |ref|  (the store's rounding to bf16: 8 significant bits, round to nearest: relative 2^-8 at the most)
                     + 2^-8 A      (each normalised probability rounded once to bf16, relative 2^-8, weighted by |v_j|)
                     + 2 e A       (the fp32 part: a score is 64 exact bf16 products summed in fp32, |error| <= 64 * 2^-24 * sum_c |q k|
                                    = 2^-18 Q with Q = max_ij sum_c |q_ic k_jc|, then one multiplication by scale and v_exp_f32: a
                                    probability's relative error e = ln 2 * scale * 2^-18 * Q + 2^-20; numerator and row sum: twice)
                     + 2^-30

    Observed on the MI355X: worst err / bound 0.66, 0.69, 0.61, 0.69, 0.58 and 0.50 for the six shapes in KERNEL_SHAPES' order (the
    largest: 0.69 at (2, 12, 16, 257) and (3, 2, 5, 77))."""
    q, kx, vx, kl, vl = operands(H, n, t, B)
    got = launch(gpu, q, kx, vx, kl, vl, H=H, scale=SCALE)
    _RUNS[(B, H, n, t)] = got
    ref, A, Q = reference(q, kx, vx, kl, vl, H, SCALE)
    g64 = got.to(torch.float64)
    assert bool(torch.isfinite(g64).all())
    e = math.log(2.0) * SCALE * 2.0 ** -18 * Q + 2.0 ** -20
    bound = 2.0 ** -8 * ref.abs() + (2.0 ** -8 + 2.0 * e) * A + 2.0 ** -30
    worst = float(((g64 - ref).abs() / bound).max())
    print(f"perceiver_attention {(B, H, n, t)}: max |err| {float((g64 - ref).abs().max()):.3e}, worst err / bound {worst:.3f}")
    assert worst <= 1.0, worst
    tight = launch(gpu, q, kx, vx, kl, vl, H=H, scale=SCALE, wide=False)     # the bits do not depend on the leading dimensions
    assert np.array_equal(bits(tight), bits(got))
    if (1, 12, 16, 257) in _RUNS and (2, 12, 16, 257) in _RUNS:               # a sample's bits do not depend on its batch
        assert np.array_equal(bits(_RUNS[(2, 12, 16, 257)][0]), bits(_RUNS[(1, 12, 16, 257)][0]))


def test_perceiver_attention_sample_bits_do_not_depend_on_the_batch(gpu):
    for shape in ((1, 12, 16, 257), (2, 12, 16, 257)):
        if shape not in _RUNS:
            test_perceiver_attention_against_float64(gpu, *shape)
    one, two = _RUNS[(1, 12, 16, 257)], _RUNS[(2, 12, 16, 257)]
    assert np.array_equal(bits(two[0]), bits(one[0])) and not np.array_equal(bits(two[0]), bits(two[1]))


REFUSALS = [(dict(n=17), -1, b"n = 17"), (dict(n=0), -1, b"n = 0"), (dict(head_dim=80), -3, b"head_dim 80"), (dict(head_dim=40), -3, b"head_dim 40"),
            (dict(t_x=MAX_TX + 1, vtx_ld=MAX_TX + 8), -1, b"t_x = 273"), (dict(t_x=0), -1, b"t_x = 0"), (dict(q_ld=772), -1, b"q_ld = 772"),
            (dict(kx_ld=770), -1, b"kx_ld = 770"), (dict(vtx_ld=266), -1, b"vtx_ld = 266"), (dict(kl_ld=780), -1, b"kl_ld = 780"),
            (dict(vtl_ld=20), -1, b"vtl_ld = 20"), (dict(o_ld=769), -1, b"o_ld = 769"), (dict(vtx_ld=256), -1, b"vtx_ld = 256 < t_x"),
            (dict(vtl_ld=8), -1, b"vtl_ld = 8 < n"), (dict(o_ld=760), -1, b"smaller than heads"), (dict(scale=NAN), -1, b"scale"),
            (dict(batch=0), -1, b"batch 0"), (dict(heads=0), -1, b"heads 0")]


@pytest.mark.parametrize("bad,rc,text", REFUSALS, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_perceiver_attention_refusals_launch_nothing(gpu, bad, rc, text):
    """Each bad argument returns the library's error code with the field named, and the output buffer keeps its bits."""
    from minsdtf_amd import _lib_resampler, ops

    q, kx, vx, kl, vl = operands(12, 16, 257, 1)
    g, args, out = guarded(gpu, q, kx, vx, kl, vl, H=12, scale=SCALE)
    before = bits(out.clone())
    call = ops.perceiver_attention(**dict(args, **bad))
    assert call.fn(*call.args, torch.cuda.current_stream().cuda_stream) == rc
    msg = _lib_resampler.load().msdr_last_error()
    assert b"perceiver_attention" in msg and text in msg, msg
    torch.cuda.synchronize()
    g.check()
    after = bits(out.clone())
    assert np.array_equal(before.view(np.uint16), after.view(np.uint16))     # (NaN: compared as bits)


# --------------------------------------------------------------------------------------------------------------- the model
_HIDDEN = (1.2 * np.random.default_rng(53).standard_normal((2, 257, 1280))).astype(np.float32)   # the residual stream behind the tower's
_MODELS = {}                                                                                      # pre-LayerNorm and a few layers: unit scale


def _resampler(gpu, depth):
    """(the synthetic resampler, forward_host of both samples in float64), made once per depth."""
    if depth not in _MODELS:
        from minsdtf_amd import resampler
        from minsdtf_amd.models import IPResampler

        m = IPResampler(depth=depth, device=gpu)
        state = m.load_synthetic(seed=depth)
        _MODELS[depth] = (m, resampler.forward_host(state, _HIDDEN))
    return _MODELS[depth]


@pytest.mark.parametrize("depth,B", [(1, 1), (1, 2), (2, 1), (2, 2), (4, 1)])
def test_resampler_against_forward_host(gpu, depth, B):
    """Observed on the MI355X: 60.8 / 60.9 dB (depth 1, B = 1 / 2), 59.8 / 60.3 dB (depth 2), 59.0 dB (depth 4, B = 1)."""
    m, ref = _resampler(gpu, depth)
    got = m.predict_on_batch(_HIDDEN[:B])
    assert got.dtype == np.float32 and got.shape == (B, 16, 768) and np.isfinite(got).all()
    p = psnr(got, ref[:B])
    print(f"ip_resampler depth {depth}, B = {B}: {p:.1f} dB")
    assert p >= PSNR_MIN, p
    assert np.array_equal(got.view(np.int32), m.predict_on_batch(_HIDDEN[:B]).view(np.int32))   # a run repeats


def test_resampler_sample_bits_do_not_depend_on_the_batch(gpu):
    m, _ref = _resampler(gpu, 2)
    m.compile(jit_compile=True)   # (graph replay, as the pipeline runs it)
    try:
        one, two = m.predict_on_batch(_HIDDEN[:1]), m.predict_on_batch(_HIDDEN)
        assert np.array_equal(one[0].view(np.int32), two[0].view(np.int32)) and not np.array_equal(two[0], two[1])
        assert np.array_equal(two.view(np.int32), m.predict_on_batch(_HIDDEN).view(np.int32))
    finally:
        m.compile(jit_compile=False)
    eager = m.predict_on_batch(_HIDDEN[:1])
    assert np.array_equal(eager.view(np.int32), one.view(np.int32))


# ----------------------------------------------------------------------------------------------------------------- the job
_RNG = np.random.default_rng(79)
CTX = _RNG.standard_normal((77, 768)).astype(np.float32)
UNC = _RNG.standard_normal((77, 768)).astype(np.float32)
PICTURE = _RNG.integers(0, 256, (64, 64, 3)).astype(np.uint8)
PICTURE_B = _RNG.integers(0, 256, (90, 120, 3)).astype(np.uint8)
KW = dict(batch_size=1, num_steps=3, unconditional_guidance_scale=7.5, guidance_rescale=0.7, seed=5, return_latent=True)


def test_plus_job_from_a_picture(gpu, monkeypatch):
    """Observed on the MI355X: tokens_u of the zero-normalised picture 60.7 dB against forward_host on vision.forward_host's
    penultimate of exactly-zero normalised pixels."""
    from minsdtf_amd import resampler, vision
    from minsdtf_amd.models import ClipVisionEncoder, DiffusionModel, ImageDecoder, IPAdapter
    from minsdtf_amd.stable_diffusion import StableDiffusion

    unet = DiffusionModel(64, 64, device=gpu)
    unet.load_synthetic(seed=0, bias_scale=0.05)
    dec = ImageDecoder(device=gpu)
    dec.load_synthetic(seed=0, bias_scale=0.05)
    tower = ClipVisionEncoder(layers=2, device=gpu)
    tower_state = tower.load_synthetic(seed=2)
    plus = IPAdapter.synthetic_plus(5, depth=1, device=gpu)
    assert plus.tokens == 16 and plus.resampler is not None and plus.resampler.depth == 1
    sd = StableDiffusion(64, 64, jit_compile=True, device=gpu)
    sd._diffusion_model, sd._image_decoder = unet, dec
    sd.unconditional_context = UNC
    sd.clip_vision = tower
    calls = {"tower": 0, "resampler": 0}
    t_orig, r_orig = tower.predict_on_batch, plus.resampler.predict_on_batch
    monkeypatch.setattr(tower, "predict_on_batch", lambda *a, **k: (calls.__setitem__("tower", calls["tower"] + 1), t_orig(*a, **k))[1])
    monkeypatch.setattr(plus.resampler, "predict_on_batch", lambda *a, **k: (calls.__setitem__("resampler", calls["resampler"] + 1), r_orig(*a, **k))[1])

    from_picture = sd.generate_image(CTX, ip_adapter=dict(image=PICTURE, model=plus), **KW)
    assert calls == {"tower": 2, "resampler": 2}                       # the picture and the zero-normalised one
    tok_u, tok_c = sd.image_prompt_tokens(PICTURE, plus)
    assert calls == {"tower": 2, "resampler": 2} and tok_u.shape == tok_c.shape == (16, 768) and tok_c.dtype == np.float32
    from_tokens = sd.generate_image(CTX, ip_adapter=dict(tokens=tok_c, negative_tokens=tok_u, model=plus), **KW)
    assert np.array_equal(from_picture.view(np.int32), from_tokens.view(np.int32))
    again = sd.generate_image(CTX, ip_adapter=dict(image=PICTURE, model=plus), **KW)
    assert calls == {"tower": 2, "resampler": 2} and np.array_equal(again.view(np.int32), from_picture.view(np.int32))
    other = sd.generate_image(CTX, ip_adapter=dict(image=PICTURE_B, model=plus), **KW)
    assert calls == {"tower": 3, "resampler": 3} and not np.array_equal(other, from_picture)   # a new picture: not the negative again
    assert not np.array_equal(sd.generate_image(CTX, **KW), from_picture)
    # the negative: the zero-normalised picture through both networks, against float64 on exactly-zero normalised pixels
    scale, shift = vision.pixel_affine()
    zero = np.ascontiguousarray(np.broadcast_to(np.asarray([-b / a for a, b in zip(scale, shift)], dtype=np.float64), (224, 224, 3)))
    hidden = vision.forward_host(tower_state, zero, 2)["penultimate"]
    ref = resampler.forward_host(plus.resampler.state, hidden)[0]
    p = psnr(tok_u, ref)
    print(f"tokens_u of the zero-normalised picture: {p:.1f} dB")
    assert p >= PSNR_MIN, p
    assert not np.array_equal(tok_u, tok_c)
