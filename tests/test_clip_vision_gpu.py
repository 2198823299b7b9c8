"""The CLIP ViT-H/14 vision tower on the device: the three kernels of libminsdtf_hip_vision.so between guard bands against float64,
synthetic 2- and 3-layer towers against vision.forward_host, and an ip_adapter job that starts from a picture."""
import numpy as np
import pytest
import torch

import _extents_vision as XV
import _guard as G
from conftest import run_calls

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAN = float("nan")
PSNR_MIN = 40.0   # the project's bar for every bf16 stack against its fp32 / float64 reference (test_text_encoder_gpu.py)


def bf(x):
    return x.to(BF16).to(torch.float32)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32).cpu().numpy()


def psnr(test, ref):
    ref, test = np.asarray(ref, dtype=np.float64), np.asarray(test, dtype=np.float64)
    mse = float(np.mean((ref - test) ** 2))
    return float("inf") if mse == 0 else 10.0 * np.log10(float(ref.max() - ref.min()) ** 2 / mse)


# ------------------------------------------------------------------------------------------------------------------ msdv_gelu
def _gelu_input(rows, cols):
    g = torch.Generator().manual_seed(rows * 7 + cols)
    special = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 30.0, -30.0, -13.2])
    n = rows * cols
    body = torch.cat([torch.linspace(-9.0, 9.0, n // 2), 3.0 * torch.randn(n - n // 2, generator=g)])
    body = body[torch.randperm(n, generator=g)]
    body[:min(n, len(special))] = special[:min(n, len(special))]
    return body.reshape(rows, cols).to(torch.float32)


@pytest.mark.parametrize("rows,cols,ld_in,ld_out", [(257, 5120, 5120, 5120), (1, 8, 8, 8), (3, 5120, 5128, 5136)])
def test_gelu_against_float64(gpu, rows, cols, ld_in, ld_out):
    from minsdtf_amd import ops

    x = _gelu_input(rows, cols)
    geo = dict(rows=rows, cols=cols, ld_in=ld_in, ld_out=ld_out)
    g = G.Guard(gpu, XV.gelu(**geo))
    xd = g.inp(x, "x", ld=ld_in if ld_in > cols else None)
    out = g.out((rows, cols), BF16, NAN, "out", ld=ld_out if ld_out > cols else None)
    run_calls(ops.gelu(x=xd, out=out, **geo))
    g.check()
    got = out.clone().cpu().to(torch.float64)
    x64 = x.to(torch.float64)
    ref = 0.5 * x64 * (1.0 + torch.erf(x64 * (0.5 ** 0.5)))
    assert bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -20
    worst = float((err / bound).max())
    print(f"gelu {rows}x{cols}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------ msdv_patch_embed
_PATCH = {}


def _patch_data():
    """Operands for B = 3 and the float64 reference on the same bf16-rounded pixels and weights, made once and never changed."""
    if _PATCH:
        return _PATCH
    from minsdtf_amd import vision

    rng = np.random.default_rng(41)
    px = rng.uniform(0.0, 255.0, (3, 224, 224, 3)).astype(np.float32)
    w = bf(torch.from_numpy(rng.uniform(-0.05, 0.05, (1280, 588)).astype(np.float32)))
    cls, pos = (torch.from_numpy((0.5 * rng.standard_normal(s)).astype(np.float32)) for s in ((1280,), (257, 1280)))
    gamma = torch.from_numpy(rng.uniform(0.8, 1.2, 1280).astype(np.float32))
    beta = torch.from_numpy(rng.uniform(-0.1, 0.1, 1280).astype(np.float32))
    scale, shift = vision.pixel_affine()
    sc, sh = np.asarray(scale, dtype=np.float32).astype(np.float64), np.asarray(shift, dtype=np.float32).astype(np.float64)
    x = bf(torch.from_numpy((px.astype(np.float64) * sc + sh).astype(np.float32))).to(torch.float64)   # the fma, then the one rounding
    patches = x.reshape(3, 16, 14, 16, 14, 3).permute(0, 1, 3, 2, 4, 5).reshape(3, 256, 588)
    e = patches @ w.to(torch.float64).t() + pos[1:].to(torch.float64)
    e = torch.cat([(cls + 0.0).to(torch.float64).add(pos[0].to(torch.float64)).expand(3, 1, 1280), e], dim=1)
    mean = e.mean(-1, keepdim=True)
    var = ((e - mean) ** 2).mean(-1, keepdim=True)
    ref = (e - mean) / torch.sqrt(var + 1e-5) * gamma.to(torch.float64) + beta.to(torch.float64)
    _PATCH.update(px=torch.from_numpy(px), w=w, cls=cls, pos=pos, gamma=gamma, beta=beta, ref=ref, scale=scale, shift=shift, runs={})
    return _PATCH


@pytest.mark.parametrize("B,w_ld,o_ld", [(1, 592, 1280), (3, 600, 1288)])
def test_patch_embed_against_float64(gpu, B, w_ld, o_ld):
    from minsdtf_amd import ops

    d = _patch_data()
    geo = dict(batch=B, w_ld=w_ld, o_ld=o_ld)
    g = G.Guard(gpu, XV.patch_embed(pixels=1, w=1, cls=1, pos=1, gamma=1, beta=1, out=1, **geo))
    args = dict(pixels=g.inp(d["px"][:B], "pixels"), w=g.inp(d["w"].to(BF16), "w", ld=w_ld), cls=g.inp(d["cls"], "cls"), pos=g.inp(d["pos"], "pos"),
                gamma=g.inp(d["gamma"], "gamma"), beta=g.inp(d["beta"], "beta"))
    out = g.out((B * 257, 1280), BF16, NAN, "out", ld=o_ld if o_ld > 1280 else None)
    run_calls(ops.patch_embed(out=out, scale=d["scale"], shift=d["shift"], **args, **geo))
    g.check()
    got = out.clone().cpu().reshape(B, 257, 1280)
    d["runs"][B] = got
    ref = d["ref"][:B]
    got64 = got.to(torch.float64)
    assert bool(torch.isfinite(got64).all())
    err = (got64 - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -16
    worst = float((err / bound).max())
    print(f"patch_embed B={B}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert worst <= 1.0, worst
    for b in range(1, B):   # token 0 is cls + pos[0] through the same LayerNorm for every sample
        assert np.array_equal(bits(got[b, 0]), bits(got[0, 0]))
    if 1 in d["runs"] and 3 in d["runs"]:   # a sample's bits do not depend on its batch (nor on w_ld / o_ld)
        assert np.array_equal(bits(d["runs"][3][0]), bits(d["runs"][1][0]))


def test_patch_embed_sample_bits_do_not_depend_on_the_batch(gpu):
    d = _patch_data()
    for B, w_ld, o_ld in ((1, 592, 1280), (3, 600, 1288)):
        if B not in d["runs"]:
            test_patch_embed_against_float64(gpu, B, w_ld, o_ld)
    assert np.array_equal(bits(d["runs"][3][0]), bits(d["runs"][1][0]))


# ----------------------------------------------------------------------------------------------------------- msdv_pool_project
def test_pool_project_against_float64(gpu):
    from minsdtf_amd import ops, packing

    rng = np.random.default_rng(43)
    stride = 257 * 1280
    x = bf(torch.from_numpy((0.3 + 1.5 * rng.standard_normal((3, 1280))).astype(np.float32)))
    lim = float(np.sqrt(6.0 / (1280 + 1024)))
    w = bf(torch.from_numpy(rng.uniform(-lim, lim, (1024, 1280)).astype(np.float32)))
    gamma = torch.from_numpy(rng.uniform(0.8, 1.2, 1280).astype(np.float32))
    beta = torch.from_numpy(rng.uniform(-0.1, 0.1, 1280).astype(np.float32))

    def formulas(dt):
        xx, ww, ga, be = (t.to(dt) for t in (x, w, gamma, beta))
        mean = xx.sum(-1, keepdim=True) / 1280
        dev = xx - mean
        var = (dev * dev).sum(-1, keepdim=True) / 1280
        y = dev * (1.0 / torch.sqrt(var + torch.tensor(1e-5, dtype=dt))) * ga + be
        return y @ ww.t()

    ref = formulas(torch.float64)
    e32 = float((formulas(torch.float32).to(torch.float64) - ref).abs().max())
    runs = {}
    for B in (1, 3):
        for lay in (0, 1):
            geo = dict(batch=B, x_stride=stride)
            g = G.Guard(gpu, XV.pool_project(x=1, gamma=1, beta=1, w=1, out=1, **geo))
            xd = g.inp(x[:B].to(BF16), "x", ld=stride)
            wd = g.inp(packing.chunk_major(w.to(BF16)) if lay else w.to(BF16), "w")
            out = g.out((B, 1024), torch.float32, NAN, "out")
            run_calls(ops.pool_project(x=xd, gamma=g.inp(gamma, "gamma"), beta=g.inp(beta, "beta"), w=wd, out=out, w_layout=lay, **geo))
            g.check()
            runs[(B, lay)] = out.clone().cpu()
    got = runs[(3, 0)]
    assert bool(torch.isfinite(got).all())
    err = float((got.to(torch.float64) - ref).abs().max())
    print(f"pool_project: fp32 torch on the CPU is off by {e32:.3e} from float64, the device by {err:.3e} (allowed: 8x = {8 * e32:.3e})")
    assert err <= 8.0 * e32, (err, e32)
    assert np.array_equal(bits(runs[(3, 0)]), bits(runs[(3, 1)])) and np.array_equal(bits(runs[(1, 0)]), bits(runs[(1, 1)]))   # either layout
    assert np.array_equal(bits(runs[(3, 0)][0]), bits(runs[(1, 0)][0]))   # a sample's bits do not depend on its batch


# ------------------------------------------------------------------------------------------------------------------- the tower
_PIX = np.random.default_rng(47).uniform(0.0, 255.0, (2, 224, 224, 3)).astype(np.float32)
_TOWERS = {}


def _tower(gpu, layers):
    """(the synthetic tower, its checkpoint-layout state, forward_host of both pictures in float64), made once per depth."""
    if layers not in _TOWERS:
        from minsdtf_amd import vision
        from minsdtf_amd.models import ClipVisionEncoder

        m = ClipVisionEncoder(layers=layers, device=gpu)
        state = m.load_synthetic(seed=layers)
        _TOWERS[layers] = (m, state, vision.forward_host(state, _PIX, layers))
    return _TOWERS[layers]


@pytest.mark.parametrize("layers,B", [(2, 1), (2, 2), (3, 1), (3, 2)])
def test_tower_against_forward_host(gpu, layers, B):
    m, _state, ref = _tower(gpu, layers)
    for output in ("image_embeds", "last_hidden_state", "penultimate"):
        got = m.predict_on_batch(_PIX[:B], output=output)
        assert got.dtype == np.float32 and got.shape == ref[output][:B].shape and np.isfinite(got).all()
        p = psnr(got, ref[output][:B])
        print(f"clip_vision {layers} layers, B = {B}: {output} {p:.1f} dB")
        assert p >= PSNR_MIN, (output, p)


def test_tower_sample_bits_do_not_depend_on_the_batch_and_runs_repeat(gpu):
    m, _state, _ref = _tower(gpu, 2)
    m.compile(jit_compile=True)   # (graph replay, as the pipeline runs it)
    try:
        one = m.predict_on_batch(_PIX[:1])
        two = m.predict_on_batch(_PIX)
        assert np.array_equal(one.view(np.int32), m.predict_on_batch(_PIX[:1]).view(np.int32))
        assert np.array_equal(two.view(np.int32), m.predict_on_batch(_PIX).view(np.int32))
        assert np.array_equal(one[0].view(np.int32), two[0].view(np.int32))
        h1, h2 = m.predict_on_batch(_PIX[:1], output="penultimate"), m.predict_on_batch(_PIX, output="penultimate")
        assert np.array_equal(h1[0].view(np.int32), h2[0].view(np.int32))
        assert not np.array_equal(two[0], two[1])
    finally:
        m.compile(jit_compile=False)


# --------------------------------------------------------------------------------------------------------------------- the job
_RNG = np.random.default_rng(78)
CTX = _RNG.standard_normal((77, 768)).astype(np.float32)
UNC = _RNG.standard_normal((77, 768)).astype(np.float32)
PICTURE = _RNG.integers(0, 256, (64, 64, 3)).astype(np.uint8)
PICTURE_B = _RNG.integers(0, 256, (90, 120, 3)).astype(np.uint8)
KW = dict(batch_size=1, num_steps=3, unconditional_guidance_scale=7.5, guidance_rescale=0.7, seed=5, return_latent=True)


def test_ip_adapter_job_from_a_picture(gpu, monkeypatch):
    from minsdtf_amd.models import DiffusionModel, ImageDecoder, IPAdapter
    from minsdtf_amd.stable_diffusion import StableDiffusion

    unet = DiffusionModel(64, 64, device=gpu)
    unet.load_synthetic(seed=0, bias_scale=0.05)
    dec = ImageDecoder(device=gpu)
    dec.load_synthetic(seed=0, bias_scale=0.05)
    adapter = IPAdapter.synthetic(5, 4, device=gpu)
    tower = _tower(gpu, 2)[0]
    sd = StableDiffusion(64, 64, jit_compile=True, device=gpu)
    sd._diffusion_model, sd._image_decoder = unet, dec
    sd.unconditional_context = UNC
    sd.clip_vision = tower
    calls = []
    orig = tower.predict_on_batch
    monkeypatch.setattr(tower, "predict_on_batch", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])

    from_picture = sd.generate_image(CTX, ip_adapter=dict(image=PICTURE, model=adapter), **KW)
    assert len(calls) == 1
    emb = sd.encode_image_prompt(PICTURE)
    assert emb.shape == (1024,) and len(calls) == 1   # (the job's embedding was kept)
    from_embeds = sd.generate_image(CTX, ip_adapter=dict(embeds=emb, model=adapter), **KW)
    assert np.array_equal(from_picture.view(np.int32), from_embeds.view(np.int32))
    again = sd.generate_image(CTX, ip_adapter=dict(image=PICTURE, model=adapter), **KW)
    assert len(calls) == 1 and np.array_equal(again.view(np.int32), from_picture.view(np.int32))   # the tower did not run again
    plain = sd.generate_image(CTX, **KW)
    assert not np.array_equal(plain, from_picture)
    other = sd.generate_image(CTX, ip_adapter=dict(image=PICTURE_B, model=adapter), **KW)
    assert len(calls) == 2 and not np.array_equal(other, from_picture)
