"""Self-attention guidance on the device: msdx_attention_colsum against a float64 softmax of the same bf16 operands,
msdx_sag_degrade against sag.degrade_host, the d rows of the engine against predict_on_batch of the standalone kernel's latent, the
one-token case, the device loop against host_loop=True, batch independence, the sharded job and the oracle fixtures
(tests/golden/sag_*.npz, tools/make_sag_fixtures.py).

The two kernel bounds are 4 x the maximum error tools/sag_parity.py measured over THESE cases (profiles/sag_parity.json): the kernels
are deterministic, the margin covers other seeds, not noise."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _extents_sag as XS
import _guard as G

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
PSNR_MIN = 40.0        # the project's bar for every job
HOST_PSNR_MIN = 45.0   # device loop vs host_loop=True of a samplers.py txt2img job (test_pag_gpu.py)
MARGIN = 4.0

# (batch, heads, head_dim, S): the 512 x 512 shape; a partial tile; one token; a tail in every tile dimension; multi-tile and no
# multiple of 64; four whole tiles
COLSUM_SHAPES = [(1, 8, 160, 64), (2, 8, 160, 16), (3, 8, 160, 1), (1, 8, 160, 77), (1, 8, 160, 144), (2, 8, 160, 256)]
# (h, w, mh, mw): the reflect limit; one map cell; a 16 x 16 tile boundary with an integer ratio; a non-integer ratio
DEGRADE_SHAPES = [(5, 5, 1, 1), (8, 8, 1, 1), (16, 24, 2, 3), (9, 9, 2, 2)]
THRESHOLD = 1.0


def parity():
    with open(os.path.join(ROOT, "profiles", "sag_parity.json")) as f:
        return json.load(f)


def run_calls(calls):
    if not isinstance(calls, (list, tuple)):
        calls = [calls]
    st = torch.cuda.current_stream().cuda_stream
    for c in calls:
        c(st)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ colsum
def colsum_inputs(shape):
    """q, k as bf16 (batch + 1, S, C): row 0 is never launched on (the launches take offset pointers, as the engine's do).  q is
    scaled so that the base-2 logits have a standard deviation near 2: attention is peaky, few keys sit at the threshold."""
    batch, heads, d, S = shape
    g = torch.Generator().manual_seed(7919 * S + batch)
    q = (torch.randn(batch + 1, S, heads * d, generator=g) * (2.0 / d ** 0.5)).to(torch.bfloat16)
    k = torch.randn(batch + 1, S, heads * d, generator=g).to(torch.bfloat16)
    return q, k


def colsum_reference(q, k, heads):
    """float64: A[b][j] = mean_h sum_i softmax2_j(q_h k_h^T)[i][j] from the bf16 values."""
    q, k = q.double().numpy(), k.double().numpy()
    B, S, C = q.shape
    d = C // heads
    out = np.zeros((B, S))
    for b in range(B):
        for h in range(heads):
            s = q[b, :, h * d:(h + 1) * d] @ k[b, :, h * d:(h + 1) * d].T
            p = np.exp2(s - s.max(axis=1, keepdims=True))
            out[b] += (p / p.sum(axis=1, keepdims=True)).sum(axis=0)
    return out / heads


def colsum_run(gpu, shape, q, k, first=1, rows=None, pad=64):
    """One guarded launch on rows first .. first + rows - 1 of q / k, the operands `pad` columns wider than they carry: (A fp32
    (rows, S) on the host, the guard)."""
    from minsdtf_amd import ops

    batch, heads, d, S = shape
    rows = batch if rows is None else rows
    C = heads * d
    ld = C + pad
    dims = dict(batch=rows, heads=heads, head_dim=d, s=S, q_ld=ld, k_ld=ld)
    gd = G.Guard(gpu, XS.attention_colsum(q=True, k=True, out=True, workspace=True, **dims))
    qv = gd.inp(q[first:first + rows].reshape(rows * S, C), "q", ld=ld)
    kv = gd.inp(k[first:first + rows].reshape(rows * S, C), "k", ld=ld)
    out = gd.out((rows, S), torch.float32, float("nan"), "out")   # (what the previous tenant left: NaN)
    ws = gd.out((rows * heads * S * 2,), torch.float32, float("nan"), "workspace")
    run_calls(ops.attention_colsum(q=qv, k=kv, out=out, workspace=ws, **dims))
    gd.check()
    return out.cpu().numpy(), gd


def colsum_error(got, ref):
    return float((np.abs(got.astype(np.float64) - ref) / ref).max())


@pytest.mark.parametrize("shape", COLSUM_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_colsum(gpu, shape):
    batch, heads, d, S = shape
    bound = MARGIN * parity()["colsum_max_rel_err"]
    q, k = colsum_inputs(shape)
    ref = colsum_reference(q[1:], k[1:], heads)
    got, _gd = colsum_run(gpu, shape, q, k)
    assert got.shape == (batch, S) and np.all(np.isfinite(got))
    err = colsum_error(got, ref)
    print(f"colsum {shape}: max relative error {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    # every query's probabilities sum to 1: the map sums to S
    assert np.all(np.abs(got.astype(np.float64).sum(axis=1) - S) <= bound * S)
    if S == 1:
        np.testing.assert_array_equal(got, np.ones((batch, 1), dtype=np.float32))   # exactly 1.0f: never above the default threshold
    else:
        # the mask A > threshold, away from the entries the reference itself puts within the bound of the threshold
        near = np.abs(ref - THRESHOLD) < bound * np.maximum(ref, THRESHOLD)
        assert near.mean() <= 0.05, f"{near.mean():.1%} of the reference lies at the threshold"
        np.testing.assert_array_equal((got > np.float32(THRESHOLD))[~near], (ref > THRESHOLD)[~near])
        assert (ref > THRESHOLD).any() and (ref <= THRESHOLD).any()
    # a sample's bits do not depend on its batch, and a launch is reproducible
    again, _gd = colsum_run(gpu, shape, q, k)
    np.testing.assert_array_equal(again.view(np.int32), got.view(np.int32))
    for b in range(batch):
        alone, _gd = colsum_run(gpu, shape, q, k, first=1 + b, rows=1, pad=0 if b else 8)
        np.testing.assert_array_equal(alone[0].view(np.int32), got[b].view(np.int32))


def test_colsum_ignores_what_lies_outside(gpu):
    """NaN in the row in front of the launched ones, in the gap columns (the guard's) and left in the workspace by its previous
    tenant: none reaches the map."""
    shape = (2, 8, 160, 77)
    q, k = colsum_inputs(shape)
    q[0], k[0] = float("nan"), float("nan")
    got, _gd = colsum_run(gpu, shape, q, k)
    assert np.all(np.isfinite(got))
    q2, k2 = colsum_inputs(shape)
    want, _gd = colsum_run(gpu, shape, q2, k2)
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))


def test_colsum_argument_errors(gpu):
    from minsdtf_amd import _lib_ext, ops

    B, H, S = 2, 8, 16
    C = H * 160
    q = torch.zeros(B, S, C, dtype=torch.bfloat16, device=gpu)
    k = torch.zeros(B, S, C, dtype=torch.bfloat16, device=gpu)
    out = torch.zeros(B, S, device=gpu)
    ws = torch.zeros(B * H * S * 2, device=gpu)
    good = dict(q=q, k=k, out=out, workspace=ws, batch=B, heads=H, head_dim=160, s=S, q_ld=C, k_ld=C)
    st = torch.cuda.current_stream().cuda_stream
    for bad in (dict(q=None), dict(out=None), dict(workspace=None), dict(head_dim=80), dict(s=0), dict(s=4097), dict(heads=0), dict(batch=0),
                dict(q_ld=C - 8), dict(k_ld=C + 4), dict(workspace_floats=B * H * S * 2 - 1), dict(out=ws), dict(out=q), dict(workspace=k),
                dict(q=q.data_ptr() + 8)):
        call = ops.attention_colsum(**{**good, **bad})
        assert call.fn(*call.args, st) == -1, bad
        assert b"attention_colsum" in _lib_ext.load().msdx_last_error(), bad
    run_calls(ops.attention_colsum(**good))
    np.testing.assert_allclose(out.cpu().numpy(), 1.0, rtol=1e-6)   # all-zero logits: uniform attention, every key receives 1


# ----------------------------------------------------------------------------------------------------------------- degrade
def degrade_inputs(shape, stride, kind):
    """B = 2: latent, eps, the coefficient table [3][stride] (row 1 is the step's; the others hold values that would show), the
    map of `kind` ("none": every cell below the threshold, "all": above, "mixed": another pattern per sample)."""
    h, w, mh, mw = shape
    rng = np.random.default_rng(1000 * h + w + stride)
    x = rng.standard_normal((2, h, w, 4)).astype(np.float32)
    e = rng.standard_normal((2, h, w, 4)).astype(np.float32)
    coef = rng.uniform(0.1, 0.3, (3, stride)).astype(np.float32)
    coef[1, 0], coef[1, 1] = 0.8, 0.6
    A = {"none": np.full((2, mh * mw), 0.5), "all": np.full((2, mh * mw), 1.5),
         "mixed": np.stack([np.where(np.arange(mh * mw) % 2 == 0, 1.25, 0.75), np.where(np.arange(mh * mw) % 2 == 0, 1.0, 1.0000001)])}[kind]
    return x, e, coef, A.astype(np.float32)


def degrade_run(gpu, shape, stride, x, e, coef, A, blur_sigma=1.0):
    from minsdtf_amd import ops, sag

    h, w, mh, mw = shape
    dims = dict(batch=2, h=h, w=w, mh=mh, mw=mw, coef_stride=stride, num_steps=3)
    gd = G.Guard(gpu, XS.sag_degrade(latent=True, eps=True, out=True, coef=True, colsum=True, params=True, step_ptr=True, **dims))
    par = sag.params(sag.parse(dict(blur_sigma=blur_sigma, threshold=THRESHOLD)))
    t = dict(latent=gd.inp(torch.from_numpy(x), "latent"), eps=gd.inp(torch.from_numpy(e), "eps"),
             coef=gd.inp(torch.from_numpy(coef.reshape(-1)[:2 * stride + 2].copy()), "coef"), colsum=gd.inp(torch.from_numpy(A), "colsum"),
             params=gd.inp(torch.from_numpy(par), "params"), step_ptr=gd.inp(torch.tensor([1], dtype=torch.int32), "step_ptr"),
             out=gd.out((2, h, w, 4), torch.float32, G.CANARY, "out"))
    run_calls(ops.sag_degrade(**t, **dims))
    gd.check()
    return t["out"].cpu().numpy(), par


def degrade_error(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("stride", [4, 8])
@pytest.mark.parametrize("shape", DEGRADE_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_degrade(gpu, shape, stride):
    from minsdtf_amd import sag

    h, w, mh, mw = shape
    bound = MARGIN * parity()["degrade_max_err"]
    # nothing masked: the latent's own bits
    x, e, coef, A = degrade_inputs(shape, stride, "none")
    got, par = degrade_run(gpu, shape, stride, x, e, coef, A)
    np.testing.assert_array_equal(got.view(np.int32), x.view(np.int32))
    # everything masked: against the float64 statement
    x, e, coef, A = degrade_inputs(shape, stride, "all")
    got, par = degrade_run(gpu, shape, stride, x, e, coef, A)
    ref = sag.degrade_host(x, e, coef[1, 0], coef[1, 1], A, (mh, mw), par[:9], par[9])
    err = degrade_error(got, ref)
    print(f"degrade {shape}, stride {stride}: max error / max |reference| {err:.3e} (bound {bound:.3e})")
    assert err <= bound and not np.array_equal(got, x)
    # another map per sample; exactly the threshold is NOT above it, the next float is
    x, e, coef, A = degrade_inputs(shape, stride, "mixed")
    got, par = degrade_run(gpu, shape, stride, x, e, coef, A)
    ref = sag.degrade_host(x, e, coef[1, 0], coef[1, 1], A, (mh, mw), par[:9], par[9])
    m = sag.mask_host(A, (mh, mw), h, w, THRESHOLD)
    assert m.shape == (2, h, w) and (mh * mw == 1 or (m.any() and not m.all()))
    np.testing.assert_array_equal(got[~m].view(np.int32), x[~m].view(np.int32))
    assert degrade_error(got, ref) <= bound
    if m.any():
        assert not np.array_equal(got[m], x[m])


def test_degrade_argument_errors(gpu):
    from minsdtf_amd import _lib_ext, ops

    h = w = 8
    x, e, out = (torch.zeros(2, h, w, 4, device=gpu) for _ in range(3))
    coef, A, par = torch.ones(3, 4, device=gpu), torch.zeros(2, 1, device=gpu), torch.zeros(10, device=gpu)
    good = dict(latent=x, eps=e, coef=coef, coef_stride=4, colsum=A, params=par, out=out, batch=2, h=h, w=w, mh=1, mw=1, num_steps=3)
    st = torch.cuda.current_stream().cuda_stream
    for bad in (dict(latent=None), dict(params=None), dict(out=None), dict(h=4), dict(w=4), dict(mh=0), dict(mw=9), dict(batch=0),
                dict(coef_stride=1), dict(num_steps=0), dict(out=x), dict(out=e), dict(out=x.data_ptr() + 16), dict(latent=x.data_ptr() + 4)):
        call = ops.sag_degrade(**{**good, **bad})
        assert call.fn(*call.args, st) == -1, bad
        assert b"sag_degrade" in _lib_ext.load().msdx_last_error(), bad
    run_calls(ops.sag_degrade(**good))


# ---------------------------------------------------------------------------------------------------------------- pipelines
@pytest.fixture(scope="module")
def nets(gpu):
    """The synthetic UNet at 64x64 (mid block: one token) and, on the same packed weights, at 128x128 (2 x 2) and 256x256 (4 x 4);
    the decoder."""
    from minsdtf_amd.models import DiffusionModel, ImageDecoder

    unet = DiffusionModel(64, 64, device=gpu)
    unet.load_synthetic(seed=0, bias_scale=0.05)
    out = {64: unet}
    for size in (128, 256):
        out[size] = DiffusionModel(size, size, device=gpu)
        out[size].share_weights(unet)
    out["dec"] = ImageDecoder(device=gpu)
    out["dec"].load_synthetic(seed=0, bias_scale=0.05)
    return out


def _pipe(gpu, nets, size=128, jit=True):
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sd = StableDiffusion(size, size, jit_compile=jit, device=gpu)
    sd._diffusion_model = nets[size]
    sd._image_decoder = nets["dec"]
    rng = np.random.default_rng(41)
    sd.unconditional_context = rng.standard_normal((77, 768)).astype(np.float32)
    return sd, rng.standard_normal((77, 768)).astype(np.float32)


SAG = dict(scale=3.0, blur_sigma=1.0, threshold=1.0)


@pytest.mark.parametrize("sampler", [None, "dpmpp_2m"])
def test_d_rows_of_the_engine(gpu, nets, sampler):
    """One step of a batch-2 job at 128x128: the engine's eps groups are (u, c, d, copy of u, c').  From the start latent, the u rows,
    the map and the uploads the engine holds, msdx_sag_degrade standalone gives the engine's degraded latent, and predict_on_batch on
    it with the unconditional context gives the d rows - bit for bit; the u rows are predict_on_batch's, the copy is exact and c' is
    sag.combine_host's."""
    from minsdtf_amd import ops, sag

    sd, P = _pipe(gpu, nets)
    unet = nets[128]
    B, h, w = 2, unet.h, unet.w
    lat = np.random.default_rng(2).standard_normal((B, h, w, 4)).astype(np.float32)
    sd.generate_image(P, batch_size=B, num_steps=1, diffusion_noise=lat, guidance_rescale=0.0, return_latent=True, sag=SAG, sampler=sampler)
    eng = next(iter(sd._engines.values()))
    assert eng.sag and eng.passes == [(0, 4, 77, "both")] and eng.eps.shape[0] == 5 * B
    names = [c.name for c in eng.calls]
    mid = "mid_block.attentions.0.transformer_blocks.0.attn1"
    i = names.index(mid)
    assert names[i + 1] == mid + ".colsum" and names.count(mid + ".colsum") == 1 and names.count(mid) == 2
    j = names.index("sag.degrade")
    assert j > i and names[j + 1] == "conv_in" and names.count("conv_in") == 2
    assert names[-3:] == ["sag.copy_u", "sag.combine", "cfg_step" if sampler is None else "sampler_step"]
    eps = eng.eps.cpu().numpy().reshape(5, B, h, w, 4)
    A = eng.sag_A.cpu().numpy()
    assert A.shape == (B, 4) and np.all(np.abs(A.sum(axis=1) - 4.0) < 1e-4) and (A > 1.0).any() and (A <= 1.0).any()
    unc = np.repeat(sd.unconditional_context[None], B, axis=0)
    # the standalone kernel on the downloaded operands
    dev_lat, dev_eps = torch.from_numpy(lat).to(gpu), torch.from_numpy(eps[0]).to(gpu)
    out = torch.zeros(B, h, w, 4, device=gpu)
    step0 = torch.zeros(1, dtype=torch.int32, device=gpu)
    run_calls(ops.sag_degrade(latent=dev_lat, eps=dev_eps, coef=eng.coef, coef_stride=int(eng.coef.shape[1]), step_ptr=step0,
                              colsum=eng.sag_A, params=eng.sag_params, out=out, batch=B, h=h, w=w, mh=2, mw=2, num_steps=1))
    np.testing.assert_array_equal(out.cpu().numpy().view(np.int32), eng.sag_latent.cpu().numpy().view(np.int32))
    degraded = out.cpu().numpy()
    m = sag.mask_host(A, (2, 2), h, w, 1.0)
    np.testing.assert_array_equal(degraded[~m], lat[~m])
    assert not np.array_equal(degraded[m], lat[m])
    temb = eng.temb_in[:1].cpu().numpy().repeat(B, axis=0)   # the time embedding of the step, as the engine uploaded it
    np.testing.assert_array_equal(eps[0], unet.predict_on_batch([lat, temb, unc]))
    np.testing.assert_array_equal(eps[2], unet.predict_on_batch([degraded, temb, unc]))
    np.testing.assert_array_equal(eps[3], eps[0])
    np.testing.assert_array_equal(eps[4], sag.combine_host(eps[0], eps[1], eps[2], sag.weights(3.0, 7.5, h, w)))
    # predict_sag_map: the same eps, the same map
    e2, A2 = unet.predict_sag_map([lat, temb, unc])
    np.testing.assert_array_equal(e2, eps[0])
    np.testing.assert_array_equal(A2.view(np.int32), A.view(np.int32))


def test_one_token_d_rows_are_the_u_rows(gpu, nets):
    """64x64: the mid block has one token, A = 1 exactly, nothing exceeds the threshold of 1: the degraded latent is the latent and
    the d rows are the u rows, bit for bit - so the job is the plain job's arithmetic plus c' = k u + c - k u."""
    sd, P = _pipe(gpu, nets, 64)
    lat = np.random.default_rng(3).standard_normal((2, 8, 8, 4)).astype(np.float32)
    sd.generate_image(P, batch_size=2, num_steps=1, diffusion_noise=lat, guidance_rescale=0.0, return_latent=True, sag=SAG)
    eng = next(iter(sd._engines.values()))
    eps = eng.eps.cpu().numpy().reshape(5, 2, -1)
    np.testing.assert_array_equal(eng.sag_A.cpu().numpy(), np.ones((2, 1), dtype=np.float32))
    np.testing.assert_array_equal(eng.sag_latent.cpu().numpy(), lat)
    np.testing.assert_array_equal(eps[2], eps[0])


@pytest.mark.parametrize("sampler, g", [(None, 7.5), ("dpmpp_2m", 7.5), ("euler_a", 7.5), (None, 0.0)])
def test_device_loop_vs_host_loop(gpu, nets, sampler, g):
    """The device loop against host_loop=True (predict_sag_map, sag.degrade_host, predict_on_batch, sag.combine_host) with
    test_pag_gpu.py's bars: 45 dB for a samplers.py sampler, the project's 40 dB for the default step.  And SAG is not a no-op."""
    from oracle import sd_oracle as O

    sd, P = _pipe(gpu, nets)
    kw = dict(batch_size=1, num_steps=4, seed=11, sampler=sampler, unconditional_guidance_scale=g, guidance_rescale=0.7 if g else 0.0,
              return_latent=True, sag=SAG)
    dev = sd.generate_image(P, **kw)
    eng = next(iter(sd._engines.values()))
    assert eng.sag and eng.eps.shape[0] == (5 if g else 2)
    host = sd.generate_image(P, host_loop=True, **kw)
    p = O.psnr(dev, host)
    bar = HOST_PSNR_MIN if sampler is not None else PSNR_MIN
    plain = O.psnr(sd.generate_image(P, **{**kw, "sag": None}), dev)
    print(f"SAG, {sampler or 'default step'}, g = {g}: device loop vs host loop {p:.1f} dB (bar {bar:.0f}); the plain job against it {plain:.1f} dB")
    assert np.all(np.isfinite(dev)) and p >= bar
    assert plain < p


def test_unconditional_context_of_another_length(gpu, nets):
    """154 unconditional tokens against 77: two passes; the SAG half (degrade, second forward over the 154-token K/V) follows the
    pass of the u rows, in front of the c rows' pass; against host_loop=True at the sampler bar."""
    from oracle import sd_oracle as O

    sd, P = _pipe(gpu, nets)
    neg = np.random.default_rng(5).standard_normal((154, 768)).astype(np.float32)
    kw = dict(batch_size=2, num_steps=3, seed=11, sampler="dpmpp_2m", guidance_rescale=0.7, return_latent=True, negative_prompt=neg, sag=SAG)
    dev = sd.generate_image(P, **kw)
    eng = next(iter(sd._engines.values()))
    assert eng.passes == [(0, 2, 154, "uncond"), (2, 2, 77, "cond")] and eng.eps.shape[0] == 10
    names = [c.name for c in eng.calls]
    assert names.count("conv_in") == 3 and names.index("sag.degrade") < [i for i, n in enumerate(names) if n == "conv_in"][2]
    host = sd.generate_image(P, host_loop=True, **kw)
    p = O.psnr(dev, host)
    print(f"SAG, 154 unconditional tokens: device loop vs host loop {p:.1f} dB")
    assert p >= HOST_PSNR_MIN


def test_a_sample_does_not_depend_on_its_batch(gpu, nets):
    """The same sample in a batch of 1 and as row 0 / row 1 of a batch of 2: the same bits; the whole-loop graph, the per-step
    graphs and another scale on the resident engine."""
    sd, P = _pipe(gpu, nets)
    lat = np.random.default_rng(5).standard_normal((2, 16, 16, 4)).astype(np.float32)
    kw = dict(num_steps=3, guidance_rescale=0.7, return_latent=True, sag=SAG)
    two = sd.generate_image(P, batch_size=2, diffusion_noise=lat, **kw)
    for b in range(2):
        one = sd.generate_image(P, batch_size=1, diffusion_noise=lat[b:b + 1], **kw)
        np.testing.assert_array_equal(one[0], two[b])
    eng = next(iter(sd._engines.values()))
    calls = []
    stepped = sd.generate_image(P, batch_size=1, diffusion_noise=lat[1:], callback=calls.append, **kw)
    assert calls == [1, 2, 3] and eng._loop_graph is not None and eng._step_graph is not None
    np.testing.assert_array_equal(stepped[0], two[1])
    other = sd.generate_image(P, batch_size=1, diffusion_noise=lat[1:], **{**kw, "sag": dict(SAG, scale=1.0, blur_sigma=2.0)})
    assert next(iter(sd._engines.values())) is eng and len(sd._engines) == 1 and not np.array_equal(other[0], two[1])


def test_sharded_sag_equals_unsharded(gpu):
    """A one-rank process group with forced collectives (as tests/test_pag_gpu.py): the sharded SAG job == the unsharded one."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(HERE, "_sag_world1_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=570)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert any(line.startswith("OK ") for line in p.stdout.splitlines()), p.stdout[-2000:]
    print(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("size", [128, 256])
def test_sag_vs_oracle_fixture(gpu, nets, size):
    """The fixture jobs against the fp32 oracle's composition (tools/make_sag_fixtures.py: unet_forward with the mid block's
    probabilities captured, diffusers' sag_masking, a second unet_forward, the float64 formula): final latent PSNR >= 40 dB, where
    the same job WITHOUT SAG stays under 35 dB (`plain_psnr` in the file) and no map entry of any step lies within 8 x the colsum
    bound of the threshold (`margin`)."""
    from oracle import sd_oracle as O

    g = np.load(os.path.join(GOLD, f"sag_{size}.npz"))
    assert (int(g["weight_seed"]), float(g["bias_scale"])) == (0, 0.05) and float(g["plain_psnr"]) < 35.0
    assert float(g["margin"]) >= 8.0 * MARGIN * parity()["colsum_max_rel_err"]
    sd, _P = _pipe(gpu, nets, size)
    rng = np.random.default_rng(int(g["context_seed"]))
    ctx = (rng.standard_normal((1, 77, 768)) * float(g["context_scale"])).astype(np.float32)[0]
    sd.unconditional_context = (rng.standard_normal((1, 77, 768)) * float(g["context_scale"])).astype(np.float32)[0]
    got = sd.generate_image(ctx, batch_size=1, num_steps=int(g["steps"]), unconditional_guidance_scale=float(g["guidance"]),
                            seed=int(g["noise_seed"]), guidance_rescale=0.0, return_latent=True,
                            sag=dict(scale=float(g["scale"]), blur_sigma=float(g["blur_sigma"]), threshold=float(g["threshold"])))
    p = O.psnr(got, g["latent"])
    print(f"SAG fixture {size}x{size} (scale {float(g['scale'])}): final latent PSNR {p:.1f} dB; the plain job: {float(g['plain_psnr']):.1f} dB; "
          f"map margin {float(g['margin']):.2e}")
    assert p >= PSNR_MIN
