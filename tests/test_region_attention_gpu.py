"""msd_region_attention on the GPU: the kernel against an fp32 / float64 reference between guard bands, its bit-for-bit promises
(the zero-weight rule, the workgroup skip, batch independence), and the attention-mode regional job through the pipeline."""
import math

import numpy as np
import pytest
import torch

import _extents_region_attention as XR
import _guard as G
from _checks import bf, close
from conftest import run_calls

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAN = float("nan")
LOG2E = 1.4426950408889634


def guarded(dev, q, k, v, w, *, H, d, q_ld=None, vt_ld=None, o_ld=None, w_ld=None, poison=True):
    """The operands of one launch between guard bands, sized by the header's extents: q [B, S, C] as rows of a q_ld-wide buffer,
    k / v [R B, T, C] region-major (v stored transposed, vt_ld >= T columns), w [R, S] as rows of w_ld, out [B, S, C] as rows of
    o_ld.  The padding - V^T's columns [T, vt_ld), the q buffer outside the head block, w's columns [S, w_ld) - holds NaN (poison)
    or zeros; out's unused columns hold a canary.  Returns (guard, keyword arguments of ops.region_attention, out)."""
    B, S, C = q.shape
    RB, T, _ = k.shape
    R = w.shape[0]
    assert C == H * d and RB == R * B and w.shape[1] == S
    q_ld, o_ld, w_ld = q_ld or C, o_ld or C, w_ld or S
    vt_ld = vt_ld or (T + 7) // 8 * 8
    geo = dict(batch=B, heads=H, head_dim=d, s=S, t=T, regions=R, q_ld=q_ld, k_ld=C, vt_ld=vt_ld, w_ld=w_ld, o_ld=o_ld)
    g = G.Guard(dev, XR.region_attention(q=1, k=1, vt=1, w=1, out=1, **geo))
    pad = None if poison else 0.0
    qd = g.inp(q.to(BF16).reshape(B * S, C), "q", ld=q_ld if q_ld > C else None, gap=pad)
    kd = g.inp(k.to(BF16), "k")
    vt = g.out((RB, C, vt_ld), BF16, 0.0, "vt")
    vt[:, :, :T] = v.permute(0, 2, 1).to(BF16).to(dev)
    g.operands[-1].role = "in"
    g.gaps(vt, T, gap=pad)
    wd = g.inp(w.to(torch.float32), "w", ld=w_ld if w_ld > S else None, gap=pad)
    out = g.out((B * S, C), BF16, NAN, "out", ld=o_ld if o_ld > C else None)
    return g, dict(q=qd, k=kd, vt=vt, w=wd, out=out, **geo), out


def launch(dev, q, k, v, w, **kw):
    from minsdtf_amd import ops

    g, args, out = guarded(dev, q, k, v, w, **kw)
    run_calls(ops.region_attention(**args))
    g.check()
    B, S, C = q.shape
    return out.reshape(B, S, C).clone()


def per_region(q, k, v, H, d, R):
    """fp32 torch attention of every region on the bf16-rounded inputs: [R, B, S, C] (q carries scale * log2(e))."""
    B, S, C = q.shape
    T = k.shape[1]
    qh = q.view(B, S, H, d).permute(0, 2, 1, 3)
    outs = []
    for r in range(R):
        kh = k[r * B:(r + 1) * B].view(B, T, H, d).permute(0, 2, 1, 3)
        vh = v[r * B:(r + 1) * B].view(B, T, H, d).permute(0, 2, 1, 3)
        outs.append((torch.softmax((qh @ kh.transpose(-1, -2)) * math.log(2.0), -1) @ vh).permute(0, 2, 1, 3).reshape(B, S, C))
    return torch.stack(outs)


def reference(q, k, v, w, H, d):
    """The per-region fp32 attentions combined in float64."""
    R = w.shape[0]
    o = per_region(q, k, v, H, d, R).double()
    return (w.double()[:, None, :, None] * o).sum(0).float()


def operands(seed, B, H, d, S, T, R, spike=False):
    gen = torch.Generator().manual_seed(seed)
    C = H * d
    q = bf(torch.randn(B, S, C, generator=gen) * (d ** -0.5 * LOG2E))
    k, v = bf(torch.randn(R * B, T, C, generator=gen)), bf(torch.randn(R * B, T, C, generator=gen))
    if spike:
        k[:, T // 2] *= 8.0
        k = bf(k)
    return q, k, v


def soft_weights(seed, R, S):
    """Normalised in float64 and rounded once, like regions.level_weights; with stretches of exact zeros: region R - 1 is absent
    from the first 64 queries (a whole workgroup skips it), region 0 from queries [100, 140) (part of a workgroup)."""
    rng = np.random.default_rng(seed)
    m = rng.random((R, S)) + 0.05
    if R > 1:
        m[R - 1, :64] = 0.0
        m[0, 100:140] = 0.0
    return torch.from_numpy((m / m.sum(0)[None]).astype(np.float32))


KERNEL_CASES = [
    dict(B=2, H=2, d=40, S=200, T=77, R=3),                 # ragged query tile
    dict(B=1, H=2, d=80, S=128, T=96, R=2),                 # the largest context
    dict(B=3, H=1, d=160, S=64, T=13, R=16, spike=True),    # every region the ABI takes, one dominant key
    dict(B=1, H=8, d=160, S=1, T=77, R=1),                  # the one-token mid block
]


@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "-".join(f"{k}{int(v)}" for k, v in c.items()))
def test_kernel_against_reference(gpu, case):
    """A convex combination of attentions that each meet test_attention's bound (P rounded to bf16 before the PV product), so
    the same bound: rtol 2e-2, atol 1.5e-2 max(1, max|ref|).  The padding (V^T's columns >= T, the 3C-wide q buffer, w's and
    out's spare columns) holds NaN, then zeros: the same bits."""
    B, H, d, S, T, R = (case[x] for x in "BHdSTR")
    C = H * d
    q, k, v = operands(11, B, H, d, S, T, R, case.get("spike", False))
    w = soft_weights(5, R, S)
    ref = reference(q, k, v, w, H, d)
    wide = dict(H=H, d=d, q_ld=3 * C, vt_ld=(T + 7) // 8 * 8 + 8, o_ld=C + 16, w_ld=S + 3)
    a = launch(gpu, q, k, v, w, poison=True, **wide)
    b = launch(gpu, q, k, v, w, poison=False, **wide)
    close(a, ref, rtol=2e-2, atol=1.5e-2 * max(1.0, float(ref.abs().max())), what=str(case))
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{case}: the content of a padding region reached the result"
    # the project's float64 statement of the kernel says the same
    from minsdtf_amd import regions

    ref64 = regions.attention_reference(q.numpy(), k.numpy(), v.numpy(), w.numpy(), H)
    close(a, torch.from_numpy(ref64).float(), rtol=2e-2, atol=1.5e-2 * max(1.0, float(np.abs(ref64).max())), what=f"{case} float64")


def test_one_region_queries_take_that_regions_attention(gpu):
    """Two complementary 0/1 planes whose border (query 37) lies inside a workgroup: every query equals the R = 1, w = 1 launch of
    its region, bit for bit."""
    B, H, d, S, T = 2, 2, 40, 200, 77
    q, k, v = operands(3, B, H, d, S, T, 2)
    w = torch.zeros(2, S)
    w[0, :37] = 1.0
    w[1, 37:] = 1.0
    got = launch(gpu, q, k, v, w, H=H, d=d)
    one = torch.ones(1, S)
    r0 = launch(gpu, q, k[:B], v[:B], one, H=H, d=d)
    r1 = launch(gpu, q, k[B:], v[B:], one, H=H, d=d)
    assert torch.equal(got[:, :37].view(torch.int16), r0[:, :37].view(torch.int16))
    assert torch.equal(got[:, 37:].view(torch.int16), r1[:, 37:].view(torch.int16))
    assert not torch.equal(r0.view(torch.int16), r1.view(torch.int16))


def test_region_of_weight_zero_may_hold_nan(gpu):
    """A third region that is nowhere positive, its K / V all NaN: the output is the two-region launch's, bit for bit."""
    B, H, d, S, T = 1, 2, 80, 150, 77
    q, k, v = operands(4, B, H, d, S, T, 2)
    w2 = soft_weights(9, 2, S)
    two = launch(gpu, q, k, v, w2, H=H, d=d)
    nan = torch.full((B, T, H * d), NAN)
    # (the dead region in the middle: the regions after it still accumulate)
    k3, v3 = torch.cat([k[:B], nan, k[B:]]), torch.cat([v[:B], nan, v[B:]])
    w3 = torch.stack([w2[0], torch.zeros(S), w2[1]])
    three = launch(gpu, q, k3, v3, w3, H=H, d=d)
    assert bool(torch.isfinite(three.float()).all())
    assert torch.equal(two.view(torch.int16), three.view(torch.int16))


def test_sample_bits_do_not_depend_on_the_batch_and_runs_repeat(gpu):
    B, H, d, S, T, R = 3, 2, 160, 100, 50, 3
    q, k, v = operands(6, B, H, d, S, T, R)
    w = soft_weights(2, R, S)
    full = launch(gpu, q, k, v, w, H=H, d=d)
    again = launch(gpu, q, k, v, w, H=H, d=d)
    assert torch.equal(full.view(torch.int16), again.view(torch.int16))
    for b in range(B):
        rows = [r * B + b for r in range(R)]
        alone = launch(gpu, q[b:b + 1], k[rows], v[rows], w, H=H, d=d)
        assert torch.equal(alone[0].view(torch.int16), full[b].view(torch.int16)), f"sample {b}"


@pytest.mark.parametrize("d,S,T", [(40, 200, 77), (80, 128, 96), (160, 64, 13)])
def test_one_region_against_msd_attention(gpu, d, S, T):
    """R = 1, w = 1 is a plain cross-attention: within the attention bound of the msd_attention launch it replaces (the two
    kernels tile and normalise differently: bit equality is not asked)."""
    from minsdtf_amd import ops

    B, H = 2, 2
    C = H * d
    q, k, v = operands(8, B, H, d, S, T, 1)
    got = launch(gpu, q, k, v, torch.ones(1, S), H=H, d=d)
    Tp = (T + 7) // 8 * 8
    qd, kd = q.to(BF16).to(gpu), k.to(BF16).to(gpu)
    vt = torch.zeros(B, C, Tp, dtype=BF16, device=gpu)
    vt[:, :, :T] = v.permute(0, 2, 1).to(BF16).to(gpu)
    out = torch.empty(B, S, C, dtype=BF16, device=gpu)
    run_calls(ops.attention(q=qd, k=kd, vt=vt, out=out, batch=B, heads=H, head_dim=d, s=S, t=T, q_ld=C, k_ld=C, vt_ld=Tp, o_ld=C,
                            scale=1.0, q_prescaled=True))
    ref = out.float().cpu()
    close(got, ref, rtol=2e-2, atol=1.5e-2 * max(1.0, float(ref.abs().max())), what=f"d={d}")


# ---------------------------------------------------------------------------------------------------------------- pipelines
PSNR_MIN = 40.0        # the project's bar for every job
SAMPLER_PSNR_MIN = 45.0   # ... for a samplers.py sampler's txt2img job against another route (test_samplers_gpu.py)


@pytest.fixture(scope="module")
def nets(gpu):
    from minsdtf_amd.models import DiffusionModel, ImageDecoder

    unet = DiffusionModel(64, 64, device=gpu)
    unet.load_synthetic(seed=0, bias_scale=0.05)
    dec = ImageDecoder(device=gpu)
    dec.load_synthetic(seed=0, bias_scale=0.05)
    return {"unet": unet, "dec": dec}


def _pipe(gpu, nets, jit=True):
    """(pipeline, four contexts P, Q, S, T)"""
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sd = StableDiffusion(64, 64, jit_compile=jit, device=gpu)
    sd._diffusion_model = nets["unet"]
    sd._image_decoder = nets["dec"]
    rng = np.random.default_rng(41)
    sd.unconditional_context = rng.standard_normal((77, 768)).astype(np.float32)
    return sd, [rng.standard_normal((77, 768)).astype(np.float32) for _ in range(4)]


def _halves():
    from minsdtf_amd import regions

    return regions.boxes(8, 8, 1, 2)


def _job(prompts, masks, weights=None, base_weight=0.0, mode="attention"):
    weights = weights or [1.0] * len(prompts)
    return dict(regions=[dict(prompt=p, mask=m, weight=v) for p, m, v in zip(prompts, masks, weights)], base_weight=base_weight, mode=mode)


def _soft_masks():
    y, x = np.mgrid[0:64, 0:64] / 63.0
    return [1.0 - x, x, np.exp(-((x - 0.5) ** 2 + (y - 0.5) ** 2) / 0.08) + 0.05]


def _names(eng):
    return [c.name for c in eng.calls]


def test_one_prompt_in_two_halves_equals_one_full_region(gpu, nets):
    """Binary halves give exactly 0 / 1 at levels 0 to 2 (each query copies one of two identical attentions) and 0.5 / 0.5 at the
    1 x 1 level, where 0.5 O + fma(0.5, O, .) is O exactly: the bits of the one-region job.  The UNet runs the plain job's rows."""
    sd, (P, Q, _S, _T) = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=3, seed=6, guidance_rescale=0.7, return_latent=True)
    two = sd.generate_image(Q, regions=_job([P, P], _halves()), **kw)
    eng = next(iter(sd._engines.values()))
    assert eng.regions == 2 and eng.region_attn and eng.eps.shape[0] == 4 and eng.passes == [(0, 4, 77, "both")]
    names = _names(eng)
    assert sum(n.endswith(".attn2.regions") for n in names) == 16 and "region_combine" not in names
    one = sd.generate_image(Q, regions=_job([P], [np.ones((8, 8))]), **kw)
    np.testing.assert_array_equal(two, one)
    assert np.all(np.isfinite(two))


@pytest.mark.parametrize("sampler", [None, "dpmpp_2m"])
def test_one_full_region_against_the_plain_job(gpu, nets, sampler):
    """One full-mask region is the plain job on another attn2 route (to_q + msd_region_attention instead of the fused launch):
    the project's bars, 40 dB, or 45 dB with a samplers.py sampler."""
    from oracle import sd_oracle as O

    sd, (P, Q, _S, _T) = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=4, seed=6, guidance_rescale=0.7, return_latent=True, sampler=sampler)
    plain = sd.generate_image(P, **kw)
    got = sd.generate_image(Q, regions=_job([P], [np.ones((8, 8))]), **kw)
    p = O.psnr(got, plain)
    bar = SAMPLER_PSNR_MIN if sampler else PSNR_MIN
    print(f"attention-mode job, one full region vs the plain job ({sampler or 'default sampler'}): {p:.1f} dB (bar {bar:.0f})")
    assert p >= bar


def test_masks_route_the_prompts(gpu, nets):
    sd, (P, Q, _S, _T) = _pipe(gpu, nets)
    left, right = _halves()
    kw = dict(batch_size=1, num_steps=3, seed=3, guidance_rescale=0.7, return_latent=True)
    got = sd.generate_image(P, regions=_job([P, Q], [left, right]), **kw)
    assert np.all(np.isfinite(got))
    assert not np.array_equal(got, sd.generate_image(P, regions=_job([P, Q], [right, left]), **kw))
    assert not np.array_equal(got, sd.generate_image(P, **kw))


def test_graph_forms_agree(gpu, nets):
    """The whole-loop graph == per-step graphs (a callback is installed) == eager launches (jit_compile=False), bit for bit."""
    sd, (P, Q, S, T) = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=3, seed=8, return_latent=True, sampler="dpmpp_2m", guidance_rescale=0.7,
              regions=_job([P, Q, S], _soft_masks(), [1.0, 2.0, 0.5], 0.3))
    whole = sd.generate_image(T, **kw)
    calls = []
    stepped = sd.generate_image(T, callback=calls.append, **kw)
    assert calls == [1, 2, 3]
    eng = next(iter(sd._engines.values()))
    assert eng._loop_graph is not None and eng._step_graph is not None and eng.regions == 4
    eager_sd, _ = _pipe(gpu, nets, jit=False)
    np.testing.assert_array_equal(stepped, whole)
    np.testing.assert_array_equal(eager_sd.generate_image(T, **kw), whole)
    assert np.all(np.isfinite(whole))


def test_residency(gpu, nets, monkeypatch):
    """Other masks, weights and prompts with the same number of regions build no engine and capture no graph."""
    import minsdtf_amd.stable_diffusion as sdm

    built = []
    init = sdm.DenoiseEngine.__init__

    def counting(self, *a, **k):
        built.append((a[1], k.get("regions"), k.get("region_mode")))
        init(self, *a, **k)

    monkeypatch.setattr(sdm.DenoiseEngine, "__init__", counting)
    sd, (P, Q, S, T) = _pipe(gpu, nets)
    kw = dict(batch_size=1, num_steps=3, seed=5, guidance_rescale=0.7, return_latent=True)
    left, right = _halves()
    soft = _soft_masks()
    first = sd.generate_image(P, regions=_job([P, Q], [left, right]), **kw)
    assert built == [(1, 2, "attention")]
    eng = next(iter(sd._engines.values()))
    graph = eng._loop_graph
    other = _job([S, T], soft[:2], [0.5, 3.0])
    second = sd.generate_image(P, regions=other, **kw)
    assert len(built) == 1 and next(iter(sd._engines.values())) is eng and eng._loop_graph is graph
    assert not np.array_equal(first, second)
    fresh, _ = _pipe(gpu, nets)
    np.testing.assert_array_equal(second, fresh.generate_image(P, regions=other, **kw))
    # the same regions in latent mode are another engine
    sd.generate_image(P, regions=dict(other, mode="latent"), **kw)
    assert built[-1] == (1, 2, "latent")


def test_unconditional_context_of_another_length(gpu, nets):
    """154 unconditional tokens: B unconditional rows on msd_attention alone, then B conditional rows on the R region contexts."""
    sd, (P, Q, S, T) = _pipe(gpu, nets)
    neg = np.random.default_rng(5).standard_normal((154, 768)).astype(np.float32)
    kw = dict(batch_size=2, num_steps=3, seed=11, return_latent=True, guidance_rescale=0.7,
              regions=_job([P, Q, S], _soft_masks(), [1.0, 2.0, 0.5], 0.3))
    got = sd.generate_image(T, negative_prompt=neg, **kw)
    eng = next(iter(sd._engines.values()))
    assert eng.passes == [(0, 2, 154, "uncond"), (2, 2, 77, "cond")] and eng.eps.shape[0] == 4
    assert eng.ctx_in["uncond"].shape[0] == 2 and eng.ctx_in["cond"].shape[0] == 8
    assert np.all(np.isfinite(got)) and not np.array_equal(got, sd.generate_image(T, **kw))


def test_sixteen_regions(gpu, nets):
    """R = 16 at batch 1: 2 UNet rows; latent mode refuses the same job (17 rows)."""
    from minsdtf_amd import regions

    sd, ctxs = _pipe(gpu, nets)
    masks = regions.boxes(8, 8, 4, 4)
    prompts = [ctxs[i % 4] * (1.0 + 0.1 * (i // 4)) for i in range(16)]
    kw = dict(batch_size=1, num_steps=2, seed=1, guidance_rescale=0.7, return_latent=True)
    got = sd.generate_image(ctxs[0], regions=_job(prompts, masks), **kw)
    eng = next(iter(sd._engines.values()))
    assert eng.regions == 16 and eng.eps.shape[0] == 2 and np.all(np.isfinite(got))
    with pytest.raises(ValueError, match="MAX_VIEW_BATCH"):
        sd.generate_image(ctxs[0], regions=_job(prompts, masks, mode="latent"), **kw)


@pytest.mark.parametrize("sampler", [None, "dpmpp_2m"])
def test_device_loop_vs_host_loop(gpu, nets, sampler):
    """The device loop against host_loop=True (DiffusionModel.predict_regional through _guided_eps): 40 dB, or 45 dB with a
    samplers.py sampler - the bars test_regions_gpu.py holds latent mode's two routes to."""
    from oracle import sd_oracle as O

    sd, (P, Q, S, T) = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=4, seed=11, return_latent=True, sampler=sampler, guidance_rescale=0.7,
              regions=_job([P, Q, S], _soft_masks(), [1.0, 2.0, 0.5], 0.3))
    calls_d, calls_h = [], []
    dev = sd.generate_image(T, callback=calls_d.append, **kw)
    host = sd.generate_image(T, host_loop=True, callback=calls_h.append, **kw)
    assert calls_d == calls_h == [1, 2, 3, 4]
    p = O.psnr(dev, host)
    bar = SAMPLER_PSNR_MIN if sampler else PSNR_MIN
    print(f"attention-mode job ({sampler or 'default sampler'}): device loop vs host loop {p:.1f} dB (bar {bar:.0f})")
    assert p >= bar


def test_predict_regional_one_region_is_predict_on_batch(gpu, nets):
    """One region of weight 1 everywhere against predict_on_batch (the fused attn2 route): 40 dB on the prediction."""
    from minsdtf_amd import engine
    from oracle import sd_oracle as O

    unet = nets["unet"]
    rng = np.random.default_rng(2)
    lat = rng.standard_normal((2, 8, 8, 4)).astype(np.float32)
    temb = O.timestep_embedding(500, 2)
    ctx = rng.standard_normal((2, 77, 768)).astype(np.float32)
    planes = [np.ones((1,) + lv, dtype=np.float32) for lv in engine.unet_levels(8, 8)]
    got = unet.predict_regional([lat, temb], [ctx], planes)
    ref = unet.predict_on_batch([lat, temb, ctx])
    assert O.psnr(got, ref) >= PSNR_MIN
    with pytest.raises(ValueError):
        unet.predict_regional([lat, temb], [ctx], planes[:3])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_against_the_oracle_fixture(gpu, nets, tag):
    """tests/golden/oracle_region_attention_{a,b}.npz (tools/make_region_attention_fixtures.py): final latent PSNR >= 40 dB on the
    whole batch and on each sample; the fixture's plain job is below 30 dB, so the bar tells the feature from its absence."""
    import os

    from minsdtf_amd.models import DiffusionModel
    from minsdtf_amd.stable_diffusion import StableDiffusion
    from oracle import sd_oracle as O

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"oracle_region_attention_{tag}.npz"))
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
    scale = float(g["context_scale"])
    prompts = [(scale * rng.standard_normal((1, 77, 768))).astype(np.float32)[0] for _ in g["masks"]]
    job = _job(prompts, list(g["masks"]), [float(v) for v in g["region_weights"]], float(g["base_weight"]))
    got = sd.generate_image(base, batch_size=B, num_steps=int(g["steps"]), unconditional_guidance_scale=float(g["guidance"]),
                            seed=int(g["noise_seed"]), guidance_rescale=float(g["guidance_rescale"]), return_latent=True,
                            sampler=str(g["sampler"]) or None, regions=job)
    eng = next(iter(sd._engines.values()))
    assert eng.region_attn and eng.regions == len(prompts) + (1 if float(g["base_weight"]) > 0 else 0)
    p = O.psnr(got, g["latent"])
    per = [round(O.psnr(got[b], g["latent"][b]), 1) for b in range(B)]
    print(f"attention-mode job {tag}: final latent PSNR {p:.1f} dB (per sample {per}); the plain job is at {float(g['plain_psnr']):.1f} dB")
    assert p >= PSNR_MIN and min(per) >= PSNR_MIN


def test_sharded_job_equals_unsharded(gpu):
    """A one-rank process group with forced collectives (as tests/test_regions_gpu.py): the sharded attention-mode job == the
    unsharded one.  (A child process is what the test is about: the group must exist before anything touches the GPU.)"""
    import os
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(here, "_region_attention_world1_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=570)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert any(line.startswith("OK ") for line in p.stdout.splitlines()), p.stdout[-2000:]
    print(p.stdout.strip().splitlines()[-1])
