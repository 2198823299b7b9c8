"""The multistep / ancestral samplers on the device: msd_sampler_step against a float64 restatement, the three full-size fixture
jobs against the fp32 oracle (tests/golden/oracle_sampler_*.npz, tools/make_sampler_fixtures.py), the run modes (whole-loop
graph, per-step graph, eager, two streams), batch independence of the draws, and the device loop against host_loop=True."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
PSNR_MIN = 40.0
# device loop vs host_loop=True (fp32 device steps against float64 host steps, both over the device UNet): this bound was not
# measured before the tests were written; it was set from their first run on an MI355X, 8 steps of dpmpp_2m_karras at 64x64:
# txt2img 52.4 dB, img2img 50.3, inpaint 54.0.  ControlNet measured 44.2: its host loop takes the 13 residuals across the model
# boundary in fp32 (DiffusionModel.predict_on_batch), the device loop adds them in the zero convs' epilogue, so the two routes
# differ by more than the sampler step; that case is held to 40 dB (the ControlNet device-vs-oracle bar of test_configs_gpu.py)
# and to within 3 dB of the default sampler's own device-vs-host figure on the same inputs
HOST_PSNR_MIN = 45.0
HOST_PSNR_MIN_CONTROLNET = 40.0


def run_calls(calls):
    if not isinstance(calls, (list, tuple)):
        calls = [calls]
    st = torch.cuda.current_stream().cuda_stream
    for c in calls:
        c(st)
    torch.cuda.synchronize()


def _rows(name, steps, start=0):
    from minsdtf_amd import samplers
    from minsdtf_amd.scheduler import Scheduler

    sch = Scheduler()
    sch.set_timesteps(steps)
    sc = samplers.schedule(samplers.parse(name), sch, steps)
    return samplers.rows(sc, start)


@pytest.mark.parametrize("extra", ["plain", "inpaint_noise"])
@pytest.mark.parametrize("guidance,rescale", [(7.5, 0.7), (7.5, 0.0), (0.0, 0.0)])
@pytest.mark.parametrize("advance", [2, 1])
@pytest.mark.parametrize("hw", [8, 64, 96, 100])   # the 8x8 / 64x64 / 96x96 register forms' sizes and the re-reading loop (100x100)
def test_sampler_step(gpu, extra, guidance, rescale, advance, hw):
    """CFG + rescale + the general linear update, every step of a 5-step run at batch 3, against float64 numpy: the latent,
    P (= D after every step), the step counter.  P starts as NaN: the first row must not read it.  "plain": DPM++ 2M (c_P, no
    draws); "inpaint_noise": DPM++ 2M SDE on Karras sigmas with per-step draws and the inpaint blend."""
    from minsdtf_amd import ops
    from oracle import sd_oracle as O

    rng = np.random.default_rng(19)
    B, n, steps = 3, hw * hw * 4, 5
    name = "dpmpp_2m" if extra == "plain" else "dpmpp_2m_sde_karras"
    import _extents as X
    import _guard as G

    tab = _rows(name, steps)
    geo = dict(batch=B, n=n, num_steps=steps, guidance=guidance, guidance_rescale=rescale, advance=advance)
    more = dict(step_noise=1, inpaint_init=1, inpaint_noise=1, inpaint_mask=1) if extra != "plain" else {}
    g = G.Guard(gpu, X.sampler_step(eps=1, latent=1, coef=1, step_ptr=1, denoised_prev=1, **more, **geo))   # every operand between guard bands
    coef = g.inp(torch.from_numpy(tab.astype(np.float32)), "coef")
    lat = rng.standard_normal((B, n)).astype(np.float32)
    lat_d = g.inp(torch.from_numpy(lat.copy()), "latent")
    prev_d = g.out((B, n), torch.float32, float("nan"), "denoised_prev")
    step = g.inp(torch.zeros(2 if advance == 2 else 1, dtype=torch.int32), "step_ptr")   # {step, ticket}: the ticket only with advance = 2
    kw = {}
    z = ip_init = ip_noise = ip_mask = None
    if extra != "plain":
        z = rng.standard_normal((steps, B, n)).astype(np.float32)
        ip_init = rng.standard_normal(n).astype(np.float32)
        ip_noise = rng.standard_normal((B, n)).astype(np.float32)
        ip_mask = np.repeat((rng.random((hw * hw, 1)) > 0.4).astype(np.float32), 4, axis=1).reshape(-1)
        kw = dict(step_noise=g.inp(torch.from_numpy(z), "step_noise"), inpaint_init=g.inp(torch.from_numpy(ip_init), "inpaint_init"),
                  inpaint_noise=g.inp(torch.from_numpy(ip_noise), "inpaint_noise"), inpaint_mask=g.inp(torch.from_numpy(ip_mask), "inpaint_mask"))
    ref, P = lat.astype(np.float64), None
    for i in range(steps):
        u = rng.standard_normal((B, n)).astype(np.float32)
        c = (u + 0.3 * rng.standard_normal((B, n))).astype(np.float32)
        if guidance > 0:
            e = u + guidance * (c - u)
            if rescale > 0:
                e = O.rescale_noise_cfg(e, c, rescale)
            eps_d = g.inp(torch.from_numpy(np.concatenate([u, c])), "eps", label=f"eps of step {i}")
        else:
            e = c
            eps_d = g.inp(torch.from_numpy(c), "eps", label=f"eps of step {i}")
        a, s, cx, cd, cp, cz = tab[i, :6].astype(np.float32).astype(np.float64)
        D = (ref - s * e) / a
        x = cx * ref + cd * D + (cp * P if cp != 0 else 0.0) + (cz * z[i] if z is not None else 0.0)
        if ip_mask is not None:
            org = a * ip_init[None] + s * ip_noise
            x = org * (1.0 - ip_mask[None]) + x * ip_mask[None]
        ref, P = x, D
        run_calls(ops.sampler_step(eps=eps_d, latent=lat_d, coef=coef, step_ptr=step, denoised_prev=prev_d, **geo, **kw))
        got = lat_d.cpu().numpy()
        np.testing.assert_allclose(got, ref, rtol=2e-4, atol=2e-4 * np.abs(ref).max(), err_msg=f"step {i}")
        np.testing.assert_allclose(prev_d.cpu().numpy(), D, rtol=2e-4, atol=2e-4 * np.abs(D).max(), err_msg=f"P after step {i}")
        assert step.tolist() == [i + 1, 0][:step.numel()]
    g.check()


def test_sampler_step_argument_errors(gpu):
    """Bad calls return MSD_E_ARG and launch nothing (the latent and the counter stay as they were)."""
    from minsdtf_amd import _lib, ops

    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    B, n = 2, 64
    eps = torch.zeros(2 * B, n, device=gpu)
    lat = torch.ones(B, n, device=gpu)
    coef = torch.from_numpy(_rows("euler_a", 3).astype(np.float32)).to(gpu)
    prev = torch.zeros(B, n, device=gpu)
    step = torch.zeros(2, dtype=torch.int32, device=gpu)
    good = dict(eps=eps, latent=lat, coef=coef, step_ptr=step, denoised_prev=prev, batch=B, n=n, num_steps=3, guidance=7.5,
                guidance_rescale=0.7, advance=2)
    bad = [dict(denoised_prev=None), dict(coef=None), dict(eps=None), dict(batch=0), dict(n=0), dict(num_steps=0),
           dict(advance=3), dict(advance=-1), dict(step_ptr=None), dict(inpaint_mask=prev)]
    for b in bad:
        c = ops.sampler_step(**{**good, **b})
        assert c.fn(*c.args, st) == -1, b
    torch.cuda.synchronize()
    assert torch.equal(lat, torch.ones(B, n, device=gpu)) and step.tolist() == [0, 0]
    run_calls(ops.sampler_step(**good))
    assert step.tolist() == [1, 0]


@pytest.fixture(scope="module")
def nets(gpu):
    from minsdtf_amd.models import ControlNet, DiffusionModel, HintNet, ImageEncoder

    out = {}
    out["unet"] = DiffusionModel(64, 64, device=gpu)
    out["unet"].load_synthetic(seed=0, bias_scale=0.05)
    out["cn"] = ControlNet(64, 64, device=gpu)
    out["cn"].load_synthetic(seed=0, bias_scale=0.05)
    out["hn"] = HintNet(64, 64, device=gpu)
    out["hn"].load_synthetic(seed=0, bias_scale=0.05)
    out["enc"] = ImageEncoder(device=gpu)
    out["enc"].load_synthetic(seed=0, bias_scale=0.05)
    return out


def _pipe(gpu, nets, control=False, jit=True, tcd=False):
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sd = StableDiffusion(64, 64, jit_compile=jit, device=gpu, controlnet_path="synthetic" if control else None, active_tcd=tcd)
    sd._diffusion_model, sd._image_encoder = nets["unet"], nets["enc"]
    if control:
        sd._control_net, sd._hint_net = nets["cn"], nets["hn"]
    rng = np.random.default_rng(41)
    sd.unconditional_context = rng.standard_normal((77, 768)).astype(np.float32)
    return sd, rng.standard_normal((77, 768)).astype(np.float32)


@pytest.mark.parametrize("name", ["dpmpp_2m_karras", "dpmpp_2m_sde_karras", "euler_a"])
def test_sampler_vs_oracle_fixture(gpu, name):
    """512x512, batch 1, CFG 7.5 / rescale 0.7, seed 0, against the fp32 oracle's own sigma-space loop: final latent >= 40 dB;
    the per-step curve (stride-2 grid) is printed."""
    from minsdtf_amd.stable_diffusion import StableDiffusion
    from oracle import sd_oracle as O

    steps = {"dpmpp_2m_karras": 20, "dpmpp_2m_sde_karras": 10, "euler_a": 10}[name]
    g = np.load(os.path.join(GOLD, f"oracle_sampler_{name}_{steps}.npz"))
    assert str(g["sampler"]) == name and int(g["steps"]) == steps
    sd = StableDiffusion(512, 512, jit_compile=True, device=gpu)
    sd.diffusion_model.load_synthetic(seed=int(g["weight_seed"]))
    rng = np.random.default_rng(int(g["context_seed"]))
    ctx = rng.standard_normal((1, 77, 768)).astype(np.float32)
    unc = rng.standard_normal((1, 77, 768)).astype(np.float32)
    sd.unconditional_context = unc[0]
    snaps = {}
    box = {}
    orig = sd._engine

    def _engine(*a, **k):
        box["eng"] = orig(*a, **k)
        return box["eng"]

    sd._engine = _engine
    got = sd.generate_image(ctx[0], batch_size=1, num_steps=steps, unconditional_guidance_scale=float(g["guidance"]), seed=0,
                            guidance_rescale=float(g["guidance_rescale"]), return_latent=True, sampler=name,
                            callback=lambda i: snaps.__setitem__(i - 1, box["eng"].latent.cpu().numpy()))
    p = O.psnr(got, g["latent"])
    curve = [round(O.psnr(snaps[i][:, ::2, ::2, :], g["trace"][i]), 1) for i in range(steps)]
    print(f"{name} x {steps} at 512x512: final-latent PSNR {p:.1f} dB; per-step {curve}")
    assert p >= PSNR_MIN
    whole = sd.generate_image(ctx[0], batch_size=1, num_steps=steps, unconditional_guidance_scale=float(g["guidance"]), seed=0,
                              guidance_rescale=float(g["guidance_rescale"]), return_latent=True, sampler=name)
    np.testing.assert_array_equal(whole, got)   # whole-loop graph == per-step graph


@pytest.mark.parametrize("name", ["dpmpp_2m_sde_karras", "dpmpp_2m", "euler_a_karras"])
def test_run_modes_are_bit_identical(gpu, nets, name):
    """Whole-loop graph, per-step graph (callback), eager and a repeat give the same bits; two streams agree to rounding."""
    kw = dict(batch_size=2, num_steps=6, seed=3, sampler=name, guidance_rescale=0.7, return_latent=True)
    sd, ctx = _pipe(gpu, nets)
    whole = sd.generate_image(ctx, **kw)
    calls = []
    stepped = sd.generate_image(ctx, callback=calls.append, **kw)
    assert calls == [1, 2, 3, 4, 5, 6]
    again = sd.generate_image(ctx, **kw)
    eager_sd, _ = _pipe(gpu, nets, jit=False)
    eager = eager_sd.generate_image(ctx, **kw)
    for other in (stepped, again, eager):
        np.testing.assert_array_equal(other, whole)
    assert np.all(np.isfinite(whole))
    from oracle import sd_oracle as O

    sd.denoise_streams = 2
    dual = sd.generate_image(ctx, **kw)
    assert O.psnr(dual, whole) >= 60.0
    # another sampler changes the picture, the default one is still there
    assert not np.array_equal(sd.generate_image(ctx, **{**kw, "sampler": None}), whole)


def test_draws_are_batch_independent(gpu, nets):
    """euler_a with a seed: sample 0 is bit-identical at batch 1 and batch 3."""
    sd, ctx = _pipe(gpu, nets)
    kw = dict(num_steps=5, seed=7, sampler="euler_a", guidance_rescale=0.7, return_latent=True)
    one = sd.generate_image(ctx, batch_size=1, **kw)
    three = sd.generate_image(ctx, batch_size=3, **kw)
    np.testing.assert_array_equal(one[0], three[0])
    assert not np.array_equal(three[0], three[1])   # (every sample has its own draws)


@pytest.mark.parametrize("case", ["txt2img", "img2img", "inpaint", "controlnet"])
def test_device_loop_vs_host_loop(gpu, nets, case):
    """dpmpp_2m_karras: the device loop (fp32 rows, one kernel per step) against host_loop=True (float64 host steps over
    predict_on_batch), txt2img, img2img at strength 0.6, inpaint and ControlNet."""
    from oracle import sd_oracle as O

    sd, ctx = _pipe(gpu, nets, control=case == "controlnet")
    rng = np.random.default_rng(43)
    kw = dict(batch_size=2, num_steps=8, seed=11, sampler="dpmpp_2m_karras", guidance_rescale=0.7, return_latent=True)
    image = rng.integers(0, 256, (64, 64, 3)).astype(np.uint8)
    if case in ("img2img", "inpaint"):
        kw.update(reference_image=image, reference_image_strength=0.6)
    if case == "inpaint":
        mask = np.zeros((64, 64), np.uint8)
        mask[16:48, 8:40] = 255
        kw.update(inpaint_mask=mask, mask_blur_strength=5)
    if case == "controlnet":
        kw.update(control_net_image=image.astype(np.float32))
    calls_d, calls_h = [], []
    dev = sd.generate_image(ctx, callback=calls_d.append, **kw)
    host = sd.generate_image(ctx, host_loop=True, callback=calls_h.append, **kw)
    run = 5 if case in ("img2img", "inpaint") else 8   # int(8 * 0.6 + 0.5)
    assert calls_d == calls_h == list(range(1, run + 1))
    p = O.psnr(dev, host)
    print(f"dpmpp_2m_karras {case}: device loop vs host loop {p:.1f} dB")
    if case != "controlnet":
        assert p >= HOST_PSNR_MIN
        return
    # (ControlNet beside the UNet's down path on a side stream, inside the captured loop)
    assert next(iter(sd._engines.values())).cn_plan is not None
    np.testing.assert_array_equal(sd.generate_image(ctx, **kw), dev)
    base = {k: v for k, v in kw.items() if k not in ("sampler", "seed")}
    noise = sd._get_initial_diffusion_noise(2, 11)
    p0 = O.psnr(sd.generate_image(ctx, diffusion_noise=noise, **base), sd.generate_image(ctx, diffusion_noise=noise, host_loop=True, **base))
    print(f"default sampler controlnet: device loop vs host loop {p0:.1f} dB")
    assert p >= HOST_PSNR_MIN_CONTROLNET and p >= p0 - 3.0, (p, p0)


def test_sampler_name_errors(gpu, nets):
    sd, ctx = _pipe(gpu, nets)
    with pytest.raises(ValueError, match="unknown sampler"):
        sd.generate_image(ctx, batch_size=1, num_steps=3, seed=0, sampler="dpm_fast")
    tcd, _ = _pipe(gpu, nets, tcd=True)
    for nm in ("dpmpp_2m", "dpmpp_2m_sde_karras", "euler_a"):
        with pytest.raises(ValueError, match="TCD"):
            tcd.generate_image(ctx, batch_size=1, num_steps=3, seed=0, sampler=nm)
    with pytest.raises(ValueError, match="TCD"):
        tcd.text_to_image(ctx, batch_size=1, num_steps=3, seed=0, sampler="euler_a")
