"""Hires fix on the device: msd_latent_resample against torch's float64 interpolate plus the re-noise, the two oracle fixture
jobs (tests/golden/oracle_hires_*.npz, tools/make_hires_fixtures.py), the hires= job against its manual composition from public
calls, two-engine residency, batch independence, a LoRA switch that reaches both sizes, the sharded job, refused combinations."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
PSNR_MIN = 40.0        # the project's bar for every job (test_samplers_gpu.py, test_baseline_configs_gpu.py)
LORA_PSNR_MIN = 45.0   # switched against load-time-merged weights (test_lora_switch_gpu.py)
SIZE_PAIRS = [(8, 16), (32, 64), (64, 96), (64, 128), (40, 72), (24, 40)]
MODES = ["nearest", "nearest-exact", "bilinear", "bicubic"]


def run_calls(calls):
    if not isinstance(calls, (list, tuple)):
        calls = [calls]
    st = torch.cuda.current_stream().cuda_stream
    for c in calls:
        c(st)
    torch.cuda.synchronize()


def _interpolate64(x, h_out, w_out, mode):
    kw = {} if mode.startswith("nearest") else {"align_corners": False}
    t = torch.from_numpy(np.asarray(x, dtype=np.float64)).permute(0, 3, 1, 2)
    return F.interpolate(t, size=(h_out, w_out), mode=mode, **kw).permute(0, 2, 3, 1).contiguous().numpy()


def _device_rows(n_in, n_out, mode, dev):
    from minsdtf_amd import hires

    return torch.from_numpy(hires.pack_rows(*hires.taps(n_in, n_out, mode))).to(dev)


def _resample(x, h_out, w_out, mode, dev, a=1.0, s=0.0, noise=None):
    from minsdtf_amd import ops

    B, h_in, w_in, _ = x.shape
    xd = torch.from_numpy(x).to(dev)
    zd = None if noise is None else torch.from_numpy(noise).to(dev)
    out = torch.full((B, h_out, w_out, 4), float("nan"), dtype=torch.float32, device=dev)
    wx, wy = _device_rows(w_in, w_out, mode, dev), _device_rows(h_in, h_out, mode, dev)
    run_calls(ops.latent_resample(x=xd, out=out, wx=wx, wy=wy, batch=B, h_in=h_in, w_in=w_in, h_out=h_out, w_out=w_out, a=a, s=s,
                                  noise=zd))
    return out.cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
def test_latent_resample_vs_float64(gpu, mode):
    """Every size pair on the rows with the next pair on the columns (two ratios per launch), batch 1 and 3, with and without
    the re-noise.  Bound (derived, not measured): about 20 fp32 operations per output, 2^-24 each, with sum |w| <= 1.6 for the
    2-D bicubic stencil: max abs error <= 2^-18 (a max|x| + s max|z|).  Sample 0 of the batch-3 launch == the batch-1 launch."""
    rng = np.random.default_rng(17)
    a, s = 0.8306, 0.5568
    worst = 0.0
    for k, (h_in, h_out) in enumerate(SIZE_PAIRS):
        w_in, w_out = SIZE_PAIRS[(k + 1) % len(SIZE_PAIRS)]
        x = rng.standard_normal((3, h_in, w_in, 4)).astype(np.float32)
        z = rng.standard_normal((3, h_out, w_out, 4)).astype(np.float32)
        up = _interpolate64(x, h_out, w_out, mode)
        for noise in (None, z):
            want = a * up + (0.0 if noise is None else s * noise.astype(np.float64))
            bound = 2.0 ** -18 * (a * np.abs(x).max() + (0.0 if noise is None else s * np.abs(z).max()))
            three = _resample(x, h_out, w_out, mode, gpu, a, s, noise)
            one = _resample(x[:1], h_out, w_out, mode, gpu, a, s, None if noise is None else noise[:1])
            assert np.all(np.isfinite(three))
            for got, ref in ((three, want), (one, want[:1])):
                err = float(np.abs(got - ref).max())
                worst = max(worst, err / bound)
                assert err <= bound, (mode, h_in, h_out, w_in, w_out, noise is not None, err, bound)
            np.testing.assert_array_equal(three[0], one[0])
    print(f"msd_latent_resample {mode}: worst error / bound = {worst:.3f}")


def test_latent_resample_argument_errors(gpu):
    from minsdtf_amd import _lib, ops

    x = torch.zeros(1, 8, 8, 4, device=gpu)
    out = torch.zeros(1, 16, 16, 4, device=gpu)
    z = torch.zeros(1, 16, 16, 4, device=gpu)
    rows = _device_rows(8, 16, "bilinear", gpu)
    good = dict(x=x, out=out, wx=rows, wy=rows, batch=1, h_in=8, w_in=8, h_out=16, w_out=16, a=1.0, s=1.0, noise=z)
    st = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    for bad in (dict(x=None), dict(out=None), dict(wx=None), dict(wy=None), dict(batch=0), dict(h_in=0), dict(w_in=-1),
                dict(h_out=4), dict(w_out=1 << 20), dict(x=x.data_ptr() + 4), dict(out=out.data_ptr() + 8),
                dict(noise=z.data_ptr() + 4), dict(wx=rows.data_ptr() + 4), dict(out=x)):
        c = ops.latent_resample(**{**good, **bad})
        assert c.fn(*c.args, st) == -1, bad
        assert lib.msd_last_error()
    run_calls(ops.latent_resample(**good))


# ---------------------------------------------------------------------------------------------------------------- pipelines
@pytest.fixture(scope="module")
def nets(gpu):
    from minsdtf_amd.models import DiffusionModel, ImageDecoder

    unet = DiffusionModel(64, 64, device=gpu)
    unet.load_synthetic(seed=0, bias_scale=0.05)
    dec = ImageDecoder(device=gpu)
    dec.load_synthetic(seed=0, bias_scale=0.05)
    return {"unet": unet, "dec": dec}


def _pipe(gpu, nets, size=64, jit=True):
    """A pipeline at `size` over the module's weights (another size: a view that shares them)."""
    from minsdtf_amd.models import DiffusionModel
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sd = StableDiffusion(size, size, jit_compile=jit, device=gpu)
    if size == 64:
        sd._diffusion_model = nets["unet"]
    else:
        sd._diffusion_model = DiffusionModel(size, size, device=gpu)
        sd._diffusion_model.share_weights(nets["unet"])
    sd._image_decoder = nets["dec"]
    rng = np.random.default_rng(41)
    sd.unconditional_context = rng.standard_normal((77, 768)).astype(np.float32)
    return sd, rng.standard_normal((77, 768)).astype(np.float32)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_hires_vs_oracle_fixture(gpu, tag):
    """The two fixture jobs against the fp32 oracle's composition (denoise_loop / the sigma-space loop, torch's float64
    interpolate, the img2img entry): final-latent PSNR >= 40 dB.
    a: 256 -> 512, bilinear, default sampler, batch 1, 10 + 8 steps at strength 0.5;
    b: 512 -> 768, bicubic, dpmpp_2m_karras, batch 2, 20 + 10 steps at strength 0.6."""
    from minsdtf_amd.stable_diffusion import StableDiffusion
    from oracle import sd_oracle as O

    g = np.load(os.path.join(GOLD, f"oracle_hires_{tag}.npz"))
    base, target, B = int(g["base"]), int(g["target"]), int(g["batch"])
    sd = StableDiffusion(base, base, jit_compile=True, device=gpu)
    sd.diffusion_model.load_synthetic(seed=int(g["weight_seed"]))
    rng = np.random.default_rng(int(g["context_seed"]))
    ctx = rng.standard_normal((1, 77, 768)).astype(np.float32)
    unc = rng.standard_normal((1, 77, 768)).astype(np.float32)
    sd.unconditional_context = unc[0]
    kw = dict(batch_size=B, num_steps=int(g["steps"]), unconditional_guidance_scale=float(g["guidance"]), seed=int(g["noise_seed"]),
              guidance_rescale=float(g["guidance_rescale"]), return_latent=True, sampler=str(g["sampler"]) or None)
    hires = dict(size=(target, target), steps=int(g["hires_steps"]), strength=float(g["strength"]), upscaler=str(g["upscaler"]))
    got = sd.generate_image(ctx[0], hires=hires, **kw)
    assert got.shape == (B, target // 8, target // 8, 4)
    p = O.psnr(got, g["latent"])
    p1 = O.psnr(sd.generate_image(ctx[0], **kw), g["base_latent"])
    per = [round(O.psnr(got[b], g["latent"][b]), 1) for b in range(B)]
    print(f"hires job {tag} ({base} -> {target}, {g['upscaler']}, {str(g['sampler']) or 'default sampler'}, batch {B}): final-latent PSNR "
          f"{p:.1f} dB (per sample {per}); pass 1 alone {p1:.1f} dB")
    assert p >= PSNR_MIN


@pytest.mark.parametrize("sampler,upscaler", [(None, "bilinear"), ("dpmpp_2m_karras", "bicubic"), ("euler_a", "nearest-exact")])
def test_device_handoff_equals_manual_composition(gpu, nets, sampler, upscaler):
    """hires= against the same job put together by hand: return_latent=True at the base size, the op on its own, an engine of a
    second pipeline at the target size entered at the same rates and start index.  Bit-identical."""
    from minsdtf_amd import hires, ops
    from minsdtf_amd import samplers as smp

    steps1, steps2, strength, seed, B = 5, 6, 0.5, 3, 2
    sd, ctx = _pipe(gpu, nets)
    kw = dict(batch_size=B, num_steps=steps1, seed=seed, sampler=sampler, guidance_rescale=0.7, return_latent=True)
    calls = []
    got = sd.generate_image(ctx, hires=dict(scale=2, steps=steps2, strength=strength, upscaler=upscaler), callback=calls.append, **kw)
    assert calls == list(range(1, steps1 + 3 + 1)) and got.shape == (B, 16, 16, 4)
    whole = sd.generate_image(ctx, hires=hires.HiresSpec(size=(128, 128), steps=steps2, strength=strength, upscaler=upscaler), **kw)
    np.testing.assert_array_equal(whole, got)   # whole-loop graphs == per-step graphs; a HiresSpec == its dict

    lat1 = sd.generate_image(ctx, **kw)
    sd2, _ = _pipe(gpu, nets, size=128)
    spec = smp.parse(sampler)
    a, s, start, run = hires.entry(sd2.scheduler, spec, steps2, strength)
    assert run == 3
    x = torch.from_numpy(lat1).to(gpu)
    z = torch.from_numpy(hires.draw_noise(B, 16, 16, seed)).to(gpu)
    up = torch.empty(B, 16, 16, 4, dtype=torch.float32, device=gpu)
    rows = _device_rows(8, 16, upscaler, gpu)
    run_calls(ops.latent_resample(x=x, out=up, wx=rows, wy=rows, batch=B, h_in=8, w_in=8, h_out=16, w_out=16, a=a, s=s, noise=z))
    sd2.scheduler.set_timesteps(steps2)
    eng = sd2._engine(B, 77, 77, steps2, 7.5, 0.7, False, sampler=sampler)
    c = np.repeat(ctx[None], B, axis=0)
    u = np.repeat(sd2.unconditional_context[None], B, axis=0)
    sched = None if spec is None else smp.schedule(spec, sd2.scheduler, steps2)
    z2 = smp.draw_step_noise(B, steps2, 16, 16, seed, stream_key=3) if spec is not None and spec.stochastic else None
    eng.prepare(eng.contexts(u, c), up, sd2.scheduler, sd2.scheduler.timesteps, start, step_noise=z2, sampler=sched)
    eng.run_steps(run)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(eng.latent.cpu().numpy(), got)
    # the decoded picture has the target size
    img = sd.generate_image(ctx, hires=dict(scale=2, steps=steps2, strength=strength, upscaler=upscaler),
                            **{**kw, "return_latent": False})
    assert img.shape == (B, 128, 128, 3) and img.dtype == np.uint8
    np.testing.assert_array_equal(img, nets["dec"].decode_to_uint8(torch.from_numpy(got).to(gpu)).cpu().numpy())


def test_residency(gpu, nets, monkeypatch):
    """The first hires job builds two engines, a repeat builds none and captures nothing; a plain job afterwards leaves one."""
    import minsdtf_amd.stable_diffusion as sdm

    built = []
    init = sdm.DenoiseEngine.__init__

    def counting(self, *a, **k):
        built.append((self.__class__.__name__, a[0].h))
        init(self, *a, **k)

    monkeypatch.setattr(sdm.DenoiseEngine, "__init__", counting)
    sd, ctx = _pipe(gpu, nets)
    kw = dict(batch_size=1, num_steps=4, seed=5, guidance_rescale=0.7, return_latent=True)
    hr = dict(scale=2, steps=4, strength=0.5)
    first = sd.generate_image(ctx, hires=hr, **kw)
    assert [h for _n, h in built] == [8, 16] and len(sd._engines) == 2
    graphs = [e._loop_graph for e in sd._engines.values()]
    assert all(g is not None for g in graphs)
    second = sd.generate_image(ctx, hires=hr, **kw)
    assert len(built) == 2 and [e._loop_graph for e in sd._engines.values()] == graphs
    np.testing.assert_array_equal(first, second)
    base_engine = next(iter(sd._engines.values()))
    plain = sd.generate_image(ctx, **kw)
    assert len(sd._engines) == 1 and next(iter(sd._engines.values())) is base_engine and len(built) == 2   # (pass 1's engine IS the plain job's)
    assert plain.shape == (1, 8, 8, 4)
    sd.generate_image(ctx, **{**kw, "num_steps": 3})
    assert len(sd._engines) == 1 and len(built) == 3
    third = sd.generate_image(ctx, hires=hr, **kw)
    assert len(sd._engines) == 2 and len(built) == 5
    np.testing.assert_array_equal(first, third)
    # the target-size UNet is a view of the same packed weights, kept per size
    view = sd._unet_for(128, 128)
    assert view._W is sd.diffusion_model._W and sd._unet_for(128, 128) is view and sd._unet_for(64, 64) is sd.diffusion_model


@pytest.mark.parametrize("sampler", [None, "euler_a"])
def test_batch_independence(gpu, nets, sampler):
    """Sample 0 of a batch-2 hires job == the batch-1 job with that sample's noises, with a seed (the draws are made for the
    global batch, sample-major) and with explicit noises."""
    from minsdtf_amd import hires

    sd, ctx = _pipe(gpu, nets)
    kw = dict(num_steps=4, sampler=sampler, guidance_rescale=0.7, return_latent=True, hires=dict(scale=2, steps=4, strength=0.5, upscaler="bicubic"))
    two = sd.generate_image(ctx, batch_size=2, seed=9, **kw)
    one = sd.generate_image(ctx, batch_size=1, seed=9, **kw)
    np.testing.assert_array_equal(one[0], two[0])
    assert not np.array_equal(two[0], two[1])
    if sampler is None:
        n1, n2 = sd._get_initial_diffusion_noise(2, 9), hires.draw_noise(2, 16, 16, 9)
        np.testing.assert_array_equal(sd.generate_image(ctx, batch_size=2, diffusion_noise=n1, hires_noise=n2, **kw), two)
        np.testing.assert_array_equal(sd.generate_image(ctx, batch_size=1, diffusion_noise=n1[1], hires_noise=n2[1], **kw)[0], two[1])


def _lora_sd(seed, rank=4, std=0.03):
    """kohya-named factors for all 278 UNet layers (as tests/test_lora_switch_gpu.py makes them)."""
    from minsdtf_amd import weights as Wt

    rng = np.random.default_rng(seed)
    spec_of = {s.alt_key: s for s in Wt.table("civitai_model") if s.alt_key}
    sd = {}
    for n, k in Wt._lora_unet_name_map().items():
        ts = spec_of[k].torch_shape
        up, down = ((ts[0], rank), (rank, ts[1])) if len(ts) == 2 else ((ts[0], rank, 1, 1), (rank, ts[1], ts[2], ts[3]))
        sd[n + ".lora_up.weight"] = torch.from_numpy((rng.standard_normal(up) * std).astype(np.float32))
        sd[n + ".lora_down.weight"] = torch.from_numpy((rng.standard_normal(down) * std).astype(np.float32))
        sd[n + ".alpha"] = torch.tensor(float(rank))
    return sd


def test_lora_switch_reaches_both_sizes(gpu, tmp_path):
    """After set_loras both passes run on the merged weights: the hires result moves, equals a fresh lora_path= pipeline's hires
    job to the bar test_lora_switch_gpu.py uses for that comparison, and [] brings the base result back bit for bit."""
    from safetensors.torch import save_file

    from minsdtf_amd import weights as Wt
    from minsdtf_amd.stable_diffusion import StableDiffusion
    from oracle import sd_oracle as O

    ck, lp = str(tmp_path / "sd15.safetensors"), str(tmp_path / "unet_lora.safetensors")
    Wt.write_synthetic_checkpoint(ck, kinds=("civitai_model", "decoder"), seed=0, bias_scale=0.05)
    save_file(_lora_sd(7), lp)
    rng = np.random.default_rng(31)
    ctx, unc = rng.standard_normal((77, 768)).astype(np.float32), rng.standard_normal((77, 768)).astype(np.float32)
    kw = dict(batch_size=1, num_steps=2, unconditional_guidance_scale=7.5, seed=4, guidance_rescale=0.7, return_latent=True,
              hires=dict(scale=2, steps=4, strength=0.5))

    def run(sd):
        sd.unconditional_context = unc
        return sd.generate_image(ctx, **kw)

    sw = StableDiffusion(64, 64, jit_compile=True, unet_ckpt=ck, vae_ckpt=ck, lora_switch=True, device=gpu)
    base = run(sw)
    engines = list(sw._engines.values())
    sw.set_loras([(lp, 1.0)])
    got = run(sw)
    assert list(sw._engines.values()) == engines and len(engines) == 2   # (in place: nothing re-recorded)
    assert not np.array_equal(got, base)
    # one packed image, one LoRA master: the target-size view switched with the base model
    view = sw._unet_for(128, 128)
    assert view.lora_version == sw.diffusion_model.lora_version == 1
    loaded = run(StableDiffusion(64, 64, jit_compile=True, unet_ckpt=ck, vae_ckpt=ck, lora_path=lp, device=gpu))
    p, p_base = O.psnr(got, loaded), O.psnr(base, loaded)
    print(f"hires after set_loras vs a fresh lora_path= pipeline: {p:.1f} dB (the base weights' result: {p_base:.1f} dB)")
    assert p >= LORA_PSNR_MIN and p_base < p - 6.0
    sw.set_loras([])
    np.testing.assert_array_equal(run(sw), base)


def test_sharded_hires_equals_unsharded(gpu):
    """A one-rank process group with forced collectives (as tests/test_rccl_gpu.py): the sharded hires job == the unsharded one."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(HERE, "_job_world1_child.py"), "hires"], env=env,
                       stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=570)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert any(line.startswith("OK ") for line in p.stdout.splitlines()), p.stdout[-2000:]
    print(p.stdout.strip().splitlines()[-1])


def test_refused_combinations(gpu, nets):
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sd, ctx = _pipe(gpu, nets)
    img = np.zeros((64, 64, 3), dtype=np.uint8)
    kw = dict(batch_size=1, num_steps=3, seed=0, hires=dict(scale=2))
    for extra in (dict(reference_image=img), dict(inpaint_mask=img[..., 0]), dict(reference_image=img, inpaint_mask=img[..., 0]),
                  dict(control_net_image=img.astype(np.float32)), dict(host_loop=True)):
        with pytest.raises(ValueError, match="hires"):
            sd.generate_image(ctx, **kw, **extra)
    tcd = StableDiffusion(64, 64, jit_compile=True, device=gpu, active_tcd=True)
    with pytest.raises(ValueError, match="hires"):
        tcd.generate_image(ctx, **kw)
    with pytest.raises(ValueError, match="hires"):
        sd.image_to_image(ctx, reference_image=img, **kw)
    with pytest.raises(ValueError, match="hires"):
        sd.inpaint(ctx, reference_image=img, inpaint_mask=img[..., 0], **kw)
    with pytest.raises(ValueError, match="hires_noise has shape"):
        sd.generate_image(ctx, hires_noise=np.zeros((1, 8, 8, 4), np.float32), **kw)
    with pytest.raises(ValueError, match="multiple of 64"):
        sd.text_to_image(ctx, batch_size=1, num_steps=3, seed=0, hires=dict(size=(96, 128)))
    assert not sd._engines
    assert sd.text_to_image(ctx, batch_size=1, num_steps=3, seed=0, hires=dict(scale=2, strength=0.5)).shape == (1, 128, 128, 3)
