"""Perturbed-attention guidance on the device: msd_attention_identity against torch's transpose, predict_perturbed against
predict_on_batch, the p rows of the engine against predict_perturbed, pag= jobs against plain jobs where the two must agree bit for
bit (scale 0), the device loop against host_loop=True, the two oracle fixture jobs (tests/golden/oracle_pag_*.npz,
tools/make_pag_fixtures.py), the three graph forms, residency, no guidance, an unconditional context of another length, the
sharded job, the shared prefix."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
PSNR_MIN = 40.0        # the project's bar for every job (test_regions_gpu.py, test_tiled_gpu.py, test_hires_gpu.py)
HOST_PSNR_MIN = 45.0   # device loop vs host_loop=True of a samplers.py txt2img job (test_regions_gpu.py, test_samplers_gpu.py)
SENTINEL = 7.0
LAYERS_B = ["down_blocks.1.attentions.0", "mid_block.attentions.0", "up_blocks.2.attentions.2"]


def run_calls(calls):
    if not isinstance(calls, (list, tuple)):
        calls = [calls]
    st = torch.cuda.current_stream().cuda_stream
    for c in calls:
        c(st)
    torch.cuda.synchronize()


def bits(t):
    return t.view(torch.int16).cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("s, channels, vt_ld", [(1, 1280, 8), (4, 1280, 8), (16, 640, 16), (35, 320, 40), (64, 320, 64), (1024, 320, 1024)])
def test_identity_is_the_transpose(gpu, s, channels, vt_ld):
    """out[b][k][c] == vt[b][c][k] bit for bit.  A batch of 3 of which only the LAST row is converted, through offset pointers (how
    the engine records the perturbed rows): the other rows of out keep the sentinel.  Then the last two rows in one launch.  The
    padding columns of vt hold NaN, which must not reach out."""
    from minsdtf_amd import ops

    g = torch.Generator().manual_seed(1000 * s + channels)
    vt = torch.randn(3, channels, vt_ld, generator=g).to(torch.bfloat16).to(gpu)
    vt[:, :, s:] = float("nan")
    want = bits(vt[:, :, :s].transpose(1, 2).contiguous())   # (3, s, channels)
    for rows in (1, 2):
        out = torch.full((3, s, channels), SENTINEL, dtype=torch.bfloat16, device=gpu)
        first = 3 - rows
        run_calls(ops.attention_identity(vt=vt.data_ptr() + first * channels * vt_ld * 2, out=out.data_ptr() + first * s * channels * 2,
                                         batch=rows, channels=channels, s=s, vt_ld=vt_ld, o_ld=channels))
        got = bits(out)
        np.testing.assert_array_equal(got[first:], want[first:])
        assert not torch.isnan(out.float()).any()
        np.testing.assert_array_equal(got[:first], bits(torch.full((first, s, channels), SENTINEL, dtype=torch.bfloat16)))


def test_identity_with_a_wider_output_row(gpu):
    """o_ld > channels: the gap behind every row keeps the sentinel, and so does a guard row behind the last one."""
    from minsdtf_amd import ops

    s, channels, vt_ld, o_ld = 35, 320, 40, 328
    vt = torch.randn(2, channels, vt_ld, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).to(gpu)
    vt[:, :, s:] = float("nan")
    out = torch.full((2 * s + 1, o_ld), SENTINEL, dtype=torch.bfloat16, device=gpu)
    run_calls(ops.attention_identity(vt=vt, out=out, batch=2, channels=channels, s=s, vt_ld=vt_ld, o_ld=o_ld))
    np.testing.assert_array_equal(bits(out[:2 * s, :channels].reshape(2, s, channels)), bits(vt[:, :, :s].transpose(1, 2).contiguous()))
    assert bool((out[:, channels:] == SENTINEL).all()) and bool((out[2 * s] == SENTINEL).all())


def test_identity_argument_errors(gpu):
    from minsdtf_amd import _lib, ops

    B, C, s, ld = 2, 320, 35, 40
    vt = torch.zeros(B, C, ld, dtype=torch.bfloat16, device=gpu)
    out = torch.zeros(B, s, C, dtype=torch.bfloat16, device=gpu)
    big = torch.zeros(16, device=gpu)   # (only its address is used: every bad call returns before a launch)
    good = dict(vt=vt, out=out, batch=B, channels=C, s=s, vt_ld=ld, o_ld=C)
    st = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    for bad in (dict(vt=None), dict(out=None), dict(vt=vt.data_ptr() + 8), dict(out=out.data_ptr() + 2), dict(batch=0), dict(batch=65536),
                dict(s=0), dict(channels=0), dict(channels=324), dict(vt_ld=36), dict(vt_ld=32), dict(o_ld=312), dict(o_ld=324),
                dict(vt=big, out=big.data_ptr() + 64, batch=4096, channels=1280, s=512, vt_ld=512, o_ld=1280),   # 2^31 elements of vt
                dict(vt=big, out=big.data_ptr() + 64, batch=4096, channels=8, s=2048, vt_ld=2048, o_ld=320),      # ... of out
                dict(out=vt), dict(out=vt.data_ptr() + B * C * ld * 2 - 16), dict(vt=out.data_ptr() + B * s * C * 2 - 16)):
        call = ops.attention_identity(**{**good, **bad})
        assert call.fn(*call.args, st) == -1, bad
        assert lib.msd_last_error(), bad
    run_calls(ops.attention_identity(**good))


# ---------------------------------------------------------------------------------------------------------------- pipelines
@pytest.fixture(scope="module")
def nets(gpu):
    """The synthetic UNet at 64x64 and, on the same packed weights, at 128x128 (mid block: 4 tokens); the decoder."""
    from minsdtf_amd.models import DiffusionModel, ImageDecoder

    unet = DiffusionModel(64, 64, device=gpu)
    unet.load_synthetic(seed=0, bias_scale=0.05)
    big = DiffusionModel(128, 128, device=gpu)
    big.share_weights(unet)
    dec = ImageDecoder(device=gpu)
    dec.load_synthetic(seed=0, bias_scale=0.05)
    return {64: unet, 128: big, "dec": dec}


def _pipe(gpu, nets, size=64, jit=True, tcd=False):
    """(pipeline, two contexts P, Q)"""
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sd = StableDiffusion(size, size, jit_compile=jit, device=gpu, active_tcd=tcd)
    sd._diffusion_model = nets[size]
    sd._image_decoder = nets["dec"]
    rng = np.random.default_rng(41)
    sd.unconditional_context = rng.standard_normal((77, 768)).astype(np.float32)
    return sd, [rng.standard_normal((77, 768)).astype(np.float32) for _ in range(2)]


def _fixture_job(tag):
    """The fixture job `tag` (tools/make_pag_fixtures.py: a = 128x128 px, "mid", default sampler, batch 1, rescale 0; b = 64x64 px,
    three layers, dpmpp_2m, batch 2, rescale 0.7; each at its recorded scale) -> (pipeline size, generate_image keywords)."""
    g = np.load(os.path.join(GOLD, f"oracle_pag_{tag}.npz"))
    return int(g["size"]), dict(sampler=str(g["sampler"]) or None, guidance_rescale=float(g["guidance_rescale"]), batch_size=int(g["batch"]),
                                pag=dict(scale=float(g["scale"]), layers=[str(n) for n in g["layers"]]))


def _inputs(unet, B, seed=2):
    from minsdtf_amd.stable_diffusion import get_timestep_embedding

    rng = np.random.default_rng(seed)
    return [rng.standard_normal((B, unet.h, unet.w, 4)).astype(np.float32), get_timestep_embedding(0, B).astype(np.float32),
            rng.standard_normal((B, 77, 768)).astype(np.float32)]


def test_one_token_is_the_identity_already(gpu, nets):
    """64x64 px: the mid block has ONE token, softmax over one key is 1, so the perturbed forward is the plain one bit for bit."""
    x = _inputs(nets[64], 2)
    np.testing.assert_array_equal(nets[64].predict_perturbed(x, ["mid_block.attentions.0"]), nets[64].predict_on_batch(x))


def test_perturbed_forward_differs(gpu, nets):
    """128x128 px: four tokens in the mid block - another prediction, finite, and the plain plan is untouched by it."""
    x = _inputs(nets[128], 1)
    plain = nets[128].predict_on_batch(x)
    pert = nets[128].predict_perturbed(x, "mid_block.attentions.0")
    assert pert.shape == plain.shape and np.all(np.isfinite(pert)) and not np.array_equal(pert, plain)
    np.testing.assert_array_equal(nets[128].predict_on_batch(x), plain)
    names = [c.name for c in next(bp for k, bp in nets[128]._plans.items() if k[0][-1] == ("pag", ("mid_block.attentions.0",))).plan.calls]
    tb = "mid_block.attentions.0.transformer_blocks.0.attn1"
    assert tb + ".identity" in names and tb not in names   # perturbed == B: no attention launch in that block
    with pytest.raises(ValueError, match="PAG_LAYERS"):
        nets[128].predict_perturbed(x, ["mid"])


@pytest.mark.parametrize("layers", [LAYERS_B, ["down_blocks.0.attentions.0"]])
def test_p_rows_of_the_engine_are_predict_perturbed(gpu, nets, layers):
    """One step of a batch-2 job: the engine's rows are [u: 2][c: 2][p: 2]; after the step the p rows still hold the UNet's
    output, which is predict_perturbed of the same latent, time embedding and context bit for bit (a sample's bits do not depend
    on its batch), and the u rows are predict_on_batch's."""
    sd, (P, _Q) = _pipe(gpu, nets)
    lat, temb, _ = _inputs(nets[64], 2)
    sd.generate_image(P, batch_size=2, num_steps=1, diffusion_noise=lat, guidance_rescale=0.0, return_latent=True,
                      pag=dict(scale=3.0, layers=layers))
    eng = next(iter(sd._engines.values()))
    assert eng.pag == frozenset(layers) and eng.passes == [(0, 6, 77, "both")] and eng.eps.shape[0] == 6
    eps = eng.eps.cpu().numpy().reshape(3, 2, 8, 8, 4)
    ctx = np.repeat(P[None], 2, axis=0)
    np.testing.assert_array_equal(eps[2], nets[64].predict_perturbed([lat, temb, ctx], layers))
    np.testing.assert_array_equal(eps[0], nets[64].predict_on_batch([lat, temb, np.repeat(sd.unconditional_context[None], 2, axis=0)]))
    assert not np.array_equal(eps[2], nets[64].predict_on_batch([lat, temb, ctx]))
    names = [c.name for c in eng.calls]
    assert names[-2] == "pag_combine" and names[-1] == "cfg_step"
    for blk in layers:
        i = names.index(blk + ".transformer_blocks.0.attn1")
        assert names[i + 1] == blk + ".transformer_blocks.0.attn1.identity"
    assert sum(n.endswith(".identity") for n in names) == len(layers)


@pytest.mark.parametrize("sampler", [None, "euler_a"])
def test_scale_zero_is_the_plain_job(gpu, nets, sampler):
    sd, (P, _Q) = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=4, seed=6, sampler=sampler, guidance_rescale=0.7)
    plain = sd.generate_image(P, return_latent=True, **kw)
    got = sd.generate_image(P, return_latent=True, pag=dict(scale=0.0, layers=LAYERS_B), **kw)
    assert len(sd._engines) == 1 and next(iter(sd._engines.values())).pag is None
    np.testing.assert_array_equal(got, plain)
    assert [c.name for c in next(iter(sd._engines.values())).calls].count("pag_combine") == 0
    np.testing.assert_array_equal(sd.text_to_image(P, pag=dict(scale=0.0), **kw), sd.generate_image(P, **kw))
    assert sd.text_to_image(P, pag=dict(scale=2.0, layers=LAYERS_B), **kw).shape == (2, 64, 64, 3)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_device_loop_vs_host_loop(gpu, nets, tag):
    """The device loop against host_loop=True (predict_on_batch, predict_perturbed, pag.combine_host), with test_regions_gpu.py's
    bars: job b (a samplers.py sampler) 45 dB, job a (the default sampler) the project's 40 dB.  And PAG is not a no-op."""
    from oracle import sd_oracle as O

    size, kw = _fixture_job(tag)
    sd, (P, _Q) = _pipe(gpu, nets, size)
    kw = dict(kw, num_steps=4, seed=11, return_latent=True)
    calls_d, calls_h = [], []
    dev = sd.generate_image(P, callback=calls_d.append, **kw)
    host = sd.generate_image(P, host_loop=True, callback=calls_h.append, **kw)
    assert calls_d == calls_h == [1, 2, 3, 4]
    p = O.psnr(dev, host)
    bar = HOST_PSNR_MIN if kw["sampler"] is not None else PSNR_MIN
    plain = O.psnr(sd.generate_image(P, **{**kw, "pag": None}), dev)
    print(f"PAG job {tag}: device loop vs host loop {p:.1f} dB (bar {bar:.0f}); the plain job against it {plain:.1f} dB")
    assert p >= bar
    assert plain < p   # (the job without PAG is further away than the other route)


@pytest.mark.parametrize("sampler", ["dpmpp_2m_sde", "euler_a", "dpmpp_2m_karras"])
def test_other_samplers_vs_host_loop(gpu, nets, sampler):
    from oracle import sd_oracle as O

    sd, (P, _Q) = _pipe(gpu, nets)
    kw = dict(batch_size=1, num_steps=3, seed=4, sampler=sampler, guidance_rescale=0.7, return_latent=True,
              pag=dict(scale=2.0, layers="down_blocks.1.attentions.0"))
    p = O.psnr(sd.generate_image(P, **kw), sd.generate_image(P, host_loop=True, **kw))
    print(f"PAG, {sampler}: device loop vs host loop {p:.1f} dB")
    assert p >= HOST_PSNR_MIN


def test_tcd_pipeline(gpu, nets):
    """PAG on a TCD pipeline: the device loop against host_loop=True with the same draws (numpy's global stream, as the
    reference's TCD step takes them), at the project's 40 dB."""
    from oracle import sd_oracle as O

    sd, (P, _Q) = _pipe(gpu, nets, tcd=True)
    kw = dict(batch_size=1, num_steps=3, seed=4, guidance_rescale=0.0, return_latent=True, pag=dict(scale=2.0, layers=LAYERS_B))
    np.random.seed(9)
    dev = sd.generate_image(P, **kw)
    np.random.seed(9)
    host = sd.generate_image(P, host_loop=True, **kw)
    p = O.psnr(dev, host)
    print(f"PAG, TCD: device loop vs host loop {p:.1f} dB")
    assert p >= PSNR_MIN


@pytest.mark.parametrize("tag", ["a", "b"])
def test_pag_vs_oracle_fixture(gpu, nets, tag):
    """The two fixture jobs against the fp32 oracle's composition (unet_forward three times per step, the third with the selected
    self-attentions replaced by to_out(to_v(x)); the float64 formula; rescale against c'; the scheduler / DPM++ 2M step): final
    latent PSNR >= 40 dB overall and per sample - where the same job WITHOUT PAG lies below 30 dB (`plain_psnr` in the file)."""
    from oracle import sd_oracle as O

    g = np.load(os.path.join(GOLD, f"oracle_pag_{tag}.npz"))
    assert (int(g["weight_seed"]), float(g["bias_scale"])) == (0, 0.05) and float(g["plain_psnr"]) < 30.0   # the module's nets
    size, B = int(g["size"]), int(g["batch"])
    sd, _ctxs = _pipe(gpu, nets, size)
    rng = np.random.default_rng(int(g["context_seed"]))
    ctx = rng.standard_normal((1, 77, 768)).astype(np.float32)[0]
    sd.unconditional_context = rng.standard_normal((1, 77, 768)).astype(np.float32)[0]
    layers = [str(n) for n in g["layers"]]
    got = sd.generate_image(ctx, batch_size=B, num_steps=int(g["steps"]), unconditional_guidance_scale=float(g["guidance"]),
                            seed=int(g["noise_seed"]), guidance_rescale=float(g["guidance_rescale"]), return_latent=True,
                            sampler=str(g["sampler"]) or None, pag=dict(scale=float(g["scale"]), layers=layers))
    assert got.shape == (B, size // 8, size // 8, 4)
    eng = next(iter(sd._engines.values()))
    assert eng.pag == frozenset(layers)
    p = O.psnr(got, g["latent"])
    per = [round(O.psnr(got[b], g["latent"][b]), 1) for b in range(B)]
    print(f"PAG job {tag} (scale {float(g['scale'])}, {len(layers)} layer(s), {str(g['sampler']) or 'default sampler'}, batch {B}): "
          f"final latent PSNR {p:.1f} dB (per sample {per}); the plain job: {float(g['plain_psnr']):.1f} dB")
    assert p >= PSNR_MIN and min(per) >= PSNR_MIN


@pytest.mark.parametrize("tag", ["a", "b"])
def test_graph_forms_agree(gpu, nets, tag):
    """The whole-loop graph == per-step graphs (a callback is installed) == eager launches (jit_compile=False), bit for bit."""
    size, kw = _fixture_job(tag)
    sd, (P, _Q) = _pipe(gpu, nets, size)
    kw = dict(kw, num_steps=4, seed=8, return_latent=True)
    whole = sd.generate_image(P, **kw)
    calls = []
    stepped = sd.generate_image(P, callback=calls.append, **kw)
    assert calls == [1, 2, 3, 4]
    eng = next(iter(sd._engines.values()))
    assert eng._loop_graph is not None and eng._step_graph is not None and eng.pag
    eager_sd, _ = _pipe(gpu, nets, size, jit=False)
    eager = eager_sd.generate_image(P, callback=calls.append, **kw)
    np.testing.assert_array_equal(stepped, whole)
    np.testing.assert_array_equal(eager, whole)
    assert np.all(np.isfinite(whole))


def test_residency(gpu, nets, monkeypatch):
    """A second job with another scale builds no engine, records no plan and captures no graph, and its result is a fresh
    pipeline's; other layers are another engine; a plain job is not a PAG engine."""
    import minsdtf_amd.engine as eng_mod
    import minsdtf_amd.stable_diffusion as sdm

    built, plans = [], []
    init, plan_init = sdm.DenoiseEngine.__init__, eng_mod.Plan.__init__

    def counting(self, *a, **k):
        built.append(k.get("pag"))
        init(self, *a, **k)

    def counting_plan(self, *a, **k):
        plans.append(1)
        plan_init(self, *a, **k)

    monkeypatch.setattr(sdm.DenoiseEngine, "__init__", counting)
    monkeypatch.setattr(eng_mod.Plan, "__init__", counting_plan)
    sd, (P, _Q) = _pipe(gpu, nets)
    kw = dict(batch_size=1, num_steps=3, seed=5, guidance_rescale=0.7, return_latent=True)
    first = sd.generate_image(P, pag=dict(scale=3.0, layers=LAYERS_B), **kw)
    assert built == [tuple(sorted(LAYERS_B))] and len(sd._engines) == 1
    eng = next(iter(sd._engines.values()))
    graph, n_plans = eng._loop_graph, len(plans)
    assert graph is not None
    second = sd.generate_image(P, pag=dict(scale=1.25, layers=LAYERS_B), **kw)
    assert len(built) == 1 and len(plans) == n_plans and next(iter(sd._engines.values())) is eng and eng._loop_graph is graph
    assert not np.array_equal(first, second)
    fresh, _ = _pipe(gpu, nets)
    np.testing.assert_array_equal(second, fresh.generate_image(P, pag=dict(scale=1.25, layers=LAYERS_B), **kw))
    assert len(built) == 2
    np.testing.assert_array_equal(sd.generate_image(P, pag=dict(scale=3.0, layers=LAYERS_B), **kw), first)
    assert len(built) == 2 and eng._loop_graph is graph
    sd.generate_image(P, pag=dict(scale=3.0, layers=LAYERS_B[:1]), **kw)
    assert built[-1] == (LAYERS_B[0],) and len(built) == 3 and len(sd._engines) == 1
    sd.generate_image(P, **kw)
    assert built[-1] is None and len(built) == 4 and len(sd._engines) == 1


def test_without_guidance(gpu, nets):
    """unconditional_guidance_scale = 0: rows [c][p], k = s, the step sees c' alone; against host_loop=True (default sampler: the
    project's 40 dB)."""
    from oracle import sd_oracle as O

    sd, (P, _Q) = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=4, seed=11, unconditional_guidance_scale=0.0, return_latent=True,
              pag=dict(scale=0.8, layers=LAYERS_B))
    dev = sd.generate_image(P, **kw)
    eng = next(iter(sd._engines.values()))
    assert eng.passes == [(0, 4, 77, "cond")] and eng.eps.shape[0] == 4 and not eng.cfg
    np.testing.assert_array_equal(eng.pag_w.cpu().numpy()[:, 0, 0], np.asarray([1.8, -0.8], dtype=np.float32))
    host = sd.generate_image(P, host_loop=True, **kw)
    p = O.psnr(dev, host)
    print(f"PAG without guidance: device loop vs host loop {p:.1f} dB")
    assert p >= PSNR_MIN
    assert not np.array_equal(dev, sd.generate_image(P, **{**kw, "pag": None}))


def test_unconditional_context_of_another_length(gpu, nets):
    """154 unconditional tokens against 77: two passes, the second holding [c][p]; against host_loop=True at the sampler bar."""
    from oracle import sd_oracle as O

    sd, (P, _Q) = _pipe(gpu, nets)
    neg = np.random.default_rng(5).standard_normal((154, 768)).astype(np.float32)
    kw = dict(_fixture_job("b")[1], num_steps=4, seed=11, return_latent=True, negative_prompt=neg)
    dev = sd.generate_image(P, **kw)
    eng = next(iter(sd._engines.values()))
    assert eng.passes == [(0, 2, 154, "uncond"), (2, 4, 77, "cond")] and eng.eps.shape[0] == 6
    host = sd.generate_image(P, host_loop=True, **kw)
    p = O.psnr(dev, host)
    print(f"PAG job b, 154 unconditional tokens: device loop vs host loop {p:.1f} dB")
    assert p >= HOST_PSNR_MIN
    assert not np.array_equal(dev, sd.generate_image(P, **{**kw, "negative_prompt": None}))


def test_sharded_pag_equals_unsharded(gpu):
    """A one-rank process group with forced collectives (as tests/test_rccl_gpu.py): the sharded PAG job == the unsharded one."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(HERE, "_pag_world1_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=570)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert any(line.startswith("OK ") for line in p.stdout.splitlines()), p.stdout[-2000:]
    print(p.stdout.strip().splitlines()[-1])


def test_first_block_with_and_without_the_shared_prefix(gpu, nets, monkeypatch):
    """down_blocks.0.attentions.0 selected: its front is no longer identical across the copies of the fused batch, so nothing is
    shared there - the same bits with MSD_SHARE_CFG_PREFIX at 1 and at 0 (engine.SHARE_CFG_PREFIX, read when a plan is recorded),
    while a job that does not select it still shares the prefix."""
    import minsdtf_amd.engine as eng_mod

    kw = dict(batch_size=2, num_steps=3, seed=7, guidance_rescale=0.7, return_latent=True)
    first = dict(scale=3.0, layers=["down_blocks.0.attentions.0", "mid_block.attentions.0"])
    out, replicas = {}, {}
    for flag in (True, False):
        monkeypatch.setattr(eng_mod, "SHARE_CFG_PREFIX", flag)
        sd, (P, _Q) = _pipe(gpu, nets)
        out[flag] = sd.generate_image(P, pag=first, **kw)
        replicas[flag] = sum(c.name.endswith(".replicate") for c in next(iter(sd._engines.values())).calls)
        if flag:
            other = sd.generate_image(P, pag=dict(scale=3.0, layers=LAYERS_B), **kw)
            assert sum(c.name.endswith(".replicate") for c in next(iter(sd._engines.values())).calls) > 0
            assert not np.array_equal(other, out[flag])
    assert replicas == {True: 0, False: 0}
    np.testing.assert_array_equal(out[True], out[False])
    assert np.all(np.isfinite(out[True]))
