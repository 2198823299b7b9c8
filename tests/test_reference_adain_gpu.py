"""msd_reference_adain on the GPU: the kernel against the float64 statement between guard bands, the bit-for-bit promises of the
header (mix = NULL / 1, a copy of the reference, one changed reference channel, independence of the launch's other rows), and the
reference-only job with reference AdaIN through the pipeline (device loop against host loop, graph forms, residency, oracle
fixtures, sharding)."""
import os

import numpy as np
import pytest
import torch

import _extents_reference_adain as XA
import _guard as G
from _checks import bf
from conftest import run_calls

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAN = float("nan")
EPS = 1e-6
HW_MAX = 4096   # the longest sum of the cases below: the bound's second term is HW_MAX * 2^-24


def bits(x):
    return x.view(torch.int16)


def launch(dev, x, ref, mix):
    """x [rows, hw, c] and ref [hw, c] (fp32 holding bf16 values) as two operands between guard bands, mix a list or None ->
    (the rewritten rows, fp32 on the CPU).  The reference operand and every band must come back untouched."""
    from minsdtf_amd import ops

    rows, hw, c = x.shape
    geo = dict(rows=rows, hw=hw, c=c)
    g = G.Guard(dev, XA.reference_adain(x=1, ref=1, mix=None if mix is None else 1, **geo))
    xd = g.inp(x.to(BF16), "x")
    rd = g.inp(ref.to(BF16), "ref")
    md = None if mix is None else g.inp(torch.as_tensor(mix, dtype=torch.float32), "mix")
    before = rd.clone()
    run_calls(ops.reference_adain(x=xd, ref=rd, mix=md, eps=EPS, **geo))
    g.check()
    assert torch.equal(bits(rd), bits(before)), "the reference row was written"
    return xd.clone().cpu()


def data(seed, rows, hw, c, x_stat=(0.0, 1.0), r_stat=(0.0, 1.0)):
    """Rows with per-channel offsets and scales around (mean, std) `x_stat`, a reference likewise around `r_stat`: bf16 values."""
    gen = torch.Generator().manual_seed(seed)

    def draw(n, stat):
        mean = stat[0] + stat[1] * torch.randn(n, 1, c, generator=gen)
        std = stat[1] * (0.5 + torch.rand(n, 1, c, generator=gen))
        return bf(mean + std * torch.randn(n, hw, c, generator=gen))

    return draw(rows, x_stat), draw(1, r_stat)[0]


def check(got, x, ref, mix, what):
    """|out - want| <= 2^-8 |want| + 2^-12 (|x A| + |Bc|): one bf16 rounding with a factor two of margin, and HW_MAX * 2^-24, the
    worst-case bound of an fp32 sum of 4096 terms in any order, on the two terms of the FMA (A, Bc in float64)."""
    from minsdtf_amd import reference as R

    x64, r64 = x.double().numpy(), ref.double().numpy()
    rows = x.shape[0]
    m = np.zeros(rows) if mix is None else np.asarray(mix, dtype=np.float64)
    want = R.adain_reference(x64, r64, mix, EPS)
    mean_r = r64.mean(0)
    std_r = np.sqrt(((r64 - mean_r) ** 2).mean(0) + EPS)
    for b in range(rows):
        mean = x64[b].mean(0)
        s = std_r / np.sqrt(((x64[b] - mean) ** 2).mean(0) + EPS)
        g_ = 1.0 - m[b]
        A, Bc = g_ * s + m[b], g_ * (mean_r - mean * s)
        tol = 2.0 ** -8 * np.abs(want[b]) + (HW_MAX * 2.0 ** -24) * (np.abs(x64[b] * A) + np.abs(Bc))
        out = got[b].double().numpy()
        assert np.isfinite(out).all(), f"{what}: row {b} holds a value that is not finite"
        err = np.abs(out - want[b])
        worst = float((err / np.maximum(tol, 1e-300)).max())
        print(f"{what}, row {b} (mix {m[b]:g}): max |err| {float(err.max()):.3g}, worst err / bound {worst:.3f}")
        assert worst <= 1.0, f"{what}: row {b}: err / bound = {worst:.3f}"


def mixes(rows):
    full = [[0.0, 0.5], [1.0, 0.25]]
    return [m[-rows:] if rows < 2 else (m * rows)[:rows] for m in full] + [None]


# (rows, hw, c): the default sites of a 512 px job (8 x 8, 16 x 16 at C = 1280), a 32 x 32 level, a 3 x 3 level, one pixel, c no
# multiple of the 64-channel slab with hw no multiple of the 32 pixel lanes, the re-reading path, and both sides of every hw at
# which the kernel changes form (64 / 65, 256 / 257, ops.ADAIN_RESIDENT_HW = 1024 / 1025)
CASES = [(2, 64, 1280), (2, 256, 1280), (1, 1024, 640), (2, 9, 640), (1, 1, 1280), (2, 70, 24), (1, 4096, 640),
         (2, 65, 72), (2, 257, 72), (2, 1025, 72)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernel_against_reference(gpu, case):
    from minsdtf_amd import ops

    assert ops.ADAIN_RESIDENT_HW == 1024 and max(c[1] for c in CASES) == HW_MAX
    rows, hw, c = case
    x, ref = data(21, rows, hw, c)
    for mix in mixes(rows):
        got = launch(gpu, x, ref, mix)
        check(got.float(), x, ref, mix, f"{case} mix {mix}")
        if mix is not None:
            for b, f in enumerate(mix):
                if f == 1.0:
                    assert torch.equal(bits(got[b]), bits(x[b].to(BF16)))


@pytest.mark.parametrize("x_stat, r_stat", [((200.0, 2.0), (-12.0, 3.0)), ((-12.0, 3.0), (200.0, 2.0))], ids=["x200-r-12", "x-12-r200"])
@pytest.mark.parametrize("case", [(2, 256, 1280), (2, 1025, 72)], ids=lambda c: "x".join(map(str, c)))
def test_offset_data(gpu, case, x_stat, r_stat):
    """A mean a hundred standard deviations from zero: E[x^2] - mean^2 would lose the variance; the two-pass form keeps the bound."""
    rows, hw, c = case
    gen = torch.Generator().manual_seed(5)
    x = bf(x_stat[0] + x_stat[1] * torch.randn(rows, hw, c, generator=gen))
    ref = bf(r_stat[0] + r_stat[1] * torch.randn(hw, c, generator=gen))
    for mix in ([0.0, 0.5], None):
        check(launch(gpu, x, ref, mix).float(), x, ref, mix, f"{case} x~N{x_stat} ref~N{r_stat} mix {mix}")


def test_null_mix_is_mix_zero(gpu):
    x, ref = data(3, 2, 100, 136)
    assert torch.equal(bits(launch(gpu, x, ref, None)), bits(launch(gpu, x, ref, [0.0, 0.0])))


@pytest.mark.parametrize("hw", [70, 1100])
def test_mix_one_row_is_neither_read_nor_written(gpu, hw):
    x, ref = data(4, 3, hw, 72)
    x[1] = NAN
    got = launch(gpu, x, ref, [0.5, 1.0, 0.0])
    assert torch.equal(bits(got[1]), bits(x[1].to(BF16)))
    assert bool(torch.isfinite(got[0].float()).all()) and bool(torch.isfinite(got[2].float()).all())
    clean = x.clone()
    clean[1] = 0.0
    other = launch(gpu, clean, ref, [0.5, 1.0, 0.0])
    assert torch.equal(bits(got[0]), bits(other[0])) and torch.equal(bits(got[2]), bits(other[2]))


@pytest.mark.parametrize("hw", [64, 300, 1030])
def test_copy_of_the_reference_comes_back_bit_identical(gpu, hw):
    """s = 1 and Bc = 0 exactly, at every mix: both statistics run through the same arithmetic in the same order."""
    x, ref = data(6, 4, hw, 136)
    for b in (0, 2, 3):
        x[b] = ref
    got = launch(gpu, x, ref, [0.0, 0.3, 0.5, 0.9])
    want = ref.to(BF16)
    for b in (0, 2, 3):
        assert torch.equal(bits(got[b]), bits(want)), f"row {b}"
    assert not torch.equal(bits(got[1]), bits(x[1].to(BF16)))


def test_one_reference_channel_moves_one_output_channel(gpu):
    x, ref = data(7, 2, 90, 136)
    base = launch(gpu, x, ref, [0.0, 0.5])
    for ch in (0, 71, 135):
        other = ref.clone()
        other[:, ch] = bf(other[:, ch] * 1.5 + 0.75)
        got = launch(gpu, x, other, [0.0, 0.5])
        same = torch.ones(136, dtype=torch.bool)
        same[ch] = False
        assert torch.equal(bits(got[:, :, same]), bits(base[:, :, same])), f"channel {ch} reached another channel"
        assert not torch.equal(bits(got[0, :, ch]), bits(base[0, :, ch])) and not torch.equal(bits(got[1, :, ch]), bits(base[1, :, ch]))


@pytest.mark.parametrize("hw", [256, 1100])
def test_row_bits_do_not_depend_on_the_launch_and_runs_repeat(gpu, hw):
    x, ref = data(8, 5, hw, 136)
    mix = [0.0, 0.5, 1.0, 0.25, 0.75]
    full = launch(gpu, x, ref, mix)
    assert torch.equal(bits(full), bits(launch(gpu, x, ref, mix)))
    two = launch(gpu, x[[3, 1]], ref, [mix[3], mix[1]])
    assert torch.equal(bits(two[0]), bits(full[3])) and torch.equal(bits(two[1]), bits(full[1]))


# ---------------------------------------------------------------------------------------------------------------- pipelines
PSNR_MIN = 40.0           # the project's bar for every job
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


COMBOS = {"auto+attn": dict(adain="auto", layers="all"), "all-alone": dict(adain="all", layers=[])}


@pytest.mark.parametrize("fidelity, sampler", [(0.0, None), (0.5, None), (1.0, None), (0.5, "dpmpp_2m")])
@pytest.mark.parametrize("combo", list(COMBOS))
def test_device_loop_vs_host_loop(gpu, nets, combo, fidelity, sampler):
    """The device loop against host_loop=True (DiffusionModel.predict_reference(..., adain=...) through _guided_eps): 40 dB, or
    45 dB with a samplers.py sampler."""
    from oracle import sd_oracle as O

    sd, (P, _Q) = _pipe(gpu, nets)
    spec = dict(latent=_z(), fidelity=fidelity, **COMBOS[combo])
    kw = dict(batch_size=2, num_steps=4, seed=11, return_latent=True, sampler=sampler, guidance_rescale=0.7, reference_only=spec)
    dev = sd.generate_image(P, **kw)
    eng = next(iter(sd._engines.values()))
    names = _names(eng)
    n_sites, n_joint = (7, 16) if combo == "auto+attn" else (15, 0)
    assert eng.passes == [(0, 5, 77, "both")] and len(eng.adain) == n_sites
    assert sum(n.endswith(".adain") for n in names) == n_sites and sum(n.endswith(".attn1.joint") for n in names) == n_joint
    host = sd.generate_image(P, host_loop=True, **kw)
    p = O.psnr(dev, host)
    bar = SAMPLER_PSNR_MIN if sampler else PSNR_MIN
    print(f"reference AdaIN job {combo}, fidelity {fidelity} ({sampler or 'default sampler'}): device loop vs host loop {p:.1f} dB (bar {bar:.0f})")
    assert p >= bar
    off = sd.generate_image(P, **dict(kw, reference_only=dict(spec, adain=None, layers="all")))
    assert not np.array_equal(dev, off)


def test_predict_reference_with_mix_one_is_predict_on_batch(gpu, nets):
    """mix = 1 everywhere: no site touches a generated row (and no block mixes the reference keys in): predict_on_batch's bits."""
    from minsdtf_amd import reference as R

    unet = nets["unet"]
    rng = np.random.default_rng(2)
    lat = rng.standard_normal((2, 8, 8, 4)).astype(np.float32)
    from oracle import sd_oracle as O

    temb = O.timestep_embedding(500, 2)
    ctx = rng.standard_normal((2, 77, 768)).astype(np.float32)
    ref = unet.predict_on_batch([lat, temb, ctx])
    sites = [n for n, _gw in R.ADAIN_SITES]
    got = unet.predict_reference([lat, temb, ctx], 3.0 * _z(5), [], 1.0, adain=sites)
    np.testing.assert_array_equal(got, ref)
    moved = unet.predict_reference([lat, temb, ctx], 3.0 * _z(5), [], [0.0, 1.0], adain=sites)
    np.testing.assert_array_equal(moved[1], ref[1])
    assert not np.array_equal(moved[0], ref[0]) and np.all(np.isfinite(moved))
    with pytest.raises(ValueError, match="adain site"):
        unet.predict_reference([lat, temb, ctx], _z(5), [], 1.0, adain=["mid_block.resnets.0"])
    with pytest.raises(ValueError, match="layers"):
        unet.predict_reference([lat, temb, ctx], _z(5), [], 1.0)


def test_graph_forms_agree(gpu, nets):
    """The whole-loop graph == per-step graphs (a callback is installed) == eager launches (jit_compile=False), bit for bit."""
    sd, (P, _Q) = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=3, seed=8, return_latent=True, sampler="dpmpp_2m", guidance_rescale=0.7,
              reference_only=dict(latent=_z(), fidelity=0.5, adain="all"))
    whole = sd.generate_image(P, **kw)
    calls = []
    stepped = sd.generate_image(P, callback=calls.append, **kw)
    assert calls == [1, 2, 3]
    eng = next(iter(sd._engines.values()))
    assert eng._loop_graph is not None and eng._step_graph is not None and len(eng.reference) == 16 and len(eng.adain) == 15
    eager_sd, _ = _pipe(gpu, nets, jit=False)
    np.testing.assert_array_equal(stepped, whole)
    np.testing.assert_array_equal(eager_sd.generate_image(P, **kw), whole)
    assert np.all(np.isfinite(whole))


def test_residency(gpu, nets, monkeypatch):
    """Another latent, draw and fidelity with the same sites build no engine and capture no graph; another site set builds one."""
    import minsdtf_amd.stable_diffusion as sdm

    built = []
    init = sdm.DenoiseEngine.__init__

    def counting(self, *a, **k):
        built.append((k.get("reference"), k.get("adain")))
        init(self, *a, **k)

    monkeypatch.setattr(sdm.DenoiseEngine, "__init__", counting)
    sd, (P, _Q) = _pipe(gpu, nets)
    kw = dict(batch_size=1, num_steps=3, seed=5, guidance_rescale=0.7, return_latent=True)
    first = sd.generate_image(P, reference_only=dict(latent=_z(1), layers="mid", fidelity=0.5, adain="auto"), **kw)
    assert len(built) == 1 and built[0][0] == ("mid_block.attentions.0",) and len(built[0][1]) == 7
    eng = next(iter(sd._engines.values()))
    graph = eng._loop_graph
    other = dict(latent=_z(2, 2.0), layers="mid", fidelity=0.9, noise=_z(3), adain=1.0)
    second = sd.generate_image(P, reference_only=other, **kw)
    assert len(built) == 1 and next(iter(sd._engines.values())) is eng and eng._loop_graph is graph
    assert not np.array_equal(first, second)
    sd.generate_image(P, reference_only=dict(other, adain=0.5), **kw)
    assert len(built) == 2 and len(built[-1][1]) == 4
    sd.generate_image(P, reference_only=dict(other, adain=None), **kw)
    assert len(built) == 3 and built[-1][1] is None


def test_guidance_zero_job_runs(gpu, nets):
    sd, (P, _Q) = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=3, seed=2, unconditional_guidance_scale=0.0, return_latent=True)
    got = sd.generate_image(P, reference_only=dict(latent=_z(), layers=[], adain="auto"), **kw)
    eng = next(iter(sd._engines.values()))
    assert eng.passes == [(0, 3, 77, "cond")] and eng.eps.shape[0] == 3 and eng.ref_mix.shape[0] == 2 and eng.reference == frozenset()
    assert np.all(np.isfinite(got)) and not np.array_equal(got, sd.generate_image(P, **kw))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_against_the_oracle_fixture(gpu, nets, tag):
    """tests/golden/oracle_reference_adain_{a,b}.npz (tools/make_reference_adain_fixtures.py): final latent PSNR >= 40 dB on the
    whole batch and on each sample; the plain job and the job with adain off are below 30 dB, so the bar tells them apart."""
    from minsdtf_amd.models import DiffusionModel
    from minsdtf_amd.stable_diffusion import StableDiffusion
    from oracle import sd_oracle as O

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"oracle_reference_adain_{tag}.npz"))
    assert (int(g["weight_seed"]), float(g["bias_scale"])) == (0, 0.05) and float(g["plain_psnr"]) < 30.0 and float(g["attn_only_psnr"]) < 30.0
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
    job = dict(latent=z_ref, noise=n_ref, fidelity=float(g["fidelity"]), layers=[str(n) for n in g["layers"]], adain=str(g["adain"]))
    got = sd.generate_image(base, batch_size=B, num_steps=int(g["steps"]), unconditional_guidance_scale=float(g["guidance"]),
                            seed=int(g["noise_seed"]), guidance_rescale=float(g["guidance_rescale"]), return_latent=True,
                            sampler=str(g["sampler"]) or None, reference_only=job)
    eng = next(iter(sd._engines.values()))
    assert eng.adain == frozenset(str(n) for n in g["sites"]) and eng.reference == frozenset(job["layers"]) and eng.eps.shape[0] == 2 * B + 1
    p = O.psnr(got, g["latent"])
    per = [round(O.psnr(got[b], g["latent"][b]), 1) for b in range(B)]
    print(f"reference AdaIN job {tag}: final latent PSNR {p:.1f} dB (per sample {per}); the plain job is at {float(g['plain_psnr']):.1f} dB, "
          f"the job with adain off at {float(g['attn_only_psnr']):.1f} dB")
    assert p >= PSNR_MIN and min(per) >= PSNR_MIN


def test_sharded_job_equals_unsharded(gpu):
    """A one-rank process group with forced collectives (as tests/test_regions_gpu.py): the sharded job == the unsharded one.  (A
    child process is what the test is about: the group must exist before anything touches the GPU.)"""
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(here, "_reference_adain_world1_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=570)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert any(line.startswith("OK ") for line in p.stdout.splitlines()), p.stdout[-2000:]
    print(p.stdout.strip().splitlines()[-1])
