"""msdi_attention_decoupled on the GPU: the kernel against the float64 statement (ipadapter.attention_reference) and an fp32 torch
reference between guard bands, its promises (scale 0 reads no image operand, the table row and column, batch independence), and the
image-prompt job through the pipeline."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _extents_ipadapter as XI
import _guard as G
from _checks import bf, close
from conftest import run_calls

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
NAN = float("nan")
LOG2E = 1.4426950408889634


def guarded(dev, q, k, v, k_ip, v_ip, table, *, H, d, step=0, layer=0, wide=True, poison=True):
    """The operands of one launch between guard bands, sized by the header's extents.  wide: q / k / k_ip / out are rows of wider
    buffers and vt / vt_ip have spare columns; that padding holds NaN (poison) or zeros, out's spare columns a canary."""
    B, S, C = q.shape
    T, N = k.shape[1], k_ip.shape[1]
    assert C == H * d
    q_ld, k_ld, kip_ld, o_ld = (3 * C, C + 8, C + 16, C + 16) if wide else (C, C, C, C)
    vt_ld = (T + 7) // 8 * 8 + (8 if wide else 0)
    vtip_ld = (N + 7) // 8 * 8 + (8 if wide else 0)
    geo = dict(batch=B, heads=H, head_dim=d, s=S, t=T, n=N, q_ld=q_ld, k_ld=k_ld, vt_ld=vt_ld, kip_ld=kip_ld, vtip_ld=vtip_ld, o_ld=o_ld,
               layer=layer, num_steps=table.shape[0])
    g = G.Guard(dev, XI.ip_attention(q=1, k=1, vt=1, k_ip=1, vt_ip=1, scales=1, step_ptr=1, out=1, **geo))
    pad = None if poison else 0.0

    def rows(x, name, ld):
        x2 = x.to(BF16).reshape(-1, C)
        return g.inp(x2, name, ld=ld if ld > C else None, gap=pad)

    def transposed(x, name, ld):
        n = x.shape[1]
        t = g.out((B, C, ld), BF16, 0.0, name)
        t[:, :, :n] = x.permute(0, 2, 1).to(BF16).to(dev)
        g.operands[-1].role = "in"
        g.gaps(t, n, gap=pad)
        return t

    qd, kd, kid = rows(q, "q", q_ld), rows(k, "k", k_ld), rows(k_ip, "k_ip", kip_ld)
    vt, vti = transposed(v, "vt", vt_ld), transposed(v_ip, "vt_ip", vtip_ld)
    sc = g.inp(table.to(torch.float32), "scales")
    sp = g.inp(torch.tensor([step], dtype=torch.int32), "step_ptr")
    out = g.out((B * S, C), BF16, NAN, "out", ld=o_ld if o_ld > C else None)
    return g, dict(q=qd, k=kd, vt=vt, k_ip=kid, vt_ip=vti, scales=sc, step_ptr=sp, out=out, **geo), out


def launch(dev, q, k, v, k_ip, v_ip, table, **kw):
    from minsdtf_amd import ops

    g, args, out = guarded(dev, q, k, v, k_ip, v_ip, table, **kw)
    run_calls(ops.ip_attention(**args))
    g.check()
    B, S, C = q.shape
    return out.reshape(B, S, C).clone().cpu()


def table_of(s, steps=1, layer=0):
    t = torch.zeros(steps, 16)
    t[:, layer] = s
    return t


def attention32(q, k, v, H, d):
    """fp32 torch attention on the bf16-rounded inputs (q carries scale * log2(e))."""
    B, S, C = q.shape
    qh = q.view(B, S, H, d).permute(0, 2, 1, 3)
    kh = k.view(B, -1, H, d).permute(0, 2, 1, 3)
    vh = v.view(B, -1, H, d).permute(0, 2, 1, 3)
    return (torch.softmax((qh @ kh.transpose(-1, -2)) * math.log(2.0), -1) @ vh).permute(0, 2, 1, 3).reshape(B, S, C)


def operands(seed, B, H, d, S, T, N, spike=False):
    gen = torch.Generator().manual_seed(seed)
    C = H * d
    q = bf(torch.randn(B, S, C, generator=gen) * (d ** -0.5 * LOG2E))
    k, v = bf(torch.randn(B, T, C, generator=gen)), bf(torch.randn(B, T, C, generator=gen))
    k_ip, v_ip = bf(torch.randn(B, N, C, generator=gen)), bf(torch.randn(B, N, C, generator=gen))
    if spike:
        k_ip[:, N // 2] *= 8.0
        k_ip = bf(k_ip)
    return q, k, v, k_ip, v_ip


def bound(text, image, s):
    """Each term meets test_attention's bound (rtol 2e-2, atol 1.5e-2 max(1, max|term|)): their sum the same rtol and the atols added."""
    return 1.5e-2 * (max(1.0, float(text.abs().max())) + abs(s) * max(1.0, float(image.abs().max())))


KERNEL_CASES = [
    dict(B=2, H=2, d=40, S=200, T=77, N=4, s=1.0),                  # ragged query tile, pad keys 77 .. 79
    dict(B=1, H=2, d=80, S=128, T=80, N=16, s=0.6),                 # the full tile
    dict(B=3, H=1, d=160, S=64, T=13, N=16, s=1.5, spike=True),     # short text, one dominant image key
    dict(B=1, H=8, d=160, S=1, T=77, N=4, s=1.0),                   # the one-token mid block
    dict(B=1, H=2, d=40, S=64, T=77, N=1, s=1.0),                   # a single image token: its softmax is 1
]


@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "-".join(f"{k}{v:g}" for k, v in c.items()))
def test_kernel_against_reference(gpu, case):
    """The padding (V^T's columns >= T / >= N, the wide q / k / k_ip buffers, out's spare columns) holds NaN, then zeros: the same
    bits.  Against the fp32 torch reference and the project's float64 statement, at the bound of bound()."""
    from minsdtf_amd import ipadapter

    B, H, d, S, T, N, s = (case[x] for x in ("B", "H", "d", "S", "T", "N", "s"))
    q, k, v, k_ip, v_ip = operands(11, B, H, d, S, T, N, case.get("spike", False))
    text, image = attention32(q, k, v, H, d), attention32(q, k_ip, v_ip, H, d)
    ref = (text.double() + s * image.double()).float()
    atol = bound(text, image, s)
    a = launch(gpu, q, k, v, k_ip, v_ip, table_of(s), H=H, d=d, poison=True)
    b = launch(gpu, q, k, v, k_ip, v_ip, table_of(s), H=H, d=d, poison=False)
    err = float((a.float() - ref).abs().max())
    print(f"{case}: max |got - ref| = {err:.4g}, atol = {atol:.4g}, max |ref| = {float(ref.abs().max()):.4g}")
    close(a, ref, rtol=2e-2, atol=atol, what=str(case))
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{case}: the content of a padding region reached the result"
    ref64 = ipadapter.attention_reference(q.numpy(), k.numpy(), v.numpy(), k_ip.numpy(), v_ip.numpy(), s, H)
    close(a, torch.from_numpy(ref64).float(), rtol=2e-2, atol=atol, what=f"{case} float64")
    if N == 1:   # the image term is s * v_ip itself
        assert float((image - v_ip.expand(B, S, H * d)).abs().max()) < 1e-5


@pytest.mark.parametrize("d,S,T,N", [(40, 200, 77, 4), (160, 70, 77, 16)])
def test_scale_zero_reads_no_image_operand(gpu, d, S, T, N):
    """s == 0 in the table: the same bits with k_ip / vt_ip holding NaN as with random data, within the attention bound of
    msd_attention on the text keys."""
    from minsdtf_amd import ops

    B, H = 2, 2
    C = H * d
    q, k, v, k_ip, v_ip = operands(4, B, H, d, S, T, N)
    nan = torch.full((B, N, C), NAN)
    a = launch(gpu, q, k, v, k_ip, v_ip, table_of(0.0), H=H, d=d)
    b = launch(gpu, q, k, v, nan, nan, table_of(0.0), H=H, d=d)
    assert bool(torch.isfinite(b.float()).all())
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    Tp = (T + 7) // 8 * 8
    qd, kd = q.to(BF16).to(gpu), k.to(BF16).to(gpu)
    vt = torch.zeros(B, C, Tp, dtype=BF16, device=gpu)
    vt[:, :, :T] = v.permute(0, 2, 1).to(BF16).to(gpu)
    out = torch.empty(B, S, C, dtype=BF16, device=gpu)
    run_calls(ops.attention(q=qd, k=kd, vt=vt, out=out, batch=B, heads=H, head_dim=d, s=S, t=T, q_ld=C, k_ld=C, vt_ld=Tp, o_ld=C,
                            scale=1.0, q_prescaled=True))
    ref = out.float().cpu()
    close(a, ref, rtol=2e-2, atol=1.5e-2 * max(1.0, float(ref.abs().max())), what=f"d={d} against msd_attention")


def test_table_row_and_column_are_the_ones_read(gpu):
    """Two rows, two scales: *step_ptr selects the row; a column other than `layer` holds NaN and is not read."""
    B, H, d, S, T, N = 1, 2, 80, 100, 77, 4
    q, k, v, k_ip, v_ip = operands(5, B, H, d, S, T, N)
    text, image = attention32(q, k, v, H, d), attention32(q, k_ip, v_ip, H, d)
    layer = 9
    table = torch.full((2, 16), NAN)
    table[0, layer], table[1, layer] = 0.25, 2.0
    got = [launch(gpu, q, k, v, k_ip, v_ip, table, H=H, d=d, step=i, layer=layer) for i in (0, 1)]
    for g_, s in zip(got, (0.25, 2.0)):
        close(g_, (text.double() + s * image.double()).float(), rtol=2e-2, atol=bound(text, image, s), what=f"scale {s}")
    assert not torch.equal(got[0].view(torch.int16), got[1].view(torch.int16))
    # the same scale in column 0 of a one-row table: the same bits
    same = launch(gpu, q, k, v, k_ip, v_ip, table_of(2.0), H=H, d=d)
    assert torch.equal(same.view(torch.int16), got[1].view(torch.int16))


def test_sample_bits_do_not_depend_on_the_batch_and_runs_repeat(gpu):
    B, H, d, S, T, N = 3, 2, 160, 100, 50, 16
    q, k, v, k_ip, v_ip = operands(6, B, H, d, S, T, N)
    full = launch(gpu, q, k, v, k_ip, v_ip, table_of(0.8), H=H, d=d)
    again = launch(gpu, q, k, v, k_ip, v_ip, table_of(0.8), H=H, d=d)
    assert torch.equal(full.view(torch.int16), again.view(torch.int16))
    for b in (0, 2):
        alone = launch(gpu, q[b:b + 1], k[b:b + 1], v[b:b + 1], k_ip[b:b + 1], v_ip[b:b + 1], table_of(0.8), H=H, d=d, wide=False)
        assert torch.equal(alone[0].view(torch.int16), full[b].view(torch.int16)), f"sample {b}"


# ------------------------------------------------------------------------------------------------------------------- jobs
GOLD = os.path.join(ROOT, "tests", "golden")
PSNR_MIN = 40.0        # the project's bar for every job
HOST_PSNR_MIN = 45.0   # device loop vs host_loop=True of a samplers.py txt2img job (test_pag_gpu.py, test_regions_gpu.py)


@pytest.fixture(scope="module")
def nets(gpu):
    """The synthetic UNet, decoder, encoder and ControlNet / HintNet at 64 x 64 (the fixture sizes share the UNet's packed weights),
    and two synthetic adapters of 4 image tokens."""
    from minsdtf_amd.models import ControlNet, DiffusionModel, HintNet, ImageDecoder, ImageEncoder, IPAdapter

    out = {}
    for name, cls in (("unet", DiffusionModel), ("cn", ControlNet), ("hn", HintNet)):
        m = cls(64, 64, device=gpu)
        m.load_synthetic(seed=0, bias_scale=0.05)
        out[(name, 64)] = m
    for size in (128, 256):
        v = DiffusionModel(size, size, device=gpu)
        v.share_weights(out[("unet", 64)])
        out[("unet", size)] = v
    out["dec"] = ImageDecoder(device=gpu)
    out["dec"].load_synthetic(seed=0, bias_scale=0.05)
    out["enc"] = ImageEncoder(device=gpu)
    out["enc"].load_synthetic(seed=0, bias_scale=0.05)
    out["ip"] = IPAdapter.synthetic(5, 4, device=gpu)
    return out


def _pipe(gpu, nets, size=64, jit=True, control=False, **kw):
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sd = StableDiffusion(size, size, jit_compile=jit, device=gpu, **(dict(controlnet_path="synthetic") if control else {}), **kw)
    sd._diffusion_model, sd._image_decoder, sd._image_encoder = nets[("unet", size)], nets["dec"], nets["enc"]
    if control:
        sd._control_net, sd._hint_net = nets[("cn", size)], nets[("hn", size)]
    return sd


_RNG = np.random.default_rng(78)
CTX = _RNG.standard_normal((77, 768)).astype(np.float32)
UNC = _RNG.standard_normal((77, 768)).astype(np.float32)
UNC_SHORT = _RNG.standard_normal((40, 768)).astype(np.float32)
EMB_A, EMB_B = _RNG.standard_normal(1024), _RNG.standard_normal(1024)
IMG = _RNG.integers(0, 256, (64, 64, 3)).astype(np.float32)
PICTURE = _RNG.integers(0, 256, (64, 64, 3)).astype(np.uint8)
KW = dict(batch_size=1, num_steps=3, unconditional_guidance_scale=7.5, guidance_rescale=0.7, seed=5, return_latent=True)


def _ipa(nets, emb=EMB_A, **kw):
    return dict(embeds=emb, model=nets["ip"], **kw)


def _job(sd, **kw):
    sd.unconditional_context = UNC
    return sd.generate_image(CTX, **{**KW, **kw})


@pytest.mark.parametrize("size", [128, 256])
def test_vs_oracle_fixture(gpu, nets, size):
    """The fixture jobs against the fp32 oracle's composition (tools/make_ip_adapter_fixtures.py: sd_oracle.cross_attention wrapped
    for every attn2): final latent PSNR >= 40 dB, where the plain job stays under 35 dB (`plain_psnr` in the file)."""
    from minsdtf_amd.models import IPAdapter
    from oracle import sd_oracle as O

    g = np.load(os.path.join(GOLD, f"ip_adapter_{size}.npz"))
    assert (int(g["weight_seed"]), float(g["bias_scale"])) == (0, 0.05) and float(g["plain_psnr"]) < 35.0
    sd = _pipe(gpu, nets, size)
    rng = np.random.default_rng(int(g["context_seed"]))
    ctx = rng.standard_normal((1, 77, 768)).astype(np.float32)[0]
    sd.unconditional_context = rng.standard_normal((1, 77, 768)).astype(np.float32)[0]
    adapter = nets["ip"] if int(g["adapter_seed"]) == 5 else IPAdapter.synthetic(int(g["adapter_seed"]), int(g["tokens"]), device=gpu)
    spec = dict(embeds=np.random.default_rng(int(g["embed_seed"])).standard_normal(1024), model=adapter, weight=float(g["weight"]),
                start=float(g["start"]), end=float(g["end"]), weight_type=str(g["weight_type"]))
    kw = dict(batch_size=1, num_steps=int(g["steps"]), unconditional_guidance_scale=float(g["guidance"]), seed=int(g["noise_seed"]),
              return_latent=True)
    got = sd.generate_image(ctx, ip_adapter=spec, **kw)
    p = O.psnr(got, g["latent"])
    plain = O.psnr(sd.generate_image(ctx, **kw), g["latent"])
    print(f"ip_adapter fixture {size}x{size} ({spec['weight_type']}, weight {spec['weight']}): final latent PSNR {p:.1f} dB; the plain job "
          f"{plain:.1f} dB on the device, {float(g['plain_psnr']):.1f} dB in the oracle")
    assert p >= PSNR_MIN
    assert plain < PSNR_MIN   # (by construction)


@pytest.mark.parametrize("sampler, steps", [(None, 3), ("dpmpp_2m_karras", 8)])
def test_device_loop_vs_host_loop(gpu, nets, sampler, steps):
    """The device loop against host_loop=True (DiffusionModel.predict_ip per half) at test_pag_gpu.py's bars for those two routes:
    the default step 40 dB, a samplers.py sampler 45 dB."""
    from oracle import sd_oracle as O

    sd = _pipe(gpu, nets)
    kw = dict(ip_adapter=_ipa(nets, weight=0.9, end=0.75), sampler=sampler, num_steps=steps)
    dev = _job(sd, **kw)
    host = _job(sd, host_loop=True, **kw)
    plain = _job(sd, sampler=sampler, num_steps=steps)
    p, q = O.psnr(dev, host), O.psnr(plain, host)
    bar = HOST_PSNR_MIN if sampler is not None else PSNR_MIN
    print(f"ip_adapter, sampler {sampler}, {steps} steps: device loop vs host loop {p:.1f} dB (bar {bar:.0f}); the plain job against it {q:.1f} dB")
    assert p >= bar and q < p


@pytest.mark.parametrize("form", ["euler_a", "tcd", "short_negative", "no_guidance", "dynamic_threshold", "inpaint", "eager"])
def test_forms_run_and_repeat(gpu, nets, form):
    """Every sampler route, a TCD pipeline, two passes, no guidance, dynamic thresholding and inpainting: the job runs, repeats its bits
    and differs from the job without the image prompt."""
    sd = _pipe(gpu, nets, jit=form != "eager", **(dict(active_tcd=True) if form == "tcd" else {}))
    kw = {"euler_a": dict(sampler="euler_a"), "short_negative": dict(negative_prompt=UNC_SHORT), "no_guidance": dict(unconditional_guidance_scale=0.0),
          "dynamic_threshold": dict(dynamic_threshold=dict(mimic_scale=5.0)),
          "inpaint": dict(reference_image=PICTURE, reference_image_strength=0.7, inpaint_mask=np.pad(np.full((32, 32), 255.0), 16))}.get(form, {})

    def run(**more):
        np.random.seed(3)   # (the TCD sampler's draws come from numpy's global stream)
        return _job(sd, **kw, **more)

    a = run(ip_adapter=_ipa(nets))
    eng = next(iter(sd._engines.values()))
    assert eng.ip_tokens == 4 and len(eng.passes) == (2 if form == "short_negative" else 1)
    assert sum(c.name.endswith(".attn2.ip") for c in eng.calls) == 16 * len(eng.passes)
    assert np.isfinite(a).all()
    np.testing.assert_array_equal(run(ip_adapter=_ipa(nets)), a)
    assert not np.array_equal(run(), a)


def test_with_control_units_and_image_to_image(gpu, nets):
    sd = _pipe(gpu, nets, control=True)
    units = dict(weight=0.8, mode="prompt", end=0.7)
    both = _job(sd, control_net_image=IMG, control=units, ip_adapter=_ipa(nets))
    eng = next(iter(sd._engines.values()))
    assert eng.control_units == 1 and eng.ip_tokens == 4 and eng.has_control
    # the ControlNet's own encoder stays plain: the 16 decoupled launches are the UNet's
    assert sum(c.name.endswith(".attn2.ip") for c in eng.calls) == 16
    assert not np.array_equal(both, _job(sd, control_net_image=IMG, control=units))
    assert not np.array_equal(both, _job(sd, ip_adapter=_ipa(nets)))
    plain_cn = _job(sd, control_net_image=IMG, ip_adapter=_ipa(nets))
    assert not np.array_equal(plain_cn, both) and np.isfinite(plain_cn).all()
    # image_to_image: strength 0.5 over 4 steps executes rows 2 and 3 of the table; end = 0.5 keeps rows 0 and 1 only
    sd2 = _pipe(gpu, nets)
    kw = dict(num_steps=4, reference_image=PICTURE, reference_image_strength=0.5)
    plain = _job(sd2, **kw)
    on = _job(sd2, ip_adapter=_ipa(nets), **kw)
    assert not np.array_equal(on, plain)
    np.testing.assert_array_equal(_job(sd2, ip_adapter=_ipa(nets, start=0.5), **kw), on)
    off = _job(sd2, ip_adapter=_ipa(nets, end=0.5), **kw)
    assert len(sd2._engines) == 1 and next(iter(sd2._engines.values())).ip_tokens == 4   # (rows 0, 1 are not 0: the IP engine)
    assert not np.array_equal(off, on)
    host_off = _job(sd2, ip_adapter=_ipa(nets, end=0.5), host_loop=True, **kw)
    from oracle import sd_oracle as O

    assert O.psnr(off, host_off) >= PSNR_MIN


def test_all_zero_table_is_the_plain_job(gpu, nets):
    sd = _pipe(gpu, nets)
    plain = _job(sd)
    for spec in (dict(weight=0.0), dict(start=1.0), dict(weight_type={"mid_block.attentions.0": 0.0})):
        np.testing.assert_array_equal(_job(sd, ip_adapter=_ipa(nets, **spec)), plain)
        assert len(sd._engines) == 1 and next(iter(sd._engines.values())).ip_tokens == 0
    # on the IP engine too: a table whose executed rows are 0 has the plain job's bits only if the decoupled launch with s = 0 had
    # msd_cross_attention_q's - it has not (another kernel), so that is asked at the job bar
    from oracle import sd_oracle as O

    late = _job(sd, num_steps=4, reference_image=PICTURE, reference_image_strength=0.5, ip_adapter=_ipa(nets, end=0.5))
    plain_i2i = _job(sd, num_steps=4, reference_image=PICTURE, reference_image_strength=0.5)
    assert O.psnr(late, plain_i2i) >= PSNR_MIN


def test_other_pictures_and_weights_build_no_engine(gpu, nets, monkeypatch):
    import minsdtf_amd.stable_diffusion as sdm

    built = []
    init = sdm.DenoiseEngine.__init__

    def counting(self, *a, **k):
        built.append(k.get("ip_tokens"))
        return init(self, *a, **k)

    monkeypatch.setattr(sdm.DenoiseEngine, "__init__", counting)
    sd = _pipe(gpu, nets)
    a = _ipa(nets, EMB_A, weight=0.8, end=0.75)
    b = _ipa(nets, EMB_B, weight=1.3, start=0.3, weight_type="style")
    first = _job(sd, ip_adapter=a)
    second = _job(sd, ip_adapter=b)
    assert built == [4] and len(sd._engines) == 1
    np.testing.assert_array_equal(_job(sd, ip_adapter=a), first)
    assert built == [4] and not np.array_equal(first, second)
    np.testing.assert_array_equal(_job(_pipe(gpu, nets), ip_adapter=b), second)
    np.testing.assert_array_equal(_job(_pipe(gpu, nets), ip_adapter=a), first)


def test_sharded_job_equals_unsharded(gpu):
    """A one-rank process group with forced collectives (as tests/test_control_units_gpu.py): the sharded job == the unsharded one."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_ip_adapter_world1_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=570)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert any(line.startswith("OK ") for line in p.stdout.splitlines()), p.stdout[-2000:]
    print(p.stdout.strip().splitlines()[-1])
