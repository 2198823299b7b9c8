"""msd_attention_windowed on the GPU: the kernel against the float64 statement between guard bands, the bit-for-bit promises of the
header (a window's arithmetic is that of a launch on its gathered tokens, nothing outside a window reaches it, batch independence),
and the HyperTile job through the pipeline (device loop against host loop, the hires second pass, residency, graph forms, oracle
fixtures, sharding)."""
import numpy as np
import pytest
import torch

import _extents_hypertile as XH
import _guard as G
from _checks import bf, close
from conftest import run_calls

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAN = float("nan")
LOG2E = 1.4426950408889634
B, H = 2, 2


def guarded(dev, q, k, v, *, heads, d, h, w, wh, ww, wide=False, poison=True):
    """The operands of one launch between guard bands, sized by the header's extents: q / k [B, S, C] as rows of a wider buffer,
    v stored transposed with vt_ld >= S columns, out [B, S, C] as rows of o_ld.  The padding - V^T's columns past S, the wide buffers
    outside the head block - holds NaN (poison) or zeros; out's unused columns hold a canary.  Returns (guard, keyword arguments of
    ops.attention_windowed, out)."""
    Bn, S, C = q.shape
    assert C == heads * d and S == h * w
    q_ld, k_ld, o_ld = (3 * C, C + 24, C + 16) if wide else (C, C, C)
    vt_ld = (S + 7) // 8 * 8 + (8 if wide else 0)
    geo = dict(batch=Bn, heads=heads, head_dim=d, h=h, w=w, wh=wh, ww=ww, q_ld=q_ld, k_ld=k_ld, vt_ld=vt_ld, o_ld=o_ld)
    g = G.Guard(dev, XH.attention_windowed(q=1, k=1, vt=1, out=1, **geo))
    pad = None if poison else 0.0
    qd = g.inp(q.to(BF16).reshape(Bn * S, C), "q", ld=q_ld if wide else None, gap=pad)
    kd = g.inp(k.to(BF16).reshape(Bn * S, C), "k", ld=k_ld if wide else None, gap=pad)
    vt = g.out((Bn, C, vt_ld), BF16, 0.0, "vt")
    vt[:, :, :S] = v.permute(0, 2, 1).to(BF16).to(dev)
    g.operands[-1].role = "in"
    g.gaps(vt, S, gap=pad)
    out = g.out((Bn * S, C), BF16, NAN, "out", ld=o_ld if wide else None)
    return g, dict(q=qd, k=kd, vt=vt, out=out, **geo), out


def launch(dev, q, k, v, **kw):
    from minsdtf_amd import ops

    g, args, out = guarded(dev, q, k, v, **kw)
    run_calls(ops.attention_windowed(**args))
    g.check()
    Bn, S, C = q.shape
    return out.reshape(Bn, S, C).clone().cpu()


def bound(ref):
    """The project's attention bound (P rounded to bf16 before the PV product): rtol 2e-2, atol 1.5e-2 max(1, max|ref|)."""
    return dict(rtol=2e-2, atol=1.5e-2 * max(1.0, float(ref.abs().max())))


def bits(x):
    return x.view(torch.int16)


def windows(h, w, wh, ww):
    from minsdtf_amd import hypertile as HT

    return torch.from_numpy(HT.window_tokens(h, w, wh, ww))


# (h, w, wh, ww)
GEOMETRIES = [
    (16, 16, 8, 8),      # one full tile per window
    (24, 16, 12, 8),     # 96 keys: a partial second tile
    (8, 48, 8, 24),      # a 64-key tile ends in the middle of a window row
    (20, 16, 10, 16),    # 160 keys
    (9, 8, 9, 8),        # one window with s = 72
]
HEAD_DIMS = [40, 80, 160]
_CASES = {}


def case(dev, geo, d):
    """Operands, the float64 statement and the image launch (wide leading dimensions, NaN padding) of one geometry and head size:
    computed once, shared by the tests below, never written."""
    key = (geo, d)
    if key not in _CASES:
        h, w, wh, ww = geo
        gen = torch.Generator().manual_seed(17 + d + h * w)
        S, C = h * w, H * d
        q = bf(torch.randn(B, S, C, generator=gen) * (d ** -0.5 * LOG2E))
        k, v = bf(torch.randn(B, S, C, generator=gen)), bf(torch.randn(B, S, C, generator=gen))
        from minsdtf_amd import hypertile as HT

        ref = torch.from_numpy(HT.attention_windowed_reference(q.numpy(), k.numpy(), v.numpy(), H, h, w, wh, ww))
        got = launch(dev, q, k, v, heads=H, d=d, h=h, w=w, wh=wh, ww=ww, wide=True, poison=True)
        _CASES[key] = (q, k, v, ref, got)
    return _CASES[key]


def ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else f"d{v}"


@pytest.mark.parametrize("d", HEAD_DIMS, ids=ids)
@pytest.mark.parametrize("geo", GEOMETRIES, ids=ids)
def test_kernel_against_reference(gpu, geo, d):
    """Every leading dimension wider than its payload; the padding (V^T's columns >= s among it) holds NaN, then zeros: the same
    bits."""
    h, w, wh, ww = geo
    q, k, v, ref, got = case(gpu, geo, d)
    close(got, ref.float(), what=f"{geo} d={d}", **bound(ref))
    zeros = launch(gpu, q, k, v, heads=H, d=d, h=h, w=w, wh=wh, ww=ww, wide=True, poison=False)
    assert torch.equal(bits(got), bits(zeros)), f"{geo}: the content of a padding region reached the result"
    narrow = launch(gpu, q, k, v, heads=H, d=d, h=h, w=w, wh=wh, ww=ww)
    assert torch.equal(bits(got), bits(narrow)), f"{geo}: the result moved with the leading dimensions"


@pytest.mark.parametrize("d", HEAD_DIMS, ids=ids)
@pytest.mark.parametrize("geo", GEOMETRIES, ids=ids)
def test_window_bits_are_those_of_a_launch_on_its_gathered_tokens(gpu, geo, d):
    """For every window: a launch with h = wh, w = ww on that window's tokens gathered in window-linear order gives the bits the
    image launch gave those tokens."""
    h, w, wh, ww = geo
    q, k, v, _ref, got = case(gpu, geo, d)
    for n, idx in enumerate(windows(h, w, wh, ww)):
        alone = launch(gpu, q[:, idx], k[:, idx], v[:, idx], heads=H, d=d, h=wh, w=ww, wh=wh, ww=ww)
        assert torch.equal(bits(alone), bits(got[:, idx])), f"{geo} d={d}: window {n}"


@pytest.mark.parametrize("d", HEAD_DIMS, ids=ids)
@pytest.mark.parametrize("geo", GEOMETRIES, ids=ids)
def test_other_windows_and_the_padding_never_reach_a_window(gpu, geo, d):
    """Every other window's q / k / v and the V^T padding hold NaN: the window's output keeps its bits (and is finite).  With one
    window the padding alone is poisoned."""
    h, w, wh, ww = geo
    q, k, v, _ref, got = case(gpu, geo, d)
    for n, idx in enumerate(windows(h, w, wh, ww)):
        qn, kn, vn = (torch.full_like(x, NAN) for x in (q, k, v))
        qn[:, idx], kn[:, idx], vn[:, idx] = q[:, idx], k[:, idx], v[:, idx]
        res = launch(gpu, qn, kn, vn, heads=H, d=d, h=h, w=w, wh=wh, ww=ww, wide=True, poison=True)
        assert bool(torch.isfinite(res[:, idx].float()).all()), f"{geo} d={d}: window {n}"
        assert torch.equal(bits(res[:, idx]), bits(got[:, idx])), f"{geo} d={d}: window {n}"


@pytest.mark.parametrize("d", HEAD_DIMS, ids=ids)
@pytest.mark.parametrize("geo", GEOMETRIES, ids=ids)
def test_against_msd_attention_on_the_gathered_windows(gpu, geo, d):
    """msd_attention on the windows gathered contiguously as batch B * nh * nw: the same FLOPs with no gather, within the
    attention bound."""
    from minsdtf_amd import ops

    h, w, wh, ww = geo
    q, k, v, _ref, got = case(gpu, geo, d)
    win = windows(h, w, wh, ww)
    nwin, T = win.shape
    C = H * d
    Tp = (T + 7) // 8 * 8

    def gather(x):   # (B, S, C) -> (B * nwin, T, C)
        return x[:, win].reshape(B * nwin, T, C)

    qd, kd = gather(q).to(BF16).to(gpu), gather(k).to(BF16).to(gpu)
    vt = torch.zeros(B * nwin, C, Tp, dtype=BF16, device=gpu)
    vt[:, :, :T] = gather(v).permute(0, 2, 1).to(BF16).to(gpu)
    out = torch.empty(B * nwin, T, C, dtype=BF16, device=gpu)
    run_calls(ops.attention(q=qd, k=kd, vt=vt, out=out, batch=B * nwin, heads=H, head_dim=d, s=T, t=T, q_ld=C, k_ld=C, vt_ld=Tp, o_ld=C,
                            scale=1.0, q_prescaled=True))
    ref = out.float().cpu()
    close(got[:, win].reshape(B * nwin, T, C), ref, what=f"{geo} d={d}", **bound(ref))


@pytest.mark.parametrize("geo, d", [((24, 16, 12, 8), 40), ((8, 48, 8, 24), 80), ((20, 16, 10, 16), 160)], ids=ids)
def test_sample_bits_do_not_depend_on_the_batch_and_runs_repeat(gpu, geo, d):
    h, w, wh, ww = geo
    q, k, v, _ref, got = case(gpu, geo, d)
    kw = dict(heads=H, d=d, h=h, w=w, wh=wh, ww=ww, wide=True)
    assert torch.equal(bits(launch(gpu, q, k, v, **kw)), bits(got))
    three = launch(gpu, torch.cat([q[1:], q]), torch.cat([k[1:], k]), torch.cat([v[1:], v]), **kw)
    assert torch.equal(bits(three[0]), bits(got[1])) and torch.equal(bits(three[1:]), bits(got))
    for b in range(B):
        alone = launch(gpu, q[b:b + 1], k[b:b + 1], v[b:b + 1], **kw)
        assert torch.equal(bits(alone[0]), bits(got[b])), f"sample {b}"


# ---------------------------------------------------------------------------------------------------------------- pipelines
PSNR_MIN = 40.0        # the project's bar for every job
SAMPLER_PSNR_MIN = 45.0   # ... for a samplers.py sampler's txt2img job against another route (test_samplers_gpu.py)
TB = ".transformer_blocks.0.attn1"


@pytest.fixture(scope="module")
def nets(gpu):
    from minsdtf_amd.models import DiffusionModel, ImageDecoder

    unet = DiffusionModel(128, 128, device=gpu)
    unet.load_synthetic(seed=0, bias_scale=0.05)
    dec = ImageDecoder(device=gpu)
    dec.load_synthetic(seed=0, bias_scale=0.05)
    return {"unet": unet, "dec": dec}


def _pipe(gpu, nets, height=128, width=128, jit=True):
    """(pipeline at this size over the module's weights - another size: a view that shares them -, a context)"""
    from minsdtf_amd.models import DiffusionModel
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sd = StableDiffusion(height, width, jit_compile=jit, device=gpu)
    if (height, width) == (128, 128):
        sd._diffusion_model = nets["unet"]
    else:
        sd._diffusion_model = DiffusionModel(height, width, device=gpu)
        sd._diffusion_model.share_weights(nets["unet"])
    sd._image_decoder = nets["dec"]
    rng = np.random.default_rng(41)
    sd.unconditional_context = rng.standard_normal((77, 768)).astype(np.float32)
    return sd, rng.standard_normal((77, 768)).astype(np.float32)


def _names(eng):
    return [c.name for c in eng.calls]


def _windowed(eng):
    return [n for n in _names(eng) if n.endswith(TB + ".windowed")]


@pytest.mark.parametrize("sampler", [None, "dpmpp_2m"])
def test_device_loop_vs_host_loop(gpu, nets, sampler):
    """128 x 128 px, tile 64 (2 x 2 windows of 8 x 8 tokens at level 0), 4 steps, batch 2: the device loop against host_loop=True
    (DiffusionModel.predict_windowed through _guided_eps): 40 dB, or 45 dB with a samplers.py sampler; and not the plain job."""
    from oracle import sd_oracle as O

    sd, P = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=4, seed=11, return_latent=True, sampler=sampler, guidance_rescale=0.7, hypertile=dict(tile=64))
    calls_d, calls_h = [], []
    dev = sd.generate_image(P, callback=calls_d.append, **kw)
    eng = next(iter(sd._engines.values()))
    assert eng.hypertile == (2, 2, 0) and eng.passes == [(0, 4, 77, "both")]
    assert len(_windowed(eng)) == 5 and sum(n.endswith(TB) for n in _names(eng)) == 11
    host = sd.generate_image(P, host_loop=True, callback=calls_h.append, **kw)
    assert calls_d == calls_h == [1, 2, 3, 4]
    p = O.psnr(dev, host)
    bar = SAMPLER_PSNR_MIN if sampler else PSNR_MIN
    print(f"hypertile job ({sampler or 'default sampler'}): device loop vs host loop {p:.1f} dB (bar {bar:.0f})")
    assert p >= bar
    plain = sd.generate_image(P, **{k: v for k, v in kw.items() if k != "hypertile"})
    assert not np.array_equal(dev, plain)
    # one window is the plain job on the plain engine
    built = len(sd._engines)
    np.testing.assert_array_equal(sd.generate_image(P, **{**kw, "hypertile": dict(tile=128)}), plain)
    assert len(sd._engines) == built and all(e.hypertile is None or e is eng for e in sd._engines.values())


def test_predict_windowed(gpu, nets):
    """One window is predict_on_batch's bits' worth (40 dB: another kernel computes the same attention); 2 x 2 windows move the
    prediction; windows the levels cannot take are refused."""
    from oracle import sd_oracle as O

    unet = nets["unet"]
    rng = np.random.default_rng(2)
    lat = rng.standard_normal((2, 16, 16, 4)).astype(np.float32)
    temb = O.timestep_embedding(500, 2)
    ctx = rng.standard_normal((2, 77, 768)).astype(np.float32)
    ref = unet.predict_on_batch([lat, temb, ctx])
    one = unet.predict_windowed([lat, temb, ctx], (1, 1), 1)
    p = O.psnr(one, ref)
    print(f"predict_windowed, one window, depth 1 vs predict_on_batch: {p:.1f} dB")
    assert one.shape == ref.shape and p >= PSNR_MIN
    moved = unet.predict_windowed([lat, temb, ctx], (2, 2), 0)
    assert np.all(np.isfinite(moved)) and O.psnr(moved, ref) < PSNR_MIN
    with pytest.raises(ValueError, match="hypertile"):
        unet.predict_windowed([lat, temb, ctx], (2, 2), 1)
    with pytest.raises(ValueError, match="hypertile"):
        unet.predict_windowed([lat, temb, ctx], (4, 4), 0)
    with pytest.raises(ValueError, match="no control"):
        unet.predict_windowed([lat, temb, ctx, ctx], (2, 2), 0)


def test_hires_applies_the_windows_to_the_second_pass_only(gpu, nets):
    """hires 64 -> 128 px with tile 64: pass 1 (64 x 64 px) records no windowed launch, pass 2 (128 x 128 px, 2 x 2 windows) five;
    and the job is not the plain hires job."""
    sd, P = _pipe(gpu, nets, 64, 64)
    kw = dict(batch_size=1, num_steps=3, seed=3, return_latent=True, guidance_rescale=0.7, hires=dict(scale=2, steps=4, strength=0.5))
    got = sd.generate_image(P, hypertile=dict(tile=64), **kw)
    assert got.shape == (1, 16, 16, 4) and np.all(np.isfinite(got))
    engines = sorted(sd._engines.values(), key=lambda e: e.h)
    assert [(e.h, e.hypertile) for e in engines] == [(8, None), (16, (2, 2, 0))]
    assert len(_windowed(engines[0])) == 0 and len(_windowed(engines[1])) == 5
    plain = sd.generate_image(P, **kw)
    assert not np.array_equal(got, plain)
    # a tile the TARGET size does not take is refused, whatever the pipeline's own size takes
    with pytest.raises(ValueError, match="does not divide the picture's height 128 px"):
        sd.generate_image(P, hypertile=dict(tile=192), **kw)


def test_residency(gpu, nets, monkeypatch):
    """A second call builds no engine and captures no graph; another tile is another engine."""
    import minsdtf_amd.stable_diffusion as sdm

    built = []
    init = sdm.DenoiseEngine.__init__

    def counting(self, *a, **k):
        built.append((a[1], k.get("hypertile")))
        init(self, *a, **k)

    monkeypatch.setattr(sdm.DenoiseEngine, "__init__", counting)
    sd, P = _pipe(gpu, nets)
    kw = dict(batch_size=1, num_steps=3, seed=5, guidance_rescale=0.7, return_latent=True)
    first = sd.generate_image(P, hypertile=dict(tile=64), **kw)
    assert built == [(1, (2, 2, 0))]
    eng = next(iter(sd._engines.values()))
    graph = eng._loop_graph
    second = sd.generate_image(P, hypertile=dict(tile=(64, 64), depth=0), **{**kw, "seed": 6})
    assert len(built) == 1 and next(iter(sd._engines.values())) is eng and eng._loop_graph is graph
    assert not np.array_equal(first, second)
    np.testing.assert_array_equal(sd.generate_image(P, hypertile=dict(tile=64), **kw), first)
    assert len(built) == 1
    # a pipeline that never saw the first job gives the same bits (it builds its own engine)
    fresh, _ = _pipe(gpu, nets)
    np.testing.assert_array_equal(first, fresh.generate_image(P, hypertile=dict(tile=64), **kw))
    assert len(built) == 2
    sd.generate_image(P, hypertile=dict(tile=(64, 128)), **kw)
    assert len(built) == 3 and built[-1][1] == (2, 1, 0)


def test_graph_forms_agree(gpu, nets):
    """The whole-loop graph == per-step graphs (a callback is installed) == eager launches (jit_compile=False), bit for bit."""
    sd, P = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=3, seed=8, return_latent=True, sampler="dpmpp_2m", guidance_rescale=0.7, hypertile=dict(tile=64))
    whole = sd.generate_image(P, **kw)
    calls = []
    stepped = sd.generate_image(P, callback=calls.append, **kw)
    assert calls == [1, 2, 3]
    eng = next(iter(sd._engines.values()))
    assert eng._loop_graph is not None and eng._step_graph is not None and eng.hypertile == (2, 2, 0)
    eager_sd, _ = _pipe(gpu, nets, jit=False)
    np.testing.assert_array_equal(stepped, whole)
    np.testing.assert_array_equal(eager_sd.generate_image(P, **kw), whole)
    assert np.all(np.isfinite(whole))


def test_batch_independence_of_the_job(gpu, nets):
    """The tile is fixed, never drawn: a sample's latent is bit-identical whatever batch it runs in."""
    sd, P = _pipe(gpu, nets)
    rng = np.random.default_rng(5)
    noise = rng.standard_normal((2, 16, 16, 4)).astype(np.float32)
    kw = dict(num_steps=3, return_latent=True, guidance_rescale=0.7, hypertile=dict(tile=64))
    both = sd.generate_image(P, batch_size=2, diffusion_noise=noise, **kw)
    for b in range(2):
        np.testing.assert_array_equal(sd.generate_image(P, batch_size=1, diffusion_noise=noise[b:b + 1], **kw)[0], both[b])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_against_the_oracle_fixture(gpu, nets, tag):
    """tests/golden/oracle_hypertile_{a,b}.npz (tools/make_hypertile_fixtures.py): final latent PSNR >= 40 dB on the whole batch and
    on each sample; the fixture's plain job is below 30 dB, so the bar tells the feature from its absence."""
    import os

    from oracle import sd_oracle as O

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"oracle_hypertile_{tag}.npz"))
    assert (int(g["weight_seed"]), float(g["bias_scale"])) == (0, 0.05) and float(g["plain_psnr"]) < 30.0
    height, width, Bn = int(g["height"]), int(g["width"]), int(g["batch"])
    sd, _ = _pipe(gpu, nets, height, width)
    rng = np.random.default_rng(int(g["context_seed"]))
    base = rng.standard_normal((1, 77, 768)).astype(np.float32)[0]
    sd.unconditional_context = rng.standard_normal((1, 77, 768)).astype(np.float32)[0]
    noise = np.random.default_rng(int(g["noise_seed"])).standard_normal((Bn, height // 8, width // 8, 4)).astype(np.float32)
    got = sd.generate_image(base, batch_size=Bn, num_steps=int(g["steps"]), unconditional_guidance_scale=float(g["guidance"]),
                            diffusion_noise=noise, guidance_rescale=float(g["guidance_rescale"]), return_latent=True,
                            sampler=str(g["sampler"]) or None, hypertile=dict(tile=int(g["tile"]), depth=int(g["depth"])))
    eng = next(iter(sd._engines.values()))
    assert eng.hypertile == tuple(int(v) for v in g["windows"]) + (int(g["depth"]),)
    assert len(_windowed(eng)) == 5 * (int(g["depth"]) + 1)
    p = O.psnr(got, g["latent"])
    per = [round(O.psnr(got[b], g["latent"][b]), 1) for b in range(Bn)]
    print(f"hypertile job {tag}: final latent PSNR {p:.1f} dB (per sample {per}); the plain job is at {float(g['plain_psnr']):.1f} dB")
    assert p >= PSNR_MIN and min(per) >= PSNR_MIN


def test_sharded_job_equals_unsharded(gpu):
    """A one-rank process group with forced collectives (as tests/test_regions_gpu.py): the sharded HyperTile job == the unsharded
    one.  (A child process is what the test is about: the group must exist before anything touches the GPU.)"""
    import os
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(here, "_hypertile_world1_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=570)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert any(line.startswith("OK ") for line in p.stdout.splitlines()), p.stdout[-2000:]
    print(p.stdout.strip().splitlines()[-1])
