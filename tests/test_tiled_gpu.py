"""Tiled diffusion on the device: msd_tile_consensus against its float64 statement, the tiled= job against plain jobs where the
two must agree bit for bit (one view; views that do not overlap), the three graph forms, the two oracle fixture jobs
(tests/golden/oracle_tiled_*.npz, tools/make_tiled_fixtures.py), decode, residency, batch independence, the sharded job, refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
PSNR_MIN = 40.0   # the project's bar for every job (test_hires_gpu.py, test_samplers_gpu.py)
U = 2.0 ** -24    # unit roundoff of fp32

# (th, tw, H, W, stride y, stride x)
GEOMETRIES = {
    "one view": (8, 8, 8, 8, 4, 4),
    "no overlap": (8, 8, 16, 24, 8, 8),
    "half overlap": (8, 8, 16, 20, 4, 4),
    "snapped last view": (8, 8, 18, 22, 4, 6),
    "3x3 views": (16, 16, 32, 32, 8, 8),
    "unequal tile sides": (8, 12, 20, 30, 6, 5),
}


def run_calls(calls):
    if not isinstance(calls, (list, tuple)):
        calls = [calls]
    st = torch.cuda.current_stream().cuda_stream
    for c in calls:
        c(st)
    torch.cuda.synchronize()


def _geometry(name, blend):
    from minsdtf_amd import tiled

    th, tw, H, W, sy, sx = GEOMETRIES[name]
    return tiled.geometry(th, tw, H, W, tiled.axis_offsets(H, th, sy), tiled.axis_offsets(W, tw, sx), blend)


def _launch(tiles, canvas, geo, dev, mode):
    """One launch on host arrays -> (tiles after, canvas after)."""
    from minsdtf_amd import ops

    td, cd = torch.from_numpy(tiles).to(dev), torch.from_numpy(canvas).to(dev)
    wy, wx = torch.from_numpy(geo.wy).to(dev), torch.from_numpy(geo.wx).to(dev)
    run_calls(ops.tile_consensus(tiles=td, canvas=cd, wy=wy, wx=wx, ys=geo.ys, xs=geo.xs, th=geo.th, tw=geo.tw, H=geo.H, W=geo.W,
                                 batch=canvas.shape[0], mode=mode))
    return td.cpu().numpy(), cd.cpu().numpy()


@pytest.mark.parametrize("blend", ["uniform", "gaussian"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_consensus_vs_float64(gpu, name, blend):
    """Bound (derived from the operation count, not measured): per covering view one product (the weight), one fma and one add
    (the weight sum), then one division: 3 n + 1 roundings of at most 2^-24 relative each; the weights are positive, so every
    intermediate is at most max|x| after the division: max abs error <= (3 n + 1) 2^-24 max|x|, n = the most views over a pixel.
    Pixels under one view are bit-exact; sample 0 of the batch-3 launch == the batch-1 launch; afterwards every tile entry equals
    its canvas pixel bitwise; gather is a bit-exact copy."""
    from minsdtf_amd import tiled

    geo = _geometry(name, blend)
    rng = np.random.default_rng(23)
    V = geo.views
    cover = np.zeros((geo.H, geo.W), dtype=np.int64)
    for (y, x) in geo.offsets():
        cover[y:y + geo.th, x:x + geo.tw] += 1
    assert cover.min() >= 1
    n = int(cover.max())
    tiles3 = rng.standard_normal((3 * V, geo.th, geo.tw, 4)).astype(np.float32)
    nan_canvas = lambda b: np.full((b, geo.H, geo.W, 4), np.nan, dtype=np.float32)
    got_t3, got_c3 = _launch(tiles3, nan_canvas(3), geo, gpu, 0)
    got_t1, got_c1 = _launch(tiles3[:V], nan_canvas(1), geo, gpu, 0)
    want_c, want_t = tiled.consensus_reference(tiles3, geo)
    assert np.all(np.isfinite(got_c3)) and np.all(np.isfinite(got_t3))
    bound = (3 * n + 1) * U * float(np.abs(tiles3).max())
    err = float(np.abs(got_c3 - want_c).max())
    print(f"msd_tile_consensus {name} / {blend}: up to {n} views per pixel, max abs error {err:.3e}, bound {bound:.3e} ({err / bound:.3f} of it)")
    assert err <= bound
    assert float(np.abs(got_t3 - want_t).max()) <= bound
    single = cover == 1
    np.testing.assert_array_equal(got_c3[:, single], want_c[:, single].astype(np.float32))   # one cover: the entry's own bits
    np.testing.assert_array_equal(got_c3[0], got_c1[0])
    np.testing.assert_array_equal(got_t3[:V], got_t1)
    np.testing.assert_array_equal(got_t3, tiled.slice_views(got_c3, geo))   # every tile entry == its canvas pixel
    # gather: canvas -> tiles, the canvas untouched
    canvas = rng.standard_normal((3, geo.H, geo.W, 4)).astype(np.float32)
    g_t, g_c = _launch(np.full_like(tiles3, np.nan), canvas, geo, gpu, 1)
    np.testing.assert_array_equal(g_c, canvas)
    np.testing.assert_array_equal(g_t, tiled.slice_views(canvas, geo))


def test_consensus_argument_errors(gpu):
    from minsdtf_amd import _lib, ops

    geo = _geometry("half overlap", "uniform")
    t = torch.zeros(geo.views, geo.th, geo.tw, 4, device=gpu)
    c = torch.zeros(1, geo.H, geo.W, 4, device=gpu)
    wy, wx = torch.ones(geo.th, device=gpu), torch.ones(geo.tw, device=gpu)
    good = dict(tiles=t, canvas=c, wy=wy, wx=wx, ys=geo.ys, xs=geo.xs, th=geo.th, tw=geo.tw, H=geo.H, W=geo.W, batch=1)
    st = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    for bad in (dict(tiles=None), dict(canvas=None), dict(wy=None), dict(wx=None), dict(batch=0), dict(th=0), dict(H=4), dict(mode=3),
                dict(tiles=t.data_ptr() + 4), dict(canvas=c.data_ptr() + 8), dict(canvas=t), dict(ys=(0, 4)), dict(xs=(0, 4, 8, 13)),
                dict(xs=(0, 12)), dict(ys=(1, 4, 8))):
        call = ops.tile_consensus(**{**good, **bad})
        assert call.fn(*call.args, st) == -1, bad
        assert lib.msd_last_error()
    run_calls(ops.tile_consensus(**good))


# ---------------------------------------------------------------------------------------------------------------- pipelines
@pytest.fixture(scope="module")
def nets(gpu):
    from minsdtf_amd.models import DiffusionModel, ImageDecoder

    unet = DiffusionModel(64, 64, device=gpu)
    unet.load_synthetic(seed=0, bias_scale=0.05)
    dec = ImageDecoder(device=gpu)
    dec.load_synthetic(seed=0, bias_scale=0.05)
    return {"unet": unet, "dec": dec}


def _pipe(gpu, nets, jit=True):
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sd = StableDiffusion(64, 64, jit_compile=jit, device=gpu)
    sd._diffusion_model = nets["unet"]
    sd._image_decoder = nets["dec"]
    rng = np.random.default_rng(41)
    sd.unconditional_context = rng.standard_normal((77, 768)).astype(np.float32)
    return sd, rng.standard_normal((77, 768)).astype(np.float32)


@pytest.mark.parametrize("sampler", [None, "euler_a"])
def test_one_view_equals_the_plain_job(gpu, nets, sampler):
    """A canvas of the tile's own size is one view, and every pixel has one cover: the plain job's bits."""
    sd, ctx = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=4, seed=6, sampler=sampler, guidance_rescale=0.7, return_latent=True)
    plain = sd.generate_image(ctx, **kw)
    got = sd.generate_image(ctx, tiled=dict(size=(64, 64)), **kw)
    np.testing.assert_array_equal(got, plain)


def test_views_that_do_not_overlap_equal_plain_jobs(gpu, nets):
    """A canvas two tiles wide at stride = tile: each half equals the plain batch-1 job on that half of the noise."""
    sd, ctx = _pipe(gpu, nets)
    noise = np.random.default_rng(12).standard_normal((1, 8, 16, 4)).astype(np.float32)
    kw = dict(batch_size=1, num_steps=4, guidance_rescale=0.7, return_latent=True)
    got = sd.generate_image(ctx, tiled=dict(size=(64, 128), stride=64), diffusion_noise=noise, **kw)
    assert got.shape == (1, 8, 16, 4)
    for k in range(2):
        half = sd.generate_image(ctx, diffusion_noise=np.ascontiguousarray(noise[:, :, 8 * k:8 * k + 8]), **kw)
        np.testing.assert_array_equal(got[:, :, 8 * k:8 * k + 8], half)


@pytest.mark.parametrize("sampler", [None, "dpmpp_2m_sde"])
def test_graph_forms_agree(gpu, nets, sampler):
    """The whole-loop graph == per-step graphs (a callback is installed) == eager launches (jit_compile=False), bit for bit; the
    callback counts 1 .. num_steps."""
    from minsdtf_amd import tiled

    spec = tiled.TiledSpec(size=(128, 128), stride=(32, 64), blend="gaussian")   # 3 x 2 views, tiled.MAX_VIEW_BATCH of them
    kw = dict(batch_size=1, num_steps=4, seed=8, sampler=sampler, guidance_rescale=0.7, return_latent=True, tiled=spec)
    sd, ctx = _pipe(gpu, nets)
    whole = sd.generate_image(ctx, **kw)
    calls = []
    stepped = sd.generate_image(ctx, callback=calls.append, **kw)
    assert calls == [1, 2, 3, 4]
    eng = next(iter(sd._engines.values()))
    assert eng._loop_graph is not None and eng._step_graph is not None and eng.B == 6 and tuple(eng.canvas.shape) == (1, 16, 16, 4)
    assert eng.calls[-1].name == "tile_consensus" and eng.calls[-2].name in ("cfg_step", "sampler_step")
    eager_sd, _ = _pipe(gpu, nets, jit=False)
    calls2 = []
    eager = eager_sd.generate_image(ctx, callback=calls2.append, **kw)
    assert calls2 == [1, 2, 3, 4]
    np.testing.assert_array_equal(stepped, whole)
    np.testing.assert_array_equal(eager, whole)
    assert np.all(np.isfinite(whole))
    # the views really were blended: the job differs from one with another blend
    other = sd.generate_image(ctx, **{**kw, "tiled": dict(size=(128, 128), stride=(32, 64))})
    assert not np.array_equal(other, whole)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_tiled_vs_oracle_fixture(gpu, tag):
    """The two fixture jobs against the fp32 oracle's composition (unet_forward / rescale_noise_cfg / the scheduler step per view,
    a float64 consensus): final canvas latent PSNR >= 40 dB.
    a: tile 256, canvas 384x384, stride 128 (2x2 views), default sampler, uniform, batch 1, 8 steps;
    b: tile 512, canvas 512x768, stride 128 (1x3 views), dpmpp_2m_karras, gaussian, batch 2, 10 steps."""
    from minsdtf_amd.stable_diffusion import StableDiffusion
    from oracle import sd_oracle as O

    g = np.load(os.path.join(GOLD, f"oracle_tiled_{tag}.npz"))
    tile, size, stride, B = [int(v) for v in g["tile"]], [int(v) for v in g["size"]], [int(v) for v in g["stride"]], int(g["batch"])
    sd = StableDiffusion(tile[0], tile[1], jit_compile=True, device=gpu)
    sd.diffusion_model.load_synthetic(seed=int(g["weight_seed"]))
    rng = np.random.default_rng(int(g["context_seed"]))
    ctx = rng.standard_normal((1, 77, 768)).astype(np.float32)
    unc = rng.standard_normal((1, 77, 768)).astype(np.float32)
    sd.unconditional_context = unc[0]
    got = sd.generate_image(ctx[0], batch_size=B, num_steps=int(g["steps"]), unconditional_guidance_scale=float(g["guidance"]),
                            seed=int(g["noise_seed"]), guidance_rescale=float(g["guidance_rescale"]), return_latent=True,
                            sampler=str(g["sampler"]) or None, tiled=dict(size=tuple(size), stride=tuple(stride), blend=str(g["blend"])))
    assert got.shape == (B, size[0] // 8, size[1] // 8, 4)
    eng = next(iter(sd._engines.values()))
    assert eng.tiled.ys == tuple(int(v) for v in g["ys"]) and eng.tiled.xs == tuple(int(v) for v in g["xs"])
    p = O.psnr(got, g["latent"])
    per = [round(O.psnr(got[b], g["latent"][b]), 1) for b in range(B)]
    print(f"tiled job {tag} (tile {tile}, canvas {size}, stride {stride}, {g['blend']}, {str(g['sampler']) or 'default sampler'}, batch {B}, "
          f"{eng.B} views): final canvas latent PSNR {p:.1f} dB (per sample {per})")
    assert p >= PSNR_MIN and min(per) >= PSNR_MIN


def test_decode_has_the_canvas_shape(gpu, nets):
    sd, ctx = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=3, seed=2, guidance_rescale=0.7, tiled=dict(size=(64, 128), stride=32))   # 2 images of 3 views
    lat = sd.generate_image(ctx, return_latent=True, **kw)
    img = sd.generate_image(ctx, **kw)
    assert lat.shape == (2, 8, 16, 4) and img.shape == (2, 64, 128, 3) and img.dtype == np.uint8
    np.testing.assert_array_equal(img, nets["dec"].decode_to_uint8(torch.from_numpy(lat).to(gpu)).cpu().numpy())
    assert sd.text_to_image(ctx, **kw).shape == (2, 64, 128, 3)


def test_residency(gpu, nets, monkeypatch):
    """The first tiled job builds one engine, a repeat builds none and captures nothing; a plain job afterwards evicts it."""
    import minsdtf_amd.stable_diffusion as sdm

    built = []
    init = sdm.DenoiseEngine.__init__

    def counting(self, *a, **k):
        built.append((a[1], k.get("tiled")))
        init(self, *a, **k)

    monkeypatch.setattr(sdm.DenoiseEngine, "__init__", counting)
    sd, ctx = _pipe(gpu, nets)
    kw = dict(batch_size=1, num_steps=3, seed=5, guidance_rescale=0.7, return_latent=True)
    spec = dict(size=(64, 128))   # three views
    first = sd.generate_image(ctx, tiled=spec, **kw)
    assert [b for b, _t in built] == [3] and built[0][1] is not None and len(sd._engines) == 1
    eng = next(iter(sd._engines.values()))
    graph = eng._loop_graph
    assert graph is not None
    second = sd.generate_image(ctx, tiled=spec, **kw)
    assert len(built) == 1 and next(iter(sd._engines.values())) is eng and eng._loop_graph is graph
    np.testing.assert_array_equal(first, second)
    # another geometry is another engine (the job's own engine survives, the other goes)
    sd.generate_image(ctx, tiled=dict(size=(64, 128), blend="gaussian"), **kw)
    assert len(built) == 2 and len(sd._engines) == 1 and next(iter(sd._engines.values())) is not eng
    # a plain job of the same engine batch is not the tiled engine
    plain = sd.generate_image(ctx, **{**kw, "batch_size": 3})
    assert len(built) == 3 and built[-1] == (3, None) and len(sd._engines) == 1 and plain.shape == (3, 8, 8, 4)
    third = sd.generate_image(ctx, tiled=spec, **kw)
    assert len(built) == 4 and len(sd._engines) == 1
    np.testing.assert_array_equal(first, third)


@pytest.mark.parametrize("sampler", [None, "euler_a"])
def test_batch_independence(gpu, nets, sampler):
    """Sample 0 of a batch-2 tiled job == the batch-1 job (the draws are made for the global batch, sample-major)."""
    sd, ctx = _pipe(gpu, nets)
    kw = dict(num_steps=4, sampler=sampler, guidance_rescale=0.7, return_latent=True, tiled=dict(size=(128, 64), stride=32, blend="gaussian"))
    two = sd.generate_image(ctx, batch_size=2, seed=9, **kw)
    one = sd.generate_image(ctx, batch_size=1, seed=9, **kw)
    np.testing.assert_array_equal(one[0], two[0])
    assert not np.array_equal(two[0], two[1])
    if sampler is None:
        n = sd._get_initial_diffusion_noise(2, 9, 128, 64)
        np.testing.assert_array_equal(sd.generate_image(ctx, batch_size=2, diffusion_noise=n, **kw), two)
        np.testing.assert_array_equal(sd.generate_image(ctx, batch_size=1, diffusion_noise=n[1], **kw)[0], two[1])


def test_sharded_tiled_equals_unsharded(gpu):
    """A one-rank process group with forced collectives (as tests/test_rccl_gpu.py): the sharded tiled job == the unsharded one."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(HERE, "_job_world1_child.py"), "tiled"], env=env,
                       stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=570)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert any(line.startswith("OK ") for line in p.stdout.splitlines()), p.stdout[-2000:]
    print(p.stdout.strip().splitlines()[-1])


def test_refused_combinations(gpu, nets):
    from minsdtf_amd import tiled
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sd, ctx = _pipe(gpu, nets)
    img = np.zeros((64, 64, 3), dtype=np.uint8)
    kw = dict(batch_size=1, num_steps=3, seed=0, tiled=dict(size=(64, 128)))
    for extra in (dict(reference_image=img), dict(inpaint_mask=img[..., 0]), dict(reference_image=img, inpaint_mask=img[..., 0]),
                  dict(control_net_image=img.astype(np.float32)), dict(hires=dict(scale=2)), dict(host_loop=True)):
        with pytest.raises(ValueError, match="tiled"):
            sd.generate_image(ctx, **kw, **extra)
    tcd = StableDiffusion(64, 64, jit_compile=True, device=gpu, active_tcd=True)
    with pytest.raises(ValueError, match="tiled"):
        tcd.generate_image(ctx, **kw)
    with pytest.raises(ValueError, match="tiled"):
        sd.image_to_image(ctx, reference_image=img, **kw)
    with pytest.raises(ValueError, match="tiled"):
        sd.inpaint(ctx, reference_image=img, inpaint_mask=img[..., 0], **kw)
    with pytest.raises(ValueError, match="MAX_VIEW_BATCH"):
        sd.generate_image(ctx, **{**kw, "batch_size": tiled.MAX_VIEW_BATCH // 3 + 1})
    with pytest.raises(ValueError, match="multiple of 64"):
        sd.text_to_image(ctx, batch_size=1, num_steps=3, seed=0, tiled=dict(size=(96, 128)))
    assert not sd._engines


def test_a_job_at_max_view_batch_runs_at_the_512_tile(gpu):
    """Exactly tiled.MAX_VIEW_BATCH views at the 512-px tile (a 1024x768 canvas at stride 256 is 3 x 2 views; further images are
    added while they fit) run to a finite result."""
    from minsdtf_amd import tiled
    from minsdtf_amd.stable_diffusion import StableDiffusion

    geo = tiled.parse(dict(size=(1024, 768), stride=256), 512, 512)
    assert geo.views == 6 and tiled.MAX_VIEW_BATCH % geo.views == 0
    B = tiled.MAX_VIEW_BATCH // geo.views
    sd = StableDiffusion(512, 512, jit_compile=True, device=gpu)
    sd.diffusion_model.load_synthetic(seed=0)
    rng = np.random.default_rng(3)
    sd.unconditional_context = rng.standard_normal((77, 768)).astype(np.float32)
    ctx = rng.standard_normal((77, 768)).astype(np.float32)
    got = sd.generate_image(ctx, batch_size=B, num_steps=2, seed=1, guidance_rescale=0.7, return_latent=True,
                            tiled=dict(size=(1024, 768), stride=256))
    eng = next(iter(sd._engines.values()))
    assert eng.B == tiled.MAX_VIEW_BATCH and got.shape == (B, 128, 96, 4) and np.all(np.isfinite(got))
    with pytest.raises(ValueError, match="MAX_VIEW_BATCH"):
        sd.generate_image(ctx, batch_size=B + 1, num_steps=2, seed=1, tiled=dict(size=(1024, 768), stride=256))
