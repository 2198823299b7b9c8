"""Regional prompting on the device: msd_region_combine against its float64 statement, the regions= job against plain jobs where
the two must agree bit for bit (one region; one prompt in two regions), mask routing, the device loop against host_loop=True, the
two oracle fixture jobs (tests/golden/oracle_regions_*.npz, tools/make_region_fixtures.py), the three graph forms, residency, the
sharded job, an unconditional context of another length, the size cap."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
PSNR_MIN = 40.0        # the project's bar for every job (test_tiled_gpu.py, test_hires_gpu.py, test_samplers_gpu.py)
HOST_PSNR_MIN = 45.0   # device loop vs host_loop=True of a samplers.py txt2img job (test_samplers_gpu.py: HOST_PSNR_MIN)
U = 2.0 ** -24         # unit roundoff of fp32


def run_calls(calls):
    if not isinstance(calls, (list, tuple)):
        calls = [calls]
    st = torch.cuda.current_stream().cuda_stream
    for c in calls:
        c(st)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ kernel
def _weights(R, h, w, rng):
    """Soft normalised weights, with a stripe of single-cover pixels (weight exactly 1.0 for region y % R, 0.0 elsewhere)."""
    from minsdtf_amd import regions

    masks = rng.random((R, h, w)) + 0.01
    single = np.zeros((h, w), dtype=bool)
    single[::2] = True
    for y in range(0, h, 2):
        masks[:, y] = 0.0
        masks[y % R, y] = 0.5 + rng.random(w)
    return regions.weights(list(masks)), single


@pytest.mark.parametrize("R", [1, 2, 5, 16])
@pytest.mark.parametrize("hw", [(8, 8), (5, 7), (1, 1), (64, 64)])
def test_combine_vs_float64(gpu, hw, R):
    """Bound (derived from the operation count, not measured).  Per element the kernel rounds R times: the first product, then
    one single-rounded FMA per further region.  Write s_k for the exact partial sum sum_{r<=k} w_r x_r and v_k for the computed
    one: v_k = (w_k x_k + v_{k-1}) (1 + d_k), |d_k| <= u = 2^-24, so |v_k - s_k| <= (1 + u) |v_{k-1} - s_{k-1}| + u |s_k|.  The
    weights are non-negative fp32 roundings (relative error <= u each) of float64 quotients that sum to 1, so
    sum_r w_r <= 1 + u and every |s_k| <= (1 + u) max|x|.  Unrolled: |v - s| <= R u (1 + u)^(R + 1) max|x| <= (R + 1) u max|x|,
    since (1 + u)^(R + 1) <= 1 + 1 / R for R <= 16.  The reference reads the same fp32 weights, so their own rounding is not
    part of the error.
    Also: single-cover pixels are bit-equal to their source; sample 0 of the batch-3 launch == the batch-1 launch; the in-place
    launch == the out-of-place one; `out` (pre-filled with NaN) is finite afterwards and a NaN guard row behind it is untouched."""
    from minsdtf_amd import ops, regions

    h, w = hw
    n = h * w * 4
    rng = np.random.default_rng(100 * R + h)
    wt, single = _weights(R, h, w, rng)
    eps3 = rng.standard_normal((R, 3, h, w, 4)).astype(np.float32)
    wd = torch.from_numpy(wt).to(gpu)

    def launch(eps, in_place):
        """eps (R, B, h, w, 4) -> (out (B, h, w, 4), the guard row, eps after the launch)."""
        B = eps.shape[1]
        ed = torch.from_numpy(np.ascontiguousarray(eps).reshape(R * B, n)).to(gpu)
        od = torch.full((B + 1, n), float("nan"), dtype=torch.float32, device=gpu)   # row B: the guard
        run_calls(ops.region_combine(eps=ed, w=wd, out=ed if in_place else od, regions=R, batch=B, n=n))
        out = (ed[:B] if in_place else od[:B]).cpu().numpy().reshape(B, h, w, 4)
        return out, od[B].cpu().numpy(), ed.cpu().numpy().reshape(R, B, h, w, 4)

    got3, guard, after = launch(eps3, False)
    np.testing.assert_array_equal(after, eps3)                      # out of place: eps is only read
    assert np.all(np.isfinite(got3)) and np.all(np.isnan(guard))    # all of out written, nothing behind it
    want = regions.combine_reference(eps3.reshape(R * 3, h, w, 4), wt)
    bound = (R + 1) * U * float(np.abs(eps3).max())
    err = float(np.abs(got3 - want).max())
    print(f"msd_region_combine {h}x{w}, {R} region(s): max abs error {err:.3e}, bound {bound:.3e} ({err / bound:.3f} of it)")
    assert err <= bound
    for y in range(0, h, 2):                                        # one cover: the source's own bits
        np.testing.assert_array_equal(got3[:, y], eps3[y % R, :, y])
    assert single.any()
    got1, _g, _a = launch(eps3[:, :1], False)
    np.testing.assert_array_equal(got1[0], got3[0])                 # batch independence
    inp, guard, after = launch(eps3, True)
    np.testing.assert_array_equal(inp, got3)                        # in place == out of place
    np.testing.assert_array_equal(after[1:], eps3[1:])              # the other regions' rows are only read
    assert np.all(np.isnan(guard))


def test_zero_weight_regions_still_propagate_nan(gpu):
    from minsdtf_amd import ops, regions

    left, right = regions.boxes(4, 4, 1, 2)
    wt = torch.from_numpy(regions.weights([left, right])).to(gpu)
    eps = torch.ones(2, 64, device=gpu)
    eps[1, :] = float("nan")   # region 1 is NaN everywhere, its weight is 0 on the left half
    out = torch.zeros(1, 64, device=gpu)
    run_calls(ops.region_combine(eps=eps, w=wt, out=out, regions=2, batch=1, n=64))
    assert torch.isnan(out).all()


def test_combine_argument_errors(gpu):
    from minsdtf_amd import _lib, ops

    R, B, n = 2, 2, 64
    eps = torch.zeros(R * B, n, device=gpu)
    w = torch.ones(R, n // 4, device=gpu)
    out = torch.zeros(B, n, device=gpu)
    big = torch.zeros(16, device=gpu)   # (only its address is used: every bad call returns before a launch)
    good = dict(eps=eps, w=w, out=out, regions=R, batch=B, n=n)
    st = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    for bad in (dict(eps=None), dict(w=None), dict(out=None), dict(eps=eps.data_ptr() + 4), dict(w=w.data_ptr() + 8),
                dict(out=out.data_ptr() + 4), dict(n=62), dict(n=0), dict(regions=0), dict(regions=17), dict(batch=0),
                dict(batch=65536), dict(eps=big, out=big, regions=16, batch=65535, n=4096),        # 2^32 elements
                dict(out=eps.data_ptr() + n * 4), dict(out=eps.data_ptr() + (R * B - 1) * n * 4),  # inside eps, not at it
                dict(w=eps), dict(w=eps.data_ptr() + (R * B - 1) * n * 4), dict(w=out), dict(w=out.data_ptr() + (B - 1) * n * 4)):
        call = ops.region_combine(**{**good, **bad})
        assert call.fn(*call.args, st) == -1, bad
        assert lib.msd_last_error(), bad
    run_calls(ops.region_combine(**good))
    run_calls(ops.region_combine(**{**good, "out": eps}))   # exactly at eps: in place


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


def _job(prompts, masks, weights=None, base_weight=0.0):
    weights = weights or [1.0] * len(prompts)
    return dict(regions=[dict(prompt=p, mask=m, weight=v) for p, m, v in zip(prompts, masks, weights)], base_weight=base_weight)


def _soft_masks():
    """Three soft masks that overlap (image resolution: reduced by the 8 x 8 block mean)."""
    y, x = np.mgrid[0:64, 0:64] / 63.0
    return [1.0 - x, x, np.exp(-((x - 0.5) ** 2 + (y - 0.5) ** 2) / 0.08) + 0.05]


def _jobs(P, Q, S):
    """The two jobs of the route comparisons: (a) two binary halves, default sampler, rescale 0.7; (b) three soft overlapping
    regions and the base prompt at 0.3, dpmpp_2m."""
    return {"a": (dict(sampler=None, guidance_rescale=0.7, batch_size=1), _job([P, Q], _halves())),
            "b": (dict(sampler="dpmpp_2m", guidance_rescale=0.7, batch_size=2), _job([P, Q, S], _soft_masks(), [1.0, 2.0, 0.5], 0.3))}


@pytest.mark.parametrize("sampler", [None, "euler_a"])
def test_one_region_equals_the_plain_job(gpu, nets, sampler):
    """One region with a full mask and no base prompt: weight exactly 1.0 everywhere, the combine copies the conditional rows bit
    for bit, and the pass is the plain job's 2B rows: the plain job's bits, latent and picture.  (The base prompt is not evaluated:
    another `encoded_text` changes nothing.)"""
    sd, (P, Q, _S, _T) = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=4, seed=6, sampler=sampler, guidance_rescale=0.7)
    job = _job([P], [np.ones((8, 8))])
    plain = sd.generate_image(P, return_latent=True, **kw)
    got = sd.generate_image(Q, return_latent=True, regions=job, **kw)
    eng = next(iter(sd._engines.values()))
    assert eng.regions == 1 and eng.calls[-2].name == "region_combine" and eng.calls[-1].name in ("cfg_step", "sampler_step")
    np.testing.assert_array_equal(got, plain)
    np.testing.assert_array_equal(sd.generate_image(Q, regions=job, **kw), sd.generate_image(P, **kw))
    assert sd.text_to_image(Q, regions=job, **{**kw, "guidance_rescale": 0.7}).shape == (2, 64, 64, 3)


def test_one_prompt_in_two_regions_equals_the_plain_job(gpu, nets):
    """Two regions with the same prompt and complementary binary masks: every pixel copies one of two identical conditional
    predictions, provided a sample's eps does not depend on the batch it runs in (here 3B rows, the shared prefix at 3 copies)."""
    sd, (P, Q, _S, _T) = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=4, seed=6, guidance_rescale=0.7, return_latent=True)
    plain = sd.generate_image(P, **kw)
    got = sd.generate_image(Q, regions=_job([P, P], _halves()), **kw)
    eng = next(iter(sd._engines.values()))
    assert eng.regions == 2 and eng.eps.shape[0] == 6 and eng.passes == [(0, 6, 77, "both")]
    np.testing.assert_array_equal(got, plain)
    # without guidance: R * B rows, combined into rows 0 .. B
    kw0 = dict(kw, unconditional_guidance_scale=0.0)
    plain0 = sd.generate_image(P, **kw0)
    np.testing.assert_array_equal(sd.generate_image(Q, regions=_job([P, P], _halves()), **kw0), plain0)
    eng = next(iter(sd._engines.values()))
    assert eng.eps.shape[0] == 4 and eng.passes == [(0, 4, 77, "cond")]


def test_masks_route_the_prompts(gpu, nets):
    sd, (P, Q, _S, _T) = _pipe(gpu, nets)
    left, right = _halves()
    kw = dict(batch_size=1, num_steps=4, seed=3, guidance_rescale=0.7, return_latent=True)
    got = sd.generate_image(P, regions=_job([P, Q], [left, right]), **kw)
    assert np.all(np.isfinite(got))
    assert not np.array_equal(got, sd.generate_image(P, **kw)) and not np.array_equal(got, sd.generate_image(Q, **kw))
    swapped_masks = sd.generate_image(P, regions=_job([P, Q], [right, left]), **kw)
    assert not np.array_equal(swapped_masks, got)
    # region order enters only through the pinned sum, which binary masks make exact
    np.testing.assert_array_equal(sd.generate_image(P, regions=_job([Q, P], [right, left]), **kw), got)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_device_loop_vs_host_loop(gpu, nets, tag):
    """The device loop against host_loop=True (one predict_on_batch per region, regions.combine_host): job b (a samplers.py
    sampler, txt2img) at test_samplers_gpu.py's bar for these two routes, 45 dB; that file has no bar for the default sampler's
    txt2img job, so job a is held to the project's 40 dB."""
    from oracle import sd_oracle as O

    sd, (P, Q, S, T) = _pipe(gpu, nets)
    kw, job = _jobs(P, Q, S)[tag]
    kw = dict(kw, num_steps=4, seed=11, return_latent=True, regions=job)
    calls_d, calls_h = [], []
    dev = sd.generate_image(T, callback=calls_d.append, **kw)
    host = sd.generate_image(T, host_loop=True, callback=calls_h.append, **kw)
    assert calls_d == calls_h == [1, 2, 3, 4]
    p = O.psnr(dev, host)
    bar = HOST_PSNR_MIN if kw["sampler"] is not None else PSNR_MIN
    print(f"regional job {tag}: device loop vs host loop {p:.1f} dB (bar {bar:.0f})")
    assert p >= bar


@pytest.mark.parametrize("tag", ["a", "b"])
def test_regions_vs_oracle_fixture(gpu, nets, tag):
    """The two fixture jobs against the fp32 oracle's composition (unet_forward per region, a float64 combine with the fp32
    weights, rescale_noise_cfg, the scheduler / DPM++ 2M step): final latent PSNR >= 40 dB.
    a: 2 binary left / right regions, default sampler, batch 1, 4 steps; b: 3 soft overlapping regions + base_weight 0.3,
    dpmpp_2m, batch 2, 4 steps."""
    from oracle import sd_oracle as O

    g = np.load(os.path.join(GOLD, f"oracle_regions_{tag}.npz"))
    assert (int(g["weight_seed"]), float(g["bias_scale"])) == (0, 0.05)   # the module's nets
    sd, _ctxs = _pipe(gpu, nets)
    B, masks = int(g["batch"]), g["masks"]
    rng = np.random.default_rng(int(g["context_seed"]))
    base = rng.standard_normal((1, 77, 768)).astype(np.float32)[0]
    sd.unconditional_context = rng.standard_normal((1, 77, 768)).astype(np.float32)[0]
    prompts = [rng.standard_normal((1, 77, 768)).astype(np.float32)[0] for _ in masks]
    job = _job(prompts, list(masks), [float(v) for v in g["region_weights"]], float(g["base_weight"]))
    got = sd.generate_image(base, batch_size=B, num_steps=int(g["steps"]), unconditional_guidance_scale=float(g["guidance"]),
                            seed=int(g["noise_seed"]), guidance_rescale=float(g["guidance_rescale"]), return_latent=True,
                            sampler=str(g["sampler"]) or None, regions=job)
    assert got.shape == (B, 8, 8, 4)
    eng = next(iter(sd._engines.values()))
    assert eng.regions == len(masks) + (1 if float(g["base_weight"]) > 0 else 0)
    p = O.psnr(got, g["latent"])
    per = [round(O.psnr(got[b], g["latent"][b]), 1) for b in range(B)]
    print(f"regional job {tag} ({eng.regions} evaluated prompts, {str(g['sampler']) or 'default sampler'}, batch {B}): "
          f"final latent PSNR {p:.1f} dB (per sample {per})")
    assert p >= PSNR_MIN and min(per) >= PSNR_MIN


@pytest.mark.parametrize("tag", ["a", "b"])
def test_graph_forms_agree(gpu, nets, tag):
    """The whole-loop graph == per-step graphs (a callback is installed) == eager launches (jit_compile=False), bit for bit."""
    sd, (P, Q, S, T) = _pipe(gpu, nets)
    kw, job = _jobs(P, Q, S)[tag]
    kw = dict(kw, num_steps=4, seed=8, return_latent=True, regions=job)
    whole = sd.generate_image(T, **kw)
    calls = []
    stepped = sd.generate_image(T, callback=calls.append, **kw)
    assert calls == [1, 2, 3, 4]
    eng = next(iter(sd._engines.values()))
    assert eng._loop_graph is not None and eng._step_graph is not None and eng.regions == len(job["regions"]) + (tag == "b")
    eager_sd, _ = _pipe(gpu, nets, jit=False)
    eager = eager_sd.generate_image(T, callback=calls.append, **kw)
    np.testing.assert_array_equal(stepped, whole)
    np.testing.assert_array_equal(eager, whole)
    assert np.all(np.isfinite(whole))


def test_residency(gpu, nets, monkeypatch):
    """A second job with other masks and prompts but the same number of regions builds no engine and captures no graph, and its
    result is a fresh pipeline's."""
    import minsdtf_amd.stable_diffusion as sdm

    built = []
    init = sdm.DenoiseEngine.__init__

    def counting(self, *a, **k):
        built.append((a[1], k.get("regions")))
        init(self, *a, **k)

    monkeypatch.setattr(sdm.DenoiseEngine, "__init__", counting)
    sd, (P, Q, S, T) = _pipe(gpu, nets)
    kw = dict(batch_size=1, num_steps=3, seed=5, guidance_rescale=0.7, return_latent=True)
    left, right = _halves()
    soft = _soft_masks()
    first = sd.generate_image(P, regions=_job([P, Q], [left, right]), **kw)
    assert built == [(1, 2)] and len(sd._engines) == 1
    eng = next(iter(sd._engines.values()))
    graph = eng._loop_graph
    assert graph is not None
    other = _job([S, T], soft[:2], [0.5, 3.0])
    second = sd.generate_image(P, regions=other, **kw)
    assert len(built) == 1 and next(iter(sd._engines.values())) is eng and eng._loop_graph is graph
    assert not np.array_equal(first, second)
    fresh, _ = _pipe(gpu, nets)
    np.testing.assert_array_equal(second, fresh.generate_image(P, regions=other, **kw))
    assert len(built) == 2
    np.testing.assert_array_equal(sd.generate_image(P, regions=_job([P, Q], [left, right]), **kw), first)
    assert len(built) == 2 and eng._loop_graph is graph
    # one region and the base prompt are R = 2 as well: the same engine
    sd.generate_image(P, regions=_job([Q], [soft[2]], base_weight=0.5), **kw)
    assert len(built) == 2 and next(iter(sd._engines.values())) is eng and eng._loop_graph is graph
    # another R is another engine; a plain job is not a regional engine
    sd.generate_image(P, regions=_job([P, Q, S], soft), **kw)
    assert built[-1] == (1, 3) and len(built) == 3 and len(sd._engines) == 1
    sd.generate_image(P, **kw)
    assert built[-1] == (1, 0) and len(built) == 4 and len(sd._engines) == 1


def test_sharded_regions_equal_unsharded(gpu):
    """A one-rank process group with forced collectives (as tests/test_rccl_gpu.py): the sharded regional job == the unsharded one."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(HERE, "_job_world1_child.py"), "regions"], env=env,
                       stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=570)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert any(line.startswith("OK ") for line in p.stdout.splitlines()), p.stdout[-2000:]
    print(p.stdout.strip().splitlines()[-1])


def test_unconditional_context_of_another_length(gpu, nets):
    """154 unconditional tokens against 77: the two-pass layout (B unconditional rows, then R * B conditional rows), against
    host_loop=True at the bar of test_device_loop_vs_host_loop's sampler job."""
    from oracle import sd_oracle as O

    sd, (P, Q, S, T) = _pipe(gpu, nets)
    neg = np.random.default_rng(5).standard_normal((154, 768)).astype(np.float32)
    kw, job = _jobs(P, Q, S)["b"]
    kw = dict(kw, num_steps=4, seed=11, return_latent=True, regions=job, negative_prompt=neg)
    dev = sd.generate_image(T, **kw)
    eng = next(iter(sd._engines.values()))
    assert eng.passes == [(0, 2, 154, "uncond"), (2, 8, 77, "cond")] and eng.eps.shape[0] == 10
    host = sd.generate_image(T, host_loop=True, **kw)
    p = O.psnr(dev, host)
    print(f"regional job b, 154 unconditional tokens: device loop vs host loop {p:.1f} dB")
    assert p >= HOST_PSNR_MIN
    assert not np.array_equal(dev, sd.generate_image(T, **{**kw, "negative_prompt": None}))


def test_at_the_cap(gpu, nets):
    """(1 + R) * batch = 12 UNet rows run to a finite result; 14 are refused."""
    from minsdtf_amd import regions

    sd, (P, Q, S, T) = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=2, seed=1, guidance_rescale=0.7, return_latent=True)
    five = _job([P, Q, S, T, P], regions.boxes(8, 8, 1, 5))
    got = sd.generate_image(P, regions=five, **kw)
    eng = next(iter(sd._engines.values()))
    assert eng.regions == 5 and eng.eps.shape[0] == 12 and got.shape == (2, 8, 8, 4) and np.all(np.isfinite(got))
    with pytest.raises(ValueError, match="MAX_VIEW_BATCH"):
        sd.generate_image(P, regions=_job([P, Q, S, T, P, Q], regions.boxes(8, 8, 1, 6)), **kw)
    assert next(iter(sd._engines.values())) is eng
