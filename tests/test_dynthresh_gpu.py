"""Dynamic thresholding on the device: msdt_dynamic_threshold through the C ABI, between guard bands, against the float64 host
statement (dynthresh.dynthresh_host); exact arithmetic bit for bit; in place against apart; the step counter; batch independence,
repeatability, the degenerate plane, padding; then jobs on the seeded synthetic nets - the device loop against host_loop=True, a
scheduled job, engine reuse, the combinations, guidance_rescale, the sharded job and the oracle fixtures
(tests/golden/dynthresh_*.npz, tools/make_dynthresh_fixtures.py).

The kernel bound is derived, not measured: |out - dynthresh_host| <= 128 * 2^-24 * S with S = max |cfg| of the plane.  A value
passes through fewer than ten rounded operations, the means through per-lane chains of at most P / 1024 terms plus a ten-level
tree.  A rank that is off by one moves the result by more than that at these shapes (asserted on the test data itself).

The kernel-test data keep |cc| away from 0 (d = +-[1, 2], a per-channel offset on top): with percentile 0 and startpoint "zero"
the divisor is the SMALLEST |cc| of the plane; on data whose smallest deviation is 1e-4 of the largest the quotient, and with it
the result, is thousands of times S, where one fp32 rounding of the result alone is above the bound - no fp32 kernel could meet
it there, and nothing about the selection would be learnt.  On these data every case of the table is well conditioned."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _extents_dynthresh as XD
import _guard as G

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
PSNR_MIN = 40.0        # the project's bar for every job
HOST_PSNR_MIN = 45.0   # device loop vs host_loop=True of a samplers.py txt2img job (test_sag_gpu.py, test_pag_gpu.py)
BOUND = 128 * 2.0 ** -24

# (batch, h, w): idle lanes; P = 960; 1023; 1024; 1025 (two pixels per lane); the workload's shape; cfg held and mim recomputed;
# the last shape of the register form (P = 8192); the first of the generic form (P = 8255); 128 x 128; 100 x 164
SHAPES = [(1, 8, 8), (2, 24, 40), (1, 33, 31), (3, 32, 32), (1, 25, 41), (2, 64, 64), (1, 64, 96), (1, 64, 128), (1, 65, 127),
          (1, 128, 128), (1, 100, 164)]
PERCENTILES = [0.0, 0.5, 0.95, 0.999, 1.0]
G_SCALE, M_SCALE = 11.5, 6.25   # (fp32 values)


def run_calls(calls):
    if not isinstance(calls, (list, tuple)):
        calls = [calls]
    st = torch.cuda.current_stream().cuda_stream
    for c in calls:
        c(st)
    torch.cuda.synchronize()


_DATA = {}


def data(shape):
    """u, c fp32 (batch, h, w, 4), made once per shape and never changed: d = c - u is +-[1, 2], u a per-channel offset plus a
    little noise, so a plane of cfg is offset +- g [1, 2] and its deviations from the mean stay away from 0."""
    if shape not in _DATA:
        B, h, w = shape
        rng = np.random.default_rng(7919 * h + 31 * w + B)
        d = rng.uniform(1.0, 2.0, (B, h, w, 4)) * rng.choice([-1.0, 1.0], (B, h, w, 4))
        u = (np.asarray([0.0, 3.0, -5.0, 0.5]) + 0.1 * rng.standard_normal((B, h, w, 4))).astype(np.float32)
        c = (u + d).astype(np.float32)
        u.setflags(write=False)
        c.setflags(write=False)
        _DATA[shape] = (u, c)
    return _DATA[shape]


def launch(gpu, u, c, spec, in_place=False, step=1, with_step_ptr=True, scales=None, params=None, eps_fill=None):
    """One guarded launch: eps = (u rows, c rows), a 3-row scale table whose row `step` holds (G_SCALE, M_SCALE) and whose other
    rows hold values that would show, the params of `spec`.  Returns (out fp32 (B, h, w, 4) on the host, the step counter after)."""
    from minsdtf_amd import dynthresh as D
    from minsdtf_amd import ops

    B, h, w, _ = u.shape
    n = h * w * 4
    dims = dict(batch=B, h=h, w=w, num_steps=3)
    gd = G.Guard(gpu, XD.dynamic_threshold(eps=True, out=None if in_place else True, scales=True, params=True,
                                           step_ptr=True if with_step_ptr else None, **dims))
    eps = gd.inp(torch.from_numpy(np.concatenate([u, c]).reshape(2 * B, n)), "eps")
    if scales is None:
        scales = np.full((3, 2), 977.0, dtype=np.float32)
        scales[step if with_step_ptr else 0] = (G_SCALE, M_SCALE)
    sc = gd.inp(torch.from_numpy(np.asarray(scales, dtype=np.float32)), "scales")
    par = gd.inp(torch.from_numpy(D.params(spec, h * w) if params is None else params), "params")
    sp = gd.inp(torch.tensor([step], dtype=torch.int32), "step_ptr") if with_step_ptr else None
    out = eps if in_place else gd.out((B, n), torch.float32, float("nan"), "out")
    run_calls(ops.dynamic_threshold(eps=eps, out=out, scales=sc, params=par, step_ptr=sp, **dims))
    gd.check()
    after = None if sp is None else int(sp.cpu()[0])
    return out[:B].cpu().numpy().reshape(B, h, w, 4), after


def plane_error(got, ref, u, c, g=G_SCALE):
    """max over the planes of max |got - ref| / max |cfg|."""
    cfg = u.astype(np.float64) + g * (c.astype(np.float64) - u.astype(np.float64))
    S = np.abs(cfg).max(axis=(1, 2), keepdims=True)
    return float((np.abs(got.astype(np.float64) - ref) / S).max())


_REF = {}


def reference(shape, spec_items):
    from minsdtf_amd import dynthresh as D

    key = (shape, spec_items)
    if key not in _REF:
        u, c = data(shape)
        _REF[key] = D.dynthresh_host(u, c, G_SCALE, M_SCALE, dict(spec_items))
        _REF[key].setflags(write=False)
    return _REF[key]


@pytest.mark.parametrize("startpoint", ["mean", "zero"])
@pytest.mark.parametrize("measure", ["ad", "std"])
@pytest.mark.parametrize("percentile", PERCENTILES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_kernel_against_the_host_statement(gpu, shape, percentile, measure, startpoint):
    u, c = data(shape)
    for phi in ((1.0, 0.4) if shape == (2, 64, 64) else (1.0,)):
        spec = (("percentile", percentile), ("measure", measure), ("startpoint", startpoint), ("phi", phi))
        ref = reference(shape, spec)
        got, after = launch(gpu, u, c, dict(spec))
        err = plane_error(got, ref, u, c)
        print(f"dynthresh {shape} q = {percentile} {measure} {startpoint} phi = {phi}: max error / S = {err:.3e} (bound {BOUND:.3e})")
        assert np.all(np.isfinite(got)) and after == 1
        assert err <= BOUND


@pytest.mark.parametrize("shape", [(3, 32, 32), (2, 64, 64)], ids=lambda s: "x".join(str(v) for v in s))
def test_the_bound_tells_a_wrong_rank(gpu, shape):
    """The host statement at rank lo + 1 and lo - 1 lies outside the bound around the one at lo: up to P = 4096 the bound is a test
    of the rank (at P = 16384 neighbouring order statistics of these data lie about one bound apart; there the exact-arithmetic
    test and the shared selection code carry it)."""
    from minsdtf_amd import dynthresh as D

    u, c = data(shape)
    P = shape[1] * shape[2]
    lo, _f = D.rank(0.95, P)
    at = lambda r: D.dynthresh_host(u, c, G_SCALE, M_SCALE, dict(percentile=r / (P - 1)))
    mid = at(lo)
    got, _ = launch(gpu, u, c, dict(percentile=lo / (P - 1)))
    assert plane_error(got, mid, u, c) <= BOUND
    for other in (lo - 1, lo + 1):
        assert plane_error(at(other), mid, u, c) > 2 * BOUND
        assert plane_error(got, at(other), u, c) > BOUND


# ------------------------------------------------------------------------------------------------------- exact arithmetic
def exact_inputs(B, h, w):
    """u = 0; every plane of c holds each of 1 .. P / 2 once with each sign, shuffled per plane: sums are 0, every |value| is a
    tie of two.  With g = 8, m = 2 every fp32 operation of the launch is exact in any order."""
    P = h * w
    assert P % 2 == 0 and P // 2 >= 256 and 2 * (P // 2) < 8 * 256
    rng = np.random.default_rng(P)
    c = np.empty((B, P, 4), dtype=np.float32)
    base = np.concatenate([np.arange(1, P // 2 + 1), -np.arange(1, P // 2 + 1)]).astype(np.float32)
    for b in range(B):
        for ch in range(4):
            c[b, :, ch] = rng.permutation(base)
    return np.zeros((B, h, w, 4), dtype=np.float32), c.reshape(B, h, w, 4)


@pytest.mark.parametrize("shape", [(2, 32, 32), (1, 24, 40)], ids=lambda s: "x".join(str(v) for v in s))
def test_exact_arithmetic_bit_for_bit(gpu, shape):
    """|cc| sorted is 8 * [1, 1, 2, 2, ...]; lo = 510 is the first of the two 2048s, so s[hi] is s[lo] again and with frac = 0.5
    cfg_ref = 2048 = mx > mim_ref = 2 * P / 2: out = clamp(8 c, -2048, 2048) / 2048 * mim_ref exactly.  At lo - 1 cfg_ref is 2044,
    at lo + 1 (the last of the tie: the smallest key above) 2052: both outputs differ."""
    from minsdtf_amd import dynthresh as D

    B, h, w = shape
    P = h * w
    u, c = exact_inputs(B, h, w)
    scales = np.asarray([[3.0, 5.0], [8.0, 2.0], [3.0, 5.0]], dtype=np.float32)

    def run(lo):
        par = D.params(True, P)
        par[0] = lo
        par[3:4] = np.asarray([0.5], dtype=np.float32).view(np.int32)
        return launch(gpu, u, c, None, scales=scales, params=par)[0]

    mim_ref = np.float32(2.0 * (P // 2))
    want = (np.clip(8.0 * c, -2048.0, 2048.0) / np.float32(2048.0) * mim_ref).astype(np.float32)
    assert np.array_equal(want.astype(np.float64), np.clip(8.0 * c.astype(np.float64), -2048, 2048) / 2048 * float(mim_ref))
    got = run(510)
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
    for lo, ref in ((509, 2044.0), (511, 2052.0)):
        other = run(lo)
        assert not np.array_equal(other, got)
        exp = np.clip(8.0 * c.astype(np.float64), -ref, ref) / ref * float(mim_ref)
        assert np.abs(other - exp).max() <= BOUND * 8.0 * (P // 2)


# ------------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("shape", [(3, 32, 32), (2, 64, 64), (1, 64, 96), (1, 65, 127)], ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("measure", ["ad", "std"])
def test_in_place_equals_apart_and_runs_repeat(gpu, shape, measure):
    u, c = data(shape)
    spec = dict(percentile=0.95, measure=measure)
    apart, _ = launch(gpu, u, c, spec)
    again, _ = launch(gpu, u, c, spec)
    placed, _ = launch(gpu, u, c, spec, in_place=True)
    np.testing.assert_array_equal(again.view(np.int32), apart.view(np.int32))
    np.testing.assert_array_equal(placed.view(np.int32), apart.view(np.int32))


def test_step_ptr_selects_the_row_and_is_not_written(gpu):
    from minsdtf_amd import dynthresh as D

    shape = (2, 24, 40)
    u, c = data(shape)
    scales = np.asarray([[9.0, 3.0], [G_SCALE, M_SCALE], [14.0, 2.5]], dtype=np.float32)
    outs = []
    for step in range(3):
        got, after = launch(gpu, u, c, dict(percentile=0.95), step=step, scales=scales)
        assert after == step
        ref = D.dynthresh_host(u, c, float(scales[step, 0]), float(scales[step, 1]), dict(percentile=0.95))
        assert plane_error(got, ref, u, c, float(scales[step, 0])) <= BOUND
        outs.append(got)
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])
    null, after = launch(gpu, u, c, dict(percentile=0.95), with_step_ptr=False, scales=scales)   # NULL: row 0
    assert after is None
    np.testing.assert_array_equal(null.view(np.int32), outs[0].view(np.int32))
    # a counter outside the table is clamped to it
    for step, row in ((-3, 0), (7, 2)):
        got, after = launch(gpu, u, c, dict(percentile=0.95), step=step, scales=scales)
        assert after == step
        np.testing.assert_array_equal(got.view(np.int32), outs[row].view(np.int32))


@pytest.mark.parametrize("hw", [(32, 32), (64, 64), (65, 127)], ids=lambda s: "x".join(str(v) for v in s))
def test_a_sample_does_not_depend_on_its_batch(gpu, hw):
    u, c = data((3,) + hw)
    three, _ = launch(gpu, u, c, dict(percentile=0.999))
    for b in range(3):
        one, _ = launch(gpu, u[b:b + 1], c[b:b + 1], dict(percentile=0.999))
        np.testing.assert_array_equal(one[0].view(np.int32), three[b].view(np.int32))


@pytest.mark.parametrize("measure, startpoint", [("ad", "mean"), ("ad", "zero"), ("std", "mean"), ("std", "zero")])
def test_degenerate_plane_gives_cfg_bit_for_bit(gpu, measure, startpoint):
    """One plane of constant u and c: its cc and mc are exactly 0 and the divisor is 0.  That plane is cfg; the others are
    thresholded as ever."""
    from minsdtf_amd import dynthresh as D

    u, c = (a.copy() for a in data((2, 24, 40)))
    u[1, :, :, 2], c[1, :, :, 2] = 0.25, 0.75
    got, _ = launch(gpu, u, c, dict(percentile=0.9, measure=measure, startpoint=startpoint))
    cfg = np.float32(0.25 + G_SCALE * 0.5)   # exact in fp32
    np.testing.assert_array_equal(got[1, :, :, 2], np.full((24, 40), cfg, dtype=np.float32))
    ref = D.dynthresh_host(u, c, G_SCALE, M_SCALE, dict(percentile=0.9, measure=measure, startpoint=startpoint))
    assert np.all(np.isfinite(got)) and plane_error(got, ref, u, c) <= BOUND


def test_nan_beyond_the_operands_does_not_reach_out(gpu):
    """The guard bands around every operand are NaN (tests/_guard.py); on top of that a NaN plane in ANOTHER sample stays in that
    sample: nothing couples two samples, and the launch ends."""
    u, c = (a.copy() for a in data((3, 32, 32)))
    clean, _ = launch(gpu, u, c, dict(percentile=0.95))
    assert np.all(np.isfinite(clean))
    c[1, :, :, 0] = float("nan")
    got, _ = launch(gpu, u, c, dict(percentile=0.95))
    for b in (0, 2):
        np.testing.assert_array_equal(got[b].view(np.int32), clean[b].view(np.int32))
    np.testing.assert_array_equal(got[1, :, :, 1:].view(np.int32), clean[1, :, :, 1:].view(np.int32))


def test_argument_errors(gpu):
    from minsdtf_amd import _lib_dynthresh, ops

    B, h, w = 2, 8, 8
    eps = torch.zeros(2 * B, h * w * 4, device=gpu)
    out = torch.zeros(B, h * w * 4, device=gpu)
    scales, params = torch.ones(3, 2, device=gpu), torch.zeros(8, dtype=torch.int32, device=gpu)
    good = dict(eps=eps, out=out, scales=scales, params=params, batch=B, h=h, w=w, num_steps=3)
    st = torch.cuda.current_stream().cuda_stream
    for bad in (dict(eps=None), dict(out=None), dict(scales=None), dict(params=None), dict(batch=0), dict(h=1, w=1), dict(num_steps=0),
                dict(out=eps.data_ptr() + 16), dict(out=eps[B:]), dict(out=eps.data_ptr() + 4), dict(out=scales)):
        call = ops.dynamic_threshold(**{**good, **bad})
        assert call.fn(*call.args, st) == -1, bad
        assert b"dynamic_threshold" in _lib_dynthresh.load().msdt_last_error(), bad
    run_calls([ops.dynamic_threshold(**good), ops.dynamic_threshold(**{**good, "out": eps})])
    assert np.all(np.isfinite(out.cpu().numpy()))   # (all zeros: every plane degenerate, out = cfg = 0)


# ---------------------------------------------------------------------------------------------------------------- pipelines
@pytest.fixture(scope="module")
def nets(gpu):
    """The synthetic UNet at 64x64 and, on the same packed weights, at 128x128 and 256x256; the decoder."""
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


DT = dict(mimic_scale=4.0, percentile=0.95)
GUIDANCE = 14.0


@pytest.mark.parametrize("sampler", [None, "dpmpp_2m", "euler_a"])
def test_device_loop_vs_host_loop(gpu, nets, sampler):
    """The device loop against host_loop=True (predict_on_batch twice, dynthresh_host) with test_sag_gpu.py's bars: 45 dB for a
    samplers.py sampler, the project's 40 dB for the default step.  The plan is the plain job's plus ONE launch in front of a step
    that combines nothing; and the feature is not a no-op."""
    from oracle import sd_oracle as O

    sd, P = _pipe(gpu, nets)
    kw = dict(batch_size=1, num_steps=4, seed=11, sampler=sampler, unconditional_guidance_scale=GUIDANCE, guidance_rescale=0.0,
              return_latent=True)
    plain = sd.generate_image(P, **kw)
    plain_names = [c.name for c in next(iter(sd._engines.values())).calls]
    dev = sd.generate_image(P, dynamic_threshold=DT, **kw)
    eng = next(iter(sd._engines.values()))
    names = [c.name for c in eng.calls]
    step = "cfg_step" if sampler is None else "sampler_step"
    assert eng.dynthresh and names[-2:] == ["dynthresh", step] and names[:-2] + names[-1:] == plain_names
    host = sd.generate_image(P, host_loop=True, dynamic_threshold=DT, **kw)
    p, away = O.psnr(dev, host), O.psnr(plain, dev)
    bar = HOST_PSNR_MIN if sampler is not None else PSNR_MIN
    print(f"dynamic thresholding, {sampler or 'default step'}: device loop vs host loop {p:.1f} dB (bar {bar:.0f}); the plain job against it {away:.1f} dB")
    assert np.all(np.isfinite(dev)) and p >= bar
    assert away < p and away < 35.0


def test_scheduled_job_vs_host_loop(gpu, nets):
    """cfg_mode = "linear_down" towards cfg_scale_min: the launch reads another row of the table every step."""
    from oracle import sd_oracle as O

    sd, P = _pipe(gpu, nets)
    kw = dict(batch_size=2, num_steps=4, seed=12, unconditional_guidance_scale=GUIDANCE, return_latent=True)
    spec = dict(DT, cfg_mode="linear_down", cfg_scale_min=6.0, mimic_mode="half_cosine_down", mimic_scale_min=1.0)
    dev = sd.generate_image(P, dynamic_threshold=spec, **kw)
    eng = next(iter(sd._engines.values()))
    np.testing.assert_allclose(eng.dt_scales.cpu().numpy()[:, 0], [14.0, 14.0 - 8.0 / 3.0, 14.0 - 16.0 / 3.0, 6.0], rtol=1e-6)
    host = sd.generate_image(P, host_loop=True, dynamic_threshold=spec, **kw)
    const = sd.generate_image(P, dynamic_threshold=DT, **kw)
    p = O.psnr(dev, host)
    print(f"dynamic thresholding, scheduled: device loop vs host loop {p:.1f} dB; the constant job against it {O.psnr(const, dev):.1f} dB")
    assert p >= PSNR_MIN and O.psnr(const, dev) < p


def test_engine_reuse_and_rescale(gpu, nets):
    """Another mimic scale, percentile, measure and schedule on the resident engine: no new engine, no new graph; and
    guidance_rescale is not applied - 0.0 and 0.7 are one engine key apart and give the same bits."""
    sd, P = _pipe(gpu, nets)
    kw = dict(batch_size=1, num_steps=3, seed=5, unconditional_guidance_scale=GUIDANCE, return_latent=True)
    a = sd.generate_image(P, dynamic_threshold=DT, **kw)
    eng = next(iter(sd._engines.values()))
    graph = eng._loop_graph
    assert graph is not None and len(sd._engines) == 1
    outs = [a]
    for spec in (dict(mimic_scale=7.0, percentile=0.95), dict(mimic_scale=4.0, percentile=1.0), dict(DT, measure="std"),
                 dict(DT, startpoint="zero"), dict(DT, phi=0.5), dict(DT, mimic_mode="linear_down")):
        outs.append(sd.generate_image(P, dynamic_threshold=spec, **kw))
        assert len(sd._engines) == 1 and next(iter(sd._engines.values())) is eng and eng._loop_graph is graph
    for i in range(len(outs)):
        for j in range(i + 1, len(outs)):
            assert not np.array_equal(outs[i], outs[j]), (i, j)
    np.testing.assert_array_equal(sd.generate_image(P, dynamic_threshold=DT, **kw), a)
    rescaled = sd.generate_image(P, dynamic_threshold=DT, guidance_rescale=0.7, **kw)
    np.testing.assert_array_equal(rescaled.view(np.int32), a.view(np.int32))
    # None leaves the plain job what it was: another engine, the plain plan
    plain = sd.generate_image(P, guidance_rescale=0.7, **kw)
    eng0 = next(iter(sd._engines.values()))
    assert not eng0.dynthresh and eng0.dt_scales is None and "dynthresh" not in [c.name for c in eng0.calls]
    assert not np.array_equal(plain, a)


def test_a_sample_of_a_job_does_not_depend_on_its_batch(gpu, nets):
    sd, P = _pipe(gpu, nets)
    lat = np.random.default_rng(5).standard_normal((2, 16, 16, 4)).astype(np.float32)
    kw = dict(num_steps=3, unconditional_guidance_scale=GUIDANCE, return_latent=True, dynamic_threshold=DT)
    two = sd.generate_image(P, batch_size=2, diffusion_noise=lat, **kw)
    for b in range(2):
        one = sd.generate_image(P, batch_size=1, diffusion_noise=lat[b:b + 1], **kw)
        np.testing.assert_array_equal(one[0], two[b])
    calls = []
    stepped = sd.generate_image(P, batch_size=1, diffusion_noise=lat[1:], callback=calls.append, **kw)   # the per-step graphs
    assert calls == [1, 2, 3]
    np.testing.assert_array_equal(stepped[0], two[1])


def _halves():
    from minsdtf_amd import regions

    rng = np.random.default_rng(17)
    return dict(regions=[dict(prompt=rng.standard_normal((77, 768)).astype(np.float32), mask=m) for m in regions.boxes(16, 16, 1, 2)],
                base_weight=0.3)


@pytest.mark.parametrize("other", ["pag", "sag", "regions"])
def test_combinations_vs_host_loop(gpu, nets, other):
    """One job each with pag, sag and regions (latent mode): their combine writes c', the launch goes behind it; against the host
    loop, which takes the same order."""
    from oracle import sd_oracle as O

    sd, P = _pipe(gpu, nets)
    extra = {"pag": dict(pag=dict(scale=3.0)), "sag": dict(sag=dict(scale=3.0)), "regions": dict(regions=_halves())}[other]
    kw = dict(batch_size=1, num_steps=3, seed=9, unconditional_guidance_scale=GUIDANCE, return_latent=True, dynamic_threshold=DT, **extra)
    dev = sd.generate_image(P, **kw)
    eng = next(iter(sd._engines.values()))
    names = [c.name for c in eng.calls]
    front = {"pag": "pag_combine", "sag": "sag.combine", "regions": "region_combine"}[other]
    assert names[-3:] == [front, "dynthresh", "cfg_step"] and eng.dynthresh
    host = sd.generate_image(P, host_loop=True, **kw)
    without = sd.generate_image(P, **{**kw, "dynamic_threshold": None})
    p = O.psnr(dev, host)
    print(f"dynamic thresholding with {other}: device loop vs host loop {p:.1f} dB; the job without it against it {O.psnr(without, dev):.1f} dB")
    assert np.all(np.isfinite(dev)) and p >= PSNR_MIN and O.psnr(without, dev) < p


def test_hires_vs_the_host_loops_composed(gpu, nets):
    """hires: both passes threshold, each over its own executed steps.  Against the same job put together from the host loops -
    pass 1 with host_loop=True, the resample op on its own, pass 2 through _host_loop from the entry timestep."""
    from minsdtf_amd import dynthresh as D
    from minsdtf_amd import hires, ops
    from oracle import sd_oracle as O

    steps1, steps2, strength, seed = 3, 6, 0.5, 3
    sd, P = _pipe(gpu, nets, 64)
    kw = dict(batch_size=1, num_steps=steps1, seed=seed, unconditional_guidance_scale=GUIDANCE, return_latent=True)
    spec = dict(DT, mimic_mode="linear_down", mimic_scale_min=2.0)
    dev = sd.generate_image(P, hires=dict(scale=2, steps=steps2, strength=strength, upscaler="bilinear"), dynamic_threshold=spec, **kw)
    assert dev.shape == (1, 16, 16, 4) and len(sd._engines) == 2 and all(e.dynthresh for e in sd._engines.values())
    e2 = [e for e in sd._engines.values() if e.h == 16][0]
    a, s, start, run = hires.entry(sd.scheduler, None, steps2, strength)
    assert run == 3 and start == 3
    want = D.scales(spec, GUIDANCE, run).astype(np.float32)   # the schedule over the EXECUTED steps of pass 2
    np.testing.assert_array_equal(e2.dt_scales.cpu().numpy()[start:], want)
    lat1 = sd.generate_image(P, host_loop=True, dynamic_threshold=spec, **kw)
    rows = torch.from_numpy(hires.pack_rows(*hires.taps(8, 16, "bilinear"))).to(gpu)
    up = torch.empty(1, 16, 16, 4, dtype=torch.float32, device=gpu)
    z = torch.from_numpy(hires.draw_noise(1, 16, 16, seed)).to(gpu)
    run_calls(ops.latent_resample(x=torch.from_numpy(lat1).to(gpu), out=up, wx=rows, wy=rows, batch=1, h_in=8, w_in=8, h_out=16, w_out=16,
                                  a=a, s=s, noise=z))
    sd2, _ = _pipe(gpu, nets, 128)
    sd2.scheduler.set_timesteps(steps2)
    ascending = sd2.scheduler.timesteps[::-1][:run]
    host = sd2._host_loop(P[None], sd2.unconditional_context[None], up.cpu().numpy(), GUIDANCE, 0.0, None, None, ascending,
                          dynthresh=D.parse(spec))
    p = O.psnr(dev, np.asarray(host, dtype=np.float32))
    print(f"dynamic thresholding with hires: the device job vs the host loops composed {p:.1f} dB")
    assert p >= PSNR_MIN


@pytest.mark.parametrize("other", ["hypertile", "reference_only"])
def test_further_combinations_run(gpu, nets, other):
    """hypertile and reference_only change the UNet, not the tail: the launch sits in front of the step as ever; against the host
    loop."""
    from oracle import sd_oracle as O

    sd, P = _pipe(gpu, nets)
    extra = {"hypertile": dict(hypertile=dict(tile=64)),
             "reference_only": dict(reference_only=dict(latent=np.random.default_rng(3).standard_normal((1, 16, 16, 4)).astype(np.float32)))}[other]
    kw = dict(batch_size=1, num_steps=3, seed=9, unconditional_guidance_scale=GUIDANCE, return_latent=True, dynamic_threshold=DT, **extra)
    dev = sd.generate_image(P, **kw)
    names = [c.name for c in next(iter(sd._engines.values())).calls]
    assert names[-2:] == ["dynthresh", "cfg_step"]
    p = O.psnr(dev, sd.generate_image(P, host_loop=True, **kw))
    print(f"dynamic thresholding with {other}: device loop vs host loop {p:.1f} dB")
    assert p >= PSNR_MIN


def test_sharded_job_equals_unsharded(gpu):
    """A one-rank process group with forced collectives (as tests/test_sag_gpu.py): the sharded job == the unsharded one."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(HERE, "_dynthresh_world1_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=570)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert any(line.startswith("OK ") for line in p.stdout.splitlines()), p.stdout[-2000:]
    print(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("size", [128, 256])
def test_vs_oracle_fixture(gpu, nets, size):
    """The fixture jobs against the fp32 oracle's composition (tools/make_dynthresh_fixtures.py: unet_forward twice, dynthresh()
    restated with torch.quantile in float64, OracleScheduler.step): final latent PSNR >= 40 dB, where the same job WITHOUT the
    feature stays under 35 dB (`plain_psnr` in the file)."""
    from oracle import sd_oracle as O

    g = np.load(os.path.join(GOLD, f"dynthresh_{size}.npz"))
    assert (int(g["weight_seed"]), float(g["bias_scale"])) == (0, 0.05) and float(g["plain_psnr"]) < 35.0
    sd, _P = _pipe(gpu, nets, size)
    rng = np.random.default_rng(int(g["context_seed"]))
    ctx = (rng.standard_normal((1, 77, 768)) * float(g["context_scale"])).astype(np.float32)[0]
    sd.unconditional_context = (rng.standard_normal((1, 77, 768)) * float(g["context_scale"])).astype(np.float32)[0]
    spec = {k: (str(g[k]) if g[k].dtype.kind in "US" else float(g[k])) for k in
            ("mimic_scale", "percentile", "mimic_mode", "cfg_mode", "mimic_scale_min", "cfg_scale_min", "sched_val", "measure", "startpoint", "phi")}
    got = sd.generate_image(ctx, batch_size=1, num_steps=int(g["steps"]), unconditional_guidance_scale=float(g["guidance"]),
                            seed=int(g["noise_seed"]), guidance_rescale=0.0, return_latent=True, dynamic_threshold=spec)
    p = O.psnr(got, g["latent"])
    print(f"dynamic thresholding fixture {size}x{size} ({spec['mimic_mode']} mimic scale {spec['mimic_scale']}, percentile {spec['percentile']}): "
          f"final latent PSNR {p:.1f} dB; the plain job: {float(g['plain_psnr']):.1f} dB")
    assert p >= PSNR_MIN
