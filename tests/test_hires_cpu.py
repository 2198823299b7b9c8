"""Hires fix, host side (no GPU): the resampler's tap tables against torch's interpolate, the job description's errors, the C
struct of msd_latent_resample, the pass-2 entry point against image_to_image's, and what a sharded hires job broadcasts."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from minsdtf_amd import hires
from minsdtf_amd import samplers as smp
from minsdtf_amd.scheduler import Scheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_PAIRS = [(8, 16), (32, 64), (64, 96), (64, 128), (40, 72), (24, 40)]


def _interpolate(x, h_out, w_out, mode):
    """torch's float64 interpolate on an NHWC array."""
    kw = {} if mode.startswith("nearest") else {"align_corners": False}
    t = torch.from_numpy(np.asarray(x, dtype=np.float64)).permute(0, 3, 1, 2)
    return F.interpolate(t, size=(h_out, w_out), mode=mode, **kw).permute(0, 2, 3, 1).contiguous().numpy()


@pytest.mark.parametrize("mode", ["nearest", "nearest-exact", "bilinear", "bicubic"])
def test_taps_match_torch_interpolate(mode):
    """taps() applied with numpy in float64 == F.interpolate in float64, every size pair on each axis (so the two axes run at
    different ratios too): max abs difference <= 1e-12 of max |x|; indices inside the source; every row sums to 1."""
    rng = np.random.default_rng(5)
    for n_in, n_out in SIZE_PAIRS:
        idx, w = hires.taps(n_in, n_out, mode)
        assert idx.shape == (n_out, 4) and w.shape == (n_out, 4) and w.dtype == np.float64 and idx.dtype == np.int32
        assert idx.min() >= 0 and idx.max() < n_in
        assert np.abs(w.sum(axis=1) - 1.0).max() <= 1e-12
    for k, (h_in, h_out) in enumerate(SIZE_PAIRS):
        w_in, w_out = SIZE_PAIRS[(k + 1) % len(SIZE_PAIRS)]   # another ratio on the other axis
        for (hi, ho, wi, wo) in ((h_in, h_out, w_in, w_out), (h_in, h_out, h_in, h_out)):
            x = rng.standard_normal((2, hi, wi, 4))
            got = hires.resample_host(x, ho, wo, mode)
            want = _interpolate(x, ho, wo, mode)
            err = np.abs(got - want).max() / np.abs(x).max()
            assert err <= 1e-12, (mode, hi, ho, wi, wo, err)


def test_pack_rows_is_the_device_row():
    idx, w = hires.taps(24, 40, "bicubic")
    rows = hires.pack_rows(idx, w)
    assert rows.dtype == np.int32 and rows.shape == (40, 8) and rows.strides == (hires.ROW_BYTES, 4)
    np.testing.assert_array_equal(rows[:, :4], idx)
    np.testing.assert_array_equal(rows[:, 4:].view(np.float32), w.astype(np.float32))


@pytest.mark.parametrize("bad,match", [
    (dict(scale=2, upscaler="lanczos"), "unknown upscaler"),
    (dict(size=(1000, 1024)), "multiple of 64"),
    (dict(size=(1024, 1000)), "multiple of 64"),
    (dict(size=(448, 1024)), "smaller than the base"),
    (dict(size=(1024, 448)), "smaller than the base"),
    (dict(scale=1), "own size"),
    (dict(size=(512, 512)), "own size"),
    (dict(scale=2, strength=0.0), "strength"),
    (dict(scale=2, strength=1.0), "strength"),
    (dict(scale=2, strength=-0.2), "strength"),
    (dict(scale=2, steps=0), "steps"),
    (dict(), "exactly one"),
    (dict(scale=2, size=(1024, 1024)), "exactly one"),
    (dict(scale=2, blur=1), "unknown field"),
])
def test_parse_errors(bad, match):
    with pytest.raises(ValueError, match=match):
        hires.parse(bad, 512, 512, 25)
    if "blur" not in bad:
        with pytest.raises(ValueError, match=match):
            hires.parse(hires.HiresSpec(**bad), 512, 512, 25)


def test_parse_resolves_the_job():
    assert hires.parse(None, 512, 512, 25) is None
    j = hires.parse(dict(scale=2), 512, 512, 25)
    assert (j.height, j.width, j.steps, j.strength, j.upscaler, j.run_steps) == (1024, 1024, 25, 0.6, "bilinear", 15)
    j = hires.parse(hires.HiresSpec(size=(768, 1024), steps=10, strength=0.5, upscaler="bicubic"), 512, 768, 30)
    assert (j.height, j.width, j.steps, j.run_steps, j.upscaler) == (768, 1024, 10, 5, "bicubic")
    assert hires.parse(dict(scale=1.5), 512, 512, 8).height == 768
    with pytest.raises(ValueError, match="must be a HiresSpec"):
        hires.parse("2x", 512, 512, 25)


def test_latent_resample_struct_matches_header():
    from minsdtf_amd import _lib

    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "minsdtf_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n", '
           'sizeof(MsdLatentResample), offsetof(MsdLatentResample, wy), offsetof(MsdLatentResample, batch), '
           'offsetof(MsdLatentResample, s), sizeof(MsdResampleRow), offsetof(MsdResampleRow, w));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    S, R = _lib.MsdLatentResample, _lib.MsdResampleRow
    assert got == [ctypes.sizeof(S), S.wy.offset, S.batch.offset, S.s.offset, ctypes.sizeof(R), R.w.offset]
    assert ctypes.sizeof(R) == hires.ROW_BYTES


def test_latent_resample_abi_and_argument_errors_without_a_gpu():
    """The export is an addition to ABI 12; argument errors come back as -1 before anything is launched (no device needed)."""
    from minsdtf_amd import _lib

    assert "msd_latent_resample" in _lib.SYMBOLS and _lib.ABI_VERSION == 12
    lib = _lib.load()
    assert lib.msd_abi_version() == 12
    assert lib.msd_latent_resample(None, None) == -1
    assert b"null" in lib.msd_last_error()
    s = _lib.MsdLatentResample()
    s.in_, s.out, s.wx, s.wy = 1 << 20, 2 << 20, 3 << 20, 4 << 20
    s.batch, s.h_in, s.w_in, s.h_out, s.w_out = 1, 8, 8, 16, 16
    for field, value in (("in_", None), ("out", None), ("wx", None), ("wy", None), ("batch", 0), ("h_in", 0), ("w_out", 4),
                         ("h_out", 1 << 20), ("in_", (1 << 20) + 4), ("out", (2 << 20) + 8), ("noise", (5 << 20) + 4),
                         ("wx", (3 << 20) + 4), ("wy", (4 << 20) + 8), ("out", 1 << 20)):
        keep = getattr(s, field)
        setattr(s, field, value)
        assert lib.msd_latent_resample(ctypes.byref(s), None) == -1, field
        assert lib.msd_last_error()
        setattr(s, field, keep)


@pytest.mark.parametrize("sampler", [None] + smp.names())
@pytest.mark.parametrize("steps,strength", [(8, 0.5), (10, 0.6), (25, 0.6), (20, 0.35)])
def test_pass2_entry_is_image_to_images(sampler, steps, strength):
    """(a, s, start) of the second pass == what image_to_image uses for the same steps and strength: restated here from
    generate_image's reference_image branch."""
    sch = Scheduler()
    spec = smp.parse(sampler)
    a, s, start, run = hires.entry(sch, spec, steps, strength)
    # generate_image: set_timesteps; run_steps = int(n * strength + 0.5); start_index = n - run_steps
    ref = Scheduler()
    ref.set_timesteps(steps)
    run_steps = int(steps * strength + 0.5)
    assert (run, start) == (run_steps, steps - run_steps)
    if spec is None:
        t_entry = ref.timesteps[::-1][run_steps]
        want_a, want_s = ref.signal_rates[t_entry], ref.noise_rates[t_entry]
        assert list(sch.timesteps) == list(ref.timesteps)   # (the pipeline's scheduler is left on the pass-2 schedule)
    else:
        sched = smp.schedule(spec, ref, steps)
        want_a, want_s = sched.alphas[start], sched.noise_rates[start]
        encoded, noise = np.ones((1, 2, 2, 4), dtype=np.float32), np.full((1, 2, 2, 4), 2.0, dtype=np.float32)
        np.testing.assert_array_equal(a * encoded + s * noise, sched.entry_latent(start, encoded, noise))
    assert (a, s) == (float(want_a), float(want_s))


def test_entry_rejects_what_leaves_nothing_to_run():
    with pytest.raises(ValueError, match="no step"):
        hires.entry(Scheduler(), None, 4, 0.1)
    with pytest.raises(ValueError, match="first timestep"):
        hires.entry(Scheduler(), None, 4, 0.9)   # (the reference's rule indexes one past the schedule there)
    assert hires.entry(Scheduler(), smp.parse("euler_a"), 4, 0.9)[2:] == (0, 4)


def test_draws_have_their_own_streams_and_are_batch_independent():
    one, three = hires.draw_noise(1, 8, 8, seed=7), hires.draw_noise(3, 8, 8, seed=7)
    np.testing.assert_array_equal(one[0], three[0])
    np.testing.assert_array_equal(three, np.random.default_rng([7, 2]).standard_normal((3, 8, 8, 4)).astype(np.float32))
    np.testing.assert_array_equal(smp.draw_step_noise(2, 3, 4, 4, 7), np.random.default_rng([7, 1]).standard_normal((2, 3, 4, 4, 4)).astype(np.float32))
    np.testing.assert_array_equal(smp.draw_step_noise(2, 3, 4, 4, 7, stream_key=3),
                                  np.random.default_rng([7, 3]).standard_normal((2, 3, 4, 4, 4)).astype(np.float32))


@pytest.mark.parametrize("sampler", [None, "dpmpp_2m_karras", "euler_a"])
def test_sharded_hires_job_broadcasts_its_draws(monkeypatch, sampler):
    """Under shard_batch the re-noise draw - and a stochastic sampler's step draws of both passes - travel as per_sample inputs of
    dist.generate_sharded, for the global batch, sample-major."""
    from minsdtf_amd import dist as mdist
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sent = {}

    def fake_sharded(local, context, uncond_context, noise, device, per_sample=(), shared=(), shard=True):
        sent["per_sample"], sent["shared"], sent["shard"] = [np.asarray(a) for a in per_sample], list(shared), shard
        return torch.zeros(int(noise.shape[0]), 128, 64, 3, dtype=torch.uint8)

    monkeypatch.setattr(mdist, "world_size", lambda: 2)
    monkeypatch.setattr(mdist, "generate_sharded", fake_sharded)
    p = StableDiffusion(64, 64, device=torch.device("cpu"))
    p.shard_batch = True
    rng = np.random.default_rng(4)
    ctx, unc = rng.standard_normal((4, 77, 768)).astype(np.float32), rng.standard_normal((4, 77, 768)).astype(np.float32)
    out = p.generate_image(ctx, negative_prompt=unc, batch_size=4, num_steps=6, seed=2, sampler=sampler,
                           hires=dict(size=(128, 64), steps=5, strength=0.6))
    assert out.shape == (4, 128, 64, 3) and sent["shard"] and sent["shared"] == []
    np.testing.assert_array_equal(sent["per_sample"][0], np.random.default_rng([2, 2]).standard_normal((4, 16, 8, 4)).astype(np.float32))
    if sampler == "euler_a":
        assert [a.shape for a in sent["per_sample"][1:]] == [(4, 6, 8 * 8 * 4), (4, 5, 16 * 8 * 4)]
        np.testing.assert_array_equal(sent["per_sample"][2],
                                      np.random.default_rng([2, 3]).standard_normal((4, 5, 16, 8, 4)).astype(np.float32).reshape(4, 5, -1))
    else:
        assert len(sent["per_sample"]) == 1
    given = rng.standard_normal((4, 16, 8, 4)).astype(np.float32)
    p.generate_image(ctx, negative_prompt=unc, batch_size=4, num_steps=6, seed=2, sampler=sampler, hires_noise=given,
                     hires=dict(size=(128, 64), steps=5, strength=0.6))
    np.testing.assert_array_equal(sent["per_sample"][0], given)


def test_refused_combinations_raise_before_any_work():
    from minsdtf_amd.stable_diffusion import StableDiffusion

    p = StableDiffusion(64, 64, device=torch.device("cpu"))
    ctx = np.zeros((77, 768), dtype=np.float32)
    p.unconditional_context = ctx
    img = np.zeros((64, 64, 3), dtype=np.uint8)
    kw = dict(batch_size=1, num_steps=4, seed=0, hires=dict(scale=2))
    for extra in (dict(reference_image=img), dict(inpaint_mask=img[..., 0]), dict(control_net_image=img.astype(np.float32)),
                  dict(host_loop=True)):
        with pytest.raises(ValueError, match="hires"):
            p.generate_image(ctx, **kw, **extra)
    with pytest.raises(ValueError, match="hires"):
        StableDiffusion(64, 64, device=torch.device("cpu"), active_tcd=True).generate_image(ctx, **kw)
    with pytest.raises(ValueError, match="hires"):
        p.image_to_image(ctx, reference_image=img, **kw)
    with pytest.raises(ValueError, match="hires_noise"):
        p.generate_image(ctx, batch_size=1, num_steps=4, seed=0, hires_noise=np.zeros((1, 16, 16, 4), np.float32))
    with pytest.raises(ValueError, match="unknown upscaler"):
        p.text_to_image(ctx, batch_size=1, num_steps=4, seed=0, hires=dict(scale=2, upscaler="area"))
    assert not p._engines
