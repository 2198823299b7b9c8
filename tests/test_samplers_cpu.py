"""The multistep / ancestral samplers of generate_image(..., sampler=...) on the host: the float64 coefficient rows against this
file's own sigma-space restatement of k-diffusion's loops, convergence on Gaussian data, the schedules, the per-step draws of
the global batch (stub engine, also under a gloo world-2 process group) and the C struct of msd_sampler_step."""
import ctypes
import os
import socket
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dpmpp_2m", "dpmpp_2m_karras", "dpmpp_2m_sde", "dpmpp_2m_sde_karras", "euler_a", "euler_a_karras"]


# ------------------------------------------------------------------ k-diffusion's loops, in sigma space (x_k = x / alpha)
def _kdiff(kind, s, xk, denoise, z):
    """sample_dpmpp_2m / sample_dpmpp_2m_sde (eta 1, midpoint) / sample_euler_ancestral (eta 1) from sigma s[0] over the
    sigmas s (last one 0).  denoise(i, x_k) -> D; z[i] the step's draw.  Returns x_k after every step."""
    x, old, h_last, out = np.array(xk, dtype=np.float64), None, None, []
    for i in range(len(s) - 1):
        d = denoise(i, x)
        if kind == "euler_a":
            up = min(s[i + 1], np.sqrt(s[i + 1] ** 2 * (s[i] ** 2 - s[i + 1] ** 2) / s[i] ** 2))
            dn = np.sqrt(s[i + 1] ** 2 - up ** 2)
            x = x + (x - d) / s[i] * (dn - s[i])
            if s[i + 1] > 0:
                x = x + z[i] * up
        elif s[i + 1] == 0:
            x = d
        else:
            h = np.log(s[i] / s[i + 1])
            if kind == "dpmpp_2m":
                dd = d if old is None else (1 + 1 / (2 * h_last / h)) * d - old / (2 * h_last / h)
                x = (s[i + 1] / s[i]) * x - np.expm1(-h) * dd
            else:
                x = (s[i + 1] / s[i]) * np.exp(-h) * x - np.expm1(-2 * h) * d
                if old is not None:
                    x = x - 0.5 * np.expm1(-2 * h) * (h / h_last) * (d - old)
                x = x + z[i] * s[i + 1] * np.sqrt(-np.expm1(-2 * h))
            h_last = h
        old = d
        out.append(x.copy())
    return out


def _sched(name, n):
    from minsdtf_amd import samplers
    from minsdtf_amd.scheduler import Scheduler

    sch = Scheduler()
    sch.set_timesteps(n)
    return samplers.schedule(samplers.parse(name), sch, n)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("start", [0, 4])
def test_table_trajectories_match_kdiffusion(name, start):
    """x' = c_x x + c_D D + c_P P + c_z z over the rows (VP latent) == k-diffusion's loop in sigma space, on random D / z
    sequences, from evaluation 0 and from evaluation 4 (img2img: that row never reads P)."""
    from minsdtf_amd import samplers

    n = 12
    sc = _sched(name, n)
    s, a = sc.sigmas, sc.alphas
    rng = np.random.default_rng(3)
    D = rng.standard_normal((n, 5, 7)) * 0.8
    Z = rng.standard_normal((n, 5, 7))
    x0 = rng.standard_normal((5, 7)) * 3.0
    want = _kdiff(sc.spec.kind, s[start:], x0 / a[start], lambda i, x: D[start + i], Z[start:])
    tab = samplers.rows(sc, start)
    assert np.all(tab[start, 4] == 0.0) and np.all(tab[:, 6:] == 0.0)
    x, prev = x0.copy(), np.full_like(x0, np.nan)   # (P is never read before it is written)
    for j, i in enumerate(range(start, n)):
        e = (x - a[i] * D[i]) / sc.noise_rates[i]   # the noise prediction whose denoised estimate is D[i]
        x, prev = samplers.host_step(tab[i], x, e, prev, Z[i])
        np.testing.assert_allclose(prev, D[i], rtol=1e-12, atol=1e-12)
        ref = want[j] * a[i + 1]
        assert np.max(np.abs(x - ref)) <= 1e-10 * max(1.0, np.max(np.abs(ref))), (name, start, i)
    if sc.spec.kind == "dpmpp_2m":
        assert not np.any(tab[:, 5])
    np.testing.assert_array_equal(tab[-1, 2:6], [0.0, 1.0, 0.0, 0.0])   # last row: x' = D
    assert samplers.coefficient_table(sc, start).dtype == np.float32


def _gaussian_run(name, n, B=40000, seed=0):
    """x0 ~ N(0.3, 0.25) and its exact denoiser; returns (final x, the closed-form ODE endpoint of the same start)."""
    from minsdtf_amd import samplers

    mu, v = 0.3, 0.25
    sc = _sched(name, n)
    s, a = sc.sigmas, sc.alphas
    rng = np.random.default_rng(seed)
    xk0 = mu + rng.standard_normal(B) * np.sqrt(v + s[0] ** 2)
    Z = rng.standard_normal((n, B))
    tab = samplers.rows(sc, 0)
    x, prev = xk0 * a[0], None
    for i in range(n):
        d = mu + (x / a[i] - mu) * v / (v + s[i] ** 2)
        x, prev = samplers.host_step(tab[i], x, (x - a[i] * d) / sc.noise_rates[i], prev, Z[i])
    return x, mu + (xk0 - mu) * np.sqrt(v / (v + s[0] ** 2))


def test_dpmpp_2m_karras_is_second_order():
    err = {n: float(np.max(np.abs(np.subtract(*_gaussian_run("dpmpp_2m_karras", n))))) for n in (10, 20, 40)}
    print("dpmpp_2m_karras max error vs the ODE endpoint:", err)
    assert err[20] <= 0.35 * err[10] and err[40] <= 0.35 * err[20], err


def test_dpmpp_2m_sde_karras_samples_the_data():
    x, _ = _gaussian_run("dpmpp_2m_sde_karras", 100)
    assert abs(x.mean() - 0.3) <= 0.005 and abs(x.var() - 0.25) <= 0.01, (x.mean(), x.var())


def test_euler_a_variance_gap_shrinks():
    """Euler ancestral on the reference's timesteps: the variance gap to the data's shrinks with every doubling of the steps
    (0.046, 0.028, 0.017 at 50 / 100 / 200: about 0.6 per doubling, the first-order rate plus the fixed t = 0 endpoint)."""
    gap = {n: abs(float(_gaussian_run("euler_a", n)[0].var()) - 0.25) for n in (50, 100, 200)}
    print("euler_a variance gap:", gap)
    assert gap[100] <= 0.7 * gap[50] and gap[200] <= 0.7 * gap[100], gap


def test_karras_schedule_endpoints_and_sigma_to_t():
    from minsdtf_amd import samplers
    from minsdtf_amd.scheduler import Scheduler

    sch = Scheduler()
    train = samplers.training_sigmas(sch)
    np.testing.assert_allclose(train, sch.noise_rates / sch.signal_rates, rtol=0)
    sc = _sched("dpmpp_2m_karras", 15)
    np.testing.assert_allclose([sc.sigmas[0], sc.sigmas[-2]], [train[999], train[0]], rtol=1e-12)
    assert sc.sigmas[-1] == 0.0 and np.all(np.diff(sc.sigmas) < 0)
    np.testing.assert_allclose([sc.timesteps[0], sc.timesteps[-1]], [999.0, 0.0], atol=1e-9)
    assert np.all(np.diff(sc.timesteps) < 0) and not np.allclose(sc.timesteps, np.round(sc.timesteps))
    grid = np.arange(1000, dtype=np.float64)
    np.testing.assert_allclose(samplers.sigma_to_t(train, train), grid, atol=1e-9)
    # between two training sigmas: linear in log sigma
    mid = np.exp(0.5 * (np.log(train[10]) + np.log(train[11])))
    assert abs(samplers.sigma_to_t([mid], train)[0] - 10.5) < 1e-9
    # VP rates at integer t are the scheduler's
    sp = _sched("euler_a", 20)
    t = sp.timesteps.astype(int)
    np.testing.assert_allclose(sp.alphas[:-1], sch.signal_rates[t], rtol=1e-12)
    np.testing.assert_allclose(sp.noise_rates[:-1], sch.noise_rates[t], rtol=1e-12)


@pytest.mark.parametrize("n", [1, 7, 25, 50])
def test_plain_names_visit_the_reference_timesteps(n):
    from minsdtf_amd.scheduler import Scheduler

    sch = Scheduler()
    sch.set_timesteps(n)
    for kind in ("dpmpp_2m", "dpmpp_2m_sde", "euler_a"):
        np.testing.assert_array_equal(_sched(kind, n).timesteps, sch.timesteps.astype(np.float64))


def test_parse():
    from minsdtf_amd import samplers

    assert samplers.parse(None) is None
    assert sorted(samplers.names()) == sorted(NAMES)
    for nm in NAMES:
        sp = samplers.parse(nm)
        assert sp.name == nm and sp.karras == nm.endswith("_karras")
        assert sp.stochastic == (sp.kind != "dpmpp_2m")
    for bad in ("ddim", "dpmpp_2m_karras_karras", "euler", "", "DPMPP_2M", 3):
        with pytest.raises(ValueError):
            samplers.parse(bad)


def test_step_noise_is_sample_major():
    from minsdtf_amd import samplers

    one = samplers.draw_step_noise(1, 6, 4, 4, seed=11)
    four = samplers.draw_step_noise(4, 6, 4, 4, seed=11)
    assert one.shape == (1, 6, 4, 4, 4) and one.dtype == np.float32
    np.testing.assert_array_equal(one[0], four[0])
    np.testing.assert_array_equal(four, np.random.default_rng([11, 1]).standard_normal((4, 6, 4, 4, 4)).astype(np.float32))


# ------------------------------------------------------------------ the public API over a stub engine (CPU)
class _SamplerStubEngine:
    """Per-sample arithmetic on what prepare() receives: the latent, the rows of the schedule and the step draws."""

    def __init__(self, b, sampler):
        self.B, self.sampler, self.latent, self.seen = b, sampler, None, {}

    def contexts(self, u, c):
        return {"u": u, "c": c}

    def prepare(self, contexts, noise, scheduler, timesteps, start_index=0, hint_image=None, inpaint=None, step_noise=None,
                sampler=None):
        from minsdtf_amd import samplers

        f = lambda a: torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a).double()
        assert sampler is not None and sampler.spec.name == self.sampler
        lat = f(noise) + f(contexts["c"]).mean(dim=(1, 2))[:, None, None, None]
        tab = torch.from_numpy(samplers.rows(sampler, start_index))
        if step_noise is not None:
            sn = f(step_noise).reshape(self.B, tab.shape[0], *lat.shape[1:])
            self.seen["step_noise"] = sn.clone()
            for i in range(start_index, tab.shape[0]):
                lat = tab[i, 2] * lat + tab[i, 5] * sn[:, i]
        self.latent = lat.float()

    def run_steps(self, n, callback=None):
        pass


def _sampler_stub_pipeline(tcd=False):
    from minsdtf_amd.stable_diffusion import StableDiffusion

    class Pipe(StableDiffusion):
        def _engine(self, B, tc, tu, steps, g, phi, control, inpaint=False, sampler=None):
            assert sampler is not None   # (sampler=None keeps today's call, without the keyword)
            self.engines.append(_SamplerStubEngine(B, sampler))
            return self.engines[-1]

    p = Pipe(32, 32, active_tcd=tcd, device=torch.device("cpu"))
    p.engines = []
    return p


def _ctx(gb, seed=4):
    r = np.random.default_rng(seed)
    return r.standard_normal((gb, 77, 768)).astype(np.float32), r.standard_normal((gb, 77, 768)).astype(np.float32)


def test_sampler_draws_do_not_depend_on_the_batch():
    p = _sampler_stub_pipeline()
    ctx, unc = _ctx(4)
    outs = {}
    for B in (1, 4):
        outs[B] = p.generate_image(ctx[:B], negative_prompt=unc[:B], batch_size=B, num_steps=6, seed=9, sampler="euler_a",
                                   return_latent=True)
        assert p.engines[-1].B == B
    np.testing.assert_array_equal(p.engines[0].seen["step_noise"][0], p.engines[1].seen["step_noise"][0])
    np.testing.assert_array_equal(outs[1][0], outs[4][0])
    # the deterministic sampler takes no draws
    p.generate_image(ctx[:1], negative_prompt=unc[:1], batch_size=1, num_steps=6, seed=9, sampler="dpmpp_2m_karras", return_latent=True)
    assert "step_noise" not in p.engines[-1].seen


def test_sampler_argument_errors():
    p = _sampler_stub_pipeline()
    ctx, unc = _ctx(1)
    with pytest.raises(ValueError, match="unknown sampler"):
        p.generate_image(ctx, negative_prompt=unc, batch_size=1, num_steps=4, seed=0, sampler="heun")
    t = _sampler_stub_pipeline(tcd=True)
    for nm in ("dpmpp_2m", "euler_a_karras"):
        with pytest.raises(ValueError, match="TCD"):
            t.generate_image(ctx, negative_prompt=unc, batch_size=1, num_steps=4, seed=0, sampler=nm)
    assert not p.engines and not t.engines


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _sharded_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist

    from minsdtf_amd import dist as mdist

    mdist.init("gloo")
    p = _sampler_stub_pipeline()
    p.shard_batch = True
    ctx, unc = _ctx(4, seed=4 + 10 * rank)   # (rank 0's inputs must win)
    np.random.seed(123 + rank)               # (no seed: rank 0's global stream makes the draws)
    got = p.generate_image(ctx, negative_prompt=unc, batch_size=4, num_steps=5, seed=None, sampler="euler_a", return_latent=True,
                           diffusion_noise=np.random.default_rng(6).standard_normal((4, 4, 4, 4)).astype(np.float32))
    assert p.engines[-1].B == 2
    np.save(os.path.join(out_dir, f"euler_a_{rank}.npy"), got)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_sharded_euler_a_equals_single_process_world2(tmp_path):
    """euler_a under a gloo world-2 process group (batch_size = the global batch) == the single-process run: the draws are made
    for the global batch on rank 0 and travel with the broadcast."""
    world = 2
    mp.spawn(_sharded_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    p = _sampler_stub_pipeline()
    ctx, unc = _ctx(4)
    np.random.seed(123)
    want = p.generate_image(ctx, negative_prompt=unc, batch_size=4, num_steps=5, seed=None, sampler="euler_a", return_latent=True,
                            diffusion_noise=np.random.default_rng(6).standard_normal((4, 4, 4, 4)).astype(np.float32))
    for r in range(world):
        np.testing.assert_array_equal(np.load(os.path.join(str(tmp_path), f"euler_a_{r}.npy")), want)


@pytest.mark.parametrize("tcd,sampler", [(True, None), (False, None), (False, "dpmpp_2m_karras"), (False, "euler_a_karras")])
def test_sharded_run_broadcasts_only_its_own_draws(monkeypatch, tcd, sampler):
    """What a sharded job (world 2) puts into the packed broadcast besides contexts and noise: the TCD draws for a TCD run, the
    sampler's draws for a stochastic sampler, nothing for a deterministic one — never a second copy of another path's draws."""
    from minsdtf_amd import dist as mdist
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sent = {}

    def fake_sharded(local, context, uncond_context, noise, device, per_sample=(), shared=(), shard=True):
        sent["per_sample"], sent["shared"] = [np.asarray(a) for a in per_sample], list(shared)
        return torch.zeros(int(noise.shape[0]), 32, 32, 3, dtype=torch.uint8)

    monkeypatch.setattr(mdist, "world_size", lambda: 2)
    monkeypatch.setattr(mdist, "generate_sharded", fake_sharded)
    p = StableDiffusion(32, 32, active_tcd=tcd, device=torch.device("cpu"))
    p.shard_batch = True
    ctx, unc = _ctx(4)
    np.random.seed(5)
    p.generate_image(ctx, negative_prompt=unc, batch_size=4, num_steps=6, seed=2, sampler=sampler)
    shapes = [a.shape for a in sent["per_sample"]]
    if tcd or sampler == "euler_a_karras":
        assert shapes == [(4, 6, 4 * 4 * 4)], shapes
    else:
        assert shapes == [], shapes
    if sampler == "euler_a_karras":   # (sample-major: sample b's rows are its own block, as drawn)
        want = np.random.default_rng([2, 1]).standard_normal((4, 6, 4, 4, 4)).astype(np.float32).reshape(4, 6, -1)
        np.testing.assert_array_equal(sent["per_sample"][0], want)
    assert sent["shared"] == []


# ------------------------------------------------------------------ the C ABI
def test_sampler_step_struct_matches_header():
    from minsdtf_amd import _lib

    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "minsdtf_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n", '
           'sizeof(MsdSamplerStep), offsetof(MsdSamplerStep, advance), offsetof(MsdSamplerStep, step_noise), '
           'offsetof(MsdSamplerStep, denoised_prev));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    S = _lib.MsdSamplerStep
    assert got == [ctypes.sizeof(S), S.advance.offset, S.step_noise.offset, S.denoised_prev.offset]
    assert _lib.ABI_VERSION == 12 and "msd_sampler_step" in _lib.SYMBOLS


def test_sampler_step_rejects_bad_arguments_without_a_gpu():
    """Argument errors come back as MSD_E_ARG before anything is launched (no device needed)."""
    from minsdtf_amd import _lib

    lib = _lib.load()
    assert lib.msd_sampler_step(None, None) == -1
    s = _lib.MsdSamplerStep()
    s.eps, s.latent, s.coef, s.batch, s.n, s.num_steps = 16, 16, 16, 1, 4, 1
    assert lib.msd_sampler_step(ctypes.byref(s), None) == -1   # denoised_prev is required
    assert b"null" in lib.msd_last_error()
    s.denoised_prev, s.advance = 16, 1
    assert lib.msd_sampler_step(ctypes.byref(s), None) == -1   # advance without step_ptr
    s.advance, s.inpaint_mask = 0, 16
    assert lib.msd_sampler_step(ctypes.byref(s), None) == -1   # inpaint_mask without inpaint_init / inpaint_noise
