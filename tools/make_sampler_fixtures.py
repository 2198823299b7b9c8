"""Generate tests/golden/oracle_sampler_<job>.npz: the fp32 CPU oracle's final latent (and a per-step trace) for the
multistep / ancestral samplers of ``generate_image(..., sampler=...)`` at the C2 shape (512x512, batch 1).

    python tools/make_sampler_fixtures.py                         (all three jobs: about 20 minutes on 8 cores)
    python tools/make_sampler_fixtures.py dpmpp_2m_karras:20      (one job)

  dpmpp_2m_karras:20      tests/golden/oracle_sampler_dpmpp_2m_karras_20.npz
  dpmpp_2m_sde_karras:10  tests/golden/oracle_sampler_dpmpp_2m_sde_karras_10.npz
  euler_a:10              tests/golden/oracle_sampler_euler_a_10.npz

The samplers are written out here a second time, in k-diffusion's own sigma space (x_k = x / alpha) and float64, over
oracle.sd_oracle.unet_forward: this file does not use minsdtf_amd.samplers (the product's table builder), so the fixture
checks that builder's algebra as well as the kernel.

Inputs are NOT stored; they are regenerated from the recorded numpy PCG64 seeds: contexts default_rng(1234) -> cond then
uncond (1,77,768); initial noise default_rng(0) (1,64,64,4); per-step draws default_rng([0, 1]) (1, steps, 64, 64, 4),
which is what generate_image(..., seed=0) draws.  Weights: the seeded synthetic UNet (seed 0).  CFG 7.5, rescale 0.7.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
JOBS = {"dpmpp_2m_karras": 20, "dpmpp_2m_sde_karras": 10, "euler_a": 10}


def training_sigmas():
    """k-diffusion sigma of every training timestep: sqrt((1 - abar) / abar), scaled-linear betas."""
    betas = np.square(np.linspace(np.sqrt(0.00085), np.sqrt(0.012), 1000))
    abar = np.cumprod(1.0 - betas)
    return np.sqrt((1.0 - abar) / abar)


def schedule(name, n):
    """(timesteps (float), sigmas with the final 0 appended)."""
    sig = training_sigmas()
    if name.endswith("_karras"):
        rho = 7.0
        ramp = np.linspace(0.0, 1.0, n)
        lo, hi = sig[0] ** (1 / rho), sig[-1] ** (1 / rho)
        s = (hi + ramp * (lo - hi)) ** rho
        # k-diffusion's sigma_to_t: linear interpolation of log sigma between its two neighbours on the training grid
        ls = np.log(sig)
        t = np.empty(n)
        for i, v in enumerate(np.log(s)):
            lo_i = min(int(np.sum(v >= ls)) - 1, 998)
            lo_i = max(lo_i, 0)
            w = (ls[lo_i] - v) / (ls[lo_i] - ls[lo_i + 1])
            t[i] = (1 - w) * lo_i + w * (lo_i + 1)
    else:
        t = np.linspace(0, 1000, n, dtype=np.int32, endpoint=False)[::-1].astype(np.float64)
        s = sig[t.astype(np.int64)]
    return t, np.append(s, 0.0)


def sample(name, n, model, x_k, z, start=0):
    """k-diffusion's sample_dpmpp_2m / sample_dpmpp_2m_sde (eta 1, midpoint) / sample_euler_ancestral (eta 1), float64.
    model(x_k, i) -> denoised.  Returns (final x_k, [x_k after every step]).  `start` > 0: the sampler is handed sigmas[start:]
    (k-diffusion's img2img: x_k is the latent at sigma[start], the first executed step has no previous estimate)."""
    t, s = schedule(name, n)
    kind = name[:-len("_karras")] if name.endswith("_karras") else name
    x = np.asarray(x_k, dtype=np.float64)
    old, h_last, trace = None, None, []
    for i in range(start, n):
        d = model(x, i, t[i], s[i])
        if kind == "euler_a":
            s_up = min(s[i + 1], np.sqrt(s[i + 1] ** 2 * (s[i] ** 2 - s[i + 1] ** 2) / s[i] ** 2))
            s_dn = np.sqrt(s[i + 1] ** 2 - s_up ** 2)
            x = x + (x - d) / s[i] * (s_dn - s[i])
            if s[i + 1] > 0:
                x = x + z[:, i] * s_up
        elif s[i + 1] == 0:
            x = d
        else:
            h = np.log(s[i]) - np.log(s[i + 1])
            if kind == "dpmpp_2m":
                if old is None:
                    x = (s[i + 1] / s[i]) * x - np.expm1(-h) * d
                else:
                    r = h_last / h
                    dd = (1 + 1 / (2 * r)) * d - (1 / (2 * r)) * old
                    x = (s[i + 1] / s[i]) * x - np.expm1(-h) * dd
            else:   # dpmpp_2m_sde, eta 1, midpoint
                x = (s[i + 1] / s[i]) * np.exp(-h) * x + (-np.expm1(-2 * h)) * d
                if old is not None:
                    r = h_last / h
                    x = x + 0.5 * (-np.expm1(-2 * h)) * (1 / r) * (d - old)
                x = x + z[:, i] * s[i + 1] * np.sqrt(-np.expm1(-2 * h))
            h_last = h
        old = d
        trace.append(x.copy())
    return x, trace


def run(name, n):
    import torch

    from minsdtf_amd import weights as Wt
    from oracle import sd_oracle as O

    torch.set_num_threads(min(8, os.cpu_count() or 1))
    W = O.named_weights(Wt.table("civitai_model"), Wt.synth_keras_weights("civitai_model", seed=0))
    rng = np.random.default_rng(1234)
    ctx = rng.standard_normal((1, 77, 768)).astype(np.float32)
    unc = rng.standard_normal((1, 77, 768)).astype(np.float32)
    noise = np.random.default_rng(0).standard_normal((1, 64, 64, 4)).astype(np.float32)
    z = np.random.default_rng([0, 1]).standard_normal((1, n, 64, 64, 4)).astype(np.float32)
    t0 = time.time()

    def model(x_k, i, tau, s):
        # the UNet sees the VP latent x = alpha x_k and predicts eps; D = x_k - s eps
        a = 1.0 / np.sqrt(1.0 + s * s)
        lat = (a * x_k).astype(np.float32)
        te = O.timestep_embedding(tau, 1)
        u = O.unet_forward(W, lat, te, unc)
        c = O.unet_forward(W, lat, te, ctx)
        e = u + 7.5 * (c - u)
        e = O.rescale_noise_cfg(e, c, 0.7)
        print(f"  {name} step {i + 1}/{n} (t = {tau:.3f}) t={time.time() - t0:.0f}s", flush=True)
        return x_k - s * e.astype(np.float64)

    _, s = schedule(name, n)
    x_k = noise.astype(np.float64) * np.sqrt(1.0 + s[0] ** 2)   # x_k = x / alpha_0: the VP start latent is the noise itself
    x, trace = sample(name, n, model, x_k, z)
    # (the last sigma is 0, alpha 1: x_k is the VP latent; earlier steps are stored in the VP form the engine keeps)
    vp = [tr / np.sqrt(1.0 + s[i + 1] ** 2) for i, tr in enumerate(trace)]
    out = os.path.join(GOLD, f"oracle_sampler_{name}_{n}.npz")
    np.savez_compressed(out, latent=np.asarray(x, dtype=np.float32),
                        trace=np.stack(vp)[:, :, ::2, ::2, :].astype(np.float32),   # every step on a stride-2 latent grid
                        sampler=name, steps=n, weight_seed=0, context_seed=1234, noise_seed=0, step_noise_seed=np.asarray([0, 1]),
                        guidance=7.5, guidance_rescale=0.7, size=512)
    print("wrote", out, os.path.getsize(out), "bytes in", f"{time.time() - t0:.0f}s", flush=True)


def main(argv):
    jobs = dict(JOBS)
    if argv:
        jobs = {}
        for a in argv:
            nm, _, k = a.partition(":")
            jobs[nm] = int(k) if k else JOBS[nm]
    for nm, k in jobs.items():
        run(nm, k)


if __name__ == "__main__":
    main(sys.argv[1:])
