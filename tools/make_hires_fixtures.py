"""Generate tests/golden/oracle_hires_<job>.npz: the fp32 CPU oracle's final latent of two hires jobs
(``generate_image(..., hires=...)``: denoise at the base size, upsample the latent, re-noise it part of the way, finish at the
target size), composed from pieces that exist without the product's hires code:

  1. pass 1: oracle.sd_oracle.denoise_loop at the base size (job b: the sigma-space loop of tools/make_sampler_fixtures.py);
  2. torch.nn.functional.interpolate on the float64 latent (align_corners=False);
  3. pass 2: denoise_loop(init_latent=..., strength=...) at the target size, per sample (job b: the same sigma-space loop
     handed sigmas[start:], entered at x_k = upsampled + sigma[start] * noise).

    python tools/make_hires_fixtures.py            (both jobs: job b is about an hour on 8 cores)
    python tools/make_hires_fixtures.py a          (one job)

  a  256x256 -> 512x512, bilinear, default sampler,   batch 1, 10 + 8 steps,  strength 0.5  (runs 4 of the 8)
  b  512x512 -> 768x768, bicubic,  dpmpp_2m_karras,   batch 2, 20 + 10 steps, strength 0.6  (runs 6 of the 10; ratio 1.5)

Inputs are NOT stored; they are regenerated from the recorded numpy PCG64 seeds: contexts default_rng(1234) -> cond then uncond
(1,77,768), tiled over the batch; initial noise default_rng(0) (B,h,w,4); re-noise default_rng([0, 2]) (B,h2,w2,4) - what
generate_image(..., seed=0, hires=...) draws.  Weights: the seeded synthetic UNet (seed 0).  CFG 7.5, rescale 0.7.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLD = os.path.join(ROOT, "tests", "golden")
JOBS = {
    "a": dict(base=256, target=512, upscaler="bilinear", sampler=None, batch=1, steps=10, hires_steps=8, strength=0.5),
    "b": dict(base=512, target=768, upscaler="bicubic", sampler="dpmpp_2m_karras", batch=2, steps=20, hires_steps=10, strength=0.6),
}
GUIDANCE, RESCALE = 7.5, 0.7


def upsample(latent, size, mode):
    """NHWC float64 -> NHWC float64 through torch's interpolate."""
    import torch
    import torch.nn.functional as F

    x = torch.from_numpy(np.asarray(latent, dtype=np.float64)).permute(0, 3, 1, 2)
    return F.interpolate(x, size=(size, size), mode=mode, align_corners=False).permute(0, 2, 3, 1).contiguous().numpy()


def run(tag):
    import torch

    import make_sampler_fixtures as MS
    from minsdtf_amd import weights as Wt
    from oracle import sd_oracle as O

    job = JOBS[tag]
    torch.set_num_threads(int(os.environ.get("HIRES_THREADS", min(8, os.cpu_count() or 1))))
    W = O.named_weights(Wt.table("civitai_model"), Wt.synth_keras_weights("civitai_model", seed=0))
    B, n1, n2, strength, name = job["batch"], job["steps"], job["hires_steps"], job["strength"], job["sampler"]
    h1, h2 = job["base"] // 8, job["target"] // 8
    rng = np.random.default_rng(1234)
    ctx = np.repeat(rng.standard_normal((1, 77, 768)).astype(np.float32), B, axis=0)
    unc = np.repeat(rng.standard_normal((1, 77, 768)).astype(np.float32), B, axis=0)
    noise = np.random.default_rng(0).standard_normal((B, h1, h1, 4)).astype(np.float32)
    noise2 = np.random.default_rng([0, 2]).standard_normal((B, h2, h2, 4)).astype(np.float32)
    run2 = int(n2 * strength + 0.5)
    t0 = time.time()
    count = [0]

    def unet(latent, t_emb, c, _controls):
        count[0] += 1
        print(f"  job {tag}: UNet call {count[0]} ({latent.shape[1] * 8} px) t={time.time() - t0:.0f}s", flush=True)
        return O.unet_forward(W, latent, t_emb, c)

    if name is None:
        base = O.denoise_loop(unet, ctx, unc, noise, num_steps=n1, guidance=GUIDANCE, guidance_rescale=RESCALE)
        up = upsample(base, h2, job["upscaler"])
        final = np.concatenate([
            O.denoise_loop(unet, ctx[b:b + 1], unc[b:b + 1], noise2[b:b + 1], num_steps=n2, guidance=GUIDANCE, guidance_rescale=RESCALE,
                           init_latent=up[b:b + 1], strength=strength) for b in range(B)], axis=0)
    else:
        def model(x_k, i, tau, s):
            # the UNet sees the VP latent x = alpha x_k and predicts eps; D = x_k - s eps
            a = 1.0 / np.sqrt(1.0 + s * s)
            lat = (a * x_k).astype(np.float32)
            te = O.timestep_embedding(tau, B)
            u = unet(lat, te, unc, None)
            c = unet(lat, te, ctx, None)
            e = u + GUIDANCE * (c - u)
            e = O.rescale_noise_cfg(e, c, RESCALE)
            return x_k - s * e.astype(np.float64)

        _, s1 = MS.schedule(name, n1)
        base, _ = MS.sample(name, n1, model, noise.astype(np.float64) * np.sqrt(1.0 + s1[0] ** 2), None)
        up = upsample(base, h2, job["upscaler"])
        _, s2 = MS.schedule(name, n2)
        start = n2 - run2
        final, _ = MS.sample(name, n2, model, up + s2[start] * noise2.astype(np.float64), None, start=start)
    out = os.path.join(GOLD, f"oracle_hires_{tag}.npz")
    np.savez_compressed(out, latent=np.asarray(final, dtype=np.float32), base_latent=np.asarray(base, dtype=np.float32),
                        sampler="" if name is None else name, upscaler=job["upscaler"], base=job["base"], target=job["target"],
                        batch=B, steps=n1, hires_steps=n2, strength=strength, run_steps=run2, weight_seed=0, context_seed=1234,
                        noise_seed=0, hires_noise_seed=np.asarray([0, 2]), guidance=GUIDANCE, guidance_rescale=RESCALE)
    print("wrote", out, os.path.getsize(out), "bytes in", f"{time.time() - t0:.0f}s", flush=True)


def main(argv):
    for tag in (argv or list(JOBS)):
        run(tag)


if __name__ == "__main__":
    main(sys.argv[1:])
