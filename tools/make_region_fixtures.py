"""Generate tests/golden/oracle_regions_<job>.npz: the fp32 CPU oracle's final latent of two regional-prompting jobs
(``generate_image(..., regions=...)``: every step the UNet's conditional half runs once per region prompt and the predictions are
summed per latent pixel with the normalised mask weights in front of the guidance / sampler step), composed from pieces that
exist without the product's regional code:

  1. per step: oracle.sd_oracle.unet_forward for the unconditional context and for every region's context;
  2. the combine, restated here in float64 with the fp32-rounded weights: c = sum_r w_r * c_r per pixel;
  3. CFG and oracle.sd_oracle.rescale_noise_cfg against the combined c;
  4. the step: OracleScheduler.step (job a), or the DPM++ 2M update in k-diffusion's sigma space on the schedule of
     tools/make_sampler_fixtures.py (job b).

    python tools/make_region_fixtures.py            (both jobs)
    python tools/make_region_fixtures.py a          (one job)

  a  64x64 px, 2 binary regions (left / right halves),                          default sampler, batch 1, 4 steps
  b  64x64 px, 3 soft overlapping regions (weights 1, 2, 0.5) + base_weight 0.3,  dpmpp_2m,        batch 2, 4 steps

Stored: the masks (latent resolution), the region weights, the base weight, the seeds and the final latent.  The other inputs
are regenerated from the recorded numpy PCG64 seeds: contexts default_rng(1234) -> the base prompt, the unconditional context,
then one (77, 768) per region; noise default_rng(0) (B, 8, 8, 4) - what generate_image(..., seed=0) draws.  Weights: the seeded
synthetic UNet (seed 0, bias_scale 0.05).  CFG 7.5, rescale 0.7.  Nothing of minsdtf_amd is used but the weight tables: the
normalisation of the weights is written out here a second time.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLD = os.path.join(ROOT, "tests", "golden")
H = W = 8   # latent of a 64x64 picture
GUIDANCE, RESCALE = 7.5, 0.7
WEIGHT_SEED, BIAS_SCALE, CONTEXT_SEED, NOISE_SEED, MASK_SEED = 0, 0.05, 1234, 0, 77


def masks_a():
    left = np.zeros((H, W))
    left[:, :W // 2] = 1.0
    return [left, 1.0 - left]


def masks_b():
    """Three soft masks that overlap: a horizontal ramp, its mirror image, and a centred bump plus a little seeded texture."""
    x = np.linspace(0.0, 1.0, W)[None, :].repeat(H, axis=0)
    y = np.linspace(0.0, 1.0, H)[:, None].repeat(W, axis=1)
    bump = np.exp(-((x - 0.5) ** 2 + (y - 0.5) ** 2) / 0.08) + 0.1 * np.random.default_rng(MASK_SEED).random((H, W))
    return [1.0 - x, x, bump]


JOBS = {
    "a": dict(masks=masks_a, region_weights=(1.0, 1.0), base_weight=0.0, sampler=None, batch=1, steps=4),
    "b": dict(masks=masks_b, region_weights=(1.0, 2.0, 0.5), base_weight=0.3, sampler="dpmpp_2m", batch=2, steps=4),
}


def normalised(masks, region_weights, base_weight):
    """weight_r * mask_r / sum in float64, rounded once to fp32 (what the device reads), the base prompt's constant mask first."""
    m = np.stack([wt * np.asarray(x, dtype=np.float64) for wt, x in zip(region_weights, masks)])
    if base_weight > 0:
        m = np.concatenate([np.full((1, H, W), float(base_weight)), m])
    return (m / m.sum(axis=0)[None]).astype(np.float32).astype(np.float64)


def run(tag):
    import torch

    import make_sampler_fixtures as MS
    from minsdtf_amd import weights as Wt
    from oracle import sd_oracle as O

    job = JOBS[tag]
    torch.set_num_threads(int(os.environ.get("REGIONS_THREADS", min(8, os.cpu_count() or 1))))
    Wn = O.named_weights(Wt.table("civitai_model"), Wt.synth_keras_weights("civitai_model", seed=WEIGHT_SEED, bias_scale=BIAS_SCALE))
    B, n, name = job["batch"], job["steps"], job["sampler"]
    masks = job["masks"]()
    w = normalised(masks, job["region_weights"], job["base_weight"])
    rng = np.random.default_rng(CONTEXT_SEED)
    base = rng.standard_normal((1, 77, 768)).astype(np.float32)
    unc = np.repeat(rng.standard_normal((1, 77, 768)).astype(np.float32), B, axis=0)
    ctxs = [np.repeat(rng.standard_normal((1, 77, 768)).astype(np.float32), B, axis=0) for _ in masks]
    if job["base_weight"] > 0:
        ctxs = [np.repeat(base, B, axis=0)] + ctxs
    assert len(ctxs) == w.shape[0]
    noise = np.random.default_rng(NOISE_SEED).standard_normal((B, H, W, 4)).astype(np.float32)
    t0 = time.time()

    def guided_eps(latent, tau):
        lat = np.asarray(latent, dtype=np.float32)
        te = O.timestep_embedding(tau, B)
        u = O.unet_forward(Wn, lat, te, unc)
        c = np.zeros(lat.shape, dtype=np.float64)
        for r, ctx in enumerate(ctxs):
            c += w[r][None, :, :, None] * np.asarray(O.unet_forward(Wn, lat, te, ctx), dtype=np.float64)
        c = c.astype(np.float32)
        e = u + GUIDANCE * (c - u)
        e = O.rescale_noise_cfg(e, c, RESCALE)
        print(f"  job {tag}: t = {tau} done at {time.time() - t0:.0f}s", flush=True)
        return e

    if name is None:
        s = O.OracleScheduler()
        s.set_timesteps(n)
        x = noise
        for t in s.timesteps:
            x = s.step(guided_eps(x, t), t, x)
        latent = np.asarray(x, dtype=np.float32)
    else:
        assert name.startswith("dpmpp_2m") and "sde" not in name
        ts, sg = MS.schedule(name, n)
        x = noise.astype(np.float64) * np.sqrt(1.0 + sg[0] ** 2)   # x_k = x / alpha
        old = h_last = None
        for i in range(n):
            a = 1.0 / np.sqrt(1.0 + sg[i] * sg[i])
            d = x - sg[i] * guided_eps(a * x, ts[i]).astype(np.float64)
            if sg[i + 1] == 0:
                x, h = d, None
            else:   # k-diffusion's sample_dpmpp_2m (tools/make_sampler_fixtures.py: sample)
                h = np.log(sg[i]) - np.log(sg[i + 1])
                dd = d
                if old is not None:
                    r = h_last / h
                    dd = (1 + 1 / (2 * r)) * d - (1 / (2 * r)) * old
                x = (sg[i + 1] / sg[i]) * x - np.expm1(-h) * dd
            old, h_last = d, h
        latent = np.asarray(x, dtype=np.float32)   # (the last sigma is 0, alpha 1: x_k is the VP latent)
    out = os.path.join(GOLD, f"oracle_regions_{tag}.npz")
    np.savez_compressed(out, latent=latent, masks=np.stack(masks).astype(np.float64), region_weights=np.asarray(job["region_weights"]),
                        base_weight=float(job["base_weight"]), sampler="" if name is None else name, batch=B, steps=n,
                        weight_seed=WEIGHT_SEED, bias_scale=BIAS_SCALE, context_seed=CONTEXT_SEED, noise_seed=NOISE_SEED,
                        guidance=GUIDANCE, guidance_rescale=RESCALE)
    print("wrote", out, os.path.getsize(out), "bytes in", f"{time.time() - t0:.0f}s", flush=True)


def main(argv):
    for tag in (argv or list(JOBS)):
        run(tag)


if __name__ == "__main__":
    main(sys.argv[1:])
