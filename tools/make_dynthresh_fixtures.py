"""Generate tests/golden/dynthresh_<size>.npz: the fp32 CPU oracle's final latent of two jobs with dynamic thresholding
(``generate_image(..., dynamic_threshold=...)``), composed from pieces that exist without the product's code for it:

  1. per step: oracle.sd_oracle.unet_forward for the unconditional and the conditional context;
  2. the extension's dynthresh() with sep_feat_channels = True restated here in float64 with torch.quantile (`dynthresh`), with
     the scales of the step from the schedule restated here (`schedule`);
  3. OracleScheduler.step on the result - no rescale.

    python tools/make_dynthresh_fixtures.py            (both sizes)
    python tools/make_dynthresh_fixtures.py 128        (one)

128x128 px and 256x256 px, batch 1, 4 steps, the seeded synthetic UNet (seed 0, bias_scale 0.05).  The contexts are
default_rng(context_seed) -> the prompt, then the unconditional context, each (77, 768) times `context_scale`; the noise is
default_rng(noise_seed) - what generate_image(..., seed=noise_seed) draws.  The 128 job holds both scales constant; the 256 job
moves the mimic scale down a cosine towards `mimic_scale_min` (a scheduled mode).

A fixture is only written when the PLAIN job at the same guidance scale lies under 35 dB against it (`plain_psnr`), so the
project's 40 dB bar tells the feature from its absence: the guidance scale is high and the mimic scale low for that.
Nothing of minsdtf_amd is used but the weight tables.
"""
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
GUIDANCE, STEPS = 14.0, 4
WEIGHT_SEED, BIAS_SCALE, NOISE_SEED, CONTEXT_SEED, CONTEXT_SCALE = 0, 0.05, 0, 1234, 1.0
PLAIN_PSNR_MAX = 35.0
JOBS = {128: dict(mimic_scale=4.0, percentile=0.95, mimic_mode="constant", cfg_mode="constant", mimic_scale_min=0.0, cfg_scale_min=0.0,
                  sched_val=1.0, measure="ad", startpoint="mean", phi=1.0),
        256: dict(mimic_scale=5.0, percentile=0.99, mimic_mode="cosine_down", cfg_mode="constant", mimic_scale_min=2.0, cfg_scale_min=0.0,
                  sched_val=1.0, measure="ad", startpoint="mean", phi=1.0)}
SIZES = (128, 256)


def shape(mode, frac, sched_val):
    return {"constant": 1.0, "linear_down": 1.0 - frac, "linear_up": frac, "cosine_down": math.cos(1.5707 * frac),
            "cosine_up": 1.0 - math.cos(1.5707 * frac), "half_cosine_down": math.cos(frac), "half_cosine_up": 1.0 - math.cos(frac),
            "power_up": frac ** sched_val, "power_down": 1.0 - frac ** sched_val}[mode]


def schedule(job, guidance, steps):
    """(g_i, m_i) per step: scale_i = min + (scale - min) * f(i / (steps - 1)), rounded to fp32 as the device table is."""
    out = []
    for i in range(steps):
        frac = i / (steps - 1) if steps > 1 else 0.0
        g = job["cfg_scale_min"] + (guidance - job["cfg_scale_min"]) * shape(job["cfg_mode"], frac, job["sched_val"])
        m = job["mimic_scale_min"] + (job["mimic_scale"] - job["mimic_scale_min"]) * shape(job["mimic_mode"], frac, job["sched_val"])
        out.append((float(np.float32(g)), float(np.float32(m))))
    return out


def dynthresh(u, c, g, m, job):
    """dynthresh() with sep_feat_channels = True on NHWC float64 arrays, through torch."""
    import torch

    u, c = (torch.from_numpy(np.asarray(a, dtype=np.float64)).permute(0, 3, 1, 2) for a in (u, c))
    d = c - u
    cfg, mim = u + g * d, u + m * d
    cfg_flat, mim_flat = cfg.flatten(2), mim.flatten(2)
    cfg_means = cfg_flat.mean(dim=2, keepdim=True)
    cfg_c, mim_c = cfg_flat - cfg_means, mim_flat - mim_flat.mean(dim=2, keepdim=True)
    if job["measure"] == "ad":
        mim_ref = mim_c.abs().max(dim=2, keepdim=True).values
        cfg_ref = torch.quantile(cfg_c.abs(), job["percentile"], dim=2, keepdim=True)
    else:
        mim_ref, cfg_ref = mim_c.std(dim=2, keepdim=True), cfg_c.std(dim=2, keepdim=True)
    if job["startpoint"] == "zero":
        r = cfg_flat * (mim_ref / cfg_ref)
    elif job["measure"] == "ad":
        mx = torch.maximum(mim_ref, cfg_ref)
        r = torch.minimum(torch.maximum(cfg_c, -mx), mx) / mx * mim_ref + cfg_means
    else:
        r = cfg_c / cfg_ref * mim_ref + cfg_means
    out = job["phi"] * r + (1.0 - job["phi"]) * cfg_flat
    return out.reshape(cfg.shape).permute(0, 2, 3, 1).numpy()


def run(size):
    import torch

    from minsdtf_amd import weights as Wt
    from oracle import sd_oracle as O

    torch.set_num_threads(int(os.environ.get("DYNTHRESH_THREADS", min(16, os.cpu_count() or 1))))
    Wn = O.named_weights(Wt.table("civitai_model"), Wt.synth_keras_weights("civitai_model", seed=WEIGHT_SEED, bias_scale=BIAS_SCALE))
    h = w = size // 8
    job = JOBS[size]
    noise = np.random.default_rng(NOISE_SEED).standard_normal((1, h, w, 4)).astype(np.float32)
    rng = np.random.default_rng(CONTEXT_SEED)
    ctx = (rng.standard_normal((1, 77, 768)) * CONTEXT_SCALE).astype(np.float32)
    unc = (rng.standard_normal((1, 77, 768)) * CONTEXT_SCALE).astype(np.float32)
    t0 = time.time()

    def loop(thresholded):
        s = O.OracleScheduler()
        s.set_timesteps(STEPS)
        table = schedule(job, GUIDANCE, STEPS)
        x = noise
        for i, t in enumerate(s.timesteps):
            lat = np.asarray(x, dtype=np.float32)
            te = O.timestep_embedding(t, 1)
            u = np.asarray(O.unet_forward(Wn, lat, te, unc), dtype=np.float64)
            c = np.asarray(O.unet_forward(Wn, lat, te, ctx), dtype=np.float64)
            e = dynthresh(u, c, table[i][0], table[i][1], job) if thresholded else u + GUIDANCE * (c - u)
            x = s.step(e, t, x)
            print(f"  {size}: {'thresholded' if thresholded else 'plain'}, t = {t} (g, m = {table[i]}) done at {time.time() - t0:.0f}s", flush=True)
        return np.asarray(x, dtype=np.float32)

    latent = loop(True)
    plain_psnr = float(O.psnr(loop(False), latent))
    print(f"{size}: the plain job against the thresholded job: {plain_psnr:.1f} dB", flush=True)
    assert np.all(np.isfinite(latent))
    assert plain_psnr < PLAIN_PSNR_MAX, f"{size}: the job moves the latent too little ({plain_psnr:.1f} dB): raise GUIDANCE or lower mimic_scale"
    out = os.path.join(GOLD, f"dynthresh_{size}.npz")
    np.savez_compressed(out, latent=latent, plain_psnr=plain_psnr, size=size, steps=STEPS, weight_seed=WEIGHT_SEED, bias_scale=BIAS_SCALE,
                        context_seed=CONTEXT_SEED, context_scale=CONTEXT_SCALE, noise_seed=NOISE_SEED, guidance=GUIDANCE, **job)
    print("wrote", out, os.path.getsize(out), "bytes in", f"{time.time() - t0:.0f}s", flush=True)


def main(argv):
    for size in ([int(a) for a in argv] or list(SIZES)):
        run(size)


if __name__ == "__main__":
    main(sys.argv[1:])
