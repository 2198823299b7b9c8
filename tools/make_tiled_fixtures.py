"""Generate tests/golden/oracle_tiled_<job>.npz: the fp32 CPU oracle's final canvas latent of two tiled-diffusion jobs
(``generate_image(..., tiled=...)``: every step the UNet runs at the tile size on overlapping views of one canvas latent, every
view takes its own sampler step, and the stepped views are averaged where they overlap), composed from pieces that exist
without the product's tiled code:

  1. per view and step: oracle.sd_oracle.unet_forward (uncond, cond), CFG, oracle.sd_oracle.rescale_noise_cfg (per view: a
     view is a sample of the UNet's batch);
  2. the step: OracleScheduler.step per view (job a), or the DPM++ 2M update in k-diffusion's sigma space on the schedule of
     tools/make_sampler_fixtures.py, each view keeping its own previous denoised estimate (job b);
  3. the consensus, restated here in float64: canvas = sum_v w_v x_v / sum_v w_v over the covering views, written back to the views.

    python tools/make_tiled_fixtures.py            (both jobs)
    python tools/make_tiled_fixtures.py a          (one job)

  a  tile 256, canvas 384x384, stride 128 (2x2 views),                    default sampler,  uniform,  batch 1,  8 steps
  b  tile 512, canvas 512x768, stride 128 (1x3 views at 0, 128, 256 px),   dpmpp_2m_karras,  gaussian, batch 2, 10 steps

Inputs are NOT stored; they are regenerated from the recorded numpy PCG64 seeds: contexts default_rng(1234) -> cond then uncond
(1,77,768), tiled over the batch and the views; canvas noise default_rng(0) (B,H/8,W/8,4) - what generate_image(..., seed=0,
tiled=...) draws.  Weights: the seeded synthetic UNet (seed 0).  CFG 7.5, rescale 0.7.  Nothing of minsdtf_amd is used but the
weight tables: offsets and blend weights are written out here a second time.
"""
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLD = os.path.join(ROOT, "tests", "golden")
JOBS = {
    "a": dict(tile=(256, 256), size=(384, 384), stride=(128, 128), blend="uniform", sampler=None, batch=1, steps=8),
    "b": dict(tile=(512, 512), size=(512, 768), stride=(128, 128), blend="gaussian", sampler="dpmpp_2m_karras", batch=2, steps=10),
}
GUIDANCE, RESCALE = 7.5, 0.7


def offsets(length, tile, stride):
    """n = ceil((L - t) / s) + 1 views, the last one snapped to the edge."""
    n = int(math.ceil((length - tile) / stride)) + 1
    return [min(i * stride, length - tile) for i in range(n)]


def weights(t, blend):
    """Separable blend row, float64 rounded to fp32 (what the device reads)."""
    if blend == "uniform":
        return np.ones(t)
    i = np.arange(t, dtype=np.float64)
    return np.exp(-(((i - (t - 1) / 2.0) / t) ** 2) / (2.0 * 0.01)).astype(np.float32).astype(np.float64)


def consensus(views, where, wy, wx, shape):
    """views[v]: (B, th, tw, 4) float64 at where[v] = (y, x) -> the canvas (B, H, W, 4): the weighted mean over the covering views."""
    acc, wsum = np.zeros(shape), np.zeros((1,) + shape[1:3] + (1,))
    w2 = np.outer(wy, wx)[None, :, :, None]
    th, tw = len(wy), len(wx)
    for x, (y0, x0) in zip(views, where):
        acc[:, y0:y0 + th, x0:x0 + tw] += w2 * x
        wsum[:, y0:y0 + th, x0:x0 + tw] += w2
    return acc / wsum


def run(tag):
    import torch

    import make_sampler_fixtures as MS
    from minsdtf_amd import weights as Wt
    from oracle import sd_oracle as O

    job = JOBS[tag]
    torch.set_num_threads(int(os.environ.get("TILED_THREADS", min(8, os.cpu_count() or 1))))
    W = O.named_weights(Wt.table("civitai_model"), Wt.synth_keras_weights("civitai_model", seed=0))
    B, n, name = job["batch"], job["steps"], job["sampler"]
    th, tw = job["tile"][0] // 8, job["tile"][1] // 8
    H, Wc = job["size"][0] // 8, job["size"][1] // 8
    ys, xs = offsets(H, th, job["stride"][0] // 8), offsets(Wc, tw, job["stride"][1] // 8)
    where = [(y, x) for y in ys for x in xs]   # row-major
    wy, wx = weights(th, job["blend"]), weights(tw, job["blend"])
    rng = np.random.default_rng(1234)
    ctx = np.repeat(rng.standard_normal((1, 77, 768)).astype(np.float32), B, axis=0)
    unc = np.repeat(rng.standard_normal((1, 77, 768)).astype(np.float32), B, axis=0)
    noise = np.random.default_rng(0).standard_normal((B, H, Wc, 4)).astype(np.float32)
    t0 = time.time()
    count = [0]

    def guided_eps(latent, tau):
        """CFG + rescale of one view's batch at time tau (the view is its own sample: the rescale's std is per view)."""
        count[0] += 1
        lat = np.asarray(latent, dtype=np.float32)
        te = O.timestep_embedding(tau, B)
        u = O.unet_forward(W, lat, te, unc)
        c = O.unet_forward(W, lat, te, ctx)
        e = u + GUIDANCE * (c - u)
        e = O.rescale_noise_cfg(e, c, RESCALE)
        print(f"  job {tag}: view evaluation {count[0]}/{n * len(where)} t={time.time() - t0:.0f}s", flush=True)
        return e

    def cut(canvas):
        return [canvas[:, y:y + th, x:x + tw] for (y, x) in where]

    shape = (B, H, Wc, 4)
    if name is None:
        scheds = [O.OracleScheduler() for _ in where]
        for s in scheds:
            s.set_timesteps(n)
        canvas = noise.astype(np.float64)
        for t in scheds[0].timesteps:
            stepped = []
            for s, x in zip(scheds, cut(canvas)):
                e = guided_eps(x, t)
                stepped.append(np.asarray(s.step(e, t, x), dtype=np.float64))
            canvas = consensus(stepped, where, wy, wx, shape)
    else:
        assert name.startswith("dpmpp_2m") and "sde" not in name
        ts, s = MS.schedule(name, n)
        canvas = noise.astype(np.float64) * np.sqrt(1.0 + s[0] ** 2)   # x_k = x / alpha: the same factor for every view of a step
        old = [None] * len(where)
        h_last = None
        for i in range(n):
            a = 1.0 / np.sqrt(1.0 + s[i] * s[i])
            stepped = []
            h = None if s[i + 1] == 0 else np.log(s[i]) - np.log(s[i + 1])
            for v, x in enumerate(cut(canvas)):
                e = guided_eps(a * x, ts[i])
                d = x - s[i] * e.astype(np.float64)
                if h is None:
                    nx = d
                else:   # k-diffusion's sample_dpmpp_2m (tools/make_sampler_fixtures.py: sample)
                    dd = d
                    if old[v] is not None:
                        r = h_last / h
                        dd = (1 + 1 / (2 * r)) * d - (1 / (2 * r)) * old[v]
                    nx = (s[i + 1] / s[i]) * x - np.expm1(-h) * dd
                old[v] = d
                stepped.append(nx)
            h_last = h
            canvas = consensus(stepped, where, wy, wx, shape)
        # (the last sigma is 0, alpha 1: x_k is the VP latent)
    out = os.path.join(GOLD, f"oracle_tiled_{tag}.npz")
    np.savez_compressed(out, latent=np.asarray(canvas, dtype=np.float32), sampler="" if name is None else name, blend=job["blend"],
                        tile=np.asarray(job["tile"]), size=np.asarray(job["size"]), stride=np.asarray(job["stride"]),
                        ys=np.asarray(ys), xs=np.asarray(xs), batch=B, steps=n, weight_seed=0, context_seed=1234, noise_seed=0,
                        guidance=GUIDANCE, guidance_rescale=RESCALE)
    print("wrote", out, os.path.getsize(out), "bytes in", f"{time.time() - t0:.0f}s", flush=True)


def main(argv):
    for tag in (argv or list(JOBS)):
        run(tag)


if __name__ == "__main__":
    main(sys.argv[1:])
