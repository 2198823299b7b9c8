"""Generate tests/golden/oracle_region_attention_<job>.npz: the fp32 CPU oracle's final latent of two attention-mode regional jobs
(``generate_image(..., regions={..., "mode": "attention"})``: every attn2 of the conditional forward computes
out(q) = sum_r w_r(q) softmax(q K_r^T) V_r with the level's weight plane), composed from pieces that exist without the product's
kernel:

  1. per step: oracle.sd_oracle.unet_forward for the unconditional context, and once for the conditional rows while this tool has
     replaced the module attribute sd_oracle.cross_attention by a function that, for every ".attn2", evaluates the attention of
     each region context (restated here from the formula, over sd_oracle.dense), sums them per query in float64 with the level's
     plane and applies to_out; everywhere else it calls the original (the attribute is restored afterwards; nothing under oracle/
     is edited);
  2. the level planes: minsdtf_amd.regions (parse -> Resolved.level_weights over the four ceil-halved levels) - the host-side rule
     under test is the kernel, not the block mean, which tests/test_region_attention_cpu.py holds to its definition;
  3. guidance, oracle.sd_oracle.rescale_noise_cfg, and the step: OracleScheduler.step (job a) or the DPM++ 2M update on the schedule of
     tools/make_sampler_fixtures.py (job b), as tools/make_pag_fixtures.py.

    python tools/make_region_attention_fixtures.py            (both jobs)
    python tools/make_region_attention_fixtures.py a          (one job)

  a  128x128 px, two binary halves,                                          default sampler, batch 1, rescale 0
  b  64x64 px, three soft overlapping masks (weights 1, 2, 0.5) + base 0.3,  dpmpp_2m,        batch 2, rescale 0.7

Stored: the masks, the region weights, the base weight, the seeds, the final latent and `plain_psnr`: the PSNR of the plain job (the
base prompt alone) against the regional latent.  The tool asserts plain_psnr < 30 dB, so the project's 40 dB bar tells the feature
from its absence; if the synthetic UNet moves too little the region contexts are scaled by CONTEXT_SCALE, recorded in the file as
`context_scale`.  Inputs are regenerated from the recorded numpy PCG64 seeds: contexts default_rng(1234) -> the base prompt, the
unconditional context, then one prompt per region, each (77, 768); noise default_rng(0) (B, h, w, 4).  Weights: the seeded synthetic
UNet (seed 0, bias_scale 0.05).  CFG 7.5, 4 steps.  Nothing of minsdtf_amd is used but the weight tables and regions.py.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLD = os.path.join(ROOT, "tests", "golden")
GUIDANCE, STEPS = 7.5, 4
WEIGHT_SEED, BIAS_SCALE, CONTEXT_SEED, NOISE_SEED = 0, 0.05, 1234, 0
PLAIN_PSNR_MAX = 30.0
CONTEXT_SCALE = {"a": 1.0, "b": 1.0}
ATTN2 = ".attn2"


def soft_masks(size):
    y, x = np.mgrid[0:size, 0:size] / (size - 1.0)
    return [1.0 - x, x, np.exp(-((x - 0.5) ** 2 + (y - 0.5) ** 2) / 0.08) + 0.05]


def halves(size):
    m = np.zeros((2, size // 8, size // 8))
    m[0, :, :size // 16] = 1.0
    m[1, :, size // 16:] = 1.0
    return list(m)


JOBS = {
    "a": dict(size=128, masks=halves, weights=(1.0, 1.0), base_weight=0.0, sampler=None, batch=1, rescale=0.0),
    "b": dict(size=64, masks=soft_masks, weights=(1.0, 2.0, 0.5), base_weight=0.3, sampler="dpmpp_2m", batch=2, rescale=0.7),
}


class regional_attention:
    """While active, sd_oracle.cross_attention mixes the region contexts `ctxs` (each (B, T, 768)) in every attn2 by the planes
    {tokens: (R, tokens) float64}."""

    def __init__(self, O, ctxs, planes):
        self.O, self.ctxs, self.planes = O, ctxs, planes

    def __enter__(self):
        import torch

        O, ctxs, planes, original = self.O, self.ctxs, self.planes, self.O.cross_attention
        self.original = original

        def cross_attention(x, context, W, name, heads=8):
            if not name.endswith(ATTN2):
                return original(x, context, W, name, heads)
            q = O.dense(x, W, name + ".to_q", bias=False)
            B, S, C = q.shape
            d = C // heads
            qh = q.view(B, S, heads, d).permute(0, 2, 1, 3)
            acc = torch.zeros(B, S, C, dtype=torch.float64)
            for r, c in enumerate(ctxs):
                c = torch.as_tensor(c)
                k = O.dense(c, W, name + ".to_k", bias=False).view(B, -1, heads, d).permute(0, 2, 3, 1)
                v = O.dense(c, W, name + ".to_v", bias=False).view(B, -1, heads, d).permute(0, 2, 1, 3)
                a = torch.matmul(torch.softmax(torch.matmul(qh, k) * (d ** -0.5), dim=-1), v).permute(0, 2, 1, 3).reshape(B, S, C)
                acc += torch.as_tensor(planes[S][r])[None, :, None] * a.double()
            return O.dense(acc.float(), W, name + ".to_out.0")

        O.cross_attention = cross_attention
        return self

    def __exit__(self, *exc):
        self.O.cross_attention = self.original
        return False


def run(tag):
    import torch

    import make_sampler_fixtures as MS
    from minsdtf_amd import regions as R
    from minsdtf_amd import weights as Wt
    from oracle import sd_oracle as O

    job = JOBS[tag]
    torch.set_num_threads(int(os.environ.get("REGION_THREADS", min(8, os.cpu_count() or 1))))
    Wn = O.named_weights(Wt.table("civitai_model"), Wt.synth_keras_weights("civitai_model", seed=WEIGHT_SEED, bias_scale=BIAS_SCALE))
    B, name, rescale, size = job["batch"], job["sampler"], job["rescale"], job["size"]
    h = w = size // 8
    masks = [np.asarray(m, dtype=np.float64) for m in job["masks"](size)]
    scale = float(CONTEXT_SCALE[tag])
    rng = np.random.default_rng(CONTEXT_SEED)
    base = rng.standard_normal((1, 77, 768)).astype(np.float32)
    unc = np.repeat(rng.standard_normal((1, 77, 768)).astype(np.float32), B, axis=0)
    prompts = [(scale * rng.standard_normal((1, 77, 768))).astype(np.float32) for _ in masks]
    res = R.parse(dict(regions=[dict(prompt=p[0], mask=m, weight=v) for p, m, v in zip(prompts, masks, job["weights"])],
                       base_weight=job["base_weight"], mode="attention"), size, size)
    levels = [(h, w)]
    for _ in range(3):
        levels.append(((levels[-1][0] + 1) // 2, (levels[-1][1] + 1) // 2))
    planes = {hl * wl: p.reshape(p.shape[0], -1).astype(np.float64) for (hl, wl), p in zip(levels, res.level_weights(levels))}
    assert len(planes) == 4
    ctxs = ([np.repeat(base, B, axis=0)] if job["base_weight"] > 0 else []) + [np.repeat(p, B, axis=0) for p in prompts]
    assert len(ctxs) == res.count
    noise = np.random.default_rng(NOISE_SEED).standard_normal((B, h, w, 4)).astype(np.float32)
    original = O.cross_attention
    t0 = time.time()

    def loop(regional):
        def guided_eps(latent, tau):
            lat = np.asarray(latent, dtype=np.float32)
            te = O.timestep_embedding(tau, B)
            u = np.asarray(O.unet_forward(Wn, lat, te, unc), dtype=np.float64)
            if regional:
                with regional_attention(O, ctxs, planes):
                    c = np.asarray(O.unet_forward(Wn, lat, te, ctxs[0]), dtype=np.float64)
                assert O.cross_attention is original
            else:
                c = np.asarray(O.unet_forward(Wn, lat, te, np.repeat(base, B, axis=0)), dtype=np.float64)
            e = u + GUIDANCE * (c - u)
            if rescale > 0:
                e = O.rescale_noise_cfg(e, c, rescale)
            print(f"  job {tag}, {'regional' if regional else 'plain'}: t = {tau} done at {time.time() - t0:.0f}s", flush=True)
            return e

        if name is None:
            s = O.OracleScheduler()
            s.set_timesteps(STEPS)
            x = noise
            for t in s.timesteps:
                x = s.step(guided_eps(x, t), t, x)
            return np.asarray(x, dtype=np.float32)
        assert name.startswith("dpmpp_2m") and "sde" not in name
        ts, sg = MS.schedule(name, STEPS)
        x = noise.astype(np.float64) * np.sqrt(1.0 + sg[0] ** 2)   # x_k = x / alpha
        old = h_last = None
        for i in range(STEPS):
            a = 1.0 / np.sqrt(1.0 + sg[i] * sg[i])
            d = x - sg[i] * np.asarray(guided_eps(a * x, ts[i]), dtype=np.float64)
            if sg[i + 1] == 0:
                x, hh = d, None
            else:   # k-diffusion's sample_dpmpp_2m (tools/make_sampler_fixtures.py: sample)
                hh = np.log(sg[i]) - np.log(sg[i + 1])
                dd = d
                if old is not None:
                    r = h_last / hh
                    dd = (1 + 1 / (2 * r)) * d - (1 / (2 * r)) * old
                x = (sg[i + 1] / sg[i]) * x - np.expm1(-hh) * dd
            old, h_last = d, hh
        return np.asarray(x, dtype=np.float32)

    latent = loop(True)
    plain = loop(False)
    plain_psnr = float(O.psnr(plain, latent))
    print(f"job {tag}: the plain job against the regional job: {plain_psnr:.1f} dB", flush=True)
    assert plain_psnr < PLAIN_PSNR_MAX, f"job {tag}: the regions move the latent too little ({plain_psnr:.1f} dB): raise CONTEXT_SCALE"
    out = os.path.join(GOLD, f"oracle_region_attention_{tag}.npz")
    np.savez_compressed(out, latent=latent, plain_psnr=plain_psnr, context_scale=scale, masks=np.stack(masks),
                        region_weights=np.asarray(job["weights"], dtype=np.float64), base_weight=job["base_weight"], size=size,
                        sampler="" if name is None else name, batch=B, steps=STEPS, weight_seed=WEIGHT_SEED, bias_scale=BIAS_SCALE,
                        context_seed=CONTEXT_SEED, noise_seed=NOISE_SEED, guidance=GUIDANCE, guidance_rescale=rescale)
    print("wrote", out, os.path.getsize(out), "bytes in", f"{time.time() - t0:.0f}s", flush=True)


def main(argv):
    for tag in (argv or list(JOBS)):
        run(tag)


if __name__ == "__main__":
    main(sys.argv[1:])
