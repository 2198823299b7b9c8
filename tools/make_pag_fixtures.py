"""Generate tests/golden/oracle_pag_<job>.npz: the fp32 CPU oracle's final latent of two perturbed-attention-guidance jobs
(``generate_image(..., pag=...)``: every step the UNet evaluates the conditional context once more with the self-attention map of
the selected blocks replaced by the identity, and eps = u + g (c - u) + s (c - p)), composed from pieces that exist without the
product's PAG code:

  1. per step: oracle.sd_oracle.unet_forward for the unconditional and the conditional context, and once more for the conditional
     context while this tool has replaced the module attribute sd_oracle.cross_attention by a function that, for the ".attn1" of a
     selected block, returns to_out(to_v(x)) - attention with the identity map - and calls the original everywhere else (the
     attribute is restored afterwards; nothing under oracle/ is edited);
  2. the combine, restated here in float64 from the formula: c' = c + k (c - p), k = s / g; eps = u + g (c' - u), which is the
     line above; oracle.sd_oracle.rescale_noise_cfg against c' (with guidance_rescale = 0 that is the plain formula);
  3. the step: OracleScheduler.step (job a), or the DPM++ 2M update in k-diffusion's sigma space on the schedule of
     tools/make_sampler_fixtures.py (job b).

    python tools/make_pag_fixtures.py            (both jobs)
    python tools/make_pag_fixtures.py a          (one job)

  a  128x128 px (mid block: 4 tokens), layers "mid",                                          default sampler, batch 1, rescale 0
  b  64x64 px, layers down_blocks.1.attentions.0, mid_block.attentions.0, up_blocks.2.attentions.2
     (16, 1 and 16 tokens),                                                                   dpmpp_2m,        batch 2, rescale 0.7

Stored: the scale, the layer names, the seeds and the final latent, and `plain_psnr`: the PSNR of the same job's latent with s = 0
(the plain job) against the PAG latent.  The tool asserts plain_psnr < 30 dB, so the project's 40 dB bar tells a PAG job from a
job without PAG; the scale of a fixture job is an input chosen for that (SCALE below), recorded in the file.  The other inputs are
regenerated from the recorded numpy PCG64 seeds: contexts default_rng(1234) -> the prompt, then the unconditional context, each
(77, 768); noise default_rng(0) (B, h, w, 4) - what generate_image(..., seed=0) draws.  Weights: the seeded synthetic UNet (seed 0,
bias_scale 0.05).  CFG 7.5, 4 steps.  Nothing of minsdtf_amd is used but the weight tables.
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
SCALE = {"a": 18.0, "b": 3.0}   # (a: at 3.0 the four mid-block tokens move the latent by 43 dB only)

JOBS = {
    "a": dict(size=128, layers=("mid_block.attentions.0",), sampler=None, batch=1, rescale=0.0),
    "b": dict(size=64, layers=("down_blocks.1.attentions.0", "mid_block.attentions.0", "up_blocks.2.attentions.2"),
              sampler="dpmpp_2m", batch=2, rescale=0.7),
}
ATTN1 = ".transformer_blocks.0.attn1"


class perturbed_attention:
    """While active, sd_oracle.cross_attention is the identity-map attention for the attn1 of `layers`."""

    def __init__(self, O, layers):
        self.O, self.layers = O, frozenset(layers)

    def __enter__(self):
        O, layers, original = self.O, self.layers, self.O.cross_attention
        self.original = original

        def cross_attention(x, context, W, name, heads=8):
            if name.endswith(ATTN1) and name[:-len(ATTN1)] in layers:
                assert context is None
                return O.dense(O.dense(x, W, name + ".to_v", bias=False), W, name + ".to_out.0")
            return original(x, context, W, name, heads)

        O.cross_attention = cross_attention
        return self

    def __exit__(self, *exc):
        self.O.cross_attention = self.original
        return False


def run(tag):
    import torch

    import make_sampler_fixtures as MS
    from minsdtf_amd import weights as Wt
    from oracle import sd_oracle as O

    job = JOBS[tag]
    torch.set_num_threads(int(os.environ.get("PAG_THREADS", min(8, os.cpu_count() or 1))))
    Wn = O.named_weights(Wt.table("civitai_model"), Wt.synth_keras_weights("civitai_model", seed=WEIGHT_SEED, bias_scale=BIAS_SCALE))
    B, name, layers, rescale = job["batch"], job["sampler"], job["layers"], job["rescale"]
    h = w = job["size"] // 8
    rng = np.random.default_rng(CONTEXT_SEED)
    ctx = np.repeat(rng.standard_normal((1, 77, 768)).astype(np.float32), B, axis=0)
    unc = np.repeat(rng.standard_normal((1, 77, 768)).astype(np.float32), B, axis=0)
    noise = np.random.default_rng(NOISE_SEED).standard_normal((B, h, w, 4)).astype(np.float32)
    original = O.cross_attention
    t0 = time.time()

    def loop(scale):
        k = scale / GUIDANCE

        def guided_eps(latent, tau):
            lat = np.asarray(latent, dtype=np.float32)
            te = O.timestep_embedding(tau, B)
            u = np.asarray(O.unet_forward(Wn, lat, te, unc), dtype=np.float64)
            c = np.asarray(O.unet_forward(Wn, lat, te, ctx), dtype=np.float64)
            if scale > 0:
                with perturbed_attention(O, layers):
                    p = np.asarray(O.unet_forward(Wn, lat, te, ctx), dtype=np.float64)
                assert O.cross_attention is original
                assert not np.array_equal(p, c) or all(s == 1 for s in tokens(layers, h, w))
                c = c + k * (c - p)
            e = u + GUIDANCE * (c - u)
            if rescale > 0:
                e = O.rescale_noise_cfg(e, c, rescale)
            print(f"  job {tag}, scale {scale}: t = {tau} done at {time.time() - t0:.0f}s", flush=True)
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
            d = x - sg[i] * guided_eps(a * x, ts[i]).astype(np.float64)
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
        return np.asarray(x, dtype=np.float32)   # (the last sigma is 0, alpha 1: x_k is the VP latent)

    scale = float(SCALE[tag])
    latent = loop(scale)
    plain = loop(0.0)
    plain_psnr = float(O.psnr(plain, latent))
    print(f"job {tag}: scale {scale}: the plain job against the PAG job: {plain_psnr:.1f} dB", flush=True)
    assert plain_psnr < PLAIN_PSNR_MAX, f"job {tag}: scale {scale} moves the latent too little ({plain_psnr:.1f} dB): raise SCALE"
    out = os.path.join(GOLD, f"oracle_pag_{tag}.npz")
    np.savez_compressed(out, latent=latent, plain_psnr=plain_psnr, scale=scale, layers=np.asarray(layers), size=job["size"],
                        sampler="" if name is None else name, batch=B, steps=STEPS, weight_seed=WEIGHT_SEED, bias_scale=BIAS_SCALE,
                        context_seed=CONTEXT_SEED, noise_seed=NOISE_SEED, guidance=GUIDANCE, guidance_rescale=rescale)
    print("wrote", out, os.path.getsize(out), "bytes in", f"{time.time() - t0:.0f}s", flush=True)


def tokens(layers, h, w):
    """Self-attention token count of each selected block."""
    lvl = {"down_blocks.0": 0, "down_blocks.1": 1, "down_blocks.2": 2, "mid_block": 3, "up_blocks.1": 2, "up_blocks.2": 1, "up_blocks.3": 0}
    return [(h >> lvl[n.rsplit(".attentions.", 1)[0]]) * (w >> lvl[n.rsplit(".attentions.", 1)[0]]) for n in layers]


def main(argv):
    for tag in (argv or list(JOBS)):
        run(tag)


if __name__ == "__main__":
    main(sys.argv[1:])
