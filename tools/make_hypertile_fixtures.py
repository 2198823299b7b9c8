"""Generate tests/golden/oracle_hypertile_<job>.npz: the fp32 CPU oracle's final latent of two HyperTile jobs
(``generate_image(..., hypertile={...})``: the self-attention of the attention blocks of the UNet levels 0 .. depth is taken inside
non-overlapping windows of the feature map), composed from pieces that exist without the product's kernel:

  1. per step: oracle.sd_oracle.unet_forward over the u rows and over the c rows while this tool has replaced the module attribute
     sd_oracle.cross_attention by a function that, for every ".attn1" of a selected level, projects q / k / v (sd_oracle.dense),
     cuts the tokens into the nh x nw windows, takes softmax(q k^T / sqrt(d)) v inside each window (restated here from the formula)
     and applies to_out; everywhere else it calls the original (the attribute is restored afterwards; nothing under oracle/ is
     edited);
  2. guidance and OracleScheduler.step (the default sampler).

    python tools/make_hypertile_fixtures.py            (both jobs)
    python tools/make_hypertile_fixtures.py a          (one job)

  a  256x128 px (height x width), tile 64,  depth 0: 4 x 2 windows of 8 x 8 tokens,                batch 2
  b  256x256 px,                  tile 128, depth 1: 2 x 2 windows of 16 x 16 and 8 x 8 tokens,    batch 1

Stored: the seeds, the tile, the depth, the final latent and `plain_psnr`: the PSNR of the plain job against the windowed latent.
The tool asserts plain_psnr < 30 dB, so the project's 40 dB bar tells the feature from its absence.  Inputs are regenerated from
the recorded numpy PCG64 seeds: contexts default_rng(1234) -> the prompt, then the unconditional context, each (77, 768); noise
default_rng(0) (B, h, w, 4).  Weights: the seeded synthetic UNet (seed 0, bias_scale 0.05).  CFG 7.5, 4 steps, rescale 0.  Nothing
of minsdtf_amd is used but the weight tables.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
GUIDANCE, STEPS = 7.5, 4
WEIGHT_SEED, BIAS_SCALE, CONTEXT_SEED, NOISE_SEED = 0, 0.05, 1234, 0
PLAIN_PSNR_MAX = 30.0
ATTN1 = ".transformer_blocks.0.attn1"

JOBS = {
    "a": dict(height=256, width=128, tile=64, depth=0, batch=2),
    "b": dict(height=256, width=256, tile=128, depth=1, batch=1),
}


def level_of(block):
    """UNet level of an attention block name, None for the mid block."""
    parts = block.split(".")
    if parts[0] == "down_blocks":
        return int(parts[1])
    if parts[0] == "up_blocks":
        return 3 - int(parts[1])
    return None


class windowed_attention:
    """While active, sd_oracle.cross_attention gives every ".attn1" of the levels 0 .. depth the windowed route: nh x nw windows
    of the level's (h >> level) x (w >> level) feature map."""

    def __init__(self, O, h, w, nh, nw, depth):
        self.O, self.geo = O, (h, w, nh, nw, depth)

    def __enter__(self):
        import torch

        O, original = self.O, self.O.cross_attention
        h, w, nh, nw, depth = self.geo
        self.original = original
        self.calls = 0

        def cross_attention(x, context, W, name, heads=8):
            lvl = level_of(name[:-len(ATTN1)]) if name.endswith(ATTN1) else None
            if lvl is None or lvl > depth:
                return original(x, context, W, name, heads)
            assert context is None
            self.calls += 1
            H, Wd = h >> lvl, w >> lvl
            wh, ww = H // nh, Wd // nw
            q = O.dense(x, W, name + ".to_q", bias=False)
            k = O.dense(x, W, name + ".to_k", bias=False)
            v = O.dense(x, W, name + ".to_v", bias=False)
            B, S, C = q.shape
            assert S == H * Wd and H % nh == 0 and Wd % nw == 0
            d = C // heads

            def split(t):   # (B, S, C) -> (B * nh * nw, heads, wh * ww, d)
                t = t.view(B, nh, wh, nw, ww, heads, d).permute(0, 1, 3, 5, 2, 4, 6)
                return t.reshape(B * nh * nw, heads, wh * ww, d)

            qh, kh, vh = split(q), split(k), split(v)
            p = torch.softmax(torch.matmul(qh, kh.transpose(-1, -2)) * (d ** -0.5), dim=-1)
            a = torch.matmul(p, vh).view(B, nh, nw, heads, wh, ww, d).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, S, C)
            return O.dense(a, W, name + ".to_out.0")

        O.cross_attention = cross_attention
        return self

    def __exit__(self, *exc):
        self.O.cross_attention = self.original
        return False


def run(tag):
    import torch

    from minsdtf_amd import weights as Wt
    from oracle import sd_oracle as O

    job = JOBS[tag]
    torch.set_num_threads(int(os.environ.get("REFERENCE_THREADS", min(8, os.cpu_count() or 1))))
    Wn = O.named_weights(Wt.table("civitai_model"), Wt.synth_keras_weights("civitai_model", seed=WEIGHT_SEED, bias_scale=BIAS_SCALE))
    B, height, width, tile, depth = (job[k] for k in ("batch", "height", "width", "tile", "depth"))
    h, w = height // 8, width // 8
    nh, nw = height // tile, width // tile
    rng = np.random.default_rng(CONTEXT_SEED)
    cond = np.repeat(rng.standard_normal((1, 77, 768)).astype(np.float32), B, axis=0)
    unc = np.repeat(rng.standard_normal((1, 77, 768)).astype(np.float32), B, axis=0)
    noise = np.random.default_rng(NOISE_SEED).standard_normal((B, h, w, 4)).astype(np.float32)
    original = O.cross_attention
    t0 = time.time()

    def loop(windowed):
        def guided_eps(latent, tau):
            lat = np.asarray(latent, dtype=np.float32)
            te = O.timestep_embedding(tau, B)
            if windowed:
                with windowed_attention(O, h, w, nh, nw, depth) as wa:
                    u = np.asarray(O.unet_forward(Wn, lat, te, unc), dtype=np.float64)
                    c = np.asarray(O.unet_forward(Wn, lat, te, cond), dtype=np.float64)
                assert wa.calls == 2 * 5 * (depth + 1) and O.cross_attention is original
            else:
                u = np.asarray(O.unet_forward(Wn, lat, te, unc), dtype=np.float64)
                c = np.asarray(O.unet_forward(Wn, lat, te, cond), dtype=np.float64)
            print(f"  job {tag}, {'windowed' if windowed else 'plain'}: t = {tau} done at {time.time() - t0:.0f}s", flush=True)
            return u + GUIDANCE * (c - u)

        s = O.OracleScheduler()
        s.set_timesteps(STEPS)
        x = noise
        for t in s.timesteps:
            x = s.step(guided_eps(x, t), t, x)
        return np.asarray(x, dtype=np.float32)

    latent = loop(True)
    plain = loop(False)
    plain_psnr = float(O.psnr(plain, latent))
    print(f"job {tag}: the plain job against the windowed job: {plain_psnr:.1f} dB", flush=True)
    assert plain_psnr < PLAIN_PSNR_MAX, f"job {tag}: the windows move the latent too little ({plain_psnr:.1f} dB)"
    out = os.path.join(GOLD, f"oracle_hypertile_{tag}.npz")
    np.savez_compressed(out, latent=latent, plain_psnr=plain_psnr, height=height, width=width, tile=tile, depth=depth, windows=(nh, nw),
                        sampler="", batch=B, steps=STEPS, weight_seed=WEIGHT_SEED, bias_scale=BIAS_SCALE, context_seed=CONTEXT_SEED,
                        noise_seed=NOISE_SEED, guidance=GUIDANCE, guidance_rescale=0.0)
    print("wrote", out, os.path.getsize(out), "bytes in", f"{time.time() - t0:.0f}s", flush=True)


def main(argv):
    for tag in (argv or list(JOBS)):
        run(tag)


if __name__ == "__main__":
    main(sys.argv[1:])
