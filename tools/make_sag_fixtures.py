"""Generate tests/golden/sag_<size>.npz: the fp32 CPU oracle's final latent of two self-attention-guidance jobs
(``generate_image(..., sag=...)``), composed after diffusers' StableDiffusionSAGPipeline from pieces that exist without the
product's SAG code:

  1. per step: oracle.sd_oracle.unet_forward for the unconditional and the conditional context.  While the unconditional forward
     runs, this tool has wrapped the module attribute sd_oracle.cross_attention by a function that, for
     mid_block.attentions.0's attn1, also computes the softmax of that layer from the same weights and keeps
     A = probabilities.mean(heads).sum(queries); it calls the original for the result (the attribute is restored afterwards; nothing
     under oracle/ is edited);
  2. diffusers' sag_masking restated in torch: mask = A > threshold reshaped to the map and F.interpolate'd (nearest) to the latent,
     x0 = (x - sigma e_u) / alpha, F.pad(mode="reflect") + conv2d with the 9 x 9 outer-product Gaussian, x0~ = blur * mask +
     x0 * (1 - mask), and the re-noised x~ = alpha x0~ + sigma e_u (everywhere, as diffusers does);
  3. a third unet_forward on x~ with the unconditional context, eps = u + g (c - u) + s (u - d) in float64, OracleScheduler.step.

    python tools/make_sag_fixtures.py            (both sizes)
    python tools/make_sag_fixtures.py 128        (one)

128x128 px (mid block 2 x 2) and 256x256 px (4 x 4), batch 1, CFG 7.5, 4 steps, no rescale, the seeded synthetic UNet (seed 0,
bias_scale 0.05).  The contexts are default_rng(context_seed) -> the prompt, then the unconditional context, each (77, 768) times
`context_scale`; the noise is default_rng(noise_seed) - what generate_image(..., seed=noise_seed) draws.

A fixture is only written when
  * every |A - threshold| over all steps is at least MIN_MARGIN[size], itself far above 8 x the bound of msdx_attention_colsum
    (4 x profiles/sag_parity.json): the device's map is computed from bf16 activations, and an entry that changes sides changes a
    whole map cell of the degraded latent.  The tool walks CONTEXT_SEEDS until one holds and records the smallest distance as
    `margin`;
  * the PLAIN job (s = 0) lies under 35 dB against the SAG latent (`plain_psnr`), so the project's 40 dB bar tells a SAG job from
    a job without it; SCALE is chosen for that.
Nothing of minsdtf_amd is used but the weight tables.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
GUIDANCE, STEPS = 7.5, 4
WEIGHT_SEED, BIAS_SCALE, NOISE_SEED = 0, 0.05, 0
SCALE, BLUR_SIGMA, THRESHOLD = 3.0, 1.0, 1.0
PLAIN_PSNR_MAX = 35.0
MIN_MARGIN = {128: 0.02, 256: 0.004}   # (64 map entries over the four steps at 256 x 256: the first seed that keeps them all this far)
CONTEXT_SEEDS = tuple(range(1234, 1274))
CONTEXT_SCALE = 1.0
SIZES = (128, 256)
MID_ATTN1 = "mid_block.attentions.0.transformer_blocks.0.attn1"


class captured_map:
    """While active, sd_oracle.cross_attention also records A of the mid block's self-attention in `self.A` (B, S)."""

    def __init__(self, O):
        self.O, self.A = O, None

    def __enter__(self):
        import torch

        O, original = self.O, self.O.cross_attention
        self.original = original

        def cross_attention(x, context, W, name, heads=8):
            if name == MID_ATTN1:
                assert context is None
                q = O.dense(x, W, name + ".to_q", bias=False)
                k = O.dense(x, W, name + ".to_k", bias=False)
                B, S, C = q.shape
                d = C // heads
                q = q.view(B, S, heads, d).permute(0, 2, 1, 3)
                k = k.view(B, S, heads, d).permute(0, 2, 3, 1)
                p = torch.softmax(torch.matmul(q, k) * (d ** -0.5), dim=-1)   # (B, heads, queries, keys)
                self.A = p.mean(dim=1).sum(dim=1).double().numpy()
            return original(x, context, W, name, heads)

        O.cross_attention = cross_attention
        return self

    def __exit__(self, *exc):
        self.O.cross_attention = self.original
        return False


def sag_masking(x, e, alpha, sigma, A, map_hw, blur_sigma, threshold):
    """diffusers' sag_masking + its re-noising on NHWC float64 arrays, through torch."""
    import torch
    import torch.nn.functional as F

    B, h, w, C = x.shape
    mh, mw = map_hw
    x0 = torch.from_numpy((x - sigma * e) / alpha).permute(0, 3, 1, 2)
    mask = (torch.from_numpy(A) > threshold).reshape(B, 1, mh, mw).to(torch.float64)
    mask = F.interpolate(mask, (h, w)).expand(B, C, h, w)
    i = torch.arange(9, dtype=torch.float64) - 4
    t = torch.exp(-0.5 * (i / blur_sigma) ** 2)
    t = t / t.sum()
    kern = (t[:, None] * t[None, :]).expand(C, 1, 9, 9)
    blur = F.conv2d(F.pad(x0, (4, 4, 4, 4), mode="reflect"), kern, groups=C)
    deg = blur * mask + x0 * (1 - mask)
    return alpha * deg.permute(0, 2, 3, 1).numpy() + sigma * e


def run(size, bound):
    import torch

    from minsdtf_amd import weights as Wt
    from oracle import sd_oracle as O

    torch.set_num_threads(int(os.environ.get("SAG_THREADS", min(16, os.cpu_count() or 1))))
    Wn = O.named_weights(Wt.table("civitai_model"), Wt.synth_keras_weights("civitai_model", seed=WEIGHT_SEED, bias_scale=BIAS_SCALE))
    h = w = size // 8
    mh, mw = h // 8, w // 8
    noise = np.random.default_rng(NOISE_SEED).standard_normal((1, h, w, 4)).astype(np.float32)
    original = O.cross_attention
    t0 = time.time()

    def loop(scale, ctx, unc):
        margins = []
        s = O.OracleScheduler()
        s.set_timesteps(STEPS)
        x = noise
        for t in s.timesteps:
            lat = np.asarray(x, dtype=np.float32)
            te = O.timestep_embedding(t, 1)
            with captured_map(O) as cap:
                u = np.asarray(O.unet_forward(Wn, lat, te, unc), dtype=np.float64)
            assert O.cross_attention is original and cap.A is not None and cap.A.shape == (1, mh * mw)
            c = np.asarray(O.unet_forward(Wn, lat, te, ctx), dtype=np.float64)
            e = u + GUIDANCE * (c - u)
            if scale > 0:
                assert abs(cap.A.sum() - mh * mw) < 1e-3
                margins.append(float(np.abs(cap.A - THRESHOLD).min()))
                deg = sag_masking(lat.astype(np.float64), u, s.signal_rates[t], s.noise_rates[t], cap.A, (mh, mw), BLUR_SIGMA, THRESHOLD)
                d = np.asarray(O.unet_forward(Wn, deg.astype(np.float32), te, unc), dtype=np.float64)
                e = e + scale * (u - d)
            x = s.step(e, t, x)
            print(f"  {size}: scale {scale}, t = {t} done at {time.time() - t0:.0f}s" + (f", margin {margins[-1]:.4f}" if margins else ""), flush=True)
            if margins and margins[-1] < MIN_MARGIN[size]:
                return None, min(margins)
        return np.asarray(x, dtype=np.float32), (min(margins) if margins else None)

    for seed in CONTEXT_SEEDS:
        rng = np.random.default_rng(seed)
        ctx = (rng.standard_normal((1, 77, 768)) * CONTEXT_SCALE).astype(np.float32)
        unc = (rng.standard_normal((1, 77, 768)) * CONTEXT_SCALE).astype(np.float32)
        latent, margin = loop(SCALE, ctx, unc)
        if latent is None:
            print(f"{size}: context seed {seed}: a map entry {margin:.4f} from the threshold (< {MIN_MARGIN[size]}): next seed", flush=True)
            continue
        assert margin >= MIN_MARGIN[size] >= 8.0 * bound
        plain, _m = loop(0.0, ctx, unc)
        plain_psnr = float(O.psnr(plain, latent))
        print(f"{size}: context seed {seed}: margin {margin:.4f}; the plain job against the SAG job: {plain_psnr:.1f} dB", flush=True)
        assert plain_psnr < PLAIN_PSNR_MAX, f"{size}: scale {SCALE} moves the latent too little ({plain_psnr:.1f} dB): raise SCALE"
        out = os.path.join(GOLD, f"sag_{size}.npz")
        np.savez_compressed(out, latent=latent, plain_psnr=plain_psnr, margin=margin, colsum_bound=bound, scale=SCALE, blur_sigma=BLUR_SIGMA,
                            threshold=THRESHOLD, size=size, steps=STEPS, weight_seed=WEIGHT_SEED, bias_scale=BIAS_SCALE, context_seed=seed,
                            context_scale=CONTEXT_SCALE, noise_seed=NOISE_SEED, guidance=GUIDANCE)
        print("wrote", out, os.path.getsize(out), "bytes in", f"{time.time() - t0:.0f}s", flush=True)
        return
    raise SystemExit(f"{size}: no context seed of {CONTEXT_SEEDS} keeps every map entry {MIN_MARGIN[size]} from the threshold")


def main(argv):
    with open(os.path.join(ROOT, "profiles", "sag_parity.json")) as f:
        bound = 4.0 * json.load(f)["colsum_max_rel_err"]
    for size in ([int(a) for a in argv] or list(SIZES)):
        run(size, bound)


if __name__ == "__main__":
    main(sys.argv[1:])
