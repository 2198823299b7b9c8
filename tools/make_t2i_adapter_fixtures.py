"""Generate tests/golden/t2i_adapter_<size>.npz: the fp32 CPU oracle's final latent of two T2I-Adapter jobs
(``generate_image(..., t2i_adapter=...)``), composed after diffusers' down_intrablock_additional_residuals from pieces that exist
without the product's T2I-Adapter code:

  1. the four features of every unit in torch float64, from the synthetic adapter's state dict (the public file layout;
     models.T2IAdapter.synthetic_state - a weight table, like the synthetic UNet's) and torch.nn.functional: pixel_unshuffle(8),
     conv_in, per level [avg_pool2d(2) | in_conv | twice block2(relu(block1(x))) + x];
  2. per step: oracle.sd_oracle.unet_forward for the unconditional and the conditional context.  While a forward runs, this tool has
     wrapped the module attributes sd_oracle.attentions and sd_oracle.res_block by functions that call the original and, behind the
     calls named down_blocks.{0,1,2}.attentions.1 and down_blocks.3.resnets.1, add sum_u s(i, u, l) * feature_u[l] to the result -
     so the skip and the onward path both see it; every other name goes through unchanged (the attributes are restored afterwards;
     nothing under oracle/ is edited);
  3. eps = u + g (c - u), OracleScheduler.step.

    python tools/make_t2i_adapter_fixtures.py            (both sizes)
    python tools/make_t2i_adapter_fixtures.py 128        (one)

128x128 px: one unit (3-channel adapter), end = 0.75, so the last of the 4 steps runs at scale 0; 256x256 px: two units - a 3-channel
adapter with four per-site weights w * SITE_WEIGHTS and a 1-channel adapter at weight w over start = 0.25.  Both: batch 1, CFG 7.5,
no rescale, the seeded synthetic UNet (seed 0, bias_scale 0.05), synthetic adapters (seeds ADAPTER_SEEDS) and seeded pictures
(default_rng([PICTURE_SEED, unit]).integers(0, 256) as uint8, divided by 255).  The contexts are default_rng(CONTEXT_SEED) -> the
prompt, then the unconditional context, each (77, 768); the noise is default_rng(NOISE_SEED) - what generate_image(...,
seed=NOISE_SEED) draws.

A fixture is only written when the PLAIN job (no adapter) lies under 35 dB against it (`plain_psnr`), so the project's 40 dB bar
tells an adapter job from a job without it: the tool walks WEIGHTS upwards until that holds and records the weight.
Nothing of minsdtf_amd is used but the weight tables.  Runs on the CPU.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
GUIDANCE, STEPS = 7.5, 4
WEIGHT_SEED, BIAS_SCALE, NOISE_SEED, CONTEXT_SEED, PICTURE_SEED = 0, 0.05, 0, 1234, 91
ADAPTER_SEEDS = (7, 8)
WEIGHTS = (1.0, 2.0, 4.0, 8.0, 16.0)
SITE_WEIGHTS = (1.0, 0.75, 0.5, 0.25)
PLAIN_PSNR_MAX = 35.0
CHANNELS = (320, 640, 1280, 1280)
SITES = ("down_blocks.0.attentions.1", "down_blocks.1.attentions.1", "down_blocks.2.attentions.1", "down_blocks.3.resnets.1")


def units_of(size, weight):
    """[(adapter seed, in_channels, four site weights, start, end)] of the fixture of this size at walk weight `weight`."""
    if size == 128:
        return [(ADAPTER_SEEDS[0], 3, (weight,) * 4, 0.0, 0.75)]
    return [(ADAPTER_SEEDS[0], 3, tuple(weight * f for f in SITE_WEIGHTS), 0.0, 1.0), (ADAPTER_SEEDS[1], 1, (weight,) * 4, 0.25, 1.0)]


def keep(i, start, end):
    """diffusers' control_guidance rule."""
    return 0.0 if (i / STEPS < start or (i + 1) / STEPS > end) else 1.0


def picture_of(size, unit, cin):
    shape = (size, size, 3) if cin == 3 else (size, size)
    return np.random.default_rng([PICTURE_SEED, unit]).integers(0, 256, shape).astype(np.uint8)


def features(state, picture, cin):
    """The full adapter in torch float64, NCHW: the four features."""
    import torch
    import torch.nn.functional as F

    w = {k[len("adapter."):]: torch.from_numpy(v).double() for k, v in state.items()}
    x = torch.from_numpy(np.asarray(picture, dtype=np.float64) / 255.0).reshape(1, picture.shape[0], picture.shape[1], cin).permute(0, 3, 1, 2)
    x = F.conv2d(F.pixel_unshuffle(x, 8), w["conv_in.weight"], w["conv_in.bias"], padding=1)
    out = []
    for l, ch in enumerate(CHANNELS):
        if l > 0:
            x = F.avg_pool2d(x, 2, 2)
            if ch != CHANNELS[l - 1]:
                x = F.conv2d(x, w[f"body.{l}.in_conv.weight"], w[f"body.{l}.in_conv.bias"])
        for j in range(2):
            n = f"body.{l}.resnets.{j}"
            h = F.relu(F.conv2d(x, w[n + ".block1.weight"], w[n + ".block1.bias"], padding=1))
            x = F.conv2d(h, w[n + ".block2.weight"], w[n + ".block2.bias"]) + x
        out.append(x)
    return out


class injected:
    """While active, sd_oracle.attentions / sd_oracle.res_block add `terms[l]` (NCHW, or None) behind the call named SITES[l]."""

    def __init__(self, O, terms):
        self.O, self.terms = O, terms

    def __enter__(self):
        O = self.O
        self.originals = (O.attentions, O.res_block)
        att, res = self.originals

        def add(y, name):
            if name in SITES and self.terms[SITES.index(name)] is not None:
                return y + self.terms[SITES.index(name)].to(y.dtype)
            return y

        def attentions(x, context, W, name):
            return add(att(x, context, W, name), name)

        def res_block(x, temb, W, name):
            return add(res(x, temb, W, name), name)

        O.attentions, O.res_block = attentions, res_block
        return self

    def __exit__(self, *exc):
        self.O.attentions, self.O.res_block = self.originals
        return False


def run(size):
    import torch

    from minsdtf_amd import weights as Wt
    from minsdtf_amd.models import T2IAdapter
    from oracle import sd_oracle as O

    torch.set_num_threads(int(os.environ.get("T2I_THREADS", min(16, os.cpu_count() or 1))))
    Wn = O.named_weights(Wt.table("civitai_model"), Wt.synth_keras_weights("civitai_model", seed=WEIGHT_SEED, bias_scale=BIAS_SCALE))
    h = w = size // 8
    noise = np.random.default_rng(NOISE_SEED).standard_normal((1, h, w, 4)).astype(np.float32)
    rng = np.random.default_rng(CONTEXT_SEED)
    ctx = rng.standard_normal((1, 77, 768)).astype(np.float32)
    unc = rng.standard_normal((1, 77, 768)).astype(np.float32)
    feats = []
    for n, (seed, cin, _w, _s, _e) in enumerate(units_of(size, 1.0)):
        with torch.no_grad():
            feats.append(features(T2IAdapter.synthetic_state(seed, cin), picture_of(size, n, cin), cin))
    originals = (O.attentions, O.res_block)
    t0 = time.time()

    def loop(weight):
        s = O.OracleScheduler()
        s.set_timesteps(STEPS)
        units = units_of(size, weight)
        x = noise
        for i, t in enumerate(s.timesteps):
            lat = np.asarray(x, dtype=np.float32)
            te = O.timestep_embedding(t, 1)
            terms = []
            for l in range(4):
                sc = [wts[l] * keep(i, start, end) for (_seed, _cin, wts, start, end) in units]
                terms.append(sum(c * f[l] for c, f in zip(sc, feats) if c != 0.0) if any(c != 0.0 for c in sc) else None)
            with injected(O, terms):
                u = np.asarray(O.unet_forward(Wn, lat, te, unc), dtype=np.float64)
                c = np.asarray(O.unet_forward(Wn, lat, te, ctx), dtype=np.float64)
            assert (O.attentions, O.res_block) == originals
            x = s.step(u + GUIDANCE * (c - u), t, x)
            print(f"  {size}: weight {weight}, step {i} (t = {t}) done at {time.time() - t0:.0f}s", flush=True)
        return np.asarray(x, dtype=np.float32)

    plain = loop(0.0)
    for weight in WEIGHTS:
        latent = loop(weight)
        plain_psnr = float(O.psnr(plain, latent))
        print(f"{size}: weight {weight}: the plain job against the adapter job: {plain_psnr:.1f} dB", flush=True)
        if plain_psnr >= PLAIN_PSNR_MAX:
            continue
        units = units_of(size, weight)
        out = os.path.join(GOLD, f"t2i_adapter_{size}.npz")
        np.savez_compressed(out, latent=latent, plain_psnr=plain_psnr, weight=weight, size=size, steps=STEPS, units=len(units),
                            adapter_seeds=np.asarray([u[0] for u in units]), in_channels=np.asarray([u[1] for u in units]),
                            site_weights=np.asarray([u[2] for u in units], dtype=np.float64), start=np.asarray([u[3] for u in units]),
                            end=np.asarray([u[4] for u in units]), picture_seed=PICTURE_SEED, weight_seed=WEIGHT_SEED, bias_scale=BIAS_SCALE,
                            context_seed=CONTEXT_SEED, noise_seed=NOISE_SEED, guidance=GUIDANCE)
        print("wrote", out, os.path.getsize(out), "bytes in", f"{time.time() - t0:.0f}s", flush=True)
        return
    raise SystemExit(f"{size}: no weight of {WEIGHTS} moves the latent under {PLAIN_PSNR_MAX} dB: extend WEIGHTS")


def main(argv):
    for size in ([int(a) for a in argv] or [128, 256]):
        run(size)


if __name__ == "__main__":
    main(sys.argv[1:])
