"""Generate tests/golden/oracle_reference_only_<job>.npz: the fp32 CPU oracle's final latent of two reference-only jobs
(``generate_image(..., reference_only={...})``: in the selected attention blocks the generated rows' self-attention also attends
to the keys of one reference row of the same forward), composed from pieces that exist without the product's kernel:

  1. per step: x_r = a z_ref + b n_ref at the step's signal / noise rate, then oracle.sd_oracle.unet_forward over the rows
     [u..., r] and likewise over [c..., r] (r with the conditional context of sample 0) while this tool has replaced the module
     attribute sd_oracle.cross_attention by a function that, for every ".attn1" of a selected block, concatenates the last row's
     K and V onto the other rows' (restated here from the formula, over sd_oracle.dense), blends the joint result with the plain
     one by `fidelity` (the u forward) or not at all (the c forward), gives the last row its plain self-attention and applies
     to_out; everywhere else it calls the original (the attribute is restored afterwards; nothing under oracle/ is edited);
  2. guidance, oracle.sd_oracle.rescale_noise_cfg, and the step: OracleScheduler.step (job a) or the DPM++ 2M update on the
     schedule of tools/make_sampler_fixtures.py (job b), as tools/make_region_attention_fixtures.py.

    python tools/make_reference_only_fixtures.py            (both jobs)
    python tools/make_reference_only_fixtures.py a          (one job)

  a  128x128 px, all 16 blocks,                   fidelity 0.5, default sampler, batch 1, rescale 0
  b  64x64 px, mid + the three up_blocks.1 blocks, fidelity 1.0, dpmpp_2m,        batch 2, rescale 0.7

Stored: the seeds, the layers, the fidelity, the final latent and `plain_psnr`: the PSNR of the same job without the reference
against the reference-only latent.  The tool asserts plain_psnr < 30 dB, so the project's 40 dB bar tells the feature from its
absence; if the synthetic UNet moves too little REFERENCE_SCALE is raised, recorded in the file as `reference_scale`.  Inputs are
regenerated from the recorded numpy PCG64 seeds: contexts default_rng(1234) -> the prompt, then the unconditional context, each
(77, 768); noise default_rng(0) (B, h, w, 4); z_ref = REFERENCE_SCALE * default_rng(77).standard_normal((1, h, w, 4)), passed as
"latent"; n_ref = default_rng(REFERENCE_NOISE_SEED).standard_normal((1, h, w, 4)).  Weights: the seeded synthetic UNet (seed 0,
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
REFERENCE_SEED, REFERENCE_NOISE_SEED = 77, 78
PLAIN_PSNR_MAX = 30.0
REFERENCE_SCALE = {"a": 1.0, "b": 1.0}
ATTN1 = ".transformer_blocks.0.attn1"

DOWN = [f"down_blocks.{lv}.attentions.{r}" for lv in range(3) for r in range(2)]
UP = [f"up_blocks.{u}.attentions.{r}" for u in (1, 2, 3) for r in range(3)]
ALL = DOWN + ["mid_block.attentions.0"] + UP    # forward order
MID_UP1 = ["mid_block.attentions.0"] + [f"up_blocks.1.attentions.{r}" for r in range(3)]

JOBS = {
    "a": dict(size=128, layers=ALL, fidelity=0.5, sampler=None, batch=1, rescale=0.0),
    "b": dict(size=64, layers=MID_UP1, fidelity=1.0, sampler="dpmpp_2m", batch=2, rescale=0.7),
}


class reference_attention:
    """While active, sd_oracle.cross_attention gives every ".attn1" of the blocks `layers` the reference route: the batch's last
    row is the reference; the rows in front of it take mix * plain + (1 - mix) * joint."""

    def __init__(self, O, layers, mix):
        self.O, self.layers, self.mix = O, frozenset(layers), float(mix)

    def __enter__(self):
        import torch

        O, layers, mix, original = self.O, self.layers, self.mix, self.O.cross_attention
        self.original = original

        def cross_attention(x, context, W, name, heads=8):
            if not (name.endswith(ATTN1) and name[:-len(ATTN1)] in layers):
                return original(x, context, W, name, heads)
            assert context is None
            q = O.dense(x, W, name + ".to_q", bias=False)
            k = O.dense(x, W, name + ".to_k", bias=False)
            v = O.dense(x, W, name + ".to_v", bias=False)
            B, S, C = q.shape
            d = C // heads

            def split(t):
                return t.view(t.shape[0], -1, heads, d).permute(0, 2, 1, 3)

            def attend(qh, kh, vh):
                p = torch.softmax(torch.matmul(qh, kh.transpose(-1, -2)) * (d ** -0.5), dim=-1)
                return torch.matmul(p, vh).permute(0, 2, 1, 3).reshape(qh.shape[0], -1, C)

            qh, kh, vh = split(q), split(k), split(v)
            plain = attend(qh, kh, vh)                       # every row, the reference row's result too
            g = B - 1
            kj = torch.cat([kh[:g], kh[g:].expand(g, -1, -1, -1)], dim=2)
            vj = torch.cat([vh[:g], vh[g:].expand(g, -1, -1, -1)], dim=2)
            joint = attend(qh[:g], kj, vj)
            a = plain.clone()
            a[:g] = joint if mix == 0.0 else plain[:g] if mix == 1.0 else mix * plain[:g] + (1.0 - mix) * joint
            return O.dense(a, W, name + ".to_out.0")

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
    torch.set_num_threads(int(os.environ.get("REFERENCE_THREADS", min(8, os.cpu_count() or 1))))
    Wn = O.named_weights(Wt.table("civitai_model"), Wt.synth_keras_weights("civitai_model", seed=WEIGHT_SEED, bias_scale=BIAS_SCALE))
    B, name, rescale, size, layers, fidelity = (job[k] for k in ("batch", "sampler", "rescale", "size", "layers", "fidelity"))
    h = w = size // 8
    scale = float(REFERENCE_SCALE[tag])
    rng = np.random.default_rng(CONTEXT_SEED)
    base = rng.standard_normal((1, 77, 768)).astype(np.float32)
    unc = np.repeat(rng.standard_normal((1, 77, 768)).astype(np.float32), B, axis=0)
    cond = np.repeat(base, B, axis=0)
    noise = np.random.default_rng(NOISE_SEED).standard_normal((B, h, w, 4)).astype(np.float32)
    z_ref = (scale * np.random.default_rng(REFERENCE_SEED).standard_normal((1, h, w, 4))).astype(np.float32)
    n_ref = np.random.default_rng(REFERENCE_NOISE_SEED).standard_normal((1, h, w, 4)).astype(np.float32)
    original = O.cross_attention
    t0 = time.time()

    def loop(with_reference):
        def guided_eps(latent, tau, rate):
            lat = np.asarray(latent, dtype=np.float32)
            if not with_reference:
                te = O.timestep_embedding(tau, B)
                u = np.asarray(O.unet_forward(Wn, lat, te, unc), dtype=np.float64)
                c = np.asarray(O.unet_forward(Wn, lat, te, cond), dtype=np.float64)
            else:
                x_r = (rate[0] * z_ref.astype(np.float64) + rate[1] * n_ref.astype(np.float64)).astype(np.float32)
                te = O.timestep_embedding(tau, B + 1)
                rows = np.concatenate([lat, x_r], axis=0)
                with reference_attention(O, layers, fidelity):
                    u = np.asarray(O.unet_forward(Wn, rows, te, np.concatenate([unc, base], axis=0)), dtype=np.float64)[:B]
                with reference_attention(O, layers, 0.0):
                    c = np.asarray(O.unet_forward(Wn, rows, te, np.concatenate([cond, base], axis=0)), dtype=np.float64)[:B]
                assert O.cross_attention is original
            e = u + GUIDANCE * (c - u)
            if rescale > 0:
                e = O.rescale_noise_cfg(e, c, rescale)
            print(f"  job {tag}, {'reference' if with_reference else 'plain'}: t = {tau} done at {time.time() - t0:.0f}s", flush=True)
            return e

        if name is None:
            s = O.OracleScheduler()
            s.set_timesteps(STEPS)
            x = noise
            for t in s.timesteps:
                x = s.step(guided_eps(x, t, (s.signal_rates[t], s.noise_rates[t])), t, x)
            return np.asarray(x, dtype=np.float32)
        assert name.startswith("dpmpp_2m") and "sde" not in name
        ts, sg = MS.schedule(name, STEPS)
        x = noise.astype(np.float64) * np.sqrt(1.0 + sg[0] ** 2)   # x_k = x / alpha
        old = h_last = None
        for i in range(STEPS):
            a = 1.0 / np.sqrt(1.0 + sg[i] * sg[i])
            d = x - sg[i] * np.asarray(guided_eps(a * x, ts[i], (a, sg[i] * a)), dtype=np.float64)
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
    print(f"job {tag}: the plain job against the reference-only job: {plain_psnr:.1f} dB", flush=True)
    assert plain_psnr < PLAIN_PSNR_MAX, f"job {tag}: the reference moves the latent too little ({plain_psnr:.1f} dB): raise REFERENCE_SCALE"
    out = os.path.join(GOLD, f"oracle_reference_only_{tag}.npz")
    np.savez_compressed(out, latent=latent, plain_psnr=plain_psnr, reference_scale=scale, reference_seed=REFERENCE_SEED,
                        reference_noise_seed=REFERENCE_NOISE_SEED, layers=np.asarray(layers), fidelity=fidelity, size=size,
                        sampler="" if name is None else name, batch=B, steps=STEPS, weight_seed=WEIGHT_SEED, bias_scale=BIAS_SCALE,
                        context_seed=CONTEXT_SEED, noise_seed=NOISE_SEED, guidance=GUIDANCE, guidance_rescale=rescale)
    print("wrote", out, os.path.getsize(out), "bytes in", f"{time.time() - t0:.0f}s", flush=True)


def main(argv):
    for tag in (argv or list(JOBS)):
        run(tag)


if __name__ == "__main__":
    main(sys.argv[1:])
