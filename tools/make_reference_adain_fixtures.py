"""Generate tests/golden/oracle_reference_adain_<job>.npz: the fp32 CPU oracle's final latent of two reference-only jobs with
reference AdaIN (``generate_image(..., reference_only={..., "adain": ...})``: behind the selected block outputs every generated
row's feature map is renormalised, channel by channel, to the mean and standard deviation of the reference row of the same
forward), composed as tools/make_reference_only_fixtures.py composes its jobs, with one more swap:

  while a forward runs, this tool has replaced the module attributes sd_oracle.res_block, sd_oracle.attentions and
  sd_oracle.padded_conv by wrappers that call the original and, when the call's `name` is a selected site, renormalise the
  result's rows in front of the last one against the last row, in fp32 torch, from the formula

      mean, var over the pixels (correction 0)     std = sqrt(max(var, 0) + 1e-6)     y = (x - mean) * (std_r / std) + mean_r
      out = mix * x + (1 - mix) * y                (mix = fidelity in the u forward, 0 in the c forward)

  (the attributes are restored afterwards; nothing under oracle/ is edited).  The attention part, where the job has one, is
  make_reference_only_fixtures.reference_attention.

    python tools/make_reference_adain_fixtures.py            (both jobs)
    python tools/make_reference_adain_fixtures.py a          (one job)

  a  128x128 px, adain "auto" (the seven sites of weight 1.0) + all 16 attention blocks, fidelity 0.5, default sampler, batch 1, rescale 0
  b  64x64 px,   adain "all" (the fifteen sites), no attention block (AdaIN alone),      fidelity 1.0, dpmpp_2m,        batch 2, rescale 0.7

Stored: the seeds, the layers, the sites, the fidelity, the final latent and two PSNRs against it: `plain_psnr`, the plain job's,
and `attn_only_psnr`, that of the same job with `adain` off (for b, which has no attention part, that job IS the plain job).  Both
must be below 30 dB, so that the project's 40 dB bar tells the three jobs apart: the tool takes the first `reference_scale` of 1, 2,
4 that meets it and records the scale; if none does it says so and writes nothing.  Inputs are regenerated from the recorded numpy
PCG64 seeds exactly as in tools/make_reference_only_fixtures.py (same seeds).  Weights: the seeded synthetic UNet (seed 0,
bias_scale 0.05).  CFG 7.5, 4 steps.  Of minsdtf_amd only the weight tables and reference.ADAIN_SITES / adain_sites are used.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLD = os.path.join(ROOT, "tests", "golden")
PSNR_MAX = 30.0
SCALES = (1.0, 2.0, 4.0)
EPS = 1e-6

JOBS = {
    "a": dict(size=128, adain="auto", layers="all", fidelity=0.5, sampler=None, batch=1, rescale=0.0),
    "b": dict(size=64, adain="all", layers=(), fidelity=1.0, sampler="dpmpp_2m", batch=2, rescale=0.7),
}


class reference_adain:
    """While active, the outputs of sd_oracle.res_block / attentions / padded_conv named in `sites` are renormalised against the
    batch's last row (NCHW: the statistics run over H and W), blended by `mix`."""

    NAMES = ("res_block", "attentions", "padded_conv")

    def __init__(self, O, sites, mix):
        self.O, self.sites, self.mix = O, frozenset(sites), float(mix)

    def __enter__(self):
        import torch

        O, sites, mix = self.O, self.sites, self.mix
        self.original = {n: getattr(O, n) for n in self.NAMES}

        def renorm(y):
            x, r = y[:-1], y[-1:]
            var, mean = torch.var_mean(x, dim=(2, 3), keepdim=True, correction=0)
            var_r, mean_r = torch.var_mean(r, dim=(2, 3), keepdim=True, correction=0)
            std, std_r = torch.sqrt(var.clamp_min(0.0) + EPS), torch.sqrt(var_r.clamp_min(0.0) + EPS)
            z = (x - mean) * (std_r / std) + mean_r
            return torch.cat([mix * x + (1.0 - mix) * z, r], dim=0)

        def wrap(fn, name_of):
            def wrapped(*a, **k):
                y = fn(*a, **k)
                return renorm(y) if name_of(*a, **k) in sites else y
            return wrapped

        O.res_block = wrap(self.original["res_block"], lambda x, temb, W, name: name)
        O.attentions = wrap(self.original["attentions"], lambda x, context, W, name: name)
        O.padded_conv = wrap(self.original["padded_conv"], lambda x, W, name, stride=1, pad=1: name)
        return self

    def __exit__(self, *exc):
        for n, fn in self.original.items():
            setattr(self.O, n, fn)
        return False


class _nothing:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def run(tag):
    import torch

    import make_reference_only_fixtures as MR
    import make_sampler_fixtures as MS
    from minsdtf_amd import reference as R
    from minsdtf_amd import weights as Wt
    from oracle import sd_oracle as O

    job = JOBS[tag]
    torch.set_num_threads(int(os.environ.get("REFERENCE_THREADS", min(8, os.cpu_count() or 1))))
    Wn = O.named_weights(Wt.table("civitai_model"), Wt.synth_keras_weights("civitai_model", seed=MR.WEIGHT_SEED, bias_scale=MR.BIAS_SCALE))
    B, name, rescale, size, fidelity = (job[k] for k in ("batch", "sampler", "rescale", "size", "fidelity"))
    layers = list(MR.ALL) if job["layers"] == "all" else list(job["layers"])
    all_sites = [n for n, _gw in R.ADAIN_SITES]
    chosen = set(all_sites) if job["adain"] == "all" else set(R.adain_sites(1.0))
    sites = [n for n in all_sites if n in chosen]   # forward order
    h = w = size // 8
    rng = np.random.default_rng(MR.CONTEXT_SEED)
    base = rng.standard_normal((1, 77, 768)).astype(np.float32)
    unc = np.repeat(rng.standard_normal((1, 77, 768)).astype(np.float32), B, axis=0)
    cond = np.repeat(base, B, axis=0)
    noise = np.random.default_rng(MR.NOISE_SEED).standard_normal((B, h, w, 4)).astype(np.float32)
    n_ref = np.random.default_rng(MR.REFERENCE_NOISE_SEED).standard_normal((1, h, w, 4)).astype(np.float32)
    originals = {n: getattr(O, n) for n in reference_adain.NAMES + ("cross_attention",)}
    t0 = time.time()

    def loop(z_ref, use_layers, use_sites, what):
        """The job with the attention blocks `use_layers` and the AdaIN sites `use_sites`; both empty: the plain job."""
        def forward(rows, te, ctx, mix):
            attn = MR.reference_attention(O, use_layers, mix) if use_layers else _nothing()
            norm = reference_adain(O, use_sites, mix) if use_sites else _nothing()
            with attn, norm:
                return np.asarray(O.unet_forward(Wn, rows, te, ctx), dtype=np.float64)[:B]

        def guided_eps(latent, tau, rate):
            lat = np.asarray(latent, dtype=np.float32)
            if not use_layers and not use_sites:
                te = O.timestep_embedding(tau, B)
                u = np.asarray(O.unet_forward(Wn, lat, te, unc), dtype=np.float64)
                c = np.asarray(O.unet_forward(Wn, lat, te, cond), dtype=np.float64)
            else:
                x_r = (rate[0] * z_ref.astype(np.float64) + rate[1] * n_ref.astype(np.float64)).astype(np.float32)
                te = O.timestep_embedding(tau, B + 1)
                rows = np.concatenate([lat, x_r], axis=0)
                u = forward(rows, te, np.concatenate([unc, base], axis=0), fidelity)
                c = forward(rows, te, np.concatenate([cond, base], axis=0), 0.0)
                assert all(getattr(O, n) is fn for n, fn in originals.items())
            e = u + MR.GUIDANCE * (c - u)
            if rescale > 0:
                e = O.rescale_noise_cfg(e, c, rescale)
            print(f"  job {tag}, {what}: t = {tau} done at {time.time() - t0:.0f}s", flush=True)
            return e

        if name is None:
            s = O.OracleScheduler()
            s.set_timesteps(MR.STEPS)
            x = noise
            for t in s.timesteps:
                x = s.step(guided_eps(x, t, (s.signal_rates[t], s.noise_rates[t])), t, x)
            return np.asarray(x, dtype=np.float32)
        assert name.startswith("dpmpp_2m") and "sde" not in name
        ts, sg = MS.schedule(name, MR.STEPS)
        x = noise.astype(np.float64) * np.sqrt(1.0 + sg[0] ** 2)   # x_k = x / alpha
        old = h_last = None
        for i in range(MR.STEPS):
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

    plain = loop(None, [], [], "plain")
    measured = []
    for scale in SCALES:
        z_ref = (scale * np.random.default_rng(MR.REFERENCE_SEED).standard_normal((1, h, w, 4))).astype(np.float32)
        latent = loop(z_ref, layers, sites, f"adain x{scale:g}")
        plain_psnr = float(O.psnr(plain, latent))
        attn_only_psnr = float(O.psnr(loop(z_ref, layers, [], f"adain off x{scale:g}"), latent)) if layers else plain_psnr
        measured.append((scale, plain_psnr, attn_only_psnr))
        print(f"job {tag}, reference_scale {scale:g}: against the AdaIN job the plain job is at {plain_psnr:.1f} dB, the job with adain off at "
              f"{attn_only_psnr:.1f} dB", flush=True)
        if plain_psnr < PSNR_MAX and attn_only_psnr < PSNR_MAX:
            break
    else:
        print(f"job {tag}: NO reference_scale of {SCALES} brings both PSNRs below {PSNR_MAX:.0f} dB: {measured}; nothing written", flush=True)
        return False
    out = os.path.join(GOLD, f"oracle_reference_adain_{tag}.npz")
    np.savez_compressed(out, latent=latent, plain_psnr=plain_psnr, attn_only_psnr=attn_only_psnr, reference_scale=scale,
                        reference_seed=MR.REFERENCE_SEED, reference_noise_seed=MR.REFERENCE_NOISE_SEED, layers=np.asarray(layers, dtype=str),
                        adain=job["adain"], sites=np.asarray(sites), fidelity=fidelity, size=size, sampler="" if name is None else name,
                        batch=B, steps=MR.STEPS, weight_seed=MR.WEIGHT_SEED, bias_scale=MR.BIAS_SCALE, context_seed=MR.CONTEXT_SEED,
                        noise_seed=MR.NOISE_SEED, guidance=MR.GUIDANCE, guidance_rescale=rescale)
    print("wrote", out, os.path.getsize(out), "bytes in", f"{time.time() - t0:.0f}s", flush=True)
    return True


def main(argv):
    ok = [run(tag) for tag in (argv or list(JOBS))]
    return 0 if all(ok) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
