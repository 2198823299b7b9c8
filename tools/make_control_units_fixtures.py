"""Generate tests/golden/control_units_<size>.npz: the fp32 CPU oracle's final latent of two jobs with ControlNet units
(``generate_image(..., control_net_image=img, control=...)``), composed from pieces that exist without the product's code for it:

  1. per step and half of the guidance pair: oracle.sd_oracle.controlnet_forward of every unit on its own hint
     (oracle.sd_oracle.hintnet_forward of its picture), the 13 residuals scaled by the rule restated here (`scale`) and summed;
  2. oracle.sd_oracle.unet_forward(controls=...) for the unconditional and the conditional context;
  3. guidance, rescale, OracleScheduler.step.

    python tools/make_control_units_fixtures.py            (both jobs)
    python tools/make_control_units_fixtures.py 128        (one)

Batch 1, 4 steps, guidance 7.5, rescale 0.7, the seeded synthetic UNet (seed 0, bias_scale 0.05); unit n's ControlNet and HintNet are
the synthetic ones of seed n.  The contexts are default_rng(context_seed) -> the prompt, then the unconditional context, each
(77, 768); the noise is default_rng(noise_seed) - what generate_image(..., seed=noise_seed) draws; unit n's picture is
default_rng(hint_seed + n).integers(0, 256, (size, size, 3)).
Job A (128 px): one unit, weight 0.6, end 0.5, mode "prompt".  Job B (256 px): unit 0 at weight 1.0, mode "control"; unit 1 at
weight 0.7, start 0.25, "balanced", on a second picture.

A fixture is only written when the PLAIN ControlNet job (unit 0 alone, full strength, every step, both halves) and the job WITHOUT
a ControlNet both lie under 35 dB against it (`plain_psnr`, `none_psnr`), so the project's 40 dB bar tells the feature from its
absence.  Nothing of minsdtf_amd is used but the weight tables.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
GUIDANCE, RESCALE, STEPS = 7.5, 0.7, 4
WEIGHT_SEED, BIAS_SCALE, NOISE_SEED, CONTEXT_SEED, HINT_SEED = 0, 0.05, 0, 1234, 77
PLAIN_PSNR_MAX = 35.0
JOBS = {128: [dict(weight=0.6, start=0.0, end=0.5, mode="prompt")],
        256: [dict(weight=1.0, start=0.0, end=1.0, mode="control"), dict(weight=0.7, start=0.25, end=1.0, mode="balanced")]}
PLAIN = [dict(weight=1.0, start=0.0, end=1.0, mode="balanced")]
SIZES = (128, 256)


def scale(unit, i, k, half, steps):
    """s(i, n, k, half): weight * keep(i) * (0.825 ** (12 - k) unless "balanced"), 0 on the unconditional half (0) in mode "control";
    keep(i) is diffusers' rule; rounded to fp32 as the device table is."""
    keep = 0.0 if (i / steps < unit["start"] or (i + 1) / steps > unit["end"]) else 1.0
    s = unit["weight"] * keep * (0.825 ** (12 - k) if unit["mode"] != "balanced" else 1.0)
    if unit["mode"] == "control" and half == 0:
        s = 0.0
    return float(np.float32(s))


def run(size):
    import torch

    from minsdtf_amd import weights as Wt
    from oracle import sd_oracle as O

    torch.set_num_threads(int(os.environ.get("CONTROL_UNITS_THREADS", min(16, os.cpu_count() or 1))))
    synth = lambda table, seed: O.named_weights(Wt.table(table), Wt.synth_keras_weights(table, seed=seed, bias_scale=BIAS_SCALE))
    Wn = synth("civitai_model", WEIGHT_SEED)
    h = w = size // 8
    job = JOBS[size]
    nets = [(synth("controlnet", n), synth("hintnet", n)) for n in range(len(job))]
    pictures = [np.random.default_rng(HINT_SEED + n).integers(0, 256, (size, size, 3)).astype(np.float32) for n in range(len(job))]
    hints = [O.hintnet_forward(Wh, pic[None] / 255.0) for (_Wc, Wh), pic in zip(nets, pictures)]
    noise = np.random.default_rng(NOISE_SEED).standard_normal((1, h, w, 4)).astype(np.float32)
    rng = np.random.default_rng(CONTEXT_SEED)
    ctx = rng.standard_normal((1, 77, 768)).astype(np.float32)
    unc = rng.standard_normal((1, 77, 768)).astype(np.float32)
    t0 = time.time()

    def loop(units, label):
        s = O.OracleScheduler()
        s.set_timesteps(STEPS)
        x = noise
        for i, t in enumerate(s.timesteps):
            lat = np.asarray(x, dtype=np.float32)
            te = O.timestep_embedding(t, 1)

            def eps(context, half):
                controls = None
                for n, unit in enumerate(units or ()):
                    sc = [scale(unit, i, k, half, STEPS) for k in range(13)]
                    if not any(sc):
                        continue
                    r = O.controlnet_forward(nets[n][0], lat, te, context, hints[n])
                    controls = controls or [np.zeros_like(a, dtype=np.float64) for a in r]
                    controls = [acc + sk * np.asarray(a, dtype=np.float64) for acc, sk, a in zip(controls, sc, r)]
                return np.asarray(O.unet_forward(Wn, lat, te, context, controls=controls), dtype=np.float64)

            u, c = eps(unc, 0), eps(ctx, 1)
            e = O.rescale_noise_cfg(u + GUIDANCE * (c - u), c, RESCALE)
            x = s.step(e, t, x)
            print(f"  {size}: {label}, t = {t} done at {time.time() - t0:.0f}s", flush=True)
        return np.asarray(x, dtype=np.float32)

    latent = loop(job, "units")
    plain_psnr = float(O.psnr(loop(PLAIN, "plain ControlNet"), latent))
    none_psnr = float(O.psnr(loop(None, "no ControlNet"), latent))
    print(f"{size}: against the job with units: the plain ControlNet job {plain_psnr:.1f} dB, the job without ControlNet {none_psnr:.1f} dB", flush=True)
    assert np.all(np.isfinite(latent))
    assert plain_psnr < PLAIN_PSNR_MAX and none_psnr < PLAIN_PSNR_MAX, \
        f"{size}: the units move the latent too little ({plain_psnr:.1f} / {none_psnr:.1f} dB against the plain job / no ControlNet)"
    out = os.path.join(GOLD, f"control_units_{size}.npz")
    np.savez_compressed(out, latent=latent, plain_psnr=plain_psnr, none_psnr=none_psnr, size=size, steps=STEPS, weight_seed=WEIGHT_SEED,
                        bias_scale=BIAS_SCALE, context_seed=CONTEXT_SEED, noise_seed=NOISE_SEED, hint_seed=HINT_SEED, guidance=GUIDANCE,
                        rescale=RESCALE, units=len(job), **{f"unit{n}_{k}": v for n, u in enumerate(job) for k, v in u.items()})
    print("wrote", out, os.path.getsize(out), "bytes in", f"{time.time() - t0:.0f}s", flush=True)


def main(argv):
    for size in ([int(a) for a in argv] or list(SIZES)):
        run(size)


if __name__ == "__main__":
    main(sys.argv[1:])
