#!/usr/bin/env python3
"""images/s of each sampler of generate_image(..., sampler=...) against the default sampler at the same step counts, on one GPU.

    python tools/sampler_bench.py [--size 512] [--batch 1] [--steps 20,25] [--rounds 5]

One job = text_to_image's device path end to end (whole-loop hipGraph, VAE decode to uint8, the host copy of the images) with
seeded synthetic SD1.5 weights and N(0,1) contexts.  Every configuration is warmed up once (engine build + graph capture), then
the configurations are timed in alternation, `rounds` times, in one process (so clock and thermal drift hit all of them alike);
the median job time of each is reported.  Prints ONE JSON line: images/s per sampler and step count, each sampler's ratio
to the default sampler at the same step count, and for the stochastic samplers the host time of drawing and uploading their
per-step noise against the job time they add (`host_split_ms`).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SAMPLERS = [None, "dpmpp_2m_karras", "dpmpp_2m_sde_karras", "euler_a"]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--steps", default="20,25")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args(argv)
    import torch

    from minsdtf_amd import host
    from minsdtf_amd.stable_diffusion import StableDiffusion

    host.fit_torch_threads()
    dev = torch.device("cuda:0")
    sd = StableDiffusion(args.size, args.size, jit_compile=True, device=dev)
    sd.diffusion_model.load_synthetic(seed=0)
    sd.image_decoder.load_synthetic(seed=0)
    rng = np.random.default_rng(1234)
    ctx = rng.standard_normal((args.batch, 77, 768)).astype(np.float32)
    sd.unconditional_context = rng.standard_normal((77, 768)).astype(np.float32)
    steps = [int(s) for s in args.steps.split(",")]
    configs = [(s, k) for k in steps for s in SAMPLERS]

    def job(sampler, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = sd.generate_image(ctx, batch_size=args.batch, num_steps=k, seed=0, guidance_rescale=0.7, sampler=sampler)
        torch.cuda.synchronize()
        assert img.shape == (args.batch, args.size, args.size, 3)
        return time.perf_counter() - t0

    times = {c: [] for c in configs}
    for r in range(args.rounds):
        for c in configs:
            # one engine is resident at a time, so each configuration rebuilds it: a warm job (build + capture) precedes every timed one
            job(*c)
            times[c].append(job(*c))   # the replayed job
            print(f"round {r}: {c[0] or 'default'} x {c[1]}: {times[c][-1] * 1e3:.1f} ms", file=sys.stderr, flush=True)
    out = {"metric": "sampler_images_per_s", "size": args.size, "batch": args.batch, "rounds": args.rounds, "results": {}}
    for k in steps:
        base = args.batch / statistics.median(times[(None, k)])
        for s in SAMPLERS:
            ips = args.batch / statistics.median(times[(s, k)])
            out["results"][f"{s or 'default'}@{k}"] = {"images_per_s": round(ips, 4), "vs_default": round(ips / base, 4),
                                                        "ms_median": round(statistics.median(times[(s, k)]) * 1e3, 2)}
    # the host's share of a stochastic sampler's job: drawing the per-step N(0,1) noise (samplers.draw_step_noise, as
    # generate_image calls it) and the upload into the engine (DenoiseEngine.prepare's copy), each the median of 5, set against
    # the job time it adds over the default sampler at the same step count
    from minsdtf_amd import samplers as smp

    h = w = args.size // 8
    out["host_split_ms"] = {}
    for k in steps:
        for s in SAMPLERS:
            if s is None or not smp.parse(s).stochastic:
                continue
            job(s, k)
            eng = next(iter(sd._engines.values()))
            draw, upload = [], []
            for _ in range(5):
                t0 = time.perf_counter()
                z = smp.draw_step_noise(args.batch, k, h, w, seed=0)
                draw.append(time.perf_counter() - t0)
                zz = z.reshape(args.batch, k, -1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.step_noise.copy_(torch.from_numpy(zz).transpose(0, 1))
                torch.cuda.synchronize()
                upload.append(time.perf_counter() - t0)
            added = statistics.median(times[(s, k)]) - statistics.median(times[(None, k)])
            d, u = statistics.median(draw), statistics.median(upload)
            out["host_split_ms"][f"{s}@{k}"] = {"job_added": round(added * 1e3, 3), "draw": round(d * 1e3, 3),
                                                "upload": round(u * 1e3, 3), "rest": round((added - d - u) * 1e3, 3)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
