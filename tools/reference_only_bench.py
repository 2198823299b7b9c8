#!/usr/bin/env python3
"""Cost of reference-only control (generate_image(..., reference_only=...), minsdtf_amd/reference.py) on one GPU, seeded synthetic
SD1.5 weights:

  (i)  the msd_attention_joint launch at the four level shapes of a 512x512 job - (S, d) = (4096, 40), (1024, 80), (256, 160),
       (64, 160), 8 heads, batch 2, t = t_ref = S - with mix 0 (no snapshot) and mix 0.5: its per-launch period inside a replayed
       hipGraph, each measured twice (A/A), next to the yardstick: msd_attention with s = S and t = 2 S on the concatenated keys,
       the same FLOPs on the tuned kernel;
  (ii) a reference-only job at batch 1 (3 UNet rows), a PAG job of the same 3 rows (mid block) and the plain job (2 rows), all
       ending in the latent, timed in alternation in this one process, and the plain job a second time (A/A): the run-to-run range
       the ratios are to be read against.

    python tools/reference_only_bench.py --out profiles/reference_only_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LEVELS = ((4096, 40), (1024, 80), (256, 160), (64, 160))


def main(argv=None):
    from regions_bench import graph_period_us

    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-job", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import torch

    from minsdtf_amd import host, ops
    from minsdtf_amd.stable_diffusion import StableDiffusion

    host.fit_torch_threads()
    dev = torch.device("cuda:0")
    out = {"metric": "reference_only", "i_levels": []}

    # (i) the launch at the four level shapes
    B, H = 2, 8
    for S, d in LEVELS:
        C = H * d
        q = (torch.randn(B, S, C, device=dev) * (d ** -0.5 * 1.4426950408889634)).to(torch.bfloat16)
        k = torch.randn(B, S, C, device=dev).to(torch.bfloat16)
        vt = torch.randn(B, C, S, device=dev).to(torch.bfloat16)
        kr = torch.randn(S, C, device=dev).to(torch.bfloat16)
        vtr = torch.randn(C, S, device=dev).to(torch.bfloat16)
        kc = torch.cat([k, kr[None].expand(B, -1, -1)], dim=1).contiguous()     # [B][2S][C]
        vtc = torch.cat([vt, vtr[None].expand(B, -1, -1)], dim=2).contiguous()  # [B][C][2S]
        o = torch.zeros(B, S, C, dtype=torch.bfloat16, device=dev)
        geo = dict(batch=B, heads=H, head_dim=d, s=S, q_ld=C, k_ld=C, o_ld=C)
        half = torch.full((B,), 0.5, dtype=torch.float32, device=dev)
        j0 = ops.attention_joint(q=q, k=k, vt=vt, k_ref=kr, vt_ref=vtr, mix=None, out=o, t=S, t_ref=S, vt_ld=S, **geo)
        j5 = ops.attention_joint(q=q, k=k, vt=vt, k_ref=kr, vt_ref=vtr, mix=half, out=o, t=S, t_ref=S, vt_ld=S, **geo)
        at = ops.attention(q=q, k=kc, vt=vtc, out=o, t=2 * S, vt_ld=2 * S, scale=d ** -0.5, q_prescaled=True, **geo)
        own = ops.attention(q=q, k=k, vt=vt, out=o, t=S, vt_ld=S, scale=d ** -0.5, q_prescaled=True, **geo)
        n = 200 if S <= 1024 else 50
        p = {name: [graph_period_us(lambda st, c=c: c(st.cuda_stream), n=n) for _ in range(2)]   # (twice: A/A)
             for name, c in (("joint_mix0", j0), ("joint_mix05", j5), ("attention_2s", at), ("attention_s", own))}
        best = {k_: min(v) for k_, v in p.items()}
        out["i_levels"].append({
            "s": S, "head_dim": d, "heads": H, "batch": B,
            "period_us": {k_: [round(x, 3) for x in v] for k_, v in p.items()},
            "aa_spread": {k_: round((max(v) - min(v)) / min(v), 4) for k_, v in p.items()},
            "mix0_over_yardstick": round(best["joint_mix0"] / best["attention_2s"], 3),
            "mix05_over_yardstick": round(best["joint_mix05"] / best["attention_2s"], 3),
            "mix05_over_mix0": round(best["joint_mix05"] / best["joint_mix0"], 3),
        })

    if not args.skip_job:
        h = w = args.size // 8
        rng = np.random.default_rng(0)
        ctx = rng.standard_normal((77, 768)).astype(np.float32)
        unc = rng.standard_normal((77, 768)).astype(np.float32)
        z_ref = rng.standard_normal((1, h, w, 4)).astype(np.float32)
        pipes = []
        for _ in range(4):   # one pipeline per timed job, so each keeps its engine resident; one set of packed weights
            p = StableDiffusion(args.size, args.size, jit_compile=True, device=dev)
            if pipes:
                p._diffusion_model = pipes[0].diffusion_model
            else:
                p.diffusion_model.load_synthetic(seed=0)
            p.unconditional_context = unc
            pipes.append(p)
        kw = dict(num_steps=args.steps, unconditional_guidance_scale=7.5, seed=0, guidance_rescale=0.7, return_latent=True, batch_size=1)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        jobs = {
            "reference": lambda: pipes[0].generate_image(ctx, reference_only=dict(latent=z_ref, fidelity=0.5), **kw),
            "pag": lambda: pipes[1].generate_image(ctx, pag=dict(scale=3.0, layers="mid"), **kw),
            "plain": lambda: pipes[2].generate_image(ctx, **kw),
            "plain_again": lambda: pipes[3].generate_image(ctx, **kw),
        }
        first = timed(jobs["reference"])
        for fn in jobs.values():
            fn()   # warm: engines built, loops captured
        times = {k_: [] for k_ in jobs}
        for _ in range(args.rounds):
            for k_, fn in jobs.items():
                times[k_].append(timed(fn))
        med = {k_: statistics.median(v) for k_, v in times.items()}
        out["ii_job"] = {"size": args.size, "batch": 1, "steps": args.steps, "rounds": args.rounds,
                         "unet_rows": {"reference": 3, "pag": 3, "plain": 2},
                         "launches_per_step": {n: len(next(iter(pipes[i]._engines.values())).calls) for i, n in enumerate(("reference", "pag", "plain"))}}
        out["ii_first_call_s"] = round(first, 3)
        for k_ in jobs:
            out[f"ii_{k_}_s"] = [round(t, 5) for t in times[k_]]
        out["ii_reference_over_pag"] = round(med["reference"] / med["pag"], 4)
        out["ii_reference_over_plain"] = round(med["reference"] / med["plain"], 4)
        out["ii_pag_over_plain"] = round(med["pag"] / med["plain"], 4)
        both = times["plain"] + times["plain_again"]
        out["ii_aa_spread"] = round((max(both) - min(both)) / statistics.median(both), 4)   # the plain job's own run-to-run range
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
